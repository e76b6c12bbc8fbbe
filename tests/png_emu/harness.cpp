// scheduler of tests/png_emu/v3d_common.h (see there)
#include "v3d_common.h"
#include <stdlib.h>
int g_misaligned;
extern "C" int emu_misaligned_loads() { return g_misaligned; }
Fiber* g_cur; ucontext_t g_sched; dim3 blockIdx, gridDim; int g_nthreads;
long g_bar_count[1024], g_bar_phase[256], g_sh_phase[256], g_sh_count[4][1024]; uint32_t g_sh_val[4][1024][64];
alignas(16) uint8_t smem[65536 + 64];
void v3d_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); }
void fiber_yield() { swapcontext(&g_cur->ctx, &g_sched); }
static std::function<void()>* g_body;
static void tramp() { (*g_body)(); g_cur->done = true; swapcontext(&g_cur->ctx, &g_sched); }
void run_grid(dim3 grid, dim3 block, size_t lds, std::function<void()> body)
{
    if (lds > 65536 || block.x > 256) { fprintf(stderr, "launch outside the emulator's range\n"); abort(); }
    g_body = &body; gridDim = grid; g_nthreads = block.x;
    static std::vector<Fiber> fibers(256);
    for (unsigned by = 0; by < grid.y; ++by) for (unsigned bx = 0; bx < grid.x; ++bx) {
        blockIdx = dim3(bx, by, 0);
        memset(g_bar_count, 0, sizeof g_bar_count); memset(g_bar_phase, 0, sizeof g_bar_phase);
        memset(g_sh_phase, 0, sizeof g_sh_phase); memset(g_sh_count, 0, sizeof g_sh_count);
        memset(smem, 0xCD, sizeof smem);                     // LDS holds garbage at launch
        for (unsigned t = 0; t < block.x; ++t) {
            Fiber& f = fibers[t]; f.done = false; f.tid = dim3(t, 0, 0); f.stack.resize(256 * 1024);
            getcontext(&f.ctx); f.ctx.uc_stack.ss_sp = f.stack.data(); f.ctx.uc_stack.ss_size = f.stack.size(); f.ctx.uc_link = &g_sched;
            makecontext(&f.ctx, tramp, 0);
        }
        for (bool any = true; any;) {
            any = false;
            for (unsigned t = 0; t < block.x; ++t) if (!fibers[t].done) { any = true; g_cur = &fibers[t]; swapcontext(&g_sched, &fibers[t].ctx); }
        }
    }
}
