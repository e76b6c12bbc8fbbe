// scheduler of tests/emu/v3d_common.h (see there)
#include "v3d_common.h"
#include <stdlib.h>
#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/common_interface_defs.h>
#include <sanitizer/asan_interface.h>
#define EMU_ASAN 1
#else
#define EMU_ASAN 0
#endif
#define EMU_MAX_LDS (160 * 1024)                               // a CDNA4 workgroup's LDS
int g_misaligned, g_nopayload;
Fiber* g_cur; static Fiber g_sched; dim3 blockIdx, gridDim, blockDim; int g_nthreads; long g_progress;
long g_bar_count[EMU_RING], g_bar_phase[EMU_MAX_THREADS], g_sh_phase[EMU_MAX_THREADS], g_sh_count[EMU_MAX_THREADS / 64][EMU_RING];
int g_bar_or[EMU_RING]; uint32_t g_sh_val[EMU_MAX_THREADS / 64][EMU_RING][64];
unsigned char* g_lds;
static int g_wg_desc, g_thr_desc, g_lds_poison = 0xCD;
struct Extent { uintptr_t a0, a1, p0, p1; };
static std::vector<Extent> g_extents;

extern "C" int emu_misaligned_loads() { return g_misaligned; }
extern "C" int emu_nopayload_loads() { return g_nopayload; }
extern "C" void emu_configure(int wg_descending, int threads_descending, int lds_poison)
{
    g_wg_desc = wg_descending; g_thr_desc = threads_descending; g_lds_poison = lds_poison;
}
extern "C" void emu_register_payload(const void* alloc, size_t alloc_bytes, const void* payload, size_t payload_bytes)
{
    g_extents.push_back({ (uintptr_t)alloc, (uintptr_t)alloc + alloc_bytes, (uintptr_t)payload, (uintptr_t)payload + payload_bytes });
}
void emu_check_block(const void* p, size_t bytes)
{
    const uintptr_t b0 = (uintptr_t)p, b1 = b0 + bytes;
    for (const Extent& e : g_extents)
        if (b0 < e.a1 && b1 > e.a0 && !(b0 < e.p1 && b1 > e.p0)) ++g_nopayload;
}
void emu_fail(const char* fmt, ...)
{
    va_list ap; va_start(ap, fmt); fputs("emulator: ", stderr); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr);
    abort();
}
void v3d_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); }

// The switch between two fibers.  On x86-64 it is the System V callee-saved registers and the stack pointer: swapcontext() costs
// a system call per switch, and under AddressSanitizer a sweep of the whole stack's shadow, which is most of a small case's time.
#if defined(__x86_64__) && defined(__linux__)
extern "C" void emu_switch(void** save_sp, void* load_sp);
asm(".text\n.globl emu_switch\n.type emu_switch,@function\nemu_switch:\n"
    "  pushq %rbp\n  pushq %rbx\n  pushq %r12\n  pushq %r13\n  pushq %r14\n  pushq %r15\n"
    "  movq %rsp, (%rdi)\n  movq %rsi, %rsp\n"
    "  popq %r15\n  popq %r14\n  popq %r13\n  popq %r12\n  popq %rbx\n  popq %rbp\n  ret\n"
    ".size emu_switch,.-emu_switch\n");
static void fiber_switch(Fiber* from, Fiber* to) { emu_switch(&from->sp, to->sp); }
static void fiber_make(Fiber* f, void (*fn)())
{
    // what emu_switch pops: six registers, then fn as its return address; fn starts as if called (rsp = 16 k + 8) and never returns
    void** sp = reinterpret_cast<void**>((reinterpret_cast<uintptr_t>(f->stack) + f->stack_size) & ~(uintptr_t)15);
    *--sp = nullptr; *--sp = reinterpret_cast<void*>(fn);
    for (int i = 0; i < 6; i++) *--sp = nullptr;
    f->sp = sp;
}
#else
static void fiber_switch(Fiber* from, Fiber* to) { swapcontext(&from->ctx, &to->ctx); }
static void fiber_make(Fiber* f, void (*fn)())
{
    getcontext(&f->ctx); f->ctx.uc_stack.ss_sp = f->stack; f->ctx.uc_stack.ss_size = f->stack_size; f->ctx.uc_link = nullptr;
    makecontext(&f->ctx, fn, 0);
}
#endif

// fiber switches, announced to AddressSanitizer (it tracks the bounds of the stack it runs on)
static void* g_fake_sched; static const void* g_sched_bottom; static size_t g_sched_size;
static void to_fiber(Fiber* f)
{
    g_cur = f;
#if EMU_ASAN
    __sanitizer_start_switch_fiber(&g_fake_sched, f->stack, f->stack_size);
#endif
    fiber_switch(&g_sched, f);
#if EMU_ASAN
    __sanitizer_finish_switch_fiber(g_fake_sched, nullptr, nullptr);
#endif
}
static void to_scheduler(bool leaving)
{
#if EMU_ASAN
    void* fake = nullptr;
    // the frames alive at a fiber's last switch are all that is never unwound: from a little below this one up to the stack's top
    if (leaving) g_cur->stale = max(g_cur->stack, reinterpret_cast<char*>(&fake) - 4096);
    __sanitizer_start_switch_fiber(leaving ? nullptr : &fake, g_sched_bottom, g_sched_size);
#endif
    Fiber* me = g_cur;
    fiber_switch(me, &g_sched);
#if EMU_ASAN
    __sanitizer_finish_switch_fiber(fake, &g_sched_bottom, &g_sched_size);
#endif
}
void fiber_yield() { to_scheduler(false); }
static std::function<void()>* g_body;
static void tramp()
{
#if EMU_ASAN
    __sanitizer_finish_switch_fiber(nullptr, &g_sched_bottom, &g_sched_size);
#endif
    (*g_body)();
    g_cur->done = true; ++g_progress;
    to_scheduler(true);
}

static Fiber g_fibers[EMU_MAX_THREADS];                                    // zero-initialised: no stacks yet; they live as long as the process
static void run_workgroup(dim3 block, size_t lds)
{
    memset(g_bar_count, 0, sizeof g_bar_count); memset(g_bar_phase, 0, sizeof g_bar_phase); memset(g_bar_or, 0, sizeof g_bar_or);
    memset(g_sh_phase, 0, sizeof g_sh_phase); memset(g_sh_count, 0, sizeof g_sh_count);
    // LDS holds garbage at launch: a fresh block of exactly `lds` bytes, so that a sanitizer's red zone starts right behind it
    void* block_lds = nullptr;
    if (lds && posix_memalign(&block_lds, 16, lds)) { fprintf(stderr, "emulator: out of memory\n"); abort(); }
    if (lds) memset(block_lds, g_lds_poison, lds);
    g_lds = (unsigned char*)block_lds;
    const int nt = g_nthreads;
    for (int t = 0; t < nt; ++t) {
        Fiber& f = g_fibers[t]; f.done = false; f.lin = t; f.tid = dim3(t % block.x, t / block.x, 0); 
        if (!f.stack) { f.stack_size = 256 * 1024; f.stack = (char*)malloc(f.stack_size); }     // untouched pages cost nothing
#if EMU_ASAN
        // a fiber that ended never unwound its frames: their red zones are still marked on the stack the next fiber reuses
        if (f.stale) __asan_unpoison_memory_region(f.stale, f.stack + f.stack_size - f.stale);
#endif
        fiber_make(&f, tramp);
    }
    for (bool any = true; any;) {
        any = false;
        const long before = g_progress;
        for (int i = 0; i < nt; ++i) {
            Fiber& f = g_fibers[g_thr_desc ? nt - 1 - i : i];
            if (!f.done) { any = true; to_fiber(&f); }
        }
        if (any && g_progress == before) {
            fprintf(stderr, "emulator: deadlock in workgroup (%u,%u,%u): some threads wait at a rendezvous the others never reach\n", blockIdx.x, blockIdx.y, blockIdx.z);
            abort();
        }
    }
    g_lds = nullptr;
    free(block_lds);
}

void run_grid(dim3 grid, dim3 block, size_t lds, std::function<void()> body)
{
    if (lds > EMU_MAX_LDS || block.x * block.y * block.z > EMU_MAX_THREADS || block.z != 1) {
        fprintf(stderr, "emulator: launch outside a workgroup's range (%zu bytes of LDS, block %u x %u x %u)\n", lds, block.x, block.y, block.z);
        abort();
    }
    g_body = &body; gridDim = grid; blockDim = block; g_nthreads = (int)(block.x * block.y);
    const unsigned long nwg = (unsigned long)grid.x * grid.y * grid.z;
    for (unsigned long i = 0; i < nwg; ++i) {
        const unsigned long w = g_wg_desc ? nwg - 1 - i : i;
        blockIdx = dim3((unsigned)(w % grid.x), (unsigned)(w / grid.x % grid.y), (unsigned)(w / ((unsigned long)grid.x * grid.y)));
        run_workgroup(block, lds);
    }
}
