// Toy kernels of tests/test_emu_selftest.py: each holds one defect that leaves a GPU's output bits alone, switched on by `bad`
#pragma once
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int toy_lds_overrun(const uint32_t* in, uint32_t* out, int bad, void* stream);
int toy_global_overread(const uint8_t* in, uint32_t* out, int bad, void* stream);
int toy_misaligned_load(const uint8_t* in, uint32_t* out, int bad, void* stream);
int toy_lds_unwritten(const uint32_t* in, uint32_t* out, int bad, void* stream);
int toy_missing_barrier(const uint32_t* in, uint32_t* out, int bad, void* stream);
int toy_workgroup_order(uint32_t* counter, uint32_t* out, int bad, void* stream);
int toy_launch(uint32_t* out, int lds_bytes, int threads, void* stream);
// the cross-lane shims against known answers: in and out hold 256 words (toy_ballot, toy_readlane: out holds two per thread)
int toy_row_shr(const uint32_t* in, uint32_t* out, int n, void* stream);
int toy_row_bcast(const uint32_t* in, uint32_t* out, int which, void* stream);
int toy_wave_scan(const uint32_t* in, uint32_t* out, int bad, void* stream);
int toy_ballot(const uint32_t* in, uint32_t* out, int threads, void* stream);
int toy_readlane(const uint32_t* in, uint32_t* out, int lane, void* stream);
int toy_wave_exit(const uint32_t* in, uint32_t* out, int live_waves, void* stream);
#ifdef __cplusplus
}
#endif
