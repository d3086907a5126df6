// vh_wave_scan.h — inclusive scans over the 64 lanes of a wave without LDS.
//
// A __shfl_up prefix sum is six ds_bpermute_b32 in a dependent chain, each behind its own s_waitcnt lgkmcnt(0) — which also drains whatever
// else the wave has outstanding on that counter — and all of them on the LDS pipe the scans' queues and ring writers live on. The DPP form is
// six VALU instructions with the lane movement built in: row_shr:1, 2, 4, 8 scan every row of 16 lanes (a lane the shift leaves without a
// source reads the identity), row_bcast:15 hands the last lane of rows 0 and 2 to rows 1 and 3, row_bcast:31 the last lane of row 1 to rows
// 2 and 3.
//
// PRECONDITION of every function here: all 64 lanes of the wave are active (the call sits in wave-uniform control flow). DPP reads an inactive
// lane's register as it stands, not as the identity.
//
// -DVH_WAVE_SCAN_SHFL=1 (VH_JIT_FLAGS for the compiled kernels): the __shfl_up loops these functions replaced, and in vj_scan the two scans per
// batch and the binary search that went with them — the in-process A/B switch.
#pragma once
#include <stdint.h>

#ifndef VH_WAVE_SCAN_SHFL
#define VH_WAVE_SCAN_SHFL 0
#endif

#if VH_WAVE_SCAN_SHFL
__device__ __forceinline__ int vh_wave_scan_lane() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ uint32_t vh_wave_incl_add(uint32_t x) {
  const int lane = vh_wave_scan_lane();
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(x, off); if (lane >= off) x += o; }
  return x;
}
__device__ __forceinline__ unsigned long long vh_wave_incl_add(unsigned long long x) {
  const int lane = vh_wave_scan_lane();
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const unsigned long long o = __shfl_up(x, off); if (lane >= off) x += o; }
  return x;
}
__device__ __forceinline__ uint32_t vh_wave_incl_max(uint32_t x) {
  const int lane = vh_wave_scan_lane();
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(x, off); if (lane >= off && o > x) x = o; }
  return x;
}
#else
// x of the lane the control names, 0 where it names none (old = 0, bound_ctrl off, lanes outside ROWS keep old)
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t vh_wave_dpp0(uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROWS, 0xf, false); }
#define VH_WAVE_SCAN_STEPS(STEP) STEP(0x111, 0xf) STEP(0x112, 0xf) STEP(0x114, 0xf) STEP(0x118, 0xf) STEP(0x142, 0xa) STEP(0x143, 0xc)

__device__ __forceinline__ uint32_t vh_wave_incl_add(uint32_t x) {
#define VH_WAVE_STEP(CTRL, ROWS) x += vh_wave_dpp0<CTRL, ROWS>(x);
  VH_WAVE_SCAN_STEPS(VH_WAVE_STEP)
#undef VH_WAVE_STEP
  return x;
}
__device__ __forceinline__ unsigned long long vh_wave_incl_add(unsigned long long x) {
#define VH_WAVE_STEP(CTRL, ROWS) x += (unsigned long long)vh_wave_dpp0<CTRL, ROWS>((uint32_t)x) | (unsigned long long)vh_wave_dpp0<CTRL, ROWS>((uint32_t)(x >> 32)) << 32;
  VH_WAVE_SCAN_STEPS(VH_WAVE_STEP)
#undef VH_WAVE_STEP
  return x;
}
// (identity 0: the maximum of unsigned values)
__device__ __forceinline__ uint32_t vh_wave_incl_max(uint32_t x) {
#define VH_WAVE_STEP(CTRL, ROWS) { const uint32_t o = vh_wave_dpp0<CTRL, ROWS>(x); x = o > x ? o : x; }
  VH_WAVE_SCAN_STEPS(VH_WAVE_STEP)
#undef VH_WAVE_STEP
  return x;
}
#endif
