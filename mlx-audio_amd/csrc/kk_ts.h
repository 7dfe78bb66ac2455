// In-kernel wall-clock marks of the instrumented CSM kernels (kk_csm_debug_timestamps; layout of the 8 words per launch: kk_csm.hip, g_ts).
// `ts` is null in production.  Included inside the anonymous namespace of each file that has such a kernel (kk_csm.hip through
// kk_csm_gemvm.h, kk_attn_cache.hip).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void ts_begin(unsigned long long* ts, int id) {
  if (ts && threadIdx.x == 0) {
    atomicMin(ts + 1, (unsigned long long)wall_clock64());
#ifdef KK_TS_PER_WG  // (tools/gridbar/gemvm_bench.hip: every workgroup's own start / end behind the 8 summary words)
    ts[8 + 2 * (blockIdx.x + 32 * blockIdx.y)] = (unsigned long long)wall_clock64();
#endif
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) {
      ts[0] = (unsigned long long)id;
      ts[4] = (unsigned long long)wall_clock64();
    }
  }
}
__device__ __forceinline__ void ts_mid(unsigned long long* ts) {
  if (ts && threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) ts[3] = (unsigned long long)wall_clock64();
}
__device__ __forceinline__ void ts_mark(unsigned long long* ts, int k) {  // k = 5, 7: further marks of workgroup 0
  if (ts && threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) ts[k] = (unsigned long long)wall_clock64();
}
__device__ __forceinline__ void ts_end(unsigned long long* ts) {
  if (ts && threadIdx.x == 0) {
    atomicMax(ts + 2, (unsigned long long)wall_clock64());
#ifdef KK_TS_PER_WG
    ts[9 + 2 * (blockIdx.x + 32 * blockIdx.y)] = (unsigned long long)wall_clock64();
    ts[8 + 2 * 256 + (blockIdx.x + 32 * blockIdx.y)] = ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32) | (unsigned)__builtin_amdgcn_s_getreg(63492);  // XCC_ID | HW_ID
#endif
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) {
      ts[6] = (unsigned long long)wall_clock64();
    }
  }
}
