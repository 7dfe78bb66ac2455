// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), counter-based: shared by the Kokoro noise source
// (kk_source.hip: Box-Muller on top), the CSM sampler's device uniforms (kk_csm.hip) and the Whisper pick's Gumbel noise (kk_whisper_text_kernels.hip).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
  const uint32_t n1 = (uint32_t)p1;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
  const uint32_t n3 = (uint32_t)p0;
  c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}
// counter words (ctr low, ctr high, sub, a fixed tag), key = seed
__device__ __forceinline__ void philox4(uint64_t seed, uint64_t ctr, uint32_t sub, uint32_t (&out)[4]) {
  uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), sub, 0x4B4B5352u};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
}
// 24 random bits -> a float strictly inside (0, 1)
__device__ __forceinline__ float philox_unit(uint32_t r) { return ((float)(r >> 8) + 0.5f) * (1.0f / 16777216.0f); }
// 23 random bits -> a float in [2^-24, 1 - 2^-24]: a 23-bit integer plus a half is exact in fp32, so neither end of the unit interval is ever
// returned (philox_unit's 24-bit integer plus a half rounds to 2^24 for the top values of r and gives exactly 1.0 there).  The Whisper pick's
// Gumbel noise -log(-log u) needs the open interval; philox_unit's users keep their bits.
__device__ __forceinline__ float philox_open(uint32_t r) { return ((float)(r >> 9) + 0.5f) * (1.0f / 8388608.0f); }
