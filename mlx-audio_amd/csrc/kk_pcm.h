// PCM wire formats of the audio edges of CSM serving (ABI minor 11): float32, little-endian int16 and the two G.711 companded
// octets, as integer ALU on the device -- no lookup table.  decode: a stored sample -> fp32, exact (a 16-bit linear value over 2^15).
// encode: fp32 -> the stored sample; s = clamp(rint(x 2^15)) with ties to even, +-inf to full scale and NaN to 0, then the G.711 segment
// search on s.  The rules are those of Python's audioop (lin2ulaw, ulaw2lin, lin2alaw, alaw2lin at width 2) on every 16-bit value and every
// octet.  Shared by resample_rows_kernel and pcm_convert_rows_kernel (kk_resample.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// (the values of KK_PCM_* in include/kokoro_hip.h)
#define PCM_F32 0
#define PCM_S16LE 1
#define PCM_MULAW 2
#define PCM_ALAW 3

__host__ __device__ static inline int pcm_bytes(int fmt) { return fmt == PCM_F32 ? 4 : fmt == PCM_S16LE ? 2 : 1; }
__host__ __device__ static inline bool pcm_known(int fmt) { return fmt >= PCM_F32 && fmt <= PCM_ALAW; }

__device__ static inline int pcm_mulaw_to_s16(int u) {
  u = ~u & 0xFF;
  const int t = (((u & 15) << 3) + 0x84) << ((u >> 4) & 7);
  return (u & 0x80) ? 0x84 - t : t - 0x84;
}

__device__ static inline int pcm_alaw_to_s16(int a) {
  a ^= 0x55;
  const int m = a & 15, e = (a >> 4) & 7;
  const int t = e == 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1);
  return (a & 0x80) ? t : -t;
}

__device__ static inline int pcm_s16_to_mulaw(int s) {
  const int v = s >> 2;  // arithmetic: floor
  const bool neg = v < 0;
  const int mag = min(neg ? -v : v, 8159) + 0x21;  // 33 .. 8192
  const int e = (31 - __clz(mag)) - 5;
  const int code = e >= 8 ? 0x7F : (e << 4) | ((mag >> (e + 1)) & 15);
  return code ^ (neg ? 0x7F : 0xFF);
}

__device__ static inline int pcm_s16_to_alaw(int s) {
  const int v = s >> 3;
  const bool pos = v >= 0;
  const int mag = min(pos ? v : -v - 1, 4095);
  const int e = mag < 32 ? 0 : (31 - __clz(mag)) - 4;
  const int m = e == 0 ? (mag >> 1) & 15 : (mag >> e) & 15;
  return (((e << 4) | m) | (pos ? 0x80 : 0)) ^ 0x55;
}

__device__ static inline int pcm_f32_to_s16(float x) {
  if (x != x) return 0;  // fmaxf(NaN, a) is a: the clamp alone would say -32768
  return (int)fminf(fmaxf(rintf(x * 32768.0f), -32768.0f), 32767.0f);
}

__device__ static inline float pcm_s16_to_f32(int s) { return (float)s / 32768.0f; }

// a stored 16-bit or 8-bit sample (zero-extended bits) -> fp32
__device__ static inline float pcm_decode_bits(int fmt, unsigned bits) {
  const int s = fmt == PCM_S16LE ? (int)(int16_t)bits : fmt == PCM_MULAW ? pcm_mulaw_to_s16((int)bits) : pcm_alaw_to_s16((int)bits);
  return pcm_s16_to_f32(s);
}

// sample i of a row of format `fmt`
__device__ static inline float pcm_load(const char* p, int fmt, long long i) {
  if (fmt == PCM_F32) return ((const float*)p)[i];
  if (fmt == PCM_S16LE) return pcm_s16_to_f32(((const int16_t*)p)[i]);
  return pcm_decode_bits(fmt, ((const uint8_t*)p)[i]);
}

// fp32 -> the 16-bit or 8-bit stored sample (not f32)
__device__ static inline unsigned pcm_encode_bits(int fmt, float x) {
  const int s = pcm_f32_to_s16(x);
  return fmt == PCM_S16LE ? (unsigned)s & 0xFFFFu : fmt == PCM_MULAW ? (unsigned)pcm_s16_to_mulaw(s) : (unsigned)pcm_s16_to_alaw(s);
}

__device__ static inline void pcm_store(char* p, int fmt, long long i, float x) {
  if (fmt == PCM_F32) ((float*)p)[i] = x;
  else if (fmt == PCM_S16LE) ((int16_t*)p)[i] = (int16_t)pcm_f32_to_s16(x);
  else ((uint8_t*)p)[i] = (uint8_t)pcm_encode_bits(fmt, x);
}

// the 16 bytes of one load: G = 8 samples of s16le or G = 16 octets of mu-law / A-law, decoded to out[0 .. G)
template <int G>
__device__ static inline void pcm_decode16(int fmt, const uint4 v, float* out) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if constexpr (G == 8) {
      out[2 * k] = pcm_s16_to_f32((int)(int16_t)(w[k] & 0xFFFFu));
      out[2 * k + 1] = pcm_s16_to_f32((int)(int16_t)(w[k] >> 16));
    } else if constexpr (G == 16) {
#pragma unroll
      for (int b = 0; b < 4; ++b) out[4 * k + b] = pcm_decode_bits(fmt, (w[k] >> (8 * b)) & 0xFFu);
    }
  }
}
