// Device kernels of the SNAC codec and their launch shapes (included by kk_snac.hip alone).  One launch function per kernel, called by the
// codec and by the single-kernel entry points (kk_op_snac_*), so a test cannot pass on a grid, block or LDS size the codec does not use.
// Tensors are frames-major [B][rows][ld]; T is float or bf16_t, arithmetic is fp32.  No result depends on B or on an item's place in the batch:
// a workgroup works on one item and every sum has a fixed order.
#pragma once
#include "kk_common.h"

namespace {

constexpr int SNAC_DW_K = 7;          // taps of every depth-wise conv and of the last conv
constexpr int SNAC_DW_TR = 128;       // output rows per workgroup of the depth-wise conv
constexpr int SNAC_DW_MAX_DIL = 9;    // LDS: (128 + 6 * 9) rows x 64 channels x 4 B = 46.6 KB
constexpr int SNAC_C1_TR = 64;        // output rows per workgroup of the last conv
constexpr int SNAC_C1_MAX_K = 16;
constexpr int SNAC_VQ_MAX_DIM = 64;   // code-book dimension the search kernel keeps in LDS
constexpr int SNAC_MAX_VQ = 8;

// snake(x) = x + sin^2(alpha x) * 1 / (alpha + 1e-9)   (layers.py:124-130); ra = 1 / (alpha + 1e-9)
__device__ __forceinline__ float snac_recip(float alpha) { return 1.0f / (alpha + 1e-9f); }
__device__ __forceinline__ float snac_snake(float x, float alpha, float ra) {
  const float s = sinf(alpha * x);
  return x + ra * (s * s);
}

// ---- depth-wise dilated conv, k = 7, pad = 3 dil, with an optional Snake on either side:
//   out[t][c] = snake_out?(sum_k w[c][k] snake_in?(x[t - 3 dil + k dil][c]) + bias[c]),  rows outside [0, L) are zeros (never loaded).
// A workgroup owns 128 rows x 64 channels: the rows and their halo are staged once in LDS with the input Snake applied (each element once, not
// once per tap), then a lane walks 32 rows of its channel.  Lanes run along channels: global and LDS accesses are unit-stride.
template <typename T>
__global__ __launch_bounds__(256) void snac_dw_conv_kernel(const T* x, long long xbs, int ldx, int L, int C, int dil, const float* w, const float* bias,
                                                           const float* a_in, const float* a_out, T* out, long long obs, int ldo) {
  extern __shared__ float dw_xs[];  // [SNAC_DW_TR + 6 dil][64]
  const int tid = threadIdx.x, cl = tid & 63, rg = tid >> 6;
  const int c = blockIdx.y * 64 + cl, b = blockIdx.z;
  const int t0 = blockIdx.x * SNAC_DW_TR, halo = 3 * dil, nrow = SNAC_DW_TR + 2 * halo;
  const bool cv = c < C;
  float ai = 0.f, rai = 0.f;
  if (a_in && cv) { ai = a_in[c]; rai = snac_recip(ai); }
  const T* xb = x + (long long)b * xbs;
  for (int rr = rg; rr < nrow; rr += 4) {
    const int r = t0 - halo + rr;
    float v = 0.f;
    if (cv && r >= 0 && r < L) {
      v = kk_ld(xb + (long long)r * ldx + c);
      if (a_in) v = snac_snake(v, ai, rai);
    }
    dw_xs[rr * 64 + cl] = v;
  }
  __syncthreads();
  if (!cv) return;
  float wk[SNAC_DW_K];
#pragma unroll
  for (int k = 0; k < SNAC_DW_K; ++k) wk[k] = w[(long long)c * SNAC_DW_K + k];
  const float bs = bias[c];
  float ao = 0.f, rao = 0.f;
  if (a_out) { ao = a_out[c]; rao = snac_recip(ao); }
  T* ob = out + (long long)b * obs;
  for (int i = 0; i < SNAC_DW_TR / 4; ++i) {
    const int rl = rg * (SNAC_DW_TR / 4) + i, t = t0 + rl;
    if (t >= L) break;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < SNAC_DW_K; ++k) acc = __builtin_fmaf(wk[k], dw_xs[(rl + k * dil) * 64 + cl], acc);
    acc += bs;
    if (a_out) acc = snac_snake(acc, ao, rao);
    kk_st(ob + (long long)t * ldo + c, acc);
  }
}

// ---- Snake on its own (before the strided / transposed conv of a block): out[t][c] = snake(x[t][c]); dense items
template <typename T>
__global__ __launch_bounds__(256) void snac_snake_kernel(const T* x, int ldx, int rows, int C, const float* alpha, T* out, int ldo) {
  const int b = blockIdx.z, c = blockIdx.y * 64 + (threadIdx.x & 63);
  if (c >= C) return;
  const float a = alpha[c], ra = snac_recip(a);
  const int r0 = blockIdx.x * 64 + (threadIdx.x >> 6) * 16;
  for (int i = 0; i < 16; ++i) {
    const int r = r0 + i;
    if (r >= rows) break;
    kk_st(out + ((long long)b * rows + r) * ldo + c, snac_snake(kk_ld(x + ((long long)b * rows + r) * ldx + c), a, ra));
  }
}

// ---- NoiseBlock's mix (layers.py:261-267): out[t][c] = x[t][c] + n[b][c] h[t][c]; x, h, out share the pitch; out may be h or x
template <typename T>
__global__ __launch_bounds__(256) void snac_noise_mix_kernel(const T* x, const T* h, const float* n, int rows, int C, int ld, T* out) {
  const int b = blockIdx.z, c = blockIdx.y * 64 + (threadIdx.x & 63);
  if (c >= C) return;
  const float nv = n[(long long)b * C + c];
  const int r0 = blockIdx.x * 64 + (threadIdx.x >> 6) * 16;
  for (int i = 0; i < 16; ++i) {
    const int r = r0 + i;
    if (r >= rows) break;
    const long long e = ((long long)b * rows + r) * ld + c;
    kk_st(out + e, kk_ld(x + e) + nv * kk_ld(h + e));
  }
}

// ---- from_codes (vq.py:109-129) as a gather-sum: out[t][c] = sum_i table_i[codes_i[t / stride_i]][c] + bias_sum[c], quantisers in ascending
// order in fp32, codes clamped into [0, bins)
struct SnacCodes {
  const int* codes[SNAC_MAX_VQ];    // [B][T / stride]
  const float* table[SNAC_MAX_VQ];  // [bins][D]
  int stride[SNAC_MAX_VQ];
  int nq;
};
template <typename T>
__global__ __launch_bounds__(256) void snac_from_codes_kernel(SnacCodes s, int bins, int D, int Tn, const float* bias_sum, T* out, int ldo) {
  const int t = blockIdx.x, b = blockIdx.y;
  for (int c = threadIdx.x; c < D; c += 256) {
    float acc = 0.f;
    for (int i = 0; i < s.nq; ++i) {
      const int Ti = Tn / s.stride[i];
      int id = s.codes[i][(long long)b * Ti + t / s.stride[i]];
      id = id < 0 ? 0 : (id >= bins ? bins - 1 : id);
      const float v = s.table[i][(long long)id * D + c];
      acc = i == 0 ? v : acc + v;
    }
    kk_st(out + ((long long)b * Tn + t) * ldo + c, acc + bias_sum[c]);
  }
}

// ---- the quantiser's average pool (vq.py:26-30: a depth-wise conv with weights 1 / stride): out[tp][c] = sum_j x[tp s + j][c] * (1 / s)
__global__ __launch_bounds__(256) void snac_avg_pool_kernel(const float* x, int Tn, int D, int s, float* out) {
  const int tp = blockIdx.x, b = blockIdx.y, To = Tn / s;
  const float inv = 1.0f / (float)s;
  for (int c = threadIdx.x; c < D; c += 256) {
    float acc = 0.f;
    for (int j = 0; j < s; ++j) acc = __builtin_fmaf(x[((long long)b * Tn + (long long)tp * s + j) * D + c], inv, acc);
    out[((long long)b * To + tp) * D + c] = acc;
  }
}

// ---- code-book search (vq.py:62-77): e = ze / max(|ze|, 1e-12); dist_j = |e|^2 - 2 e . cn_j + |cn_j|^2 in fp32; code = the first index of the
// smallest distance; zq = ze + (cb[code] - ze) with the UNNORMALISED row (vq.py:34-37).  One workgroup per (row, item).
__global__ __launch_bounds__(256) void snac_vq_search_kernel(const float* ze, int ldz, int cd, const float* cb, const float* cbn, const float* c2, int bins,
                                                             int Tn, int* codes, float* zq, int ldq) {
  __shared__ float en[SNAC_VQ_MAX_DIM];
  __shared__ float sv[256];
  __shared__ int si[256];
  __shared__ float e2s;
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const float* z = ze + ((long long)b * Tn + t) * ldz;
  if (tid == 0) {
    float ss = 0.f;
    for (int j = 0; j < cd; ++j) ss = __builtin_fmaf(z[j], z[j], ss);
    const float nrm = fmaxf(sqrtf(ss), 1e-12f);
    float e2 = 0.f;
    for (int j = 0; j < cd; ++j) {
      const float v = z[j] / nrm;
      en[j] = v;
      e2 = __builtin_fmaf(v, v, e2);
    }
    e2s = e2;
  }
  __syncthreads();
  const float e2 = e2s;
  float best = INFINITY;
  int bi = 0x7fffffff;
  for (int j = tid; j < bins; j += 256) {
    const float* cj = cbn + (long long)j * cd;
    float dot = 0.f;
    for (int k = 0; k < cd; ++k) dot = __builtin_fmaf(en[k], cj[k], dot);
    const float d = (e2 - 2.0f * dot) + c2[j];
    if (d < best) { best = d; bi = j; }  // ascending j per thread: its first minimum
  }
  sv[tid] = best; si[tid] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      const float v = sv[tid + s];
      const int i = si[tid + s];
      if (v < sv[tid] || (v == sv[tid] && i < si[tid])) { sv[tid] = v; si[tid] = i; }
    }
    __syncthreads();
  }
  const int idx = si[0] < bins ? si[0] : bins - 1;  // (every distance NaN: no minimum was found; the clamp keeps the row read in range)
  if (tid == 0) codes[(long long)b * Tn + t] = idx;
  for (int k = tid; k < cd; k += 256) {
    const float e = z[k];
    zq[((long long)b * Tn + t) * ldq + k] = e + (cb[(long long)idx * cd + k] - e);
  }
}

// ---- residual update with the repeat-interleave (vq.py:41-52,101-104): out[t][c] = res[t][c] - zo[t / s][c]
__global__ __launch_bounds__(256) void snac_residual_update_kernel(const float* res, const float* zo, int Tn, int D, int s, float* out) {
  const int t = blockIdx.x, b = blockIdx.y, To = Tn / s;
  for (int c = threadIdx.x; c < D; c += 256)
    out[((long long)b * Tn + t) * D + c] = res[((long long)b * Tn + t) * D + c] - zo[((long long)b * To + t / s) * D + c];
}

// ---- the decoder's last conv (layers.py:196-200): Cout = 1, Snake in, tanh out:
//   out[b][t] = tanh?(sum_k sum_c w[k][c] snake?(x[t - pad + k][c]) + bias);  w is the generic pack [K][Cin][ldw] read at column 0.
// A workgroup owns 64 output rows; per 64-channel chunk it stages its 64 + K - 1 rows in LDS with the Snake applied once per element, then
// four lanes per row sum 16 channels each over the taps and meet in a fixed order.
template <typename T>
__global__ __launch_bounds__(256) void snac_conv_cout1_kernel(const T* x, int ld, int L, int Cin, int K, int pad, const float* w, int ldw, const float* bias,
                                                              const float* alpha, int tanh_out, float* out) {
  extern __shared__ float c1_sm[];
  float* xs = c1_sm;                                 // [SNAC_C1_TR + K - 1][65]
  float* ws = c1_sm + (SNAC_C1_TR + K - 1) * 65;      // [K][64]
  const int tid = threadIdx.x, r = tid >> 2, q = tid & 3, cl = tid & 63;
  const int b = blockIdx.y, t0 = blockIdx.x * SNAC_C1_TR, nrow = SNAC_C1_TR + K - 1;
  float acc = 0.f;
  for (int c0 = 0; c0 < Cin; c0 += 64) {
    const int c = c0 + cl;
    float a = 0.f, ra = 0.f;
    if (alpha && c < Cin) { a = alpha[c]; ra = snac_recip(a); }
    __syncthreads();
    for (int rr = tid >> 6; rr < nrow; rr += 4) {
      const int row = t0 - pad + rr;
      float v = 0.f;
      if (c < Cin && row >= 0 && row < L) {
        v = kk_ld(x + ((long long)b * L + row) * ld + c);
        if (alpha) v = snac_snake(v, a, ra);
      }
      xs[rr * 65 + cl] = v;
    }
    for (int k = tid >> 6; k < K; k += 4) ws[k * 64 + cl] = c < Cin ? w[((long long)k * Cin + c) * ldw] : 0.f;
    __syncthreads();
    for (int k = 0; k < K; ++k) {
      const float* xr = xs + (r + k) * 65 + q * 16;
      const float* wk = ws + k * 64 + q * 16;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc = __builtin_fmaf(xr[i], wk[i], acc);
    }
  }
  acc += __shfl_xor(acc, 1);
  acc += __shfl_xor(acc, 2);
  const int t = t0 + r;
  if (q == 0 && t < L) {
    float v = acc + (bias ? bias[0] : 0.f);
    if (tanh_out) v = tanhf(v);
    out[(long long)b * L + t] = v;
  }
}

// ------------------------------------------------------------------------------------------------------------- launch shapes
#define SNAC_BY_DTYPE(dtype, CALL_BF16, CALL_F32) \
  do {                                            \
    if ((dtype) == KK_BF16) { CALL_BF16; }        \
    else { CALL_F32; }                            \
  } while (0)

int snac_launch_dw_conv(const void* x, long long xbs, int ldx, int dtype, int L, int C, int dil, const float* w, const float* bias, const float* a_in,
                        const float* a_out, void* out, long long obs, int ldo, int B, hipStream_t st) {
  const dim3 grid(kk_cdiv(L, SNAC_DW_TR), kk_cdiv(C, 64), B);
  const size_t lds = (size_t)(SNAC_DW_TR + 6 * dil) * 64 * 4;
  SNAC_BY_DTYPE(dtype,
                hipLaunchKernelGGL(snac_dw_conv_kernel<bf16_t>, grid, dim3(256), lds, st, (const bf16_t*)x, xbs, ldx, L, C, dil, w, bias, a_in, a_out, (bf16_t*)out, obs, ldo),
                hipLaunchKernelGGL(snac_dw_conv_kernel<float>, grid, dim3(256), lds, st, (const float*)x, xbs, ldx, L, C, dil, w, bias, a_in, a_out, (float*)out, obs, ldo));
  KK_CHECK_LAUNCH();
  return 0;
}
int snac_launch_snake(const void* x, int ldx, int dtype, int rows, int C, const float* alpha, void* out, int ldo, int B, hipStream_t st) {
  const dim3 grid(kk_cdiv(rows, 64), kk_cdiv(C, 64), B);
  SNAC_BY_DTYPE(dtype, hipLaunchKernelGGL(snac_snake_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)x, ldx, rows, C, alpha, (bf16_t*)out, ldo),
                hipLaunchKernelGGL(snac_snake_kernel<float>, grid, dim3(256), 0, st, (const float*)x, ldx, rows, C, alpha, (float*)out, ldo));
  KK_CHECK_LAUNCH();
  return 0;
}
int snac_launch_noise_mix(const void* x, const void* h, const float* n, int dtype, int rows, int C, int ld, void* out, int B, hipStream_t st) {
  const dim3 grid(kk_cdiv(rows, 64), kk_cdiv(C, 64), B);
  SNAC_BY_DTYPE(dtype, hipLaunchKernelGGL(snac_noise_mix_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)x, (const bf16_t*)h, n, rows, C, ld, (bf16_t*)out),
                hipLaunchKernelGGL(snac_noise_mix_kernel<float>, grid, dim3(256), 0, st, (const float*)x, (const float*)h, n, rows, C, ld, (float*)out));
  KK_CHECK_LAUNCH();
  return 0;
}
int snac_launch_from_codes(const SnacCodes& s, int bins, int D, int Tn, const float* bias_sum, void* out, int ldo, int dtype, int B, hipStream_t st) {
  SNAC_BY_DTYPE(dtype, hipLaunchKernelGGL(snac_from_codes_kernel<bf16_t>, dim3(Tn, B), dim3(256), 0, st, s, bins, D, Tn, bias_sum, (bf16_t*)out, ldo),
                hipLaunchKernelGGL(snac_from_codes_kernel<float>, dim3(Tn, B), dim3(256), 0, st, s, bins, D, Tn, bias_sum, (float*)out, ldo));
  KK_CHECK_LAUNCH();
  return 0;
}
int snac_launch_avg_pool(const float* x, int Tn, int D, int s, float* out, int B, hipStream_t st) {
  hipLaunchKernelGGL(snac_avg_pool_kernel, dim3(Tn / s, B), dim3(256), 0, st, x, Tn, D, s, out);
  KK_CHECK_LAUNCH();
  return 0;
}
int snac_launch_vq_search(const float* ze, int ldz, int cd, const float* cb, const float* cbn, const float* c2, int bins, int Tn, int* codes, float* zq, int ldq,
                          int B, hipStream_t st) {
  hipLaunchKernelGGL(snac_vq_search_kernel, dim3(Tn, B), dim3(256), 0, st, ze, ldz, cd, cb, cbn, c2, bins, Tn, codes, zq, ldq);
  KK_CHECK_LAUNCH();
  return 0;
}
int snac_launch_residual_update(const float* res, const float* zo, int Tn, int D, int s, float* out, int B, hipStream_t st) {
  hipLaunchKernelGGL(snac_residual_update_kernel, dim3(Tn, B), dim3(256), 0, st, res, zo, Tn, D, s, out);
  KK_CHECK_LAUNCH();
  return 0;
}
int snac_launch_conv_cout1(const void* x, int dtype, int ld, int L, int Cin, int K, int pad, const float* w, int ldw, const float* bias, const float* alpha,
                           int tanh_out, float* out, int B, hipStream_t st) {
  const dim3 grid(kk_cdiv(L, SNAC_C1_TR), B);
  const size_t lds = ((size_t)(SNAC_C1_TR + K - 1) * 65 + (size_t)K * 64) * 4;
  SNAC_BY_DTYPE(dtype, hipLaunchKernelGGL(snac_conv_cout1_kernel<bf16_t>, grid, dim3(256), lds, st, (const bf16_t*)x, ld, L, Cin, K, pad, w, ldw, bias, alpha, tanh_out, out),
                hipLaunchKernelGGL(snac_conv_cout1_kernel<float>, grid, dim3(256), lds, st, (const float*)x, ld, L, Cin, K, pad, w, ldw, bias, alpha, tanh_out, out));
  KK_CHECK_LAUNCH();
  return 0;
}
#undef SNAC_BY_DTYPE

}  // namespace
