// Vocos vocoder (mlx_audio/codec/models/vocos/vocos.py): features [B][T][input_channels] -> pcm [B][(T - 1) hop].
//   embed k7 -> norm -> num_layers x ConvNeXtBlock {dwconv k7 groups = dim -> LayerNorm / AdaLayerNorm -> pwconv1 -> GELU -> pwconv2 -> gamma -> + x}
//   -> final_layer_norm -> ISTFTHead {Linear to n_fft + 2 -> exp / clip / cos / sin -> irfft -> Hann -> overlap-add -> / window sum -> centre cut}.
// embed, pwconv1 + GELU, pwconv2 + residual and the head Linear are the library's conv kernels: the generic fp32 kernel (kk_conv.hip) or, for
// compute_dtype bf16, the matrix-core kernel of kk_conv_mfma.hip with an fp32 result where the residual stream or the head needs one.
// What exists only here: dwconv -> LayerNorm as ONE kernel, and the iSTFT head on an FFT.
//
// ---- vc_dwconv_ln_kernel:  out[b][t][c] = LN_c(bias[c] + sum_{k < 7} w[c][k] x[b][t - 3 + k][c]) A[b?][c] + S[b?][c],  rows outside [0, T) zero.
// A workgroup (4 waves) owns R time rows and all C channels.  It stages rows t0 - 3 .. t0 + R + 2 of x in LDS at pitch C (zeros outside [0, T)): x comes
// from HBM once, the halo rows of the neighbours from L2.  A wave takes rows wave, wave + 4, ...; lane l owns channels l, l + 64, ... (NJ = ceil(C / 64) of
// them, a template parameter), so an LDS row read is 64 consecutive floats (no bank conflict) and the seven taps + bias of the lane's channels sit in
// 8 NJ registers for all of the wave's rows.  The NJ conv values of a row stay in registers: sum -> xor-butterfly over the 64 lanes (DPP / permute, no LDS)
// -> mean -> centred squares -> the same butterfly -> rstd -> affine -> one store.  Every value is one fixed fmaf chain (bias first, taps in order; a zero
// row adds exactly nothing) and the butterfly's order is fixed, so a row's bits depend on its seven input rows only: not on B, the item's place or R.
// Without `w` the kernel is the LayerNorm alone (fp32 in, fp32 or bf16 out): the backbone's first and last norm.
//
// ---- vc_istft_kernel: a workgroup makes G consecutive output hops of one item from the G + 3 frames that touch them.  irfft of N points as a complex
// transform of M = N / 2:  Z[k] = (X[k] + conj X[M - k]) + i W^k (X[k] - conj X[M - k]),  W = exp(2 pi i / N),  z = IDFT_M(Z),  frame[2 n] = Re z[n],
// frame[2 n + 1] = Im z[n].  X[k] = min(exp(h[k]), 100) / N (cos p, sin p) is formed while h is loaded (lane k loads bins k and M - k and writes Z[k] and
// Z[M - k]; the imaginary parts of bins 0 and M are dropped as numpy.fft.irfft drops them).  The transform is a Stockham autosort FFT between two LDS
// buffers of M complex per frame: radix-4 passes while the remaining length divides by 4, then one radix-2 pass, then one radix-5 pass (N = 5 2^a), so the
// stride is always a power of two and the last pass has no twiddles.  Pass plans (M: radices):  128: 4 4 4 2;  256: 4 4 4 4;  512: 4 4 4 4 2;
// 1024: 4 4 4 4 4;  160: 4 4 2 5;  320: 4 4 4 5;  640: 4 4 4 2 5.  A wave owns whole frames (frame i of the group goes to wave i % 4), so a pass is
// 64 lanes over M / radix butterflies.  Twiddles exp(2 pi i t / M), W^k and the symmetric Hann window come from one fp32 table per N, made in float64 on the
// host and kept on the device.  Output sample (hop j, n) = sum over frames j - 1 .. j + 2 (those inside [0, T), in that order) of frame[(2 + j - f) H + n]
// w[..], times the reciprocal of the same sum of w: stored once, no atomics, no [T][N] tensor in HBM.  A frame's bits do not depend on the group it is
// transformed in, so a sample's bits do not depend on G, B or the item's place.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/kokoro_hip.h"
#include "kk_common.h"
#include "kk_kernels.h"
#include "kk_host.h"

namespace {

constexpr int VC_MAX_C = 1024;        // 16 channels per lane
constexpr int VC_LDS_BYTES = 160 * 1024;

// ------------------------------------------------------------------------------------------------------------- dwconv -> LayerNorm
__device__ __forceinline__ float vc_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <int NJ, typename TO, bool CONV>
__global__ __launch_bounds__(256) void vc_dwconv_ln_kernel(const float* x, long long xbs, int ldx, int T, int C, int R, int vec4, const float* w,
                                                           const float* bias, const float* A, const float* S, long long abs_, float eps, TO* out,
                                                           long long obs, int ldo) {
  extern __shared__ __attribute__((aligned(16))) float vc_sm[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.y, t0 = blockIdx.x * R;
  const int nrows = T - t0 < R ? T - t0 : R;
  const float* xb = x + (long long)b * xbs;
  float wr[CONV ? NJ : 1][7], bj[CONV ? NJ : 1];
  if constexpr (CONV) {
    const int nst = nrows + 6;  // staged row rr is time row t0 - 3 + rr
    if (vec4) {
      const int C4 = C >> 2;
      for (int rr = wave; rr < nst; rr += 4) {
        const int t = t0 - 3 + rr;
        const bool in = t >= 0 && t < T;
        for (int c4 = lane; c4 < C4; c4 += 64)
          *(float4*)&vc_sm[rr * C + 4 * c4] = in ? *(const float4*)(xb + (long long)t * ldx + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    } else {
      for (int rr = wave; rr < nst; rr += 4) {
        const int t = t0 - 3 + rr;
        const bool in = t >= 0 && t < T;
        for (int c = lane; c < C; c += 64) vc_sm[rr * C + c] = in ? xb[(long long)t * ldx + c] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + 64 * j;
      bj[j] = c < C ? bias[c] : 0.f;
#pragma unroll
      for (int k = 0; k < 7; ++k) wr[j][k] = c < C ? w[c * 7 + k] : 0.f;
    }
    __syncthreads();
  }
  const float* Ab = A ? A + (long long)b * abs_ : nullptr;
  const float* Sb = S ? S + (long long)b * abs_ : nullptr;
  const float invC = 1.0f / (float)C;
  for (int r = wave; r < nrows; r += 4) {
    float v[NJ];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + 64 * j;
      float acc = 0.f;
      if (c < C) {
        if constexpr (CONV) {
          acc = bj[j];
#pragma unroll
          for (int k = 0; k < 7; ++k) acc = __builtin_fmaf(wr[j][k], vc_sm[(r + k) * C + c], acc);
        } else {
          acc = xb[(long long)(t0 + r) * ldx + c];
        }
      }
      v[j] = acc;
      s += acc;
    }
    const float mean = vc_wave_sum(s) * invC;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      v[j] = lane + 64 * j < C ? v[j] - mean : 0.f;
      q = __builtin_fmaf(v[j], v[j], q);
    }
    const float rstd = 1.0f / sqrtf(vc_wave_sum(q) * invC + eps);
    TO* orow = out + (long long)b * obs + (long long)(t0 + r) * ldo;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + 64 * j;
      if (c < C) {
        float o = v[j] * rstd;
        if (Ab) o *= Ab[c];
        if (Sb) o += Sb[c];
        kk_st(orow + c, o);
      }
    }
  }
}

// rows per workgroup chosen by shape: at most 16, fewer where two workgroups' stages ((R + 6) C floats each) would not share a CU's LDS
int vc_auto_rows(int C) {
  const int fit = VC_LDS_BYTES / 2 / (4 * C) - 6;
  return std::max(4, std::min(16, fit & ~3));
}

template <int NJ, typename TO, bool CONV>
int vc_go_dwconv(const float* x, long long xbs, int ldx, int T, int C, int R, const float* w, const float* bias, const float* A, const float* S, long long abs_,
                 float eps, void* out, long long obs, int ldo, int B, hipStream_t st) {
  const size_t lds = CONV ? (size_t)(R + 6) * C * 4 : 0;
  static KKDevOnce once;  // more LDS than a kernel gets unasked; the limit is per device
  if (CONV && lds > 65536 && once.first()) {
    if (hipFuncSetAttribute((const void*)vc_dwconv_ln_kernel<NJ, TO, CONV>, hipFuncAttributeMaxDynamicSharedMemorySize, VC_LDS_BYTES) != hipSuccess)
      return kk_fail("kk_op_vocos_dwconv_ln: the kernel's LDS request was refused");
    once.done();
  }
  const int vec4 = C % 4 == 0 && ldx % 4 == 0 && xbs % 4 == 0 && ((uintptr_t)x & 15) == 0;
  hipLaunchKernelGGL((vc_dwconv_ln_kernel<NJ, TO, CONV>), dim3(kk_cdiv(T, R), B), dim3(256), lds, st, x, xbs, ldx, T, C, R, vec4, w, bias, A, S, abs_, eps,
                     (TO*)out, obs, ldo);
  KK_CHECK_LAUNCH();
  return 0;
}

// w null: the LayerNorm alone.  A / S: [C] (abs_ 0) or per item at stride abs_; either may be null (1 / 0).  rows 0 = chosen by shape.
int vc_launch_dwconv_ln(const float* x, long long xbs, int ldx, int T, int C, const float* w, const float* bias, const float* A, const float* S, long long abs_,
                        float eps, void* out, long long obs, int ldo, int out_dtype, int rows, int B, hipStream_t st) {
  const char* who = "kk_op_vocos_dwconv_ln";
  if (C < 1 || C > VC_MAX_C) return kk_failf("%s: C must be 1 .. %d, got %d", who, VC_MAX_C, C);
  const int R = rows > 0 ? rows : vc_auto_rows(C);
  if (w && (size_t)(R + 6) * C * 4 > (size_t)VC_LDS_BYTES) return kk_failf("%s: %d rows of %d channels (+ 6 halo rows) do not fit the 160 KB of LDS", who, R, C);
  const int nj = kk_cdiv(C, 64);
#define VC_GO(NJ)                                                                                                                                    \
  do {                                                                                                                                               \
    if (w) {                                                                                                                                         \
      if (out_dtype == KK_BF16) return vc_go_dwconv<NJ, bf16_t, true>(x, xbs, ldx, T, C, R, w, bias, A, S, abs_, eps, out, obs, ldo, B, st);         \
      return vc_go_dwconv<NJ, float, true>(x, xbs, ldx, T, C, R, w, bias, A, S, abs_, eps, out, obs, ldo, B, st);                                    \
    }                                                                                                                                                \
    if (out_dtype == KK_BF16) return vc_go_dwconv<NJ, bf16_t, false>(x, xbs, ldx, T, C, R, w, bias, A, S, abs_, eps, out, obs, ldo, B, st);          \
    return vc_go_dwconv<NJ, float, false>(x, xbs, ldx, T, C, R, w, bias, A, S, abs_, eps, out, obs, ldo, B, st);                                     \
  } while (0)
  if (nj <= 1) VC_GO(1);
  if (nj <= 2) VC_GO(2);
  if (nj <= 3) VC_GO(3);
  if (nj <= 4) VC_GO(4);
  if (nj <= 6) VC_GO(6);
  if (nj <= 8) VC_GO(8);
  if (nj <= 12) VC_GO(12);
  VC_GO(16);
#undef VC_GO
}

// ------------------------------------------------------------------------------------------------------------- iSTFT head
// table of one N (floats): twiddles exp(2 pi i t / M) [M][2], W^k = exp(2 pi i k / N) [M][2], window [N]
struct VcFftPlan {
  int N, M, npass, radix[6];
};

__device__ __forceinline__ float2 vc_cmul(float2 a, float2 b) {
  return make_float2(__builtin_fmaf(a.x, b.x, -(a.y * b.y)), __builtin_fmaf(a.x, b.y, a.y * b.x));
}

// one Stockham pass of radix RX over one frame: length n = RX m at stride s (a power of two, log2 ls);  a_j = src[q + s (p + j m)],
// dst[q + s (RX p + k)] = tw[p k s] sum_j a_j omega^(j k),  omega = exp(+2 pi i / RX)
template <int RX>
__device__ __forceinline__ void vc_pass(const float2* src, float2* dst, int m, int ls, int cnt, const float2* tw, int lane) {
  const int s = 1 << ls;
  for (int u = lane; u < cnt; u += 64) {
    const int p = u >> ls, q = u & (s - 1);
    float2 a[RX], o[RX];
#pragma unroll
    for (int j = 0; j < RX; ++j) a[j] = src[q + s * (p + j * m)];
    if constexpr (RX == 2) {
      o[0] = make_float2(a[0].x + a[1].x, a[0].y + a[1].y);
      o[1] = make_float2(a[0].x - a[1].x, a[0].y - a[1].y);
    } else if constexpr (RX == 4) {
      const float2 s02 = make_float2(a[0].x + a[2].x, a[0].y + a[2].y), d02 = make_float2(a[0].x - a[2].x, a[0].y - a[2].y);
      const float2 s13 = make_float2(a[1].x + a[3].x, a[1].y + a[3].y), d13 = make_float2(a[1].x - a[3].x, a[1].y - a[3].y);
      o[0] = make_float2(s02.x + s13.x, s02.y + s13.y);
      o[1] = make_float2(d02.x - d13.y, d02.y + d13.x);  // d02 + i d13
      o[2] = make_float2(s02.x - s13.x, s02.y - s13.y);
      o[3] = make_float2(d02.x + d13.y, d02.y - d13.x);  // d02 - i d13
    } else {
      // radix 5: c1 = cos(2 pi / 5), c2 = cos(4 pi / 5), s1 = sin(2 pi / 5), s2 = sin(4 pi / 5)
      const float c1 = 0.30901699437494742f, c2 = -0.80901699437494742f, s1 = 0.95105651629515357f, s2 = 0.58778525229247313f;
      const float2 p14 = make_float2(a[1].x + a[4].x, a[1].y + a[4].y), m14 = make_float2(a[1].x - a[4].x, a[1].y - a[4].y);
      const float2 p23 = make_float2(a[2].x + a[3].x, a[2].y + a[3].y), m23 = make_float2(a[2].x - a[3].x, a[2].y - a[3].y);
      o[0] = make_float2(a[0].x + (p14.x + p23.x), a[0].y + (p14.y + p23.y));
      const float2 r1 = make_float2(a[0].x + (c1 * p14.x + c2 * p23.x), a[0].y + (c1 * p14.y + c2 * p23.y));
      const float2 r2 = make_float2(a[0].x + (c2 * p14.x + c1 * p23.x), a[0].y + (c2 * p14.y + c1 * p23.y));
      const float2 i1 = make_float2(s1 * m14.x + s2 * m23.x, s1 * m14.y + s2 * m23.y);  // times i below
      const float2 i2 = make_float2(s2 * m14.x - s1 * m23.x, s2 * m14.y - s1 * m23.y);
      o[1] = make_float2(r1.x - i1.y, r1.y + i1.x);
      o[4] = make_float2(r1.x + i1.y, r1.y - i1.x);
      o[2] = make_float2(r2.x - i2.y, r2.y + i2.x);
      o[3] = make_float2(r2.x + i2.y, r2.y - i2.x);
    }
    float2* d = dst + q + s * RX * p;
    d[0] = o[0];
#pragma unroll
    for (int k = 1; k < RX; ++k) d[s * k] = m > 1 ? vc_cmul(o[k], tw[(p * k) << ls]) : o[k];
  }
}

__global__ __launch_bounds__(256) void vc_istft_kernel(const float* h, long long hbs, int ldh, int T, VcFftPlan pl, int G, const float* tab, float* out, long long obs) {
  extern __shared__ __attribute__((aligned(16))) float vc_sm[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.y;
  const int N = pl.N, M = pl.M, H = N >> 2, F = M + 1, nfr = G + 3;
  const int j0 = blockIdx.x * G, Gc = T - 1 - j0 < G ? T - 1 - j0 : G;  // output hops j0 .. j0 + Gc - 1; slot i holds frame j0 - 1 + i
  const float2* tw = (const float2*)tab;
  const float2* wk = tw + M;
  const float* win = tab + 4 * M;
  float2* buf0 = (float2*)vc_sm;        // [nfr][M]
  float2* buf1 = buf0 + (size_t)nfr * M;  // [nfr][M]
  const float invN = 1.0f / (float)N;
  const bool odd = pl.npass & 1;  // the last pass lands in buf0: an odd plan starts in buf1
  for (int i = wave; i < nfr; i += 4) {
    const int f = j0 - 1 + i;
    if (f < 0 || f > T - 1 || i > Gc + 2) continue;
    const float* hf = h + (long long)b * hbs + (long long)f * ldh;
    float2* z = (odd ? buf1 : buf0) + (size_t)i * M;
    for (int k = lane; k <= M / 2; k += 64) {
      const int km = M - k;
      float sa, ca, sb, cb;
      sincosf(hf[F + k], &sa, &ca);
      sincosf(hf[F + km], &sb, &cb);
      const float ma = fminf(expf(hf[k]), 100.0f) * invN, mb = fminf(expf(hf[km]), 100.0f) * invN;
      float2 xa = make_float2(ma * ca, ma * sa), xb = make_float2(mb * cb, mb * sb);
      if (k == 0) { xa.y = 0.f; xb.y = 0.f; }
      // Z[k] = (xa + conj xb) + i W^k (xa - conj xb);  Z[M - k] = (xb + conj xa) + i W^(M - k) (xb - conj xa)
      const float2 ea = make_float2(xa.x + xb.x, xa.y - xb.y), da = make_float2(xa.x - xb.x, xa.y + xb.y);
      const float2 oa = vc_cmul(da, wk[k]);
      z[k] = make_float2(ea.x - oa.y, ea.y + oa.x);
      if (k != 0 && km != k) {
        const float2 eb = make_float2(ea.x, -ea.y), db = make_float2(-da.x, da.y);
        const float2 ob = vc_cmul(db, wk[km]);
        z[km] = make_float2(eb.x - ob.y, eb.y + ob.x);
      }
    }
  }
  __syncthreads();
  int n = M, ls = 0;
  bool in1 = odd;
  for (int ps = 0; ps < pl.npass; ++ps) {
    const int rx = pl.radix[ps], m = n / rx;
    for (int i = wave; i < nfr; i += 4) {
      const int f = j0 - 1 + i;
      if (f < 0 || f > T - 1 || i > Gc + 2) continue;
      const float2* src = (in1 ? buf1 : buf0) + (size_t)i * M;
      float2* dst = (in1 ? buf0 : buf1) + (size_t)i * M;
      if (rx == 4) vc_pass<4>(src, dst, m, ls, M / 4, tw, lane);
      else if (rx == 2) vc_pass<2>(src, dst, m, ls, M / 2, tw, lane);
      else vc_pass<5>(src, dst, m, ls, M / 5, tw, lane);
    }
    __syncthreads();
    in1 = !in1;
    n = m;
    ls += rx == 4 ? 2 : 1;  // (the radix-5 pass is the last one: its stride is not used afterwards)
  }
  const float* fr = (const float*)buf0;  // [nfr][N]: frame[2 n] = Re z[n], frame[2 n + 1] = Im z[n]
  float* ob = out + (long long)b * obs + (long long)j0 * H;
  for (int jl = 0; jl < Gc; ++jl) {
    for (int nn = tid; nn < H; nn += 256) {
      float acc = 0.f, ws = 0.f;
#pragma unroll
      for (int d = -1; d <= 2; ++d) {
        const int f = j0 + jl + d;
        if (f < 0 || f > T - 1) continue;
        const int mm = (2 - d) * H + nn;
        const float wv = win[mm];
        acc = __builtin_fmaf(fr[(size_t)(jl + d + 1) * N + mm], wv, acc);
        ws += wv;
      }
      ob[jl * H + nn] = ws != 0.f ? acc * (1.0f / ws) : acc;
    }
  }
}

bool vc_plan(int N, int hop, VcFftPlan* pl) {
  if (N < 256 || N > 2048 || hop * 4 != N) return false;
  int r = N;
  while (r % 2 == 0) r /= 2;
  if (r != 1 && r != 5) return false;
  VcFftPlan p;
  memset(&p, 0, sizeof p);
  p.N = N; p.M = N / 2;
  int n = p.M;
  while (n % 4 == 0) { p.radix[p.npass++] = 4; n /= 4; }
  if (n % 2 == 0) { p.radix[p.npass++] = 2; n /= 2; }
  if (n == 5) { p.radix[p.npass++] = 5; n = 1; }
  if (n != 1) return false;
  if (pl) *pl = p;
  return true;
}

// the table of one N on the current device (float64 on the host, rounded once), made at first use and kept
int vc_table(int N, const float** out) {
  static std::mutex mu;
  static std::map<std::pair<int, int>, float*> cache;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find({dev, N});
  if (it == cache.end()) {
    const int M = N / 2;
    std::vector<float> t((size_t)4 * M + N);
    for (int i = 0; i < M; ++i) {
      t[2 * i] = (float)cos(2.0 * M_PI * i / M); t[2 * i + 1] = (float)sin(2.0 * M_PI * i / M);
      t[2 * M + 2 * i] = (float)cos(2.0 * M_PI * i / N); t[2 * M + 2 * i + 1] = (float)sin(2.0 * M_PI * i / N);
    }
    for (int i = 0; i < N; ++i) t[4 * M + i] = (float)(0.5 * (1.0 - cos(2.0 * M_PI * i / (N - 1))));  // utils.hanning(N): symmetric
    float* d = nullptr;
    if (hipMalloc((void**)&d, t.size() * 4) != hipSuccess) return kk_fail("kk_op_vocos_istft: hipMalloc failed");
    if (hipMemcpy(d, t.data(), t.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {  // (blocking: the table is there before any launch)
      (void)hipFree(d);
      return kk_fail("kk_op_vocos_istft: table upload failed");
    }
    it = cache.emplace(std::make_pair(dev, N), d).first;
  }
  *out = it->second;
  return 0;
}

const char* vc_istft_refusal(int n_fft, int hop, int T) {
  if (!vc_plan(n_fft, hop, nullptr)) return "n_fft must be 2^a or 5 2^a with 256 <= n_fft <= 2048, and hop_length n_fft / 4";
  if (T < 2 || T > (1 << 22)) return "T must be 2 .. 2^22 frames (T - 1 hops of output)";
  return nullptr;
}

int vc_launch_istft(const float* h, long long hbs, int ldh, int T, int n_fft, int hop, float* out, long long obs, int group, int B, hipStream_t st) {
  const char* who = "kk_op_vocos_istft";
  VcFftPlan pl;
  if (const char* why = vc_istft_refusal(n_fft, hop, T)) return kk_failf("%s: %s", who, why);
  vc_plan(n_fft, hop, &pl);
  const int G = std::min(group > 0 ? group : 5, T - 1);  // 0: 5 hops = 8 frames, two per wave
  const size_t lds = (size_t)(G + 3) * n_fft * 8;
  if (lds > (size_t)VC_LDS_BYTES) return kk_failf("%s: a group of %d hops (%d frames of %d points, twice) does not fit the 160 KB of LDS", who, G, G + 3, n_fft);
  const float* tab = nullptr;
  KK_TRY(vc_table(n_fft, &tab));
  static KKDevOnce once;
  if (lds > 65536 && once.first()) {
    if (hipFuncSetAttribute((const void*)vc_istft_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, VC_LDS_BYTES) != hipSuccess)
      return kk_failf("%s: the kernel's LDS request was refused", who);
    once.done();
  }
  hipLaunchKernelGGL(vc_istft_kernel, dim3(kk_cdiv(T - 1, G), B), dim3(256), lds, st, h, hbs, ldh, T, pl, G, tab, out, obs);
  KK_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------- the model
struct VcLin {  // a conv / Linear [O][K][I]: the generic kernel's pack [K][I][ldw] fp32, and for bf16 [K][CoutP][CinP] where the matrix-core kernel takes it
  size_t w_off = 0, b_off = 0, wb_off = 0;
  int Cin = 0, Cout = 0, K = 1, ldw = 0, CinP = 0, CoutP = 0, CoutW = 0;  // CoutW: columns the matrix-core kernel writes (Cout rounded up to 8)
  bool mfma = false;
  const float* w = nullptr;
  const float* b = nullptr;
  const bf16_t* wb = nullptr;
};
struct VcNorm {  // LayerNorm weight / bias (absent for AdaLayerNorm and a bias-free final norm)
  ArenaVec w, b;
};
struct VcBlock {
  ArenaVec dw_w, dw_b;  // [C][7], [C]
  VcNorm norm;
  VcLin pw1, pw2;
};
struct Buf {
  void* p = nullptr;
  int rows = 0, C = 0, ld = 0, dtype = KK_F32;
  long long bs() const { return (long long)rows * ld; }
};

}  // namespace

struct kk_vocos {
  kk_vocos_config cfg;
  WeightArena arena;
  bool finalized = false;
  int adt = KK_F32;
  VcLin embed, head;
  VcNorm norm, final_norm;
  std::vector<VcBlock> blocks;
  DebugNotes dbg;
  std::mutex dbg_mu;
};

namespace {

// at(o, k, i) and bias(o) in float64 -> the packs
template <typename At, typename Bi>
VcLin vc_pack(WeightArena& a, int O, int K, int I, bool bf, bool pad_cols, At at, Bi bias) {
  VcLin c;
  c.Cin = I; c.Cout = O; c.K = K; c.ldw = rup(O, 64);
  c.w_off = a.alloc((size_t)K * I * c.ldw);
  for (int o = 0; o < O; ++o)
    for (int k = 0; k < K; ++k)
      for (int i = 0; i < I; ++i) a.pack[c.w_off + ((size_t)k * I + i) * c.ldw + o] = (float)at(o, k, i);
  c.CoutW = rup(O, 8);
  c.mfma = bf && (pad_cols || O % 8 == 0) && kk_mfma_eligible(I, c.CoutW, K, KK_CONV, 1, 1);
  c.CinP = rup(I, 64); c.CoutP = rup(O, 128);
  if (c.mfma) {
    c.wb_off = a.alloc(((size_t)K * c.CoutP * c.CinP + 1) / 2);
    uint16_t* d = (uint16_t*)&a.pack[c.wb_off];
    for (int o = 0; o < O; ++o)
      for (int k = 0; k < K; ++k)
        for (int i = 0; i < I; ++i) d[((size_t)k * c.CoutP + o) * c.CinP + i] = f32_to_bf16_rne((float)at(o, k, i));
  }
  c.b_off = a.alloc(c.CoutP);
  for (int o = 0; o < O; ++o) a.pack[c.b_off + o] = (float)bias(o);
  return c;
}
void vc_resolve(const WeightArena& a, VcLin& c) {
  c.w = a.dev + c.w_off; c.b = a.dev + c.b_off;
  c.wb = c.mfma ? (const bf16_t*)(a.dev + c.wb_off) : nullptr;
}

// out = act(conv(x) + bias) (+ res), rows dense
int vc_conv(hipStream_t st, int B, const VcLin& l, const Buf& x, const Buf& out, int act, const Buf* res) {
  const int pad = (l.K - 1) / 2, rows = out.rows;
  if (l.mfma && x.dtype == KK_BF16 && x.ld >= l.CinP && out.ld % 8 == 0 && out.ld >= l.CoutW && (!res || res->ld % 8 == 0)) {
    KKMfmaArgs g;
    memset(&g, 0, sizeof g);
    g.x = (const bf16_t*)x.p; g.xbs = x.bs(); g.ldx = x.ld; g.w = l.wb; g.CinP = l.CinP; g.CoutP = l.CoutP; g.Cin = l.Cin; g.bias = l.b;
    g.out = out.p; g.obs = out.bs(); g.ldo = out.ld;
    if (res) { g.res = res->p; g.rbs = res->bs(); g.ldr = res->ld; }
    g.Cout = l.CoutW; g.Kw = l.K; g.mode = KK_CONV; g.stride = 1; g.pad = pad; g.dil = 1; g.Q = rows; g.Lo_rows = rows;
    g.lin = KKLen{nullptr, 0, x.rows}; g.lout = KKLen{nullptr, 0, rows};
    g.in_slope = 1.0f; g.scale = 1.0f; g.act = act;
    return kk_launch_conv_mfma(g, B, out.dtype, st);
  }
  KKConvArgs a;
  memset(&a, 0, sizeof a);
  a.x = x.p; a.xbs = x.bs(); a.ldx = x.ld; a.w = l.w; a.ldw = l.ldw; a.bias = l.b;
  a.out = out.p; a.obs = out.bs(); a.ldo = out.ld;
  if (res) { a.res = res->p; a.rbs = res->bs(); a.ldr = res->ld; }
  a.Cin = l.Cin; a.Cout = l.Cout; a.Kw = l.K; a.mode = KK_CONV; a.stride = 1; a.pad = pad; a.dil = 1; a.Q = rows; a.Lo_rows = rows;
  a.lin = KKLen{nullptr, 0, x.rows}; a.lout = KKLen{nullptr, 0, rows};
  a.in_slope = 1.0f; a.scale = 1.0f; a.act = act;
  return kk_launch_conv_generic(a, B, x.dtype, out.dtype, st);
}

struct Run : Workspace {
  kk_vocos* m;
  hipStream_t st;
  int B;
  Run(kk_vocos* m_, hipStream_t st_, int B_, void* ws, size_t ws_bytes) : m(m_), st(st_), B(B_) {
    base = (char*)ws; cap = ws_bytes; dry = ws == nullptr;
  }
  Buf buf(int rows, int C, int ld, int dtype) {
    Buf t;
    t.rows = rows; t.C = C; t.ld = ld; t.dtype = dtype;
    t.p = raw((size_t)B * rows * ld * (dtype == KK_BF16 ? 2 : 4));
    return t;
  }
  void note(const std::string& name, const Buf& t) {
    std::lock_guard<std::mutex> lk(m->dbg_mu);
    m->dbg.map[name] = DebugNote{t.p, t.ld, t.bs(), t.rows, t.C, t.dtype, B};
  }
  // norm index n of [n_norms][B][2][C]: the AdaLayerNorm pair of every item, or the LayerNorm's own parameters
  int ln(const Buf& x, const ArenaVec* dw_w, const ArenaVec* dw_b, const VcNorm& nm, const float* cond, int n, const Buf& out) {
    const int C = x.C;
    const float* A = cond ? cond + (long long)n * B * 2 * C : nm.w.p;
    const float* S = cond ? A + C : nm.b.p;
    return vc_launch_dwconv_ln((const float*)x.p, x.bs(), x.ld, x.rows, C, dw_w ? dw_w->p : nullptr, dw_b ? dw_b->p : nullptr, A, S, cond ? 2ll * C : 0, 1e-6f,
                               out.p, out.bs(), out.ld, out.dtype, 0, B, st);
  }
};

// Vocos.decode (vocos.py:351-354): VocosBackbone.__call__ (:241-260), ISTFTHead.__call__ (:126-140)
int run_forward(Run& r, int T, const float* feat, const float* cond, float* pcm) {
  kk_vocos* m = r.m;
  const kk_vocos_config& c = m->cfg;
  const int B = r.B, D = c.dim, I = c.intermediate_dim, dt = m->adt, NF = c.n_fft + 2;
  const bool bf = dt == KK_BF16;
  const int ldD = bf ? rup(D, 64) : D, ldI = bf ? rup(I, 64) : I;
  Buf xin = bf ? r.buf(T, c.input_channels, rup(c.input_channels, 64), KK_BF16) : Buf();
  Buf e = r.buf(T, D, D, KK_F32);
  std::vector<Buf> xs(c.num_layers + 1);  // the fp32 residual stream: after norm, after every block
  for (Buf& x : xs) x = r.buf(T, D, D, KK_F32);
  Buf a = r.buf(T, D, ldD, dt), hh = r.buf(T, I, ldI, dt), bb = r.buf(T, D, ldD, dt), hd = r.buf(T, NF, rup(NF, 8), KK_F32);
  if (r.oom) return kk_fail("kk_vocos_forward: workspace too small");
  if (r.dry) return 0;
  if (bf) {
    KK_TRY(kk_launch_convert(feat, KK_F32, (long long)T * c.input_channels, c.input_channels, xin.p, KK_BF16, xin.bs(), xin.ld, c.input_channels, T, B, r.st));
  } else {
    xin.p = const_cast<float*>(feat); xin.rows = T; xin.C = xin.ld = c.input_channels; xin.dtype = KK_F32;
  }
  const bool ada = c.adanorm_num_embeddings > 0;
  KK_TRY(vc_conv(r.st, B, m->embed, xin, e, KK_ACT_NONE, nullptr));
  r.note("embed", e);
  KK_TRY(r.ln(e, nullptr, nullptr, m->norm, ada ? cond : nullptr, 0, xs[0]));
  static const char* names[16] = {"block0", "block1", "block2",  "block3",  "block4",  "block5",  "block6",  "block7",
                                  "block8", "block9", "block10", "block11", "block12", "block13", "block14", "block15"};
  for (int i = 0; i < c.num_layers; ++i) {
    const VcBlock& k = m->blocks[i];
    KK_TRY(r.ln(xs[i], &k.dw_w, &k.dw_b, k.norm, ada ? cond : nullptr, i + 1, a));
    KK_TRY(vc_conv(r.st, B, k.pw1, a, hh, KK_ACT_GELU, nullptr));
    KK_TRY(vc_conv(r.st, B, k.pw2, hh, xs[i + 1], KK_ACT_NONE, &xs[i]));  // gamma is folded into the weights
    r.note(names[i], xs[i + 1]);
  }
  KK_TRY(r.ln(xs[c.num_layers], nullptr, nullptr, m->final_norm, nullptr, 0, bb));
  r.note("backbone", bb);
  KK_TRY(vc_conv(r.st, B, m->head, bb, hd, KK_ACT_NONE, nullptr));
  r.note("head", hd);
  return vc_launch_istft((const float*)hd.p, hd.bs(), hd.ld, T, c.n_fft, c.hop_length, pcm, (long long)(T - 1) * c.hop_length, 0, B, r.st);
}

int check_cfg(const kk_vocos_config& c) {
  const char* who = "kk_vocos_create";
  if (c.input_channels < 1 || c.input_channels > 8192 || c.intermediate_dim < 1 || c.intermediate_dim > 16384) return kk_failf("%s: bad dimension", who);
  if (c.dim < 1 || c.dim > VC_MAX_C) return kk_failf("%s: dim must be 1 .. %d (the fused dwconv -> LayerNorm kernel's channel range)", who, VC_MAX_C);
  if (c.num_layers < 1 || c.num_layers > 16) return kk_failf("%s: 1 .. 16 layers", who);
  if (c.adanorm_num_embeddings < 0) return kk_failf("%s: adanorm_num_embeddings is 0 (LayerNorm) or positive", who);
  if (c.padding_same) return kk_failf("%s: padding=\"same\" is not built (the reference's head ignores it)", who);
  if (const char* why = vc_istft_refusal(c.n_fft, c.hop_length, 2)) return kk_failf("%s: %s", who, why);
  return 0;
}

}  // namespace

extern "C" int kk_vocos_create(const kk_vocos_config* cfg, kk_vocos** out) {
  if (!cfg || !out) return kk_fail("kk_vocos_create: null argument");
  KK_TRY(check_cfg(*cfg));
  kk_vocos* m = new kk_vocos();
  m->cfg = *cfg;
  m->adt = cfg->compute_dtype == KK_BF16 ? KK_BF16 : KK_F32;
  *out = m;
  return 0;
}

extern "C" void kk_vocos_destroy(kk_vocos* m) {
  if (!m) return;
  if (m->arena.dev) (void)hipFree(m->arena.dev);
  delete m;
}

extern "C" int kk_vocos_load_tensor(kk_vocos* m, const char* name, const int64_t* shape, int ndim, const float* data) {
  return kk_host_load_tensor("kk_vocos_load_tensor", m ? &m->arena.host : nullptr, m && m->finalized, name, shape, ndim, data);
}

extern "C" int kk_vocos_finalize(kk_vocos* m, void* stream) {
  if (!m) return kk_fail("kk_vocos_finalize: null model");
  if (m->finalized) return kk_fail("kk_vocos_finalize: already finalized");
  const kk_vocos_config& c = m->cfg;
  WeightArena& a = m->arena;
  const bool bf = m->adt == KK_BF16, ada = c.adanorm_num_embeddings > 0;
  const int D = c.dim, I = c.intermediate_dim;
  // a conv / Linear p.weight [O][K][I] (+ p.bias [O]), row o scaled by gamma[o] in float64 when given
  auto lin = [&](const std::string& p, int O, int K, int In, const HostTensor* gamma, bool pad_cols) {
    const HostTensor* w = a.get(p + ".weight", (size_t)O * K * In);
    const HostTensor* b = a.get(p + ".bias", (size_t)O);
    if (!w || !b) return VcLin();
    return vc_pack(
        a, O, K, In, bf, pad_cols, [&](int o, int k, int i) { return (gamma ? (double)gamma->d[o] : 1.0) * (double)w->d[((size_t)o * K + k) * In + i]; },
        [&](int o) { return (gamma ? (double)gamma->d[o] : 1.0) * (double)b->d[o]; });
  };
  auto norm = [&](const std::string& p, bool has_w, bool has_b) {
    VcNorm n;
    if (has_w) n.w = a.vec(p + ".weight", D);
    if (has_b) n.b = a.vec(p + ".bias", D);
    return n;
  };
  m->embed = lin("backbone.embed", D, 7, c.input_channels, nullptr, false);
  m->norm = norm("backbone.norm", !ada, !ada);
  m->blocks.resize(c.num_layers);
  for (int i = 0; i < c.num_layers; ++i) {
    VcBlock& k = m->blocks[i];
    const std::string p = "backbone.convnext." + std::to_string(i);
    k.dw_w = a.vec(p + ".dwconv.weight", (size_t)D * 7);  // [C][7][1]
    k.dw_b = a.vec(p + ".dwconv.bias", D);
    k.norm = norm(p + ".norm", !ada, !ada);
    k.pw1 = lin(p + ".pwconv1", I, 1, D, nullptr, false);
    k.pw2 = lin(p + ".pwconv2", D, 1, I, a.get(p + ".gamma", D), false);
  }
  m->final_norm = norm("backbone.final_layer_norm", true, c.final_norm_bias != 0);
  m->head = lin("head.out", c.n_fft + 2, 1, D, nullptr, true);
  if (!a.err.empty()) return kk_failf("kk_vocos_finalize: %s", a.err.c_str());
  KK_TRY(a.upload((hipStream_t)stream, "kk_vocos_finalize"));
  auto rs = [&](VcNorm& n) { a.resolve(n.w); a.resolve(n.b); };
  vc_resolve(a, m->embed); vc_resolve(a, m->head);
  rs(m->norm); rs(m->final_norm);
  for (VcBlock& k : m->blocks) {
    a.resolve(k.dw_w); a.resolve(k.dw_b); rs(k.norm);
    vc_resolve(a, k.pw1); vc_resolve(a, k.pw2);
  }
  m->finalized = true;
  return 0;
}

extern "C" int64_t kk_vocos_samples(const kk_vocos* m, int T) { return (m && T >= 2) ? (int64_t)(T - 1) * m->cfg.hop_length : 0; }

extern "C" size_t kk_vocos_workspace_bytes(kk_vocos* m, int B, int T) {
  if (!m || !m->finalized || B <= 0 || B > 65535 || vc_istft_refusal(m->cfg.n_fft, m->cfg.hop_length, T)) return 0;
  Run r(m, nullptr, B, nullptr, 0);
  if (run_forward(r, T, nullptr, nullptr, nullptr) != 0) return 0;
  return r.used + 256;
}

extern "C" int kk_vocos_forward(kk_vocos* m, void* stream, int B, int T, const float* features, const float* cond, void* workspace, size_t workspace_bytes,
                                float* pcm_out) {
  const char* who = "kk_vocos_forward";
  if (!m || !m->finalized) return kk_failf("%s: model not finalized", who);
  if (B <= 0 || B > 65535 || !features || !workspace || !pcm_out) return kk_failf("%s: bad argument (B 1 .. 65535)", who);
  if (const char* why = vc_istft_refusal(m->cfg.n_fft, m->cfg.hop_length, T)) return kk_failf("%s: %s", who, why);
  if ((m->cfg.adanorm_num_embeddings > 0) != (cond != nullptr))
    return kk_failf("%s: an AdaLayerNorm model needs the scale / shift pairs [num_layers + 1][B][2][dim], a LayerNorm model takes none", who);
  const size_t need = kk_vocos_workspace_bytes(m, B, T);
  if (need == 0 || workspace_bytes < need) return kk_failf("%s: workspace too small", who);
  { std::lock_guard<std::mutex> lk(m->dbg_mu); m->dbg.map.clear(); }
  Run r(m, (hipStream_t)stream, B, workspace, workspace_bytes);
  return run_forward(r, T, features, cond, pcm_out);
}

extern "C" int kk_vocos_debug_info(kk_vocos* m, const char* name, int64_t* rows, int64_t* channels) {
  if (!m || !name) return kk_fail("kk_vocos_debug_info: bad argument");
  std::lock_guard<std::mutex> lk(m->dbg_mu);
  return m->dbg.info("kk_vocos_debug_info", name, rows, channels);
}
extern "C" int kk_vocos_debug_fetch(kk_vocos* m, void* stream, const char* name, float* dst) {
  if (!m || !name || !dst) return kk_fail("kk_vocos_debug_fetch: bad argument");
  std::lock_guard<std::mutex> lk(m->dbg_mu);
  return m->dbg.fetch("kk_vocos_debug_fetch", name, (hipStream_t)stream, dst);
}

// ------------------------------------------------------------------------------------------------ single-kernel entry points (ABI minor 34)
extern "C" int kk_op_vocos_dwconv_rows(int C) { return C >= 1 && C <= VC_MAX_C ? vc_auto_rows(C) : 0; }

extern "C" int kk_op_vocos_dwconv_ln(void* stream, int B, const float* x, long long xbs, int ldx, int T, int C, const float* w, const float* bias, const float* a,
                                     const float* s, long long as_stride, float eps, void* out, long long obs, int ldo, int out_dtype, int rows) {
  const char* who = "kk_op_vocos_dwconv_ln";
  if (C < 1 || C > VC_MAX_C) return kk_failf("%s: C must be 1 .. %d, got %d", who, VC_MAX_C, C);
  if (B <= 0 || B > 65535 || T < 1 || T > (1 << 30) || !x || !out || (const void*)x == out || (w != nullptr) != (bias != nullptr))
    return kk_failf("%s: B 1 .. 65535, T 1 .. 2^30, x / out non-null and distinct, w and bias both given or both null", who);
  if (out_dtype != KK_F32 && out_dtype != KK_BF16) return kk_failf("%s: out_dtype is KK_DTYPE_F32 or KK_DTYPE_BF16", who);
  if (ldx < C || ldo < C || xbs < (long long)T * ldx || obs < (long long)T * ldo) return kk_failf("%s: a pitch is smaller than what it spans", who);
  if (as_stride != 0 && as_stride < C) return kk_failf("%s: as_stride is 0 (one pair for every item) or at least C", who);
  if (rows < 0 || rows > (1 << 16)) return kk_failf("%s: rows is 0 (chosen by shape) or positive", who);
  return vc_launch_dwconv_ln(x, xbs, ldx, T, C, w, bias, a, s, as_stride, eps, out, obs, ldo, out_dtype, rows, B, (hipStream_t)stream);
}

extern "C" int kk_op_vocos_istft(void* stream, int B, int T, const float* h, long long hbs, int ldh, int n_fft, int hop_length, float* out, long long obs,
                                 int group) {
  const char* who = "kk_op_vocos_istft";
  if (const char* why = vc_istft_refusal(n_fft, hop_length, T)) return kk_failf("%s: %s", who, why);
  if (B <= 0 || B > 65535 || !h || !out || group < 0 || group > 1024) return kk_failf("%s: B 1 .. 65535, h / out non-null, group 0 (chosen by shape) .. 1024", who);
  if (ldh < n_fft + 2 || hbs < (long long)T * ldh || obs < (long long)(T - 1) * hop_length) return kk_failf("%s: a pitch is smaller than what it spans", who);
  return vc_launch_istft(h, hbs, ldh, T, n_fft, hop_length, out, obs, group, B, (hipStream_t)stream);
}
