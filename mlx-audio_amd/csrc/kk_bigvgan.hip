// BigVGAN vocoder (mlx_audio/codec/models/bigvgan/{bigvgan,amp,resample,activation,conv}.py): mel [B][T][num_mels] -> pcm [B][T prod(upsample_rates)].
//   conv_pre k7 -> per stage {transposed conv (k, stride u, padding (k - u) / 2), the mean of num_kernels AMP blocks} -> Activation1d -> conv_post k7
//   to one channel -> tanh or clip.  AMPBlock1: x = x + conv2(act2(conv1_dil(act1(x)))) per dilation; AMPBlock2: x = x + conv_dil(act(x)).
// Every dense conv is the library's generic fp32 kernel or, for bf16 tensors, the variant-4 matrix-core kernel (kk_codec_conv.h); the residual rides
// on the conv's epilogue, and so does the mean over the blocks: a block's last conv stores (x + conv) / num_kernels, blocks after the first add to it.
// What exists only here: Activation1d (resample.py:157-177) as ONE kernel, and the one-channel last conv with tanh / clip.
//
// Activation1d restated (resample.py:101-136 UpSample1d, :49-98 LowPassFilter1d; both filters kaiser_sinc_filter1d(0.25, 0.3, 12), symmetric):
//   up:   edge pad 5, depth-wise conv_transpose1d stride 2, times 2, slice [15 : -15]:
//           u[2 t]     = 2 sum_{d = -3 .. 2} fu[5 - 2 d] x[clamp(t + d, 0, L - 1)]
//           u[2 t + 1] = 2 sum_{d = -2 .. 3} fu[6 - 2 d] x[clamp(t + d, 0, L - 1)]
//   act:  a[j] = u[j] + 1 / (beta_c + 1e-9) sin^2(alpha_c u[j])                          (activation.py:42-51 SnakeBeta)
//   down: edge pad (5, 6), depth-wise conv1d stride 2:  out[t] = sum_{k < 12} fd[k] a[clamp(2 t - 5 + k, 0, 2 L - 1)]
// so out[t] reads x[t - 5 .. t + 5].  Both edge rules are index clamps: x into [0, L - 1], the ACTIVATED up-sampled sequence into [0, 2 L - 1].
//
// The kernel: a lane owns VEC adjacent channels (one packed load) of one time segment of S rows and walks it in time.  Per step t it loads row
// clamp(t + 5) into a 6-deep window x[t .. t + 5], from which BOTH new up-samples come (u[2 t + 5] and u[2 t + 6] read exactly that window), pushes their
// Snake values into a 12-deep ring a[2 t - 5 .. 2 t + 6], and writes the ring's dot product with fd.  Window and ring live in registers; the step loop is
// unrolled by 6, after which both have rotated through whole, so no register moves remain.  A segment warms up with 5 steps that only push (10 rows of
// halo: 5 for the window, 5 steps for the ring).  Work items (segment, channel group) are numbered flat over the grid, so a wave holds several segments
// of a narrow tensor and no lane idles; lanes never talk to each other (no LDS, no shuffles).  The 2 L intermediate never exists in memory.
// Every u, a and out is one fixed fmaf chain over clamped indices, so its bits do not depend on B, on the segment length or on the segment it fell in.
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
#include "kk_codec_conv.h"

namespace {

// ------------------------------------------------------------------------------------------------------------- kernels
struct BvFilters {
  float fu2[12];  // 2 x the up-sampling filter (the factor `ratio` of resample.py:129 folded in: exact)
  float fd[12];   // the low-pass filter of the down-sampling
};

template <typename T, int VEC>
__device__ __forceinline__ void bv_load(const T* p, float (&v)[VEC]) {
  if constexpr (VEC == 1) {
    v[0] = kk_ld(p);
  } else if constexpr (sizeof(T) == 4) {
    const float2 w = *(const float2*)p;
    v[0] = w.x; v[1] = w.y;
  } else {
    const unsigned w = *(const unsigned*)p;
    v[0] = __uint_as_float(w << 16); v[1] = __uint_as_float(w & 0xFFFF0000u);
  }
}
template <typename T, int VEC>
__device__ __forceinline__ void bv_store(T* p, const float (&v)[VEC], int nvalid) {
  if (VEC == 1 || nvalid < VEC) {  // (a pair that straddles C: the column beyond C is not written)
    kk_st(p, v[0]);
  } else if constexpr (VEC == 2 && sizeof(T) == 4) {
    *(float2*)p = make_float2(v[0], v[1]);
  } else if constexpr (VEC == 2) {
    const bf16_t lo = (bf16_t)v[0], hi = (bf16_t)v[1];
    *(unsigned*)p = (unsigned)__builtin_bit_cast(unsigned short, lo) | ((unsigned)__builtin_bit_cast(unsigned short, hi) << 16);
  }
}

// FAST (bf16 tensors): the hardware sine; fp32 tensors: sinf
template <typename T, int VEC, bool FAST>
__global__ __launch_bounds__(256) void bv_amp_act_kernel(const T* x, long long xbs, int ldx, int L, int C, int Cp, int S, int nseg, const float* alpha,
                                                         const float* invb, BvFilters f, T* out, long long obs, int ldo) {
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  const int seg = (int)(item / Cp);
  if (seg >= nseg) return;
  const int c = (int)(item - (long long)seg * Cp) * VEC, nvalid = C - c < VEC ? C - c : VEC;
  const int t0 = seg * S, t1 = t0 + S < L ? t0 + S : L, jmax = 2 * L - 1;
  const T* xb = x + (long long)blockIdx.y * xbs + c;
  T* ob = out + (long long)blockIdx.y * obs + c;
  float al[VEC], ib[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const int cc = v < nvalid ? c + v : c;
    al[v] = alpha[cc]; ib[v] = invb[cc];
  }
  float xw[VEC][6], r[VEC][12];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
#pragma unroll
    for (int k = 0; k < 12; ++k) r[v][k] = 0.f;
    xw[v][0] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {  // rows t0 - 5 .. t0 - 1: the window's halo
    const int row = t0 - 5 + i < 0 ? 0 : t0 - 5 + i;
    float nv[VEC];
    bv_load<T, VEC>(xb + (long long)row * ldx, nv);
#pragma unroll
    for (int v = 0; v < VEC; ++v) xw[v][i + 1] = nv[v];
  }
  // one step: row clamp(tau + 5) enters the window, a[2 tau + 5] and a[2 tau + 6] enter the ring
  auto push = [&](int tau) {
    int row = tau + 5;
    row = row < 0 ? 0 : (row > L - 1 ? L - 1 : row);
    float nv[VEC];
    bv_load<T, VEC>(xb + (long long)row * ldx, nv);
    const int j1 = 2 * tau + 5;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
#pragma unroll
      for (int i = 0; i < 5; ++i) xw[v][i] = xw[v][i + 1];
      xw[v][5] = nv[v];
      float u1 = 0.f, u2 = 0.f;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        u1 = __builtin_fmaf(f.fu2[10 - 2 * i], xw[v][i], u1);  // u[2 (tau + 2) + 1]
        u2 = __builtin_fmaf(f.fu2[11 - 2 * i], xw[v][i], u2);  // u[2 (tau + 3)]
      }
      const float s1 = FAST ? __sinf(al[v] * u1) : sinf(al[v] * u1), s2 = FAST ? __sinf(al[v] * u2) : sinf(al[v] * u2);
      float e1 = u1 + ib[v] * (s1 * s1), e2 = u2 + ib[v] * (s2 * s2);
      if (j1 > jmax) e1 = r[v][11];  // past the end: a[2 L - 1] again (the ring's newest entry)
      if (j1 + 1 > jmax) e2 = e1;
#pragma unroll
      for (int k = 0; k < 10; ++k) r[v][k] = r[v][k + 2];
      r[v][10] = e1; r[v][11] = e2;
    }
  };
#pragma unroll
  for (int i = 0; i < 5; ++i) push(t0 - 5 + i);  // the ring's halo: r[2 .. 11] = a[2 t0 - 5 .. 2 t0 + 4]
  if (t0 == 0) {                                  // entries before the start are a[0] (= r[7]); later segments start at 2 t0 - 5 >= 1
#pragma unroll
    for (int v = 0; v < VEC; ++v)
#pragma unroll
      for (int k = 2; k < 7; ++k) r[v][k] = r[v][7];
  }
  for (int tb = t0; tb < t1; tb += 6) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int t = tb + i;
      push(t);
      float o[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        o[v] = 0.f;
#pragma unroll
        for (int k = 0; k < 12; ++k) o[v] = __builtin_fmaf(f.fd[k], r[v][k], o[v]);
      }
      if (t < t1) bv_store<T, VEC>(ob + (long long)t * ldo, o, nvalid);
    }
  }
}

// ---- conv_post (bigvgan.py:88-95,115-120): Cout = 1, then tanh or clip(-1, 1):  out[b][t] = fin(sum_k sum_c w[k][c] x[t - pad + k][c] + bias).
// A workgroup owns 256 output rows; per 32-channel chunk it stages its 256 + K - 1 rows in LDS (pitch 33), then one lane per row sums the taps.
constexpr int BV_POST_TR = 256;
template <typename T>
__global__ __launch_bounds__(256) void bv_conv_post_kernel(const T* x, int ld, int L, int Cin, int K, int pad, const float* w, const float* bias, int tanh_out,
                                                           float* out) {
  extern __shared__ float bv_sm[];
  float* xs = bv_sm;                                  // [BV_POST_TR + K - 1][33]
  float* ws = bv_sm + (BV_POST_TR + K - 1) * 33;      // [K][32]
  const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * BV_POST_TR, nrow = BV_POST_TR + K - 1;
  float acc = 0.f;
  for (int c0 = 0; c0 < Cin; c0 += 32) {
    __syncthreads();
    for (int e = tid; e < nrow * 32; e += 256) {
      const int rr = e >> 5, cl = e & 31, row = t0 - pad + rr, c = c0 + cl;
      float v = 0.f;
      if (c < Cin && row >= 0 && row < L) v = kk_ld(x + ((long long)b * L + row) * ld + c);
      xs[rr * 33 + cl] = v;
    }
    for (int e = tid; e < K * 32; e += 256) ws[e] = c0 + (e & 31) < Cin ? w[(e >> 5) * Cin + c0 + (e & 31)] : 0.f;
    __syncthreads();
    for (int k = 0; k < K; ++k) {
      const float* xr = xs + (tid + k) * 33;
#pragma unroll
      for (int i = 0; i < 32; ++i) acc = __builtin_fmaf(xr[i], ws[k * 32 + i], acc);
    }
  }
  const int t = t0 + tid;
  if (t < L) {
    const float v = acc + (bias ? bias[0] : 0.f);
    out[(long long)b * L + t] = tanh_out ? tanhf(v) : fminf(fmaxf(v, -1.0f), 1.0f);
  }
}

// ------------------------------------------------------------------------------------------------------------- launch shapes
// segment length: the longest of 192 / 96 / 48 / 24 rows (multiples of the unroll) that still gives 2048 waves, so that the halo (10 rows a segment) stays
// small on big tensors and a short or narrow tensor still fills the machine
int bv_auto_seg(int L, int Cp, int B) {
  int S = 192;
  while (S > 24 && (long long)kk_cdiv(L, S) * Cp * B < 2048ll * 64) S /= 2;
  return S;
}
bool bv_even(const void* p, long long bs, int ld, int dtype) { return ld % 2 == 0 && bs % 2 == 0 && ((uintptr_t)p & (2 * esize(dtype) - 1)) == 0; }

int bv_launch_amp_act(const void* x, long long xbs, int ldx, int dtype, int L, int C, const float* alpha, const float* invb, const BvFilters& f, void* out,
                      long long obs, int ldo, int seg, int B, hipStream_t st) {
  const bool pair = bv_even(x, xbs, ldx, dtype) && bv_even(out, obs, ldo, dtype);  // two channels per load and store
  const int Cp = pair ? kk_cdiv(C, 2) : C;
  const int S = seg > 0 ? seg : bv_auto_seg(L, Cp, B), nseg = kk_cdiv(L, S);
  const dim3 grid((unsigned)(((long long)nseg * Cp + 255) / 256), B);
#define BV_GO(T, VEC, FAST) \
  hipLaunchKernelGGL((bv_amp_act_kernel<T, VEC, FAST>), grid, dim3(256), 0, st, (const T*)x, xbs, ldx, L, C, Cp, S, nseg, alpha, invb, f, (T*)out, obs, ldo)
  if (dtype == KK_BF16) {
    if (pair) BV_GO(bf16_t, 2, true);
    else BV_GO(bf16_t, 1, true);
  } else {
    if (pair) BV_GO(float, 2, false);
    else BV_GO(float, 1, false);
  }
#undef BV_GO
  KK_CHECK_LAUNCH();
  return 0;
}

int bv_launch_conv_post(const void* x, int dtype, int ld, int L, int Cin, int K, int pad, const float* w, const float* bias, int tanh_out, float* out, int B,
                        hipStream_t st) {
  const dim3 grid(kk_cdiv(L, BV_POST_TR), B);
  const size_t lds = ((size_t)(BV_POST_TR + K - 1) * 33 + (size_t)K * 32) * 4;
  if (dtype == KK_BF16) hipLaunchKernelGGL(bv_conv_post_kernel<bf16_t>, grid, dim3(256), lds, st, (const bf16_t*)x, ld, L, Cin, K, pad, w, bias, tanh_out, out);
  else hipLaunchKernelGGL(bv_conv_post_kernel<float>, grid, dim3(256), lds, st, (const float*)x, ld, L, Cin, K, pad, w, bias, tanh_out, out);
  KK_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------- the filter
double bessel_i0(double x) {
  double s = 1.0, t = 1.0;
  for (int k = 1; k < 200 && t > 1e-18 * s; ++k) {
    t *= (x / 2) / k * (x / 2) / k;
    s += t;
  }
  return s;
}
// kaiser_sinc_filter1d (resample.py:17-46) in float64
void kaiser_sinc(double cutoff, double half_width, int K, double* f) {
  const int half = K / 2;
  const double A = 2.285 * (half - 1) * M_PI * (4 * half_width) + 7.95;
  const double beta = A > 50.0 ? 0.1102 * (A - 8.7) : (A >= 21.0 ? 0.5842 * pow(A - 21.0, 0.4) + 0.07886 * (A - 21.0) : 0.0);
  double sum = 0;
  for (int n = 0; n < K; ++n) {
    const double r = 2.0 * n / (K - 1) - 1.0, win = bessel_i0(beta * sqrt(std::max(0.0, 1.0 - r * r))) / bessel_i0(beta);  // np.kaiser
    const double time = K % 2 == 0 ? n - half + 0.5 : n - half, v = 2 * cutoff * time;
    f[n] = 2 * cutoff * win * (v == 0 ? 1.0 : sin(M_PI * v) / (M_PI * v));
    sum += f[n];
  }
  for (int n = 0; n < K; ++n) f[n] /= sum;
}
BvFilters make_filters() {  // Activation1d(up_ratio 2, down_ratio 2, kernel 12): cutoff 0.5 / 2, half width 0.6 / 2 for both
  double f[12];
  kaiser_sinc(0.25, 0.3, 12, f);
  BvFilters o;
  for (int k = 0; k < 12; ++k) { o.fu2[k] = (float)(2.0 * f[k]); o.fd[k] = (float)f[k]; }
  return o;
}

struct AmpAct {  // SnakeBeta's per-channel constants: alpha_c and 1 / (beta_c + 1e-9), exp first when snake_logscale
  ArenaVec alpha, invb;
};
struct AmpBlock {  // AMPBlock1 (amp.py:10-58) or AMPBlock2 (amp.py:61-96: c1 and a1 only)
  int k = 3, nd = 0, dil[4] = {1, 1, 1, 1};
  PackedConv c1[4], c2[4];
  AmpAct a1[4], a2[4];
};
struct Stage {
  PackedConv up;
  int stride = 1, k = 2, pad = 0, Cin = 0, Cout = 0;
  std::vector<AmpBlock> blocks;
};

}  // namespace

struct kk_bigvgan {
  kk_bigvgan_config cfg;
  WeightArena arena;
  bool finalized = false;
  int adt = KK_F32;
  BvFilters filt;
  PackedConv conv_pre;
  std::vector<Stage> stages;
  AmpAct act_post;
  ArenaVec post_w, post_b;  // conv_post [7][C], its bias [1]
  int post_C = 0;
  DebugNotes dbg;
  std::mutex dbg_mu;
};

namespace {

int convt_len(int L, int s, int k, int pad) { return (L - 1) * s - 2 * pad + k; }

struct Run : Workspace {
  kk_bigvgan* m;
  hipStream_t st;
  int B;
  char* slot[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  Run(kk_bigvgan* m_, hipStream_t st_, int B_, void* ws, size_t ws_bytes) : m(m_), st(st_), B(B_) {
    base = (char*)ws; cap = ws_bytes; dry = ws == nullptr;
  }
  Act act(int rows, int C, int dtype) {
    Act t;
    t.dtype = dtype; t.rows = rows; t.C = C; t.ld = pitch_of(C, dtype);
    t.p = raw((size_t)B * rows * t.ld * esize(dtype));
    return t;
  }
  Act view(int i, int rows, int C, int dtype) const {
    Act t;
    t.dtype = dtype; t.rows = rows; t.C = C; t.ld = pitch_of(C, dtype); t.p = slot[i];
    return t;
  }
  void note(const std::string& name, const Act& t) {
    if (!dry) {
      std::lock_guard<std::mutex> lk(m->dbg_mu);
      m->dbg.map[name] = DebugNote{t.p, t.ld, t.bs(), t.rows, t.C, t.dtype, B};
    }
  }
  int amp(const AmpAct& a, const Act& x, const Act& out) {
    return bv_launch_amp_act(x.p, x.bs(), x.ld, x.dtype, x.rows, x.C, a.alpha.p, a.invb.p, m->filt, out.p, out.bs(), out.ld, 0, B, st);
  }
};

long long samples_of(const kk_bigvgan* m, int T) {
  long long L = T;
  for (const Stage& s : m->stages) {
    L = (L - 1) * s.stride - 2 * s.pad + s.k;
    if (L < 1 || L > (1ll << 30)) return 0;
  }
  return L;
}

// BigVGAN.__call__ (bigvgan.py:97-122)
int run_forward(Run& r, int T, const float* mel, float* pcm) {
  kk_bigvgan* m = r.m;
  const kk_bigvgan_config& c = m->cfg;
  const int B = r.B, dt = m->adt, nk = c.n_resblock_kernels;
  Act y = r.act(T, c.upsample_initial_channel, dt);
  {
    size_t mx = 0;
    int L = T;
    for (const Stage& s : m->stages) {
      L = convt_len(L, s.stride, s.k, s.pad);
      mx = std::max(mx, (size_t)L * pitch_of(s.Cout, dt));
    }
    for (int i = 0; i < 5; ++i) r.slot[i] = (char*)r.raw(mx * B * esize(dt));  // the stage's input, act, conv1's output, and two block states
  }
  if (r.oom) return kk_fail("kk_bigvgan_forward: workspace too small");
  if (!r.dry) {
    Act x;
    x.p = const_cast<float*>(mel); x.rows = T; x.C = c.num_mels; x.ld = c.num_mels; x.dtype = KK_F32;
    KK_TRY(codec_conv(r.st, B, m->conv_pre, x, y, 3, false, 1, 1, nullptr, 1.f, 0, nullptr));
    r.note("conv_pre", y);
  }
  int L = T;
  for (size_t si = 0; si < m->stages.size(); ++si) {
    const Stage& s = m->stages[si];
    const int Lo = convt_len(L, s.stride, s.k, s.pad), Cc = s.Cout;
    Act o = r.act(Lo, Cc, dt);
    if (r.oom) return kk_fail("kk_bigvgan_forward: workspace too small");
    if (!r.dry) {
      const Act u = r.view(0, Lo, Cc, dt), a = r.view(1, Lo, Cc, dt), h = r.view(2, Lo, Cc, dt), p0 = r.view(3, Lo, Cc, dt), p1 = r.view(4, Lo, Cc, dt);
      KK_TRY(codec_conv(r.st, B, s.up, y, u, s.pad, true, s.stride, 1, nullptr, 1.f, 0, nullptr));
      for (int j = 0; j < nk; ++j) {
        const AmpBlock& blk = s.blocks[j];
        const Act* cur = &u;
        for (int i = 0; i < blk.nd; ++i) {
          const bool last = i == blk.nd - 1;
          const Act* dst = last ? &o : (cur == &p0 ? &p1 : &p0);
          const int d = blk.dil[i];
          KK_TRY(r.amp(blk.a1[i], *cur, a));
          // the block's last conv carries the mean over the blocks: (x + conv) / num_kernels, added to what the blocks before it left
          const float scale = last ? 1.0f / (float)nk : 1.0f;
          const int accumulate = last && j > 0;
          if (c.resblock == 1) {
            KK_TRY(codec_conv(r.st, B, blk.c1[i], a, h, (blk.k - 1) * d / 2, false, 1, d, nullptr, 1.f, 0, nullptr));
            KK_TRY(r.amp(blk.a2[i], h, a));
            KK_TRY(codec_conv(r.st, B, blk.c2[i], a, *dst, (blk.k - 1) / 2, false, 1, 1, cur, scale, accumulate, nullptr));
          } else {
            KK_TRY(codec_conv(r.st, B, blk.c1[i], a, *dst, (blk.k - 1) * d / 2, false, 1, d, cur, scale, accumulate, nullptr));
          }
          cur = dst;
        }
      }
      static const char* names[8] = {"stage0", "stage1", "stage2", "stage3", "stage4", "stage5", "stage6", "stage7"};
      r.note(names[si], o);
    }
    y = o;
    L = Lo;
  }
  if (r.dry) return 0;
  const Act a = r.view(1, L, y.C, dt);
  KK_TRY(r.amp(m->act_post, y, a));
  r.note("activation_post", a);
  return bv_launch_conv_post(a.p, dt, a.ld, L, m->post_C, 7, 3, m->post_w.p, c.use_bias_at_final ? m->post_b.p : nullptr, c.use_tanh_at_final, pcm, B, r.st);
}

// ------------------------------------------------------------------------------------------------------------- packing
struct Packer {
  kk_bigvgan* m;
  WeightArena& a;
  // weight norm folded in float64 (conv.py:56,103): g v / |v|, v [O][K][I]; the norm runs over the axes except `keep` (0: WNConv1d, 2: WNConvTranspose1d)
  bool folded(const std::string& p, int O, int K, int I, int keep, std::vector<double>& w) {
    const HostTensor* v = a.get(p + ".weight_v", (size_t)O * K * I);
    const HostTensor* g = a.get(p + ".weight_g", (size_t)(keep == 0 ? O : I));
    if (!v || !g) return false;
    const int n = keep == 0 ? O : I;
    std::vector<double> ss(n, 0.0);
    for (int o = 0; o < O; ++o)
      for (int k = 0; k < K; ++k)
        for (int i = 0; i < I; ++i) { const double x = v->d[((size_t)o * K + k) * I + i]; ss[keep == 0 ? o : i] += x * x; }
    w.resize((size_t)O * K * I);
    for (int o = 0; o < O; ++o)
      for (int k = 0; k < K; ++k)
        for (int i = 0; i < I; ++i) {
          const size_t e = ((size_t)o * K + k) * I + i;
          const int q = keep == 0 ? o : i;
          w[e] = (double)g->d[q] * (double)v->d[e] / sqrt(ss[q]);
        }
    return true;
  }
  PackedConv conv(const std::string& p, int O, int K, int I, bool transposed, bool bias, bool mfma) {
    std::vector<double> w;
    if (!folded(p, O, K, I, transposed ? 2 : 0, w)) return PackedConv();
    return codec_pack(a, p, O, K, I, bias, mfma, [&](int o, int k, int i) { return (float)w[((size_t)o * K + k) * I + i]; });
  }
  AmpAct act(const std::string& p, int C) {  // p.act.{alpha, beta}
    AmpAct t;
    const HostTensor* al = a.get(p + ".act.alpha", (size_t)C);
    const HostTensor* be = a.get(p + ".act.beta", (size_t)C);
    if (!al || !be) return t;
    std::vector<float> fa(C), fb(C);
    for (int c = 0; c < C; ++c) {
      const double x = al->d[c], y = be->d[c];
      fa[c] = (float)(m->cfg.snake_logscale ? exp(x) : x);
      fb[c] = (float)(1.0 / ((m->cfg.snake_logscale ? exp(y) : y) + 1e-9));
    }
    t.alpha = a.put(fa.data(), C);
    t.invb = a.put(fb.data(), C);
    return t;
  }
};

void resolve(kk_bigvgan* m, AmpAct& t) { m->arena.resolve(t.alpha); m->arena.resolve(t.invb); }

int check_cfg(const kk_bigvgan_config& c) {
  const char* who = "kk_bigvgan_create";
  if (c.num_mels < 1 || c.upsample_initial_channel < 1) return kk_failf("%s: bad dimension", who);
  if (c.resblock != 1 && c.resblock != 2) return kk_failf("%s: resblock must be 1 or 2", who);
  if (c.n_upsamples < 1 || c.n_upsamples > 8) return kk_failf("%s: 1 .. 8 upsample_rates", who);
  if (c.upsample_initial_channel % (1 << c.n_upsamples) != 0) return kk_failf("%s: upsample_initial_channel must be divisible by 2^len(upsample_rates)", who);
  for (int i = 0; i < c.n_upsamples; ++i) {
    const int u = c.upsample_rates[i], k = c.upsample_kernel_sizes[i];
    if (u < 1 || u > 64 || k < u || k > 128) return kk_failf("%s: upsample rate %d with kernel %d is not built (1 <= rate <= kernel <= 128)", who, u, k);
  }
  if (c.n_resblock_kernels < 1 || c.n_resblock_kernels > 4) return kk_failf("%s: 1 .. 4 resblock_kernel_sizes", who);
  for (int j = 0; j < c.n_resblock_kernels; ++j) {
    const int k = c.resblock_kernel_sizes[j];
    if (k < 1 || k > 15 || c.n_dilations[j] < 1 || c.n_dilations[j] > 4) return kk_failf("%s: resblock kernel sizes 1 .. 15 with 1 .. 4 dilations each", who);
    for (int i = 0; i < c.n_dilations[j]; ++i) {
      const int d = c.resblock_dilation_sizes[j][i];
      if (d < 1 || d > 64 || ((k - 1) * d) % 2 != 0 || (k - 1) % 2 != 0)
        return kk_failf("%s: kernel %d with dilation %d does not keep the length (the residual add of amp.py would not broadcast)", who, k, d);
    }
  }
  return 0;
}

bool dt_ok(int d) { return d == KK_F32 || d == KK_BF16; }

}  // namespace

extern "C" int kk_bigvgan_create(const kk_bigvgan_config* cfg, kk_bigvgan** out) {
  if (!cfg || !out) return kk_fail("kk_bigvgan_create: null argument");
  KK_TRY(check_cfg(*cfg));
  kk_bigvgan* m = new kk_bigvgan();
  m->cfg = *cfg;
  m->adt = cfg->compute_dtype == KK_BF16 ? KK_BF16 : KK_F32;
  m->filt = make_filters();
  m->stages.resize(cfg->n_upsamples);
  for (int i = 0; i < cfg->n_upsamples; ++i) {  // (the shapes: kk_bigvgan_samples answers before finalize)
    Stage& s = m->stages[i];
    s.stride = cfg->upsample_rates[i]; s.k = cfg->upsample_kernel_sizes[i]; s.pad = (s.k - s.stride) / 2;
    s.Cin = cfg->upsample_initial_channel >> i; s.Cout = cfg->upsample_initial_channel >> (i + 1);
  }
  *out = m;
  return 0;
}

extern "C" void kk_bigvgan_destroy(kk_bigvgan* m) {
  if (!m) return;
  if (m->arena.dev) (void)hipFree(m->arena.dev);
  delete m;
}

extern "C" int kk_bigvgan_load_tensor(kk_bigvgan* m, const char* name, const int64_t* shape, int ndim, const float* data) {
  return kk_host_load_tensor("kk_bigvgan_load_tensor", m ? &m->arena.host : nullptr, m && m->finalized, name, shape, ndim, data);
}

extern "C" int kk_bigvgan_finalize(kk_bigvgan* m, void* stream) {
  if (!m) return kk_fail("kk_bigvgan_finalize: null model");
  if (m->finalized) return kk_fail("kk_bigvgan_finalize: already finalized");
  const kk_bigvgan_config& c = m->cfg;
  Packer P{m, m->arena};
  const bool bf = m->adt == KK_BF16;
  const int nk = c.n_resblock_kernels;
  m->conv_pre = P.conv("conv_pre", c.upsample_initial_channel, 7, c.num_mels, false, true, false);  // (fp32 input: the generic kernel)
  for (int si = 0; si < c.n_upsamples; ++si) {
    Stage& s = m->stages[si];
    s.up = P.conv("ups." + std::to_string(si) + ".0", s.Cout, s.k, s.Cin, true, true, bf);
    s.blocks.resize(nk);
    for (int j = 0; j < nk; ++j) {
      AmpBlock& b = s.blocks[j];
      const std::string p = "resblocks." + std::to_string(si * nk + j);
      b.k = c.resblock_kernel_sizes[j]; b.nd = c.n_dilations[j];
      for (int i = 0; i < b.nd; ++i) {
        b.dil[i] = c.resblock_dilation_sizes[j][i];
        const std::string is = std::to_string(i);
        if (c.resblock == 1) {
          b.c1[i] = P.conv(p + ".convs1." + is, s.Cout, b.k, s.Cout, false, true, bf);
          b.c2[i] = P.conv(p + ".convs2." + is, s.Cout, b.k, s.Cout, false, true, bf);
          b.a1[i] = P.act(p + ".activations." + std::to_string(2 * i), s.Cout);  // amp.py:53-55: activations[::2] and [1::2]
          b.a2[i] = P.act(p + ".activations." + std::to_string(2 * i + 1), s.Cout);
        } else {
          b.c1[i] = P.conv(p + ".convs." + is, s.Cout, b.k, s.Cout, false, true, bf);
          b.a1[i] = P.act(p + ".activations." + is, s.Cout);
        }
      }
    }
  }
  m->post_C = c.upsample_initial_channel >> c.n_upsamples;
  m->act_post = P.act("activation_post", m->post_C);
  {
    std::vector<double> w;
    if (P.folded("conv_post", 1, 7, m->post_C, 0, w)) {
      std::vector<float> f(w.begin(), w.end());
      m->post_w = P.a.put(f.data(), f.size());
    }
    if (c.use_bias_at_final) m->post_b = P.a.vec("conv_post.bias", 1);
  }
  if (!P.a.err.empty()) return kk_failf("kk_bigvgan_finalize: %s", P.a.err.c_str());
  KK_TRY(m->arena.upload((hipStream_t)stream, "kk_bigvgan_finalize"));
  codec_resolve(m->arena, m->conv_pre);
  for (Stage& s : m->stages) {
    codec_resolve(m->arena, s.up);
    for (AmpBlock& b : s.blocks)
      for (int i = 0; i < b.nd; ++i) {
        codec_resolve(m->arena, b.c1[i]); resolve(m, b.a1[i]);
        if (c.resblock == 1) { codec_resolve(m->arena, b.c2[i]); resolve(m, b.a2[i]); }
      }
  }
  resolve(m, m->act_post);
  m->arena.resolve(m->post_w); m->arena.resolve(m->post_b);
  m->finalized = true;
  return 0;
}

extern "C" int64_t kk_bigvgan_samples(const kk_bigvgan* m, int T) { return (m && T > 0) ? samples_of(m, T) : 0; }

extern "C" size_t kk_bigvgan_workspace_bytes(kk_bigvgan* m, int B, int T) {
  if (!m || !m->finalized || B <= 0 || B > 65535 || T <= 0 || samples_of(m, T) < 1 || (long long)B * samples_of(m, T) * 64 > (1ll << 40)) return 0;
  Run r(m, nullptr, B, nullptr, 0);
  if (run_forward(r, T, nullptr, nullptr) != 0) return 0;
  return r.used + 256;
}

extern "C" int kk_bigvgan_forward(kk_bigvgan* m, void* stream, int B, int T, const float* mel, void* workspace, size_t workspace_bytes, float* pcm_out) {
  const char* who = "kk_bigvgan_forward";
  if (!m || !m->finalized) return kk_failf("%s: model not finalized", who);
  if (B <= 0 || T <= 0 || !mel || !workspace || !pcm_out) return kk_failf("%s: bad argument", who);
  const size_t need = kk_bigvgan_workspace_bytes(m, B, T);
  if (need == 0) return kk_failf("%s: B 1 .. 65535 and a T that gives 1 .. 2^30 samples", who);
  if (workspace_bytes < need) return kk_failf("%s: workspace too small", who);
  { std::lock_guard<std::mutex> lk(m->dbg_mu); m->dbg.map.clear(); }
  Run r(m, (hipStream_t)stream, B, workspace, workspace_bytes);
  return run_forward(r, T, mel, pcm_out);
}

extern "C" int kk_bigvgan_debug_info(kk_bigvgan* m, const char* name, int64_t* rows, int64_t* channels) {
  if (!m || !name) return kk_fail("kk_bigvgan_debug_info: bad argument");
  std::lock_guard<std::mutex> lk(m->dbg_mu);
  return m->dbg.info("kk_bigvgan_debug_info", name, rows, channels);
}
extern "C" int kk_bigvgan_debug_fetch(kk_bigvgan* m, void* stream, const char* name, float* dst) {
  if (!m || !name || !dst) return kk_fail("kk_bigvgan_debug_fetch: bad argument");
  std::lock_guard<std::mutex> lk(m->dbg_mu);
  return m->dbg.fetch("kk_bigvgan_debug_fetch", name, (hipStream_t)stream, dst);
}

// ------------------------------------------------------------------------------------------------ single-kernel entry points (ABI minor 33)
extern "C" int kk_op_bigvgan_filter(int up_ratio, int down_ratio, int kernel_size, float* taps_out) {
  if (up_ratio != 2 || down_ratio != 2 || kernel_size != 12) return kk_fail("kk_op_bigvgan_filter: only up_ratio = down_ratio = 2 with 12 taps is built (the form Activation1d is instantiated in)");
  if (!taps_out) return kk_fail("kk_op_bigvgan_filter: null argument");
  const BvFilters f = make_filters();
  memcpy(taps_out, f.fd, sizeof f.fd);
  return 0;
}

extern "C" int kk_op_bigvgan_amp_act(void* stream, int B, const void* x, long long xbs, int ldx, int dtype, int L, int C, const float* alpha, const float* inv_beta,
                                     void* out, long long obs, int ldo, int seg_rows) {
  const char* who = "kk_op_bigvgan_amp_act";
  if (B <= 0 || B > 65535 || L < 1 || L > (1 << 30) || C < 1 || !x || !alpha || !inv_beta || !out || x == out)
    return kk_failf("%s: B 1 .. 65535, L 1 .. 2^30, C positive, x / alpha / inv_beta / out non-null, out != x", who);
  if (!dt_ok(dtype)) return kk_failf("%s: dtype is KK_DTYPE_F32 or KK_DTYPE_BF16", who);
  if (ldx < C || ldo < C || xbs < (long long)L * ldx || obs < (long long)L * ldo) return kk_failf("%s: a pitch is smaller than what it spans", who);
  if (seg_rows != 0 && (seg_rows < 6 || seg_rows > (1 << 20))) return kk_failf("%s: seg_rows is 0 (chosen by shape) or 6 .. 2^20 rows", who);
  return bv_launch_amp_act(x, xbs, ldx, dtype, L, C, alpha, inv_beta, make_filters(), out, obs, ldo, seg_rows, B, (hipStream_t)stream);
}
