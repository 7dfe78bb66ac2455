// Parakeet (FastConformer), audio side (gfx950): the three hot blocks of the encoder that no other kernel of the library serves, on caller-owned
// buffers, and the encoder that composes them behind a handle (at the end of the file).  Restates mlx_audio/stt/models/parakeet/attention.py:52-137 (RelPositionMultiHeadAttention with its rel_shift) and conformer.py:46-90
// (Convolution), 146-271 (DwStridingSubsampling); DESIGN 8r.
//
// ---- relative-position attention (bf16, v_mfma_f32_16x16x32_bf16), HD = 64 or 128 ---------------------------------------------------------
//   softmax_j(scale ((q_i + u) . k_j + (q_i + v) . p_r)) v_j with r = T - 1 - i + j: what rel_shift's pad / reshape / slice selects from the
//   [T][2T - 1] matrix (q + v) p^T.  That matrix is never formed: a 64-query x 64-key tile reads only the BAND of p rows
//   T - 1 - (q0 + 63) + k0 .. T - 1 - q0 + k0 + 63 (127 rows), and inside it the 16 queries of a wave read a 79-row sub-band.
//   The frame is attention_long_kernel's (kk_whisper.hip): one workgroup = 64 queries of one (item, head), 4 waves of 16 queries, keys in tiles
//   of 64 through LDS, the next tile's global loads in flight while this one is computed, scores TRANSPOSED (S^T = K Q^T, query on lane & 15,
//   keys 16 c + 4 (lane >> 4) + r in register r of block c), online softmax in the log2 domain, the bf16 probabilities in place as the B operand
//   of O^T = V^T P^T, V transposed while it is staged.  New here:
//     - the wave holds two query fragments, bf16(q + u) and bf16(q + v): the sum in fp32, rounded once (the operand contract);
//     - the band moves by 64 rows per key tile, so it lives in LDS as two 64-row halves: half hh holds rows base0 + 64 hh .. + 63
//       (base0 = T - 1 - (q0 + 63), indices clamped into [0, 2T - 2]: a clamped row is only ever read for a masked key or an unstored query) in
//       slot hh & 1, tile `it` reads halves it and it + 1, and only half it + 1 is staged with tile it: the same traffic as the K tile;
//     - wave w's sub-band starts at band row 48 - 16 w.  Five products of 16 band rows (A, from LDS) against the q + v fragment (B) give
//       BD^T[band row 16 c5 + 4 g + r][query lr]; the lane writes its 20 values to the wave's own fp32 scratch [16][83] (row = query) and
//       reads back, for key c of the tile, column 15 - lr + c: the skew IS rel_shift.  The value lands in the register of the content score of
//       the same (query, key) and is added before the scale.  The odd pitch 83 keeps the skewed reads (82 lr + 4 g + const) on distinct banks
//       per half wave.  The scratch is private to a wave: the exchange needs a wave-level fence, not a workgroup barrier.
//   Keys >= T: score -inf by SELECT, V rows staged as zeros; K, p and q rows past T - 1 are never read (clamped), query rows >= T are not stored.
//   LDS: K [64][HD + 8] bf16, Vt [HD][68] bf16, band [128][HD + 8] bf16, scratch 4 x [16][83] fp32: 57 600 bytes at HD = 64, 90 880 at HD = 128.
//
// ---- Conformer conv core (fp32 arithmetic) -----------------------------------------------------------------------------------------------
//   out = silu(bn(dwconv_k(glu(x)))) over x = bf16 [B][T][2D], with BatchNorm folded into the fp32 taps and bias by the caller.  One workgroup =
//   64 time steps x 64 channels: glu(x) = x[:D] sigmoid(x[D:]) is applied ONCE per element while the 64 + k - 1 rows (zeros outside [0, T)) go
//   to LDS as fp32, the k x 64 taps go beside them; thread (pair, seg) then owns channels 2 pair, 2 pair + 1 and outputs 8 seg .. 8 seg + 7: it
//   keeps an 8-row register window of its channel pair, multiplies it by one tap, shifts it by one row and goes on.  An output is one fmaf chain from
//   the bias over the taps in index order.
//
// ---- 3 x 3 stride-2 pad-1 Conv2d over channels-last [B][T][F][C] ---------------------------------------------------------------------------
//   One kernel, two forms: the stem (1 -> C channels, fp32 input [B][T][F], ReLU) and the depth-wise form (C -> C, bf16 input, no activation).
//   A thread owns one output position and a channel pair: channels are the fastest index, so the nine tap reads of a wave are runs of 128 bytes
//   (depth-wise) or broadcasts (stem).  One fmaf chain from the bias over (ky, kx) in index order, taps outside the input skipped.  bf16 out.
#include "kk_host.h"
#include "../../include/kokoro_hip.h"

#include <math.h>

#include <type_traits>

namespace {
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------------------- relative-position attention
constexpr int AQ = 64, AK = 64, VLD = 68, SCR_LD = 83, SCR_WAVE = 16 * SCR_LD;

template <int HD>
struct RelAttnLds {
  static constexpr int KLD = HD + 8;  // 144- / 272-byte rows: the 16-byte fragment reads of 16 consecutive rows fall on distinct bank groups
  static constexpr size_t bytes = (size_t)(AK * KLD + HD * VLD + 2 * AK * KLD) * sizeof(bf16_t) + (size_t)4 * SCR_WAVE * sizeof(float);
};

template <int HD>
__global__ __launch_bounds__(256) void rel_pos_attention_kernel(const bf16_t* qkv, long long bs, int ld, const bf16_t* pos, int ldp, const float* bias_u,
                                                                const float* bias_v, int T, int heads, bf16_t* out, long long obs, int ldo) {
  constexpr int KLD = RelAttnLds<HD>::KLD, KS = HD / 32, U = HD / 64, DB = HD / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  bf16_t* Ks = (bf16_t*)lds_raw;        // [64][KLD]
  bf16_t* Vt = Ks + AK * KLD;           // [HD][VLD]
  bf16_t* Pb = Vt + HD * VLD;           // [2][64][KLD]: the band's two halves
  float* scr_all = (float*)(Pb + 2 * AK * KLD);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z, q0 = blockIdx.x * AQ;
  const int hs = heads * HD, t_hi = T - 1, p_hi = 2 * T - 2;
  const bf16_t* base = qkv + (long long)b * bs;
  float* scr = scr_all + wave * SCR_WAVE;

  // the wave's query fragments: B[k = d][col = query], lane (lr, g) holds d = 32 ks + 8 g .. + 7 of query lr, once with u and once with v added
  const int qrow = q0 + wave * 16 + lr;
  bf16x8 qu[KS], qv[KS];
  {
    const bf16_t* qp = base + (long long)(qrow < t_hi ? qrow : t_hi) * ld + h * HD + 8 * g;
    const float* up = bias_u + h * HD + 8 * g;
    const float* vp = bias_v + h * HD + 8 * g;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const bf16x8 q = *(const bf16x8*)(qp + 32 * ks);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float qf = (float)q[j];
        qu[ks][j] = (bf16_t)(qf + up[32 * ks + j]);
        qv[ks][j] = (bf16_t)(qf + vp[32 * ks + j]);
      }
    }
  }

  // staging: thread (kp, ch) moves 8 channels (chunk ch + 8 u) of rows 2 kp and 2 kp + 1 of K, of V and of a band half
  const int kp = tid >> 3, ch = tid & 7;
  const int base0 = T - 1 - (q0 + AQ - 1);  // unclamped p row of band row 0 of tile 0
  u32x4 kr0[U], kr1[U], vr0[U], vr1[U], pr0[U], pr1[U];
  // (every register array below is indexed by constants only: the loops over u are written out through for_u)
  auto for_u = [&](auto&& f) __attribute__((always_inline)) {
    f(std::integral_constant<int, 0>());
    if constexpr (U == 2) f(std::integral_constant<int, 1>());
  };
  auto load_band = [&](int hh) __attribute__((always_inline)) {
    int r0 = base0 + 64 * hh + 2 * kp, r1 = r0 + 1;
    r0 = r0 < 0 ? 0 : (r0 > p_hi ? p_hi : r0);
    r1 = r1 < 0 ? 0 : (r1 > p_hi ? p_hi : r1);
    const bf16_t* pb = pos + h * HD + ch * 8;
    for_u([&](auto uc) __attribute__((always_inline)) {
      constexpr int u = decltype(uc)::value;
      pr0[u] = *(const u32x4*)(pb + (long long)r0 * ldp + 64 * u);
      pr1[u] = *(const u32x4*)(pb + (long long)r1 * ldp + 64 * u);
    });
  };
  auto store_band = [&](int hh) __attribute__((always_inline)) {
    bf16_t* d = Pb + (hh & 1) * (AK * KLD) + (2 * kp) * KLD + ch * 8;
    for_u([&](auto uc) __attribute__((always_inline)) {
      constexpr int u = decltype(uc)::value;
      *(u32x4*)(d + 64 * u) = pr0[u];
      *(u32x4*)(d + KLD + 64 * u) = pr1[u];
    });
  };
  auto load_tile = [&](int k0) __attribute__((always_inline)) {
    const int r0 = k0 + 2 * kp < t_hi ? k0 + 2 * kp : t_hi, r1 = k0 + 2 * kp + 1 < t_hi ? k0 + 2 * kp + 1 : t_hi;
    const bf16_t* kb = base + hs + h * HD + ch * 8;
    for_u([&](auto uc) __attribute__((always_inline)) {
      constexpr int u = decltype(uc)::value;
      kr0[u] = *(const u32x4*)(kb + (long long)r0 * ld + 64 * u);
      kr1[u] = *(const u32x4*)(kb + (long long)r1 * ld + 64 * u);
      vr0[u] = *(const u32x4*)(kb + hs + (long long)r0 * ld + 64 * u);
      vr1[u] = *(const u32x4*)(kb + hs + (long long)r1 * ld + 64 * u);
    });
  };
  auto store_tile = [&](int k0) __attribute__((always_inline)) {
    const unsigned m0 = k0 + 2 * kp < T ? 0xFFFFFFFFu : 0u, m1 = k0 + 2 * kp + 1 < T ? 0xFFFFFFFFu : 0u;  // V rows past T: exact zeros
    for_u([&](auto uc) __attribute__((always_inline)) {
      constexpr int u = decltype(uc)::value;
      *(u32x4*)(Ks + (2 * kp) * KLD + ch * 8 + 64 * u) = kr0[u];
      *(u32x4*)(Ks + (2 * kp + 1) * KLD + ch * 8 + 64 * u) = kr1[u];
      const unsigned a[4] = {vr0[u].x & m0, vr0[u].y & m0, vr0[u].z & m0, vr0[u].w & m0};
      const unsigned c[4] = {vr1[u].x & m1, vr1[u].y & m1, vr1[u].z & m1, vr1[u].w & m1};
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        *(unsigned*)(Vt + (64 * u + ch * 8 + 2 * w) * VLD + 2 * kp) = (a[w] & 0xFFFFu) | (c[w] << 16);
        *(unsigned*)(Vt + (64 * u + ch * 8 + 2 * w + 1) * VLD + 2 * kp) = (a[w] >> 16) | (c[w] & 0xFFFF0000u);
      }
    });
  };

  float m = -1e30f, l = 0.f;  // running maximum (log2 domain) and this lane's share of the running sum, of query lr
  f32x4 o[DB];                // O^T[d = 16 db + 4 g + r][query lr]
#pragma unroll
  for (int db = 0; db < DB; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float sc = (HD == 64 ? 0.125f : 0.08838834764831845f) * 1.4426950408889634f;  // HD^-0.5 log2(e)
  const int ntile = (T + AK - 1) / AK;
  const int sb = 48 - 16 * wave;  // the wave's sub-band starts at this band row
  load_band(0);
  store_band(0);  // (the first barrier of the walk is ahead of its first reader)
  load_band(1);
  load_tile(0);
  for (int it = 0; it < ntile; ++it) {
    const int k0 = it * AK;
    __syncthreads();  // the previous tile's readers are done
    store_tile(k0);
    store_band(it + 1);
    __syncthreads();
    if (it + 1 < ntile) {  // lands while this tile is computed
      load_tile(k0 + AK);
      load_band(it + 2);
    }

    // positional term of the wave's sub-band: BD^T[band row sb + 16 c5 + 4 g + r][query lr]
#pragma unroll
    for (int c5 = 0; c5 < 5; ++c5) {
      const int e = sb + 16 * c5 + lr;  // band row of this lane's A row, 0 .. 127
      const bf16_t* band = Pb + ((it + (e >> 6)) & 1) * (AK * KLD) + (e & 63) * KLD + 8 * g;
      f32x4 bd = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) bd = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(band + 32 * ks), qv[ks], bd, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) scr[lr * SCR_LD + 16 * c5 + 4 * g + r] = bd[r];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    f32x4 s[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bf16_t* kf = Ks + (16 * c + lr) * KLD + 8 * g;
      s[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) s[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(kf + 32 * ks), qu[ks], s[c], 0, 0, 0);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * c + 4 * g + r;                    // of the tile
        const float bd = scr[lr * SCR_LD + 15 - lr + key];     // rel_shift: band row T - 1 - i + j of the sub-band
        const float t = k0 + key < T ? (s[c][r] + bd) * sc : -INFINITY;
        s[c][r] = t;
        mx = fmaxf(mx, t);
      }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the scratch is rewritten for the next tile only after these reads
    __builtin_amdgcn_wave_barrier();
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx);
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    m = mn;
    float ps = 0.f;
    bf16x8 pf[2];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f(s[c][r] - mn);
        ps += p;
        pf[c >> 1][(c & 1) * 4 + r] = (bf16_t)p;
      }
    l = l * alpha + ps;
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      o[db] *= alpha;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16_t* vp = Vt + (16 * db + lr) * VLD + 32 * ks + 4 * g;
        const bf16x4 v0 = *(const bf16x4*)vp, v1 = *(const bf16x4*)(vp + 16);
        const bf16x8 vf = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
        o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[ks], o[db], 0, 0, 0);
      }
    }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (qrow < T) {
    const float inv = 1.0f / l;
    bf16_t* op = out + (long long)b * obs + (long long)qrow * ldo + h * HD + 4 * g;
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      const bf16x4 w = {(bf16_t)(o[db][0] * inv), (bf16_t)(o[db][1] * inv), (bf16_t)(o[db][2] * inv), (bf16_t)(o[db][3] * inv)};
      *(bf16x4*)(op + 16 * db) = w;
    }
  }
}

template <int HD>
int launch_rel_pos_attention_hd(hipStream_t st, int B, const void* qkv, long long bs, int ld, const void* pos, int ldp, const float* u, const float* v, int T,
                                int heads, void* out, long long obs, int ldo) {
  static KKDevOnce once;  // more LDS than a kernel gets unasked (HD = 128); the limit is per device
  if (RelAttnLds<HD>::bytes > 65536 && once.first()) {
    if (hipFuncSetAttribute((const void*)rel_pos_attention_kernel<HD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RelAttnLds<HD>::bytes) != hipSuccess)
      return kk_fail("kk_op_rel_pos_attention: the kernel's LDS request was refused");
    once.done();
  }
  dim3 grid((T + AQ - 1) / AQ, heads, B);
  hipLaunchKernelGGL(rel_pos_attention_kernel<HD>, grid, dim3(256), RelAttnLds<HD>::bytes, st, (const bf16_t*)qkv, bs, ld, (const bf16_t*)pos, ldp, u, v, T,
                     heads, (bf16_t*)out, obs, ldo);
  KK_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------- Conformer conv core
constexpr int CT = 64, CC = 64, CK_MAX = 31, CSEG = 8;

__device__ static inline float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ __launch_bounds__(256) void conformer_dwconv_kernel(const bf16_t* x, long long bs, int ld, int T, int D, int k, const float* w, const float* bias,
                                                               bf16_t* out, long long obs, int ldo) {
  __shared__ float gl[(CT + CK_MAX - 1) * CC];  // glu(x), rows t0 - pad .. t0 + 63 + pad
  __shared__ float ws[CK_MAX * CC];             // taps [k][64]
  const int tid = threadIdx.x, pair = tid & 31, seg = tid >> 5;
  const int t0 = blockIdx.x * CT, c0 = blockIdx.y * CC, b = blockIdx.z;
  const int pad = (k - 1) / 2, rows = CT + k - 1;
  const int c = c0 + 2 * pair;  // this thread's channel pair, in every phase
  const bool live = c < D;      // (D is even: a pair is inside or outside)
  const bf16_t* xb = x + (long long)b * bs;
  for (int r = seg; r < rows; r += 8) {
    const int t = t0 - pad + r;
    float g0 = 0.f, g1 = 0.f;  // the conv's zero padding
    if (live && t >= 0 && t < T) {
      const bf16x2 a = *(const bf16x2*)(xb + (long long)t * ld + c), s = *(const bf16x2*)(xb + (long long)t * ld + D + c);
      g0 = (float)a[0] * sigmoid_f32((float)s[0]);
      g1 = (float)a[1] * sigmoid_f32((float)s[1]);
    }
    gl[r * CC + 2 * pair] = g0;
    gl[r * CC + 2 * pair + 1] = g1;
  }
  for (int j = seg; j < k; j += 8) {
    ws[j * CC + 2 * pair] = live ? w[(long long)j * D + c] : 0.f;
    ws[j * CC + 2 * pair + 1] = live ? w[(long long)j * D + c + 1] : 0.f;
  }
  __syncthreads();
  if (!live) return;
  const float b0 = bias[c], b1 = bias[c + 1];
  float a0[CSEG], a1[CSEG], w0[CSEG], w1[CSEG];  // accumulators and the register window: input rows CSEG seg + j + (0 .. 7) at tap j
  const float* gp = gl + (CSEG * seg) * CC + 2 * pair;
#pragma unroll
  for (int i = 0; i < CSEG; ++i) {
    a0[i] = b0;
    a1[i] = b1;
    w0[i] = gp[i * CC];
    w1[i] = gp[i * CC + 1];
  }
  for (int j = 0; j < k; ++j) {
    const float f0 = ws[j * CC + 2 * pair], f1 = ws[j * CC + 2 * pair + 1];
#pragma unroll
    for (int i = 0; i < CSEG; ++i) {
      a0[i] = __builtin_fmaf(f0, w0[i], a0[i]);
      a1[i] = __builtin_fmaf(f1, w1[i], a1[i]);
    }
#pragma unroll
    for (int i = 0; i + 1 < CSEG; ++i) {
      w0[i] = w0[i + 1];
      w1[i] = w1[i + 1];
    }
    if (j + 1 < k) {  // row CSEG seg + j + 8 <= 63 + k - 1: inside the staged rows
      w0[CSEG - 1] = gp[(j + CSEG) * CC];
      w1[CSEG - 1] = gp[(j + CSEG) * CC + 1];
    }
  }
  bf16_t* ob = out + (long long)b * obs;
#pragma unroll
  for (int i = 0; i < CSEG; ++i) {
    const int t = t0 + CSEG * seg + i;
    if (t < T) {
      const bf16x2 y = {(bf16_t)(a0[i] * sigmoid_f32(a0[i])), (bf16_t)(a1[i] * sigmoid_f32(a1[i]))};
      *(bf16x2*)(ob + (long long)t * ldo + c) = y;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------- 3 x 3 stride-2 Conv2d
// STEM: x fp32 [B][T][F], one input channel, ReLU.  Otherwise x bf16 [B][T][F][C], depth-wise, no activation.  w fp32 [9][C] (tap ky * 3 + kx).
template <bool STEM>
__global__ __launch_bounds__(256) void conv2d_s2_kernel(const void* x, int T, int F, int C, const float* w, const float* bias, bf16_t* out, int To, int Fo) {
  const int half = C >> 1;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)Fo * half) return;
  const int fo = (int)(idx / half), c = 2 * (int)(idx - (long long)fo * half), to = blockIdx.y, b = blockIdx.z;
  float a0 = bias[c], a1 = bias[c + 1];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int t = 2 * to - 1 + ky;
    if (t < 0 || t >= T) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int f = 2 * fo - 1 + kx;
      if (f < 0 || f >= F) continue;
      const long long pos = ((long long)b * T + t) * F + f;
      float v0, v1;
      if (STEM) {
        v0 = v1 = ((const float*)x)[pos];
      } else {
        const bf16x2 v = *(const bf16x2*)((const bf16_t*)x + pos * C + c);
        v0 = (float)v[0];
        v1 = (float)v[1];
      }
      a0 = __builtin_fmaf(w[(ky * 3 + kx) * C + c], v0, a0);
      a1 = __builtin_fmaf(w[(ky * 3 + kx) * C + c + 1], v1, a1);
    }
  }
  if (STEM) {
    a0 = fmaxf(a0, 0.f);
    a1 = fmaxf(a1, 0.f);
  }
  const bf16x2 y = {(bf16_t)a0, (bf16_t)a1};
  *(bf16x2*)(out + (((long long)b * To + to) * Fo + fo) * C + c) = y;
}
}  // namespace

extern "C" int kk_op_rel_pos_attention(void* stream, int B, const void* qkv, int ld, int T_rows, int T, int heads, int head_dim, const void* pos, int ldp,
                                       const float* pos_bias_u, const float* pos_bias_v, void* out, int ldo) {
  const char* who = "kk_op_rel_pos_attention";
  if (!qkv || !pos || !pos_bias_u || !pos_bias_v || !out) return kk_failf("%s: null argument", who);
  if (head_dim != 64 && head_dim != 128) return kk_failf("%s: head_dim = %d, the kernel is built for 64 and 128", who, head_dim);
  if (B < 1 || B > 65535 || heads < 1 || heads > 65535 || T < 1 || T > T_rows || T > (1 << 29))
    return kk_failf("%s: bad argument (need 1 <= B, heads <= 65535 and 1 <= T <= T_rows)", who);
  const int hs = heads * head_dim;
  if (ld < 3 * hs) return kk_failf("%s: ld is smaller than q | k | v of %d heads of %d channels", who, heads, head_dim);
  if (ldp < hs) return kk_failf("%s: ldp is smaller than %d heads of %d channels", who, heads, head_dim);
  if (ldo < hs) return kk_failf("%s: ldo is smaller than %d heads of %d channels", who, heads, head_dim);
  if (ld % 8 != 0 || ldp % 8 != 0 || ldo % 4 != 0 || ((uintptr_t)qkv & 15) || ((uintptr_t)pos & 15) || ((uintptr_t)out & 7))
    return kk_failf("%s: qkv and pos must be 16-byte aligned with ld %% 8 == 0 and ldp %% 8 == 0, out 8-byte aligned with ldo %% 4 == 0", who);
  const long long bs = (long long)T_rows * ld, obs = (long long)T_rows * ldo;
  return head_dim == 64 ? launch_rel_pos_attention_hd<64>((hipStream_t)stream, B, qkv, bs, ld, pos, ldp, pos_bias_u, pos_bias_v, T, heads, out, obs, ldo)
                        : launch_rel_pos_attention_hd<128>((hipStream_t)stream, B, qkv, bs, ld, pos, ldp, pos_bias_u, pos_bias_v, T, heads, out, obs, ldo);
}

extern "C" int kk_op_conformer_dwconv(void* stream, int B, const void* x, int ld, int T, int D, int k, const float* w, const float* bias, void* out, int ldo) {
  const char* who = "kk_op_conformer_dwconv";
  if (!x || !w || !bias || !out) return kk_failf("%s: null argument", who);
  if (B < 1 || B > 65535 || T < 1 || D < 2 || D % 2 != 0 || D > 65535 * CC) return kk_failf("%s: bad argument (need 1 <= B <= 65535, T >= 1 and an even D >= 2)", who);
  if (k < 1 || k > CK_MAX || k % 2 == 0) return kk_failf("%s: k = %d must be odd and <= %d", who, k, CK_MAX);
  if (ld < 2 * D || ldo < D || ld % 2 != 0 || ldo % 2 != 0 || ((uintptr_t)x & 3) || ((uintptr_t)out & 3))
    return kk_failf("%s: need ld >= 2 D and ldo >= D, both even, and 4-byte aligned buffers", who);
  hipLaunchKernelGGL(conformer_dwconv_kernel, dim3((T + CT - 1) / CT, (D + CC - 1) / CC, B), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                     (long long)T * ld, ld, T, D, k, w, bias, (bf16_t*)out, (long long)T * ldo, ldo);
  KK_CHECK_LAUNCH();
  return 0;
}

extern "C" int kk_op_conv2d_s2(void* stream, int B, const void* x, int stem, int T, int F, int C, const float* w, const float* bias, void* out) {
  const char* who = "kk_op_conv2d_s2";
  if (!x || !w || !bias || !out) return kk_failf("%s: null argument", who);
  if (B < 1 || B > 65535 || T < 1 || F < 1 || C < 2 || C % 2 != 0) return kk_failf("%s: bad argument (need 1 <= B <= 65535, T, F >= 1 and an even C >= 2)", who);
  const int To = (T - 1) / 2 + 1, Fo = (F - 1) / 2 + 1;
  if (To > 65535) return kk_failf("%s: T = %d is more than the launch grid holds", who, T);
  if (((uintptr_t)x & 3) || ((uintptr_t)out & 3)) return kk_failf("%s: x and out must be 4-byte aligned", who);
  const dim3 grid((unsigned)(((long long)Fo * (C / 2) + 255) / 256), To, B);
  if (stem)
    hipLaunchKernelGGL(conv2d_s2_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, T, F, C, w, bias, (bf16_t*)out, To, Fo);
  else
    hipLaunchKernelGGL(conv2d_s2_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, T, F, C, w, bias, (bf16_t*)out, To, Fo);
  KK_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------------------ encoder
// Conformer.__call__ (conformer.py:300-331) behind a handle, in the pattern of kk_whisper: the Linears and 1 x 1 convs on the bf16 MFMA conv kernel,
// LayerNorm on the fp32 residual stream, the three kernels above, and SiLU of the feed-forward hidden rows as a small in-place bf16 launch (the fallback to an
// activation in the shared conv epilogue).  The caller loads matrices in canonical form (mlx-audio_amd/parakeet.py folds BatchNorm, the feed-forward 1/2,
// xscaling and the (c, f) -> (f, c) column order of pre_encode.out in float64, and stacks q | k | v) and passes bf16(rel_positions(T')) to encode.
namespace {
__global__ __launch_bounds__(256) void silu_inplace_kernel(bf16_t* x, long long n2) {  // n2 pairs
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n2) return;
  bf16x2 v = *(bf16x2*)(x + 2 * i);
  const float a = (float)v[0], b = (float)v[1];
  v[0] = (bf16_t)(a * sigmoid_f32(a));
  v[1] = (bf16_t)(b * sigmoid_f32(b));
  *(bf16x2*)(x + 2 * i) = v;
}

struct PLin {  // bf16 [N][K] at `w` of wdev, fp32 bias [N] at `b` of fdev
  size_t w = 0, b = 0;
  int N = 0, K = 0;
};
struct PLayer {
  PLin ff1a, ff1b, qkv, pos, o, pw1, pw2, ff2a, ff2b;
  size_t ln[5][2], dw_w = 0, dw_b = 0, u = 0, v = 0;  // ln: ff1, att, conv, ff2, out
};
}  // namespace

struct kk_parakeet {
  kk_parakeet_config cfg;
  std::map<std::string, HostTensor> host;
  bool finalized = false;
  bf16_t* wdev = nullptr;
  float* fdev = nullptr;
  int n_sub = 0, f_out = 0;  // stride-2 stages, frequency bins after them
  size_t stem_w = 0, stem_b = 0;
  std::vector<size_t> sdw_w, sdw_b;
  std::vector<PLin> spw;
  PLin pre_out;
  std::vector<PLayer> layers;
};

extern "C" int kk_parakeet_create(const kk_parakeet_config* c, kk_parakeet** out) {
  const char* who = "kk_parakeet_create";
  if (!c || !out) return kk_failf("%s: null argument", who);
  if (c->n_layers < 1 || c->n_heads < 1 || c->feat_in < 1 || c->ff_expansion_factor < 1) return kk_failf("%s: bad dimensions", who);
  if (c->d_model % 128 != 0 || c->d_model > 2048) return kk_failf("%s: d_model must be a multiple of 128, at most 2048", who);
  if (c->d_model != 64 * c->n_heads && c->d_model != 128 * c->n_heads) return kk_failf("%s: the head dimension d_model / n_heads must be 64 or 128", who);
  if (c->subsampling_conv_channels < 128 || c->subsampling_conv_channels % 128 != 0) return kk_failf("%s: subsampling_conv_channels must be a multiple of 128", who);
  if (c->conv_kernel_size < 1 || c->conv_kernel_size > CK_MAX || c->conv_kernel_size % 2 == 0) return kk_failf("%s: conv_kernel_size must be odd and <= %d", who, CK_MAX);
  int n = 0;
  while ((1 << n) < c->subsampling_factor) ++n;
  if (n < 1 || (1 << n) != c->subsampling_factor) return kk_failf("%s: subsampling_factor must be a power of two >= 2", who);
  kk_parakeet* m = new kk_parakeet();
  m->cfg = *c;
  m->n_sub = n;
  m->f_out = c->feat_in;
  for (int i = 0; i < n; ++i) m->f_out = (m->f_out - 1) / 2 + 1;
  *out = m;
  return 0;
}

extern "C" void kk_parakeet_destroy(kk_parakeet* m) {
  if (!m) return;
  if (m->wdev) (void)hipFree(m->wdev);
  if (m->fdev) (void)hipFree(m->fdev);
  delete m;
}

extern "C" int kk_parakeet_load_tensor(kk_parakeet* m, const char* name, const int64_t* shape, int ndim, const float* data) {
  return kk_host_load_tensor("kk_parakeet_load_tensor", m ? &m->host : nullptr, m && m->finalized, name, shape, ndim, data);
}

extern "C" int kk_parakeet_finalize(kk_parakeet* m, void* stream) {
  const char* who = "kk_parakeet_finalize";
  if (!m) return kk_failf("%s: null model", who);
  if (m->finalized) return kk_failf("%s: already finalized", who);
  const kk_parakeet_config& c = m->cfg;
  const int D = c.d_model, Cc = c.subsampling_conv_channels, FF = D * c.ff_expansion_factor, k = c.conv_kernel_size;
  hipStream_t st = (hipStream_t)stream;
  std::string err;
  std::vector<uint16_t> wpack;
  std::vector<float> fpack;
  auto vec = [&](const std::string& name, int n) -> size_t {
    const size_t off = (fpack.size() + 63) & ~(size_t)63;
    fpack.resize(off + n, 0.f);
    if (const HostTensor* t = kk_host_want(m->host, name, {n}, err)) memcpy(&fpack[off], t->d.data(), (size_t)n * 4);
    return off;
  };
  auto mat = [&](const std::string& name, int a, int b) -> size_t {  // an fp32 matrix kept as it is
    const size_t off = (fpack.size() + 63) & ~(size_t)63;
    fpack.resize(off + (size_t)a * b, 0.f);
    if (const HostTensor* t = kk_host_want(m->host, name, {a, b}, err)) memcpy(&fpack[off], t->d.data(), (size_t)a * b * 4);
    return off;
  };
  auto lin = [&](const std::string& name, int N, int K) -> PLin {
    PLin l;
    l.N = N; l.K = K;
    l.w = (wpack.size() + 63) & ~(size_t)63;
    wpack.resize(l.w + (size_t)N * K, 0);
    if (const HostTensor* t = kk_host_want(m->host, name + ".w", {N, K}, err)) {
      for (size_t i = 0; i < (size_t)N * K; ++i) wpack[l.w + i] = f32_to_bf16_rne(t->d[i]);
      m->host.erase(name + ".w");
    }
    l.b = vec(name + ".b", N);
    return l;
  };
  m->stem_w = mat("pre.stem.w", 9, Cc);
  m->stem_b = vec("pre.stem.b", Cc);
  for (int i = 1; i < m->n_sub; ++i) {
    const std::string p = "pre." + std::to_string(i);
    m->sdw_w.push_back(mat(p + ".dw.w", 9, Cc));
    m->sdw_b.push_back(vec(p + ".dw.b", Cc));
    m->spw.push_back(lin(p + ".pw", Cc, Cc));
  }
  m->pre_out = lin("pre.out", D, m->f_out * Cc);
  m->layers.resize(c.n_layers);
  static const char* lnn[5] = {"ff1.ln", "att.ln", "conv.ln", "ff2.ln", "out.ln"};
  for (int li = 0; li < c.n_layers; ++li) {
    PLayer& L = m->layers[li];
    const std::string p = "L" + std::to_string(li) + ".";
    for (int j = 0; j < 5; ++j) {
      L.ln[j][0] = vec(p + lnn[j] + ".w", D);
      L.ln[j][1] = vec(p + lnn[j] + ".b", D);
    }
    L.ff1a = lin(p + "ff1.a", FF, D);
    L.ff1b = lin(p + "ff1.b", D, FF);
    L.qkv = lin(p + "qkv", 3 * D, D);
    L.pos = lin(p + "pos", D, D);
    L.o = lin(p + "o", D, D);
    L.u = vec(p + "u", D);
    L.v = vec(p + "v", D);
    L.pw1 = lin(p + "pw1", 2 * D, D);
    L.dw_w = mat(p + "dw.w", k, D);
    L.dw_b = vec(p + "dw.b", D);
    L.pw2 = lin(p + "pw2", D, D);
    L.ff2a = lin(p + "ff2.a", FF, D);
    L.ff2b = lin(p + "ff2.b", D, FF);
  }
  if (!err.empty()) return kk_failf("%s: %s", who, err.c_str());
  if (hipMalloc((void**)&m->wdev, wpack.size() * 2) != hipSuccess || hipMalloc((void**)&m->fdev, fpack.size() * 4) != hipSuccess)
    return kk_failf("%s: hipMalloc failed", who);
  if (hipMemcpyAsync(m->wdev, wpack.data(), wpack.size() * 2, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(m->fdev, fpack.data(), fpack.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return kk_failf("%s: upload failed", who);
  m->host.clear();
  m->finalized = true;
  return 0;
}

namespace {
struct PEncPlan {
  bf16_t *sa, *sb, *lnb, *qkv, *pb, *att, *h, *cv;
  float *x, *y;
  int T1, Tq;  // rows after the stem, after all stages
};
void plan_parakeet(const kk_parakeet& m, int B, int T_mel, Workspace& ws, PEncPlan& p) {
  const kk_parakeet_config& c = m.cfg;
  const size_t D = c.d_model, Cc = c.subsampling_conv_channels, FF = D * c.ff_expansion_factor;
  p.T1 = (T_mel - 1) / 2 + 1;
  p.Tq = T_mel;
  for (int i = 0; i < m.n_sub; ++i) p.Tq = (p.Tq - 1) / 2 + 1;
  const size_t F1 = (c.feat_in - 1) / 2 + 1, rows = (size_t)B * p.Tq;
  p.sa = (bf16_t*)ws.raw((size_t)B * p.T1 * F1 * Cc * 2);
  p.sb = (bf16_t*)ws.raw((size_t)B * p.T1 * F1 * Cc * 2);
  p.x = (float*)ws.raw(rows * D * 4);
  p.y = (float*)ws.raw(rows * D * 4);
  p.lnb = (bf16_t*)ws.raw(rows * D * 2);
  p.qkv = (bf16_t*)ws.raw(rows * 3 * D * 2);
  p.pb = (bf16_t*)ws.raw((size_t)(2 * p.Tq - 1) * D * 2);
  p.att = (bf16_t*)ws.raw(rows * D * 2);
  p.h = (bf16_t*)ws.raw(rows * (FF > 2 * D ? FF : 2 * D) * 2);
  p.cv = (bf16_t*)ws.raw(rows * D * 2);
}
}  // namespace

extern "C" int kk_parakeet_encode_frames(const kk_parakeet* m, int T_mel) {
  if (!m || T_mel < 1) return 0;
  for (int i = 0; i < m->n_sub; ++i) T_mel = (T_mel - 1) / 2 + 1;
  return T_mel;
}

extern "C" size_t kk_parakeet_encode_workspace_bytes(const kk_parakeet* m, int B, int T_mel) {
  if (!m || B < 1 || T_mel < 1) return 0;
  Workspace ws;
  PEncPlan p;
  plan_parakeet(*m, B, T_mel, ws, p);
  return ws.used + 256;
}

extern "C" int kk_parakeet_encode(kk_parakeet* m, void* stream, int B, int T_mel, const float* mel, const void* pos_emb, void* workspace,
                                  size_t workspace_bytes, float* out) {
  const char* who = "kk_parakeet_encode";
  if (!m || !mel || !pos_emb || !workspace || !out || B < 1 || B > 65535 || T_mel < 1 || T_mel > (1 << 20)) return kk_failf("%s: bad argument", who);
  if (!m->finalized) return kk_failf("%s: model not finalized", who);
  if (((uintptr_t)pos_emb & 15) || ((uintptr_t)mel & 3)) return kk_failf("%s: pos_emb must be 16-byte aligned and mel 4-byte aligned", who);
  const kk_parakeet_config& c = m->cfg;
  const int D = c.d_model, Cc = c.subsampling_conv_channels, FF = D * c.ff_expansion_factor, H = c.n_heads, k = c.conv_kernel_size;
  hipStream_t st = (hipStream_t)stream;
  Workspace ws;
  ws.base = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  ws.cap = workspace_bytes - (size_t)(ws.base - (char*)workspace);
  PEncPlan p;
  plan_parakeet(*m, B, T_mel, ws, p);
  if (ws.oom) return kk_failf("%s: workspace too small", who);
  const int T = p.Tq;

  // one Linear on the bf16 MFMA kernel over `items` items of `rows` dense rows: o = act(x W^T + bias) (+ res)
  auto linear = [&](const PLin& l, const bf16_t* x, int items, int rows, int act, const void* res, void* o, int out_dtype) -> int {
    KKMfmaArgs g;
    memset(&g, 0, sizeof g);
    g.x = x; g.xbs = (long long)rows * l.K; g.ldx = l.K; g.w = m->wdev + l.w; g.CinP = l.K; g.CoutP = l.N; g.Cin = l.K;
    g.bias = m->fdev + l.b; g.out = o; g.obs = (long long)rows * l.N; g.ldo = l.N; g.res = res; g.rbs = (long long)rows * l.N; g.ldr = l.N;
    g.Cout = l.N; g.Kw = 1; g.mode = KK_CONV; g.stride = 1; g.pad = 0; g.dil = 1; g.Q = rows; g.Lo_rows = rows;
    g.lin = KKLen{nullptr, 0, rows}; g.lout = KKLen{nullptr, 0, rows};
    g.in_slope = 1.0f; g.scale = 1.0f; g.act = act;  // (act_slope stays 0: KK_ACT_LRELU is ReLU)
    return kk_launch_conv_mfma(g, items, out_dtype, st);
  };
  auto ln = [&](const float* x, const size_t* wb, float* dst) -> int {
    KKLnArgs a;
    memset(&a, 0, sizeof a);
    a.x = x; a.xbs = (long long)T * D; a.ldx = D; a.out = dst; a.obs = a.xbs; a.ldo = D; a.C = D; a.Lmax = T;
    a.len = KKLen{nullptr, 0, T}; a.w = m->fdev + wb[0]; a.bias = m->fdev + wb[1]; a.eps = 1e-5f;
    return kk_launch_layernorm(a, B, KK_F32, st);
  };
  auto ln_bf16 = [&](const size_t* wb) -> int {  // LayerNorm of the fp32 stream, one rounding to bf16 for the matrix cores
    KK_TRY(ln(p.x, wb, p.y));
    return kk_launch_convert(p.y, KK_F32, (long long)T * D, D, p.lnb, KK_BF16, (long long)T * D, D, D, T, B, st);
  };
  auto feed_forward = [&](const size_t* wb, const PLin& a, const PLin& b) -> int {  // x += (1/2 folded) linear2(silu(linear1(ln(x))))
    KK_TRY(ln_bf16(wb));
    KK_TRY(linear(a, p.lnb, B, T, KK_ACT_NONE, nullptr, p.h, KK_BF16));
    const long long n2 = (long long)B * T * FF / 2;
    hipLaunchKernelGGL(silu_inplace_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, st, p.h, n2);
    KK_CHECK_LAUNCH();
    return linear(b, p.h, B, T, KK_ACT_NONE, p.x, p.x, KK_F32);
  };

  // pre_encode (conformer.py:240-271), channels-last throughout
  int Tc = T_mel, Fc = c.feat_in;
  KK_TRY(kk_op_conv2d_s2(stream, B, mel, 1, Tc, Fc, Cc, m->fdev + m->stem_w, m->fdev + m->stem_b, p.sa));
  Tc = (Tc - 1) / 2 + 1; Fc = (Fc - 1) / 2 + 1;
  for (int i = 0; i + 1 < m->n_sub; ++i) {
    KK_TRY(kk_op_conv2d_s2(stream, B, p.sa, 0, Tc, Fc, Cc, m->fdev + m->sdw_w[i], m->fdev + m->sdw_b[i], p.sb));
    Tc = (Tc - 1) / 2 + 1; Fc = (Fc - 1) / 2 + 1;
    KK_TRY(linear(m->spw[i], p.sb, B, Tc * Fc, KK_ACT_LRELU, nullptr, p.sa, KK_BF16));
  }
  KK_TRY(linear(m->pre_out, p.sa, B, T, KK_ACT_NONE, nullptr, p.x, KK_F32));  // rows of (f, c): the loader has permuted out's columns

  for (size_t li = 0; li < m->layers.size(); ++li) {  // conformer.py:126-143
    const PLayer& L = m->layers[li];
    KK_TRY(feed_forward(L.ln[0], L.ff1a, L.ff1b));
    KK_TRY(ln_bf16(L.ln[1]));
    KK_TRY(linear(L.qkv, p.lnb, B, T, KK_ACT_NONE, nullptr, p.qkv, KK_BF16));
    KK_TRY(linear(L.pos, (const bf16_t*)pos_emb, 1, 2 * T - 1, KK_ACT_NONE, nullptr, p.pb, KK_BF16));  // shared by all items
    KK_TRY(kk_op_rel_pos_attention(stream, B, p.qkv, 3 * D, T, T, H, D / H, p.pb, D, m->fdev + L.u, m->fdev + L.v, p.att, D));
    KK_TRY(linear(L.o, p.att, B, T, KK_ACT_NONE, p.x, p.x, KK_F32));
    KK_TRY(ln_bf16(L.ln[2]));
    KK_TRY(linear(L.pw1, p.lnb, B, T, KK_ACT_NONE, nullptr, p.h, KK_BF16));
    KK_TRY(kk_op_conformer_dwconv(stream, B, p.h, 2 * D, T, D, k, m->fdev + L.dw_w, m->fdev + L.dw_b, p.cv, D));
    KK_TRY(linear(L.pw2, p.cv, B, T, KK_ACT_NONE, p.x, p.x, KK_F32));
    KK_TRY(feed_forward(L.ln[3], L.ff2a, L.ff2b));
    float* dst = li + 1 == m->layers.size() ? out : p.y;  // norm_out: the last one straight into the caller's output
    KK_TRY(ln(p.x, L.ln[4], dst));
    if (dst == p.y) { float* t = p.x; p.x = p.y; p.y = t; }
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------------------ features
// parakeet/audio.py:38-70 (log_mel_spectrogram) with stft of mlx_audio/utils.py:52-101, in kk_op_log_mel's manner.
//   parakeet_logmel_frames_kernel: one workgroup of 320 threads per (frame, row).  The frame's `win` windowed samples go to LDS -- the window is zero
//   from `win` up to n_fft, so those samples are never read; the clip is reflect-padded by n_fft / 2 at both ends; samples in [n, n_pad) are pad_to's
//   pad_value -- thread k < n_fft / 2 + 1 walks them in index order with the twiddle cos / sin[(i k) mod n_fft] of the host's float64 table (four
//   interleaved fmaf chains per part, combined in a fixed order), |X|^2 goes back to LDS, thread m < features sums its filter column over the bins in
//   index order and stores log(. + 1e-5).
//   parakeet_logmel_finish_kernel: one workgroup per row.  Thread m owns feature m: sum and sum of squared deviations over the frames in index order,
//   in float64 (population variance, two passes); per feature these are the statistics, globally thread 0 adds the features' sums in index order.
//   Then (x - mean) / (std + 1e-5) in fp32, in place.  A row's bits depend on its own samples alone.
namespace {
constexpr int LM_NFFT_MAX = 512, LM_THREADS = 320;

__global__ __launch_bounds__(LM_THREADS) void parakeet_logmel_frames_kernel(const float* x, long long ldx, int n, int n_pad, float pad_value, int n_fft, int hop,
                                                                            int win, int features, const float* window, const float* cs, const float* fbT,
                                                                            float* out, int F) {
  __shared__ float fr[LM_NFFT_MAX];
  __shared__ float tc[LM_NFFT_MAX], ts[LM_NFFT_MAX];
  __shared__ float pw[LM_NFFT_MAX / 2 + 4];
  const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, nbin = n_fft / 2 + 1;
  const float* xb = x + (long long)b * ldx;
  for (int i = tid; i < n_fft; i += LM_THREADS) {
    tc[i] = cs[i];
    ts[i] = cs[n_fft + i];
  }
  for (int i = tid; i < win; i += LM_THREADS) {
    int j = f * hop + i - n_fft / 2;
    j = j < 0 ? -j : j;
    j = j >= n_pad ? 2 * (n_pad - 1) - j : j;  // (the host has checked n_pad > n_fft / 2: one reflection is enough, and j stays >= 0)
    fr[i] = (j < n ? xb[j] : pad_value) * window[i];
  }
  __syncthreads();
  if (tid < nbin) {
    const int k = tid;
    float re[4] = {0.f, 0.f, 0.f, 0.f}, im[4] = {0.f, 0.f, 0.f, 0.f};
    int idx = 0;  // (i k) mod n_fft
    for (int i = 0; i < win; i += 4) {  // win % 4 == 0
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float v = fr[i + u];
        re[u] = __builtin_fmaf(v, tc[idx], re[u]);
        im[u] = __builtin_fmaf(v, ts[idx], im[u]);
        idx += k;
        idx = idx >= n_fft ? idx - n_fft : idx;
      }
    }
    const float r = (re[0] + re[1]) + (re[2] + re[3]), q = (im[0] + im[1]) + (im[2] + im[3]);
    pw[k] = __builtin_fmaf(r, r, q * q);
  }
  __syncthreads();
  if (tid < features) {
    float acc = 0.f;
    for (int k = 0; k < nbin; ++k) acc = __builtin_fmaf(pw[k], fbT[k * features + tid], acc);
    out[((long long)b * F + f) * features + tid] = logf(acc + 1e-5f);
  }
}

__global__ __launch_bounds__(128) void parakeet_logmel_finish_kernel(float* out, int F, int features, int per_feature) {
  __shared__ double part[128];
  __shared__ double stat[2];
  const int b = blockIdx.x, m = threadIdx.x;
  float* ob = out + (long long)b * F * features;
  double s = 0.0;
  if (m < features)
    for (int f = 0; f < F; ++f) s += (double)ob[(long long)f * features + m];
  double mean = s / F;
  if (!per_feature) {
    part[m] = m < features ? s : 0.0;
    __syncthreads();
    if (m == 0) {
      double t = 0.0;
      for (int j = 0; j < features; ++j) t += part[j];
      stat[0] = t / ((double)F * features);
    }
    __syncthreads();
    mean = stat[0];
  }
  double q = 0.0;
  if (m < features)
    for (int f = 0; f < F; ++f) {
      const double d = (double)ob[(long long)f * features + m] - mean;
      q += d * d;
    }
  double var = q / F;
  if (!per_feature) {
    __syncthreads();
    part[m] = m < features ? q : 0.0;
    __syncthreads();
    if (m == 0) {
      double t = 0.0;
      for (int j = 0; j < features; ++j) t += part[j];
      stat[1] = t / ((double)F * features);
    }
    __syncthreads();
    var = stat[1];
  }
  if (m >= features) return;
  const float mu = (float)mean, den = (float)sqrt(var) + 1e-5f;
  for (int f = 0; f < F; ++f) {
    float* p = ob + (long long)f * features + m;
    *p = (*p - mu) / den;
  }
}
}  // namespace

extern "C" int kk_op_parakeet_log_mel(void* stream, int B, const float* x, long long ldx, int n, int pad_to, float pad_value, int n_fft, int hop, int win,
                                      int features, int per_feature, const float* window, const float* cos_sin, const float* fbT, float* out) {
  const char* who = "kk_op_parakeet_log_mel";
  if (!x || !window || !cos_sin || !fbT || !out) return kk_failf("%s: null argument", who);
  if (B < 1 || B > 65535 || n < 1 || ldx < n || pad_to < 0 || hop < 1) return kk_failf("%s: bad argument (need 1 <= B <= 65535, 1 <= n <= ldx, hop >= 1)", who);
  if (n_fft < 4 || n_fft > LM_NFFT_MAX || n_fft % 2 != 0) return kk_failf("%s: n_fft = %d must be even and <= %d", who, n_fft, LM_NFFT_MAX);
  if (win < 4 || win > n_fft || win % 4 != 0) return kk_failf("%s: win_length = %d must be a multiple of 4, at most n_fft", who, win);
  if (features < 1 || features > 128) return kk_failf("%s: features = %d must be in [1, 128]", who, features);
  const int n_pad = n < pad_to ? pad_to : n;
  if (n_pad <= n_fft / 2) return kk_failf("%s: %d samples are too few for the reflect padding of n_fft / 2 = %d", who, n_pad, n_fft / 2);
  if (n_pad > (1 << 30) || n_pad / hop + 1 > 0x7FFFFFF) return kk_failf("%s: the clip is too long", who);
  const int F = 1 + n_pad / hop;
  hipLaunchKernelGGL(parakeet_logmel_frames_kernel, dim3(F, B), dim3(LM_THREADS), 0, (hipStream_t)stream, x, ldx, n, n_pad, pad_value, n_fft, hop, win, features,
                     window, cos_sin, fbT, out, F);
  KK_CHECK_LAUNCH();
  hipLaunchKernelGGL(parakeet_logmel_finish_kernel, dim3(B), dim3(128), 0, (hipStream_t)stream, out, F, features, per_feature);
  KK_CHECK_LAUNCH();
  return 0;
}
