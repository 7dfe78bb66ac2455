// Whisper, text side (gfx950): the decode-step kernels and their raw kk_op_whisper_* entries.  The text decoder that launches them is the handle of
// kk_whisper_text.hip, through the "Whisper text side" block of kk_kernels.h.  Restates the arithmetic of TextDecoder (mlx_audio/stt/models/whisper/
// whisper.py:202-248, blocks :140-168, attention :90-137) and the token selection of decoding.py:255-395; DESIGN 8g.
//
// The invariant of every kernel here: a row's bits depend on that row's inputs alone -- not on how many rows a call carries, not on what the
// other rows hold.  Reduction orders are fixed, split results are merged in index order by a second launch, no floating-point atomics.
//
// ---- attn_rows: one query row against a bf16 K/V store -------------------------------------------------------------------------------------
//   grid (split, head, row), one wave per workgroup.  Lane (kg = lane >> 3, ch = lane & 7) owns channels 8 ch .. 8 ch + 7 of the keys
//   k0 + 8 j + kg, j = 0 .. 7, of a 64-key tile: eight lanes read one key's 128 contiguous bytes, a load instruction covers 8 whole rows, and
//   K / V go straight to registers (nothing is shared between waves, so LDS would be a detour).  The score is the lane's 8-term dot, summed over
//   the 8 lanes of the key by xor-butterflies (1, 2, 4: every lane ends with the same bits); the probability of a key lives in the very lanes
//   that hold the key's V chunk, so P V is a per-lane fma and the 8 key groups are summed once, at the end (xor 8, 16, 32).  Running maximum and
//   sum in fp32 in the log2 domain (scale 64^-0.5 and log2 e in one multiply after the dot, v_exp_f32).  A split covers ATTN_SPLIT keys; the
//   number of splits is a function of T_rows alone.  Keys >= len[r] are not read (a tile is cut at len, the lanes past it load nothing).
//   attn_merge: per (head, row), thread d combines the splits' (max, sum, acc[d]) in index order.
//
// ---- linear_rows: out[m] = act(x[m] W^T + bias) (+ res[m]), 1 <= M <= 16, W bf16 [N][K] dense ------------------------------------------------
//   v_mfma_f32_16x16x32_bf16 with A = x (the M rows are the 16-row side; rows >= M are zero fragments) and B = W: lane (lr, g) of B holds
//   W[n0 + lr][32 ks + 8 g .. + 7], which in row-major [N][K] is one 16-byte load -- the dense matrix IS the fragment order along k, so the
//   same copy serves this kernel, the bf16 MFMA convolution kernel (set_audio's K / V projections) and the embedding gather.  One workgroup
//   owns 16 output columns and reads their 16 x K weights exactly once for all M rows; its 16 waves take the k-steps ks = wave, wave + 16, ...
//   (together they read whole 1 KiB stretches of a row), loads go straight to registers, two k-steps in flight, and the sixteen partial tiles
//   are added through LDS in wave order.  (Measured, DESIGN 8g: with 4 waves the D x D Linears, 80 workgroups each, had too few loads in flight.)  x is fp32 and is rounded to bf16 (nearest even) as the A fragment is built.  Columns >= N (the vocabulary's tail) read a
//   clamped row and are not stored.  The result can be stored as fp32 rows and / or as bf16 into row rows[m] of a strided store (the step's
//   K and V land in the self-attention cache without a copy launch).
//
// ---- pick: the token selection of one decode step, one workgroup of 1024 threads per row -----------------------------------------------------
//   Two passes over the row's fp32 logits (L2 resident).  Pass A (timestamp mode only) takes, over the logits after every mask but the last rule's,
//   the log-sum-exp of the timestamp range and the maximum of the text range (decoding.py:381-394).  Pass B takes maximum, lowest arg-maximum and
//   sum of exponentials of the fully filtered logits, each thread online over its strided share, the shares combined by xor-butterflies and then
//   across the 16 waves in wave order.  Thread 0 updates the row's state.  The count of rows not yet ended is an integer atomic.  One body (pick_row) serves
//   the launch-wide kernel (one params, one bitmask) and the per-row kernel of row mode (each row its own; the row's state.ended is its flag).
//   The sampled form (temperature > 0) is the same body with one more branch in pass B: Gumbel-max on Philox uniforms beside the sum of
//   exponentials, so a sampled step reads the row's logits as often as a greedy one; a row's draws depend on (seed, its stream id, its history) alone.
//   The per-row kernel takes either form per block from the row's draw (PickDraw, set by kk_whisper_text_rows_set_draw), or the top-k form
//   for a row of a beam group.
#include "kk_host.h"
#include "kk_philox.h"
#include "../../include/kokoro_hip.h"

#include <math.h>

namespace {
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int ATTN_SPLIT = 128;   // keys per split
constexpr int ATTN_REC = 80;      // floats per split record: max, sum, pad to 16, acc[64]

__device__ __forceinline__ float bf_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(unsigned w) { return __uint_as_float(w & 0xFFFF0000u); }

// ---------------------------------------------------------------------------------------------------------------------------- attention
// OWNED: `item` is an owner table [row][T_rows] and key j of row r is read from item owner[r][j] -- a beam's keys stay in the physical rows
// that computed them.  The arithmetic is the direct form's, so a row's bits are those of a plain row holding the same keys.
template <bool OWNED>
__global__ __launch_bounds__(64) void attn_rows_kernel(const float* q, const bf16_t* kv, int k_off, int v_off, long long item_stride, int ld, int T_rows,
                                                       int items, const int* item, const int* len, int heads, float* scratch, int nsplit) {
  const int sp = blockIdx.x, h = blockIdx.y, r = blockIdx.z, lane = threadIdx.x, kg = lane >> 3, ch = lane & 7;
  int L = len[r];
  L = L < T_rows ? L : T_rows;
  int it = OWNED ? 0 : item[r];
  it = it < 0 ? 0 : (it >= items ? items - 1 : it);
  const int* own = item + (long long)r * T_rows;  // OWNED only
  float* rec = scratch + (((long long)r * heads + h) * nsplit + sp) * ATTN_REC;
  const int k_lo = sp * ATTN_SPLIT, k_hi = k_lo + ATTN_SPLIT < L ? k_lo + ATTN_SPLIT : L;
  if (k_lo >= k_hi) {  // (uniform) nothing of this row in the split
    if (lane == 0) { rec[0] = -INFINITY; rec[1] = 0.f; }
    rec[16 + lane] = 0.f;
    return;
  }
  const float* qp = q + ((long long)r * heads + h) * 64 + ch * 8;
  const float4 qa = *(const float4*)qp, qb = *(const float4*)(qp + 4);
  const bf16_t* base = kv + (long long)it * item_stride + h * 64 + ch * 8;
  const float sc = 0.125f * 1.4426950408889634f;  // 64^-0.5 log2(e)
  float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) acc[c] = 0.f;
  for (int k0 = k_lo; k0 < k_hi; k0 += 64) {
    uint4 kr[8], vr[8];
    int ow[8];
    if constexpr (OWNED) {  // the eight owners first: the K / V loads behind them are then in flight together
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int key = k0 + 8 * j + kg;
        const int o = key < k_hi ? own[key] : 0;
        ow[j] = o < 0 ? 0 : (o >= items ? items - 1 : o);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int key = k0 + 8 * j + kg;
      kr[j] = vr[j] = uint4{0u, 0u, 0u, 0u};
      if (key < k_hi) {
        const bf16_t* p = base + (long long)key * ld;
        if constexpr (OWNED) p += (long long)ow[j] * item_stride;
        kr[j] = *(const uint4*)(p + k_off);
        vr[j] = *(const uint4*)(p + v_off);
      }
    }
    float s[8], mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float d = qa.x * bf_lo(kr[j].x);
      d = __builtin_fmaf(qa.y, bf_hi(kr[j].x), d);
      d = __builtin_fmaf(qa.z, bf_lo(kr[j].y), d);
      d = __builtin_fmaf(qa.w, bf_hi(kr[j].y), d);
      d = __builtin_fmaf(qb.x, bf_lo(kr[j].z), d);
      d = __builtin_fmaf(qb.y, bf_hi(kr[j].z), d);
      d = __builtin_fmaf(qb.z, bf_lo(kr[j].w), d);
      d = __builtin_fmaf(qb.w, bf_hi(kr[j].w), d);
      d += __shfl_xor(d, 1);
      d += __shfl_xor(d, 2);
      d += __shfl_xor(d, 4);
      s[j] = k0 + 8 * j + kg < k_hi ? d * sc : -INFINITY;
      mx = fmaxf(mx, s[j]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 8));
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));  // finite: key k0 is below k_hi
    const float mn = fmaxf(m, mx);
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    m = mn;
    l *= alpha;
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] *= alpha;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float p = __builtin_amdgcn_exp2f(s[j] - mn);  // exactly 0 for a key past k_hi, whose V registers are zeros
      l += p;
      acc[0] = __builtin_fmaf(p, bf_lo(vr[j].x), acc[0]);
      acc[1] = __builtin_fmaf(p, bf_hi(vr[j].x), acc[1]);
      acc[2] = __builtin_fmaf(p, bf_lo(vr[j].y), acc[2]);
      acc[3] = __builtin_fmaf(p, bf_hi(vr[j].y), acc[3]);
      acc[4] = __builtin_fmaf(p, bf_lo(vr[j].z), acc[4]);
      acc[5] = __builtin_fmaf(p, bf_hi(vr[j].z), acc[5]);
      acc[6] = __builtin_fmaf(p, bf_lo(vr[j].w), acc[6]);
      acc[7] = __builtin_fmaf(p, bf_hi(vr[j].w), acc[7]);
    }
  }
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) {
    l += __shfl_xor(l, o);
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] += __shfl_xor(acc[c], o);
  }
  if (lane == 0) { rec[0] = m; rec[1] = l; }
  if (kg == 0) {
    *(float4*)(rec + 16 + ch * 8) = float4{acc[0], acc[1], acc[2], acc[3]};
    *(float4*)(rec + 16 + ch * 8 + 4) = float4{acc[4], acc[5], acc[6], acc[7]};
  }
}

__global__ __launch_bounds__(64) void attn_merge_kernel(const float* scratch, int nsplit, int heads, const int* len, float* out) {
  const int h = blockIdx.x, r = blockIdx.y, d = threadIdx.x;
  const float* rec = scratch + ((long long)r * heads + h) * nsplit * ATTN_REC;
  float* o = out + ((long long)r * heads + h) * 64 + d;
  if (len[r] < 1) {  // (the host entries refuse it; a row without keys has no softmax)
    *o = 0.f;
    return;
  }
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, rec[s * ATTN_REC]);
  float L = 0.f, a = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float w = __builtin_amdgcn_exp2f(rec[s * ATTN_REC] - M);  // 0 for an empty split
    L = __builtin_fmaf(rec[s * ATTN_REC + 1], w, L);
    a = __builtin_fmaf(rec[s * ATTN_REC + 16 + d], w, a);
  }
  *o = a / L;
}

inline int attn_nsplit(int T_rows) { return (T_rows + ATTN_SPLIT - 1) / ATTN_SPLIT; }

// ------------------------------------------------------------------------------------------------------------------------------- linear
constexpr int LIN_WAVES = 16;  // waves of a workgroup = slices of K, summed in wave order

// the end of a linear_rows workgroup (bf16 and quantised weights alike): the waves' partial tiles are added in wave order, then bias, GELU, residual
// and the fp32 / bf16 stores.  acc: the wave's D[m = 4 g + r][n = lr]
__device__ __forceinline__ void lin_finish(const KKLinRows& a, float (&red)[LIN_WAVES][16][17], const f32x4 acc, int n0) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, g = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) red[wave][4 * g + r][lr] = acc[r];
  __syncthreads();
  const int m = tid >> 4, c = tid & 15, n = n0 + c;
  if (tid >= 256 || m >= a.M || n >= a.N) return;
  float v = red[0][m][c];
#pragma unroll
  for (int w = 1; w < LIN_WAVES; ++w) v += red[w][m][c];
  if (a.bias) v += a.bias[n];
  if (a.act == KK_ACT_GELU) v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
  if (a.res) v += a.res[(long long)m * a.ldr + n];
  if (a.out) a.out[(long long)m * a.ldo + n] = v;
  if (a.ob) {
    const int row = a.rows ? a.rows[m] : m;
    if (row >= 0 && row < a.nrows) a.ob[(long long)row * a.ldb + n] = (bf16_t)v;
  }
}

__global__ __launch_bounds__(64 * LIN_WAVES) void linear_rows_kernel(KKLinRows a) {
  __shared__ float red[LIN_WAVES][16][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16, nsteps = a.K >> 5;
  const int nrow = n0 + lr < a.N ? n0 + lr : a.N - 1;  // the tail's columns read the last row; they are not stored
  const bf16_t* wp = a.w + (long long)nrow * a.K + 8 * g + wave * 32;
  const bool mvalid = lr < a.M;
  const float* xp = a.x + (long long)(mvalid ? lr : 0) * a.ldx + 8 * g + wave * 32;  // lanes past M read row 0 and SELECT zeros: the loop has no branch
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  auto frag = [&](const float4& a0, const float4& a1) __attribute__((always_inline)) {
    const bf16x8 xf = {(bf16_t)a0.x, (bf16_t)a0.y, (bf16_t)a0.z, (bf16_t)a0.w, (bf16_t)a1.x, (bf16_t)a1.y, (bf16_t)a1.z, (bf16_t)a1.w};
    return mvalid ? xf : zero;
  };
  const int mine = wave < nsteps ? (nsteps - wave + LIN_WAVES - 1) / LIN_WAVES : 0;  // k-steps wave, wave + LIN_WAVES, ...
  constexpr int STEP = 32 * LIN_WAVES;
  int i = 0;
  for (; i + 1 < mine; i += 2) {  // two k-steps' loads in flight before the first is used
    const bf16x8 w0 = *(const bf16x8*)(wp + i * STEP), w1 = *(const bf16x8*)(wp + (i + 1) * STEP);
    const float4 a0 = *(const float4*)(xp + i * STEP), a1 = *(const float4*)(xp + i * STEP + 4);
    const float4 b0 = *(const float4*)(xp + (i + 1) * STEP), b1 = *(const float4*)(xp + (i + 1) * STEP + 4);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(a0, a1), w0, acc, 0, 0, 0);  // D[m = 4 g + r][n = lr]
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(b0, b1), w1, acc, 0, 0, 0);
  }
  if (i < mine) {
    const bf16x8 w0 = *(const bf16x8*)(wp + i * STEP);
    const float4 a0 = *(const float4*)(xp + i * STEP), a1 = *(const float4*)(xp + i * STEP + 4);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(a0, a1), w0, acc, 0, 0, 0);
  }
  lin_finish(a, red, acc, n0);
}

// ---- linear_rows_q: the same Linear on the integers of an MLX affine-quantised matrix ------------------------------------------------
//   W is `words` uint32 [N][K bits / 32] (value i of a row in bits [(i % per) bits, ...) of word i / per, per = 32 / bits: the checkpoint's own
//   tensor) and `pairs` float2 [N][K / group] = (scale, bias) of the row's groups.  Row-major packing IS the fragment order along k, as for the
//   bf16 matrix: lane (lr, g) of k-step ks needs values 32 ks + 8 g .. + 7 of row n0 + lr, which are 8 bytes (BITS 8: a row is K / 4 words, the
//   lane's two at 8 ks + 2 g) or 4 bytes (BITS 4: K / 8 words, the lane's one at 4 ks + g), all in group 32 ks / group (group % 32 == 0).  Each
//   value becomes  bf16_rne(fp32(q) * scale + bias)  -- fp32 multiply, fp32 add, no contraction (wf_decode of kk_csm_gemvm.h) -- which is bit
//   for bit the element the bf16 copy of the dequantised matrix holds.  Everything else is linear_rows_kernel: the grid, the waves' k-steps, the
//   order of a wave's MFMAs, the reduction in wave order, the clamped tail row, the epilogue.  So the result carries the bf16 kernel's bits.
//   Two k-steps' words, pairs and x are requested before the first is decoded, as in the bf16 kernel.  The loads are narrower (4 or 8 bytes a lane
//   and step, plus the pair), but deeper did not pay: at width 1280 a wave has 2 or 3 k-steps, and what the launch adds over its bf16 twin is the
//   decode's vector arithmetic, not bytes in flight (DESIGN 8l has the figures).
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
template <int BITS> struct QWord;
template <> struct QWord<8> { typedef u32x2 T; };
template <> struct QWord<4> { typedef unsigned T; };
__device__ __forceinline__ __bf16 q_value(unsigned q, float2 sb) { return (__bf16)__fadd_rn(__fmul_rn((float)q, sb.x), sb.y); }
__device__ __forceinline__ bf16x8 q_decode(u32x2 q, float2 sb) {
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = q_value((q[j >> 2] >> (8 * (j & 3))) & 0xffu, sb);
  return v;
}
__device__ __forceinline__ bf16x8 q_decode(unsigned q, float2 sb) {
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = q_value((q >> (4 * j)) & 0xfu, sb);
  return v;
}

struct LinQ {
  const uint32_t* words;
  const float2* pairs;
  int gshift;  // log2(group / 32): k-step ks lies in group ks >> gshift
};

template <int BITS>
__global__ __launch_bounds__(64 * LIN_WAVES) void linear_rows_q_kernel(KKLinRows a, LinQ q) {
  typedef typename QWord<BITS>::T WQ;
  constexpr int WPS = BITS / 4;  // words of a lane per k-step
  constexpr int DEPTH = 2;       // k-steps in flight, as in the bf16 kernel (measured against 3 and 4)
  __shared__ float red[LIN_WAVES][16][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16, nsteps = a.K >> 5;
  const int nrow = n0 + lr < a.N ? n0 + lr : a.N - 1;  // the tail's columns read the last row; they are not stored
  const WQ* wp = (const WQ*)(q.words + (long long)nrow * (a.K / 32 * BITS)) + 4 * wave + g;  // k-step ks of the row: 4 ks + g, in units of WQ
  const float2* pp = q.pairs + (long long)nrow * (nsteps >> q.gshift);
  const bool mvalid = lr < a.M;
  const float* xp = a.x + (long long)(mvalid ? lr : 0) * a.ldx + 8 * g + wave * 32;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  auto frag = [&](const float4& a0, const float4& a1) __attribute__((always_inline)) {
    const bf16x8 xf = {(bf16_t)a0.x, (bf16_t)a0.y, (bf16_t)a0.z, (bf16_t)a0.w, (bf16_t)a1.x, (bf16_t)a1.y, (bf16_t)a1.z, (bf16_t)a1.w};
    return mvalid ? xf : zero;
  };
  const int mine = wave < nsteps ? (nsteps - wave + LIN_WAVES - 1) / LIN_WAVES : 0;  // k-steps wave, wave + LIN_WAVES, ...
  constexpr int STEP = 32 * LIN_WAVES, WSTEP = 4 * LIN_WAVES;
  static_assert(sizeof(WQ) == 4 * WPS, "a lane's share of a k-step");
  int i = 0;
  for (; i + DEPTH <= mine; i += DEPTH) {
    WQ w[DEPTH];
    float2 sb[DEPTH];
    float4 x0[DEPTH], x1[DEPTH];
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) {
      w[u] = wp[(i + u) * WSTEP];
      sb[u] = pp[(wave + (i + u) * LIN_WAVES) >> q.gshift];
      x0[u] = *(const float4*)(xp + (i + u) * STEP);
      x1[u] = *(const float4*)(xp + (i + u) * STEP + 4);
    }
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(x0[u], x1[u]), q_decode(w[u], sb[u]), acc, 0, 0, 0);  // in k order, as the bf16 kernel
  }
  for (; i < mine; ++i) {
    const WQ w = wp[i * WSTEP];
    const float2 sb = pp[(wave + i * LIN_WAVES) >> q.gshift];
    const float4 a0 = *(const float4*)(xp + i * STEP), a1 = *(const float4*)(xp + i * STEP + 4);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(a0, a1), q_decode(w, sb), acc, 0, 0, 0);
  }
  lin_finish(a, red, acc, n0);
}

inline int q_gshift(int group) { return group == 32 ? 0 : (group == 64 ? 1 : 2); }
// -------------------------------------------------------------------------------------------------------------------------------- embed
__global__ __launch_bounds__(256) void embed_kernel(const int* tok, const int* pos, const bf16_t* table, int n_vocab, const float* positions, int n_ctx, int D,
                                                    float* out) {
  const int r = blockIdx.x;
  int t = tok[r], p = pos[r];
  t = t < 0 ? 0 : (t >= n_vocab ? n_vocab - 1 : t);  // a bad id reads a row of the table, never past it
  p = p < 0 ? 0 : (p >= n_ctx ? n_ctx - 1 : p);
  const bf16_t* e = table + (long long)t * D;
  const float* pe = positions + (long long)p * D;
  for (int c = threadIdx.x; c < D; c += 256) out[(long long)r * D + c] = (float)e[c] + pe[c];
}

// the same gather from the quantised table (the layout of linear_rows_q): the row's values are decoded to the bf16 the dequantised table would hold
template <int BITS>
__global__ __launch_bounds__(256) void embed_q_kernel(const int* tok, const int* pos, const uint32_t* words, const float2* pairs, int group, int n_vocab,
                                                      const float* positions, int n_ctx, int D, float* out) {
  constexpr int PER = 32 / BITS;
  const int r = blockIdx.x;
  int t = tok[r], p = pos[r];
  t = t < 0 ? 0 : (t >= n_vocab ? n_vocab - 1 : t);  // a bad id reads a row of the table, never past it
  p = p < 0 ? 0 : (p >= n_ctx ? n_ctx - 1 : p);
  const uint32_t* e = words + (long long)t * (D / PER);
  const float2* sb = pairs + (long long)t * (D / group);
  const float* pe = positions + (long long)p * D;
  for (int c = threadIdx.x; c < D; c += 256)
    out[(long long)r * D + c] = (float)q_value((e[c / PER] >> (BITS * (c % PER))) & ((1u << BITS) - 1u), sb[c / group]) + pe[c];
}

// --------------------------------------------------------------------------------------------------------------------------------- pick
struct Osm {  // online softmax share: maximum, sum of exp(. - maximum), lowest index of the maximum
  float m, s;
  int i;
};
__device__ __forceinline__ void osm_add(Osm& a, float x, int i) {
  if (x == -INFINITY) return;
  if (x > a.m) {
    a.s = a.s * expf(a.m - x) + 1.0f;  // (a.m = -inf: 0 * 0 + 1)
    a.m = x;
    a.i = i;
  } else {
    a.s += expf(x - a.m);
  }
}
__device__ __forceinline__ Osm osm_merge(const Osm& a, const Osm& b) {  // symmetric in its bits: a butterfly leaves every lane with the same result
  if (b.m == -INFINITY) return a;
  if (a.m == -INFINITY) return b;
  Osm r;
  r.m = fmaxf(a.m, b.m);
  r.s = a.s * expf(a.m - r.m) + b.s * expf(b.m - r.m);
  r.i = a.m > b.m ? a.i : (b.m > a.m ? b.i : (a.i < b.i ? a.i : b.i));
  return r;
}
__device__ __forceinline__ Osm osm_block(Osm v, Osm* sh) {  // all 1024 threads; the result in every thread
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    Osm t;
    t.m = __shfl_xor(v.m, o);
    t.s = __shfl_xor(v.s, o);
    t.i = __shfl_xor(v.i, o);
    v = osm_merge(v, t);
  }
  __syncthreads();  // the previous use of sh is over
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  Osm r = sh[0];
  for (int w = 1; w < 16; ++w) r = osm_merge(r, sh[w]);
  return r;
}

// the beam's sizes, and a candidate of its top-k
constexpr int BEAM_C = KK_WHISPER_MAX_GROUP + 1;               // candidates a row offers, at most
constexpr int BEAM_N = KK_WHISPER_MAX_GROUP * BEAM_C;          // candidates of a window, at most
constexpr int BEAM_FIN = KK_WHISPER_BEAM_FIN;                  // finished sequences a window keeps, at most

struct Top {  // a candidate of the top-k: ordered by value descending, then id ascending; {-inf, -1}: none
  float v;
  int i;
};
__device__ __forceinline__ Top top_merge(const Top a, const Top b) {  // symmetric in its bits, as osm_merge is
  const bool take = b.v > a.v || (b.v == a.v && b.i >= 0 && (a.i < 0 || b.i < a.i));
  return Top{take ? b.v : a.v, take ? b.i : a.i};  // (field by field: a select between two structs goes through memory)
}
__device__ __forceinline__ Top top_block(Top v, Top* sh) {  // all 1024 threads; the result in every thread
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = top_merge(v, Top{__shfl_xor(v.v, o), __shfl_xor(v.i, o)});
  __syncthreads();  // the previous use of sh is over
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  Top r = sh[0];
  for (int w = 1; w < 16; ++w) r = top_merge(r, sh[w]);
  return r;
}

// (PickDraw, what a sampled pick adds to a row's arguments, lives in kk_kernels.h: the row mode keeps one per row)
// what the beam's top-k adds: the offers it writes (C pairs, descending) and the LDS of its block maximum
struct PickTop {
  int C;
  int32_t* token;
  float* logprob;
  Top* sh;
};
enum { PICK_GREEDY = 0, PICK_SAMPLE = 1, PICK_TOPK = 2 };

// The pick of ONE row by one workgroup: lg the row's logits, P its parameters, suppress its bitmask (or null), st its state, tokens its store of
// `cap` ids, next where its choice goes.  not_ended: the launch-wide counter, or null (the per-row form: the row's state.ended is its flag).
// SAMPLE: the token is drawn from softmax(l / T) over the filtered logits l by Gumbel-max in the same pass that takes the log-sum-exp of the
// UNTEMPERED l (decoding.py:263-270): token = argmax_i (l_i / T - log(-log u_i)), lowest index on ties, u_i = philox_open of word i & 3 of
// philox4(seed, stream << 32 | state.count, i >> 2).  A masked token gets no noise.  A row's draws depend on (seed, stream, its own history) alone.
// PICK_TOPK (the beam's offers): nothing is chosen and the state is only read.  The row's top.C best tokens over the same filtered logits go to
// top.token / top.logprob in descending order, equal logits by the lower id, never a masked one, unused slots -1: (token, l[token] - logsumexp(l)) on
// the log-sum-exp below, so the first offer is the greedy pick's token with its log-probability's bits.  Everything masked: (eot, 0) alone, as the greedy
// pick ends such a row; a dead row (sum -inf): nothing.  Each thread keeps its own best in registers in the pass that takes the log-sum-exp (its share is
// walked in rising id: a later equal stays behind), and top.C rounds of a block maximum over the threads' heads merge them.
template <int MODE>
__device__ __forceinline__ void pick_row(const float* lg, const kk_whisper_pick_params P, const uint32_t* suppress, kk_whisper_pick_state* st, int32_t* tokens,
                                         int cap, int32_t* next, int32_t* not_ended, Osm* sh, const PickDraw dr = PickDraw{0.f, 0, 0},
                                         const PickTop top = PickTop{0, nullptr, nullptr, nullptr}) {
  constexpr bool SAMPLE = MODE == PICK_SAMPLE, TOPK = MODE == PICK_TOPK;
  const int tid = threadIdx.x;
  const kk_whisper_pick_state S = *st;
  if constexpr (TOPK) {
    if (tid < top.C) {
      top.token[tid] = -1;
      top.logprob[tid] = -INFINITY;
    }
    if (S.sum_logprob == -INFINITY) return;  // (uniform) a dead slot
  }
  const int V = P.n_vocab, tb = P.timestamp_begin;
  const bool first = S.count == 0, ts = !P.without_timestamps;
  const bool last_ts = ts && S.count >= 1 && S.last >= tb, pen_ts = S.count < 2 || S.penultimate >= tb;
  const int ts_floor = S.last_timestamp >= tb ? (last_ts && !pen_ts ? S.last_timestamp : S.last_timestamp + 1) : tb;  // timestamps in [tb, ts_floor) are masked
  const int last_allowed = P.max_initial_timestamp_index >= 0 ? tb + P.max_initial_timestamp_index : V;
  auto pre = [&](int i, unsigned word) -> bool {  // SuppressBlank, SuppressTokens (word: the bitmask word of i)
    if (first && P.suppress_blank && (i == P.blank || i == P.eot)) return true;
    return (word >> (i & 31)) & 1u;
  };
  // a thread's share i = tid, tid + 1024, ... in that order, eight logits (and their bitmask words) requested before the first is used: the walk is
  // bound by the latency of its loads, not by their volume
  auto walk = [&](auto&& f) __attribute__((always_inline)) {
    for (int base = tid; base < V; base += 8 * 1024) {
      float x[8];
      unsigned w[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = base + 1024 * u;
        x[u] = i < V ? lg[i] : -INFINITY;
        w[u] = i < V && suppress ? suppress[i >> 5] : 0u;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (base + 1024 * u < V) f(base + 1024 * u, x[u], w[u]);
    }
  };
  auto rules = [&](int i) -> bool {  // ApplyTimestampRules, all but its last rule
    if (i == P.no_timestamps) return true;
    if (last_ts && (pen_ts ? i >= tb : i < P.eot)) return true;
    if (i >= tb && i < ts_floor) return true;
    if (first && (i < tb || i > last_allowed)) return true;
    return false;
  };
  bool mass = false;
  if (ts) {  // decoding.py:381-394, taken AFTER the masks above as OpenAI's original does (on the logits the filter was handed, a row can lose every token)
    Osm t = {-INFINITY, 0.f, 0};
    float mt = -INFINITY;
    walk([&](int i, float v, unsigned word) {
      const float x = pre(i, word) || rules(i) ? -INFINITY : v;
      if (i >= tb) osm_add(t, x, i);
      else mt = fmaxf(mt, x);
    });
    t = osm_block(t, sh);
    Osm u = {mt, 1.f, 0};
    u = osm_block(u, sh);
    mass = t.m != -INFINITY && t.m + logf(t.s) > u.m;
  }
  Osm f = {-INFINITY, 0.f, 0}, best = {-INFINITY, 1.f, 0};  // best (SAMPLE): the highest noisy score of the share and its lowest index
  const uint64_t ctr = ((uint64_t)dr.stream << 32) | (uint32_t)S.count;
  constexpr int NT = TOPK ? BEAM_C : 1;
  float tv[NT];  // (TOPK) the share's best, descending
  int ti[NT];
#pragma unroll
  for (int u = 0; u < NT; ++u) {
    tv[u] = -INFINITY;
    ti[u] = -1;
  }
  walk([&](int i, float v, unsigned word) {
    const bool masked = pre(i, word) || (ts && (rules(i) || (mass && i < tb)));
    osm_add(f, masked ? -INFINITY : v, i);
    if constexpr (TOPK) {
      if (!masked && v > tv[NT - 1]) {  // (never a NaN or -inf logit)
        tv[NT - 1] = v;
        ti[NT - 1] = i;
#pragma unroll
        for (int u = NT - 1; u > 0; --u) {
          const bool up = tv[u] > tv[u - 1];
          const float xv = tv[u];
          const int xi = ti[u];
          tv[u] = up ? tv[u - 1] : xv;
          ti[u] = up ? ti[u - 1] : xi;
          tv[u - 1] = up ? xv : tv[u - 1];
          ti[u - 1] = up ? xi : ti[u - 1];
        }
      }
    }
    if constexpr (SAMPLE) {
      if (!masked && v != -INFINITY) {
        uint32_t r[4];
        philox4(dr.seed, ctr, (uint32_t)i >> 2, r);
        const int k = i & 3;
        const float u = philox_open(k == 0 ? r[0] : (k == 1 ? r[1] : (k == 2 ? r[2] : r[3])));
        const float score = v * dr.inv_t - logf(-logf(u));
        if (score > best.m) {  // the share is walked in rising i: the first of equal scores stays
          best.m = score;
          best.i = i;
        }
      }
    }
  });
  f = osm_block(f, sh);  // (TOPK: its barriers order the stores of -1 above before thread 0's below)
  if constexpr (SAMPLE) best = osm_block(best, sh);  // (.s rides along unused, as in the text maximum above)
  if constexpr (TOPK) {
    if (f.m == -INFINITY) {  // everything masked
      if (tid == 0) {
        top.token[0] = P.eot;
        top.logprob[0] = 0.f;
      }
      return;
    }
    const float lse = f.m + logf(f.s);
    for (int k = 0; k < top.C; ++k) {
      const Top t = top_block(Top{tv[0], ti[0]}, top.sh);
      if (t.i < 0) break;  // (uniform) fewer than C unmasked tokens
      if (t.i == ti[0]) {  // the winner's thread moves on to its next
#pragma unroll
        for (int u = 0; u + 1 < NT; ++u) {
          tv[u] = tv[u + 1];
          ti[u] = ti[u + 1];
        }
        tv[NT - 1] = -INFINITY;
        ti[NT - 1] = -1;
      }
      if (tid == 0) {
        top.token[k] = t.i;
        top.logprob[k] = t.v - lse;
      }
    }
    return;
  }
  if (tid != 0) return;
  kk_whisper_pick_state N = S;
  int tok = SAMPLE ? best.i : f.i;
  float lp = 0.f;
  if (f.m == -INFINITY) tok = P.eot;  // everything masked: end the row
  else lp = lg[tok] - (f.m + logf(f.s));
  if (S.ended) tok = P.eot;  // decoding.py:273-274
  else N.sum_logprob = S.sum_logprob + lp;  // :271
  if (S.count < cap) tokens[S.count] = tok;
  *next = tok;
  if (!S.ended && tok == P.eot) {
    N.ended = 1;
    if (not_ended) atomicSub(not_ended, 1);
  }
  N.penultimate = S.last;
  N.last = tok;
  if (tok >= tb) N.last_timestamp = tok;
  N.last_logprob = lp;
  N.count = S.count + 1;
  *st = N;
}

// launch-wide: block b is row b, ONE params and ONE bitmask for the launch
__global__ __launch_bounds__(1024) void pick_kernel(const float* logits, long long ldl, const kk_whisper_pick_params* params, const uint32_t* suppress,
                                                    kk_whisper_pick_state* state, int32_t* tokens, int cap, int32_t* next, int32_t* not_ended) {
  __shared__ Osm sh[16];
  const int b = blockIdx.x;
  pick_row<PICK_GREEDY>(logits + (long long)b * ldl, *params, suppress, state + b, tokens + (long long)b * cap, cap, next + b, not_ended, sh);
}

// launch-wide, sampled: row b draws on its stream id streams[b]
__global__ __launch_bounds__(1024) void pick_sampled_kernel(const float* logits, long long ldl, const kk_whisper_pick_params* params, const uint32_t* suppress,
                                                            float inv_t, uint64_t seed, const uint32_t* streams, kk_whisper_pick_state* state, int32_t* tokens,
                                                            int cap, int32_t* next, int32_t* not_ended) {
  __shared__ Osm sh[16];
  const int b = blockIdx.x;
  pick_row<PICK_SAMPLE>(logits + (long long)b * ldl, *params, suppress, state + b, tokens + (long long)b * cap, cap, next + b, not_ended, sh,
                 PickDraw{inv_t, seed, streams[b]});
}

// per-row: block j picks for decoder row sel.row[j] on logits row sel.logit[j], with that row's params, bitmask (`words` words each), draw, state and
// store.  A row whose draw has inv_t > 0 samples (the bits of pick_sampled_kernel), every other row picks greedily (the bits of pick_kernel); the
// branch is uniform over the block, so each block runs one of the two bodies and the barriers inside them are met by all its threads.
__global__ __launch_bounds__(1024) void pick_rows_kernel(KKPickSel sel, const float* logits, long long ldl, const kk_whisper_pick_params* params,
                                                         const uint32_t* suppress, int words, const PickDraw* draws, kk_whisper_pick_state* state, int32_t* tokens,
                                                         int cap, int32_t* next, int32_t* cand_token, float* cand_logprob) {
  __shared__ Osm sh[16];
  __shared__ Top sht[16];
  const int r = sel.row[blockIdx.x], C = sel.topk[blockIdx.x];
  const float* lg = logits + (long long)sel.logit[blockIdx.x] * ldl;
  const PickDraw dr = draws[r];
  if (C > 0)  // a row of a beam group: its C best tokens (the bits of beam_topk_kernel) for the select launch behind this one
    pick_row<PICK_TOPK>(lg, params[r], suppress + (long long)r * words, state + r, nullptr, 0, nullptr, nullptr, sh, PickDraw{0.f, 0, 0},
                        PickTop{C, cand_token + (long long)r * BEAM_C, cand_logprob + (long long)r * BEAM_C, sht});
  else if (dr.inv_t > 0.f)
    pick_row<PICK_SAMPLE>(lg, params[r], suppress + (long long)r * words, state + r, tokens + (long long)r * cap, cap, next + r, nullptr, sh, dr);
  else
    pick_row<PICK_GREEDY>(lg, params[r], suppress + (long long)r * words, state + r, tokens + (long long)r * cap, cap, next + r, nullptr, sh);
}

__global__ void pick_reset_kernel(kk_whisper_pick_state* state, int B, int32_t* not_ended) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) state[b] = kk_whisper_pick_state{-1, -1, -1, 0, 0, 0.f, 0.f, 0};
  if (b == 0) *not_ended = B;
}

// ---------------------------------------------------------------------------------------------------------------------------------- beam
// One beam step behind a forward is two launches.  beam_topk: one workgroup per row, the pick's filters and the pick's log-sum-exp, and
// the row's K + 1 best tokens.  beam_select: one workgroup per window orders the window's at most K (K + 1) candidates, walks them as OpenAI's
// BeamSearchDecoder.update does, and writes the next live rows: parent, token, sum, pick state, owner table, and what finished.
// the beam's offers: block b is row b, ONE params and ONE bitmask for the launch; cand_token / cand_logprob [B][C]
__global__ __launch_bounds__(1024) void beam_topk_kernel(const float* logits, long long ldl, const kk_whisper_pick_params* params, const uint32_t* suppress,
                                                         const kk_whisper_pick_state* state, int C, int32_t* cand_token, float* cand_logprob) {
  __shared__ Osm sh[16];
  __shared__ Top sht[16];
  const int b = blockIdx.x;
  pick_row<PICK_TOPK>(logits + (long long)b * ldl, *params, suppress, const_cast<kk_whisper_pick_state*>(state + b), nullptr, 0, nullptr, nullptr, sh,
                      PickDraw{0.f, 0, 0}, PickTop{C, cand_token + (long long)b * C, cand_logprob + (long long)b * C, sht});
}

// owner[0][b][p] = b, nothing finished, every window incomplete
__global__ void beam_reset_kernel(kk_whisper_beam_bufs b) {
  const int B = b.n_audio * b.beam_size, n = B * b.n_ctx;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) b.owner[0][e] = e / b.n_ctx;
  if (blockIdx.x == 0) {
    for (int w = threadIdx.x; w < b.n_audio; w += blockDim.x) {
      b.fin_count[w] = 0;
      b.complete[w] = 0;
    }
    if (threadIdx.x == 0) *b.not_complete = b.n_audio;
  }
}

// What one select works on: a window of window mode (rows w K .. w K + K - 1) or a beam group of row mode (any K rows).  The K rows are
// named by SLOT through s_row (LDS, filled by the kernel): slots order the candidates and the next prefixes, while the owner tables, the parent
// pointers and every token lookup name physical rows.  The arrays are indexed by physical row; the finished stores are this window's own.
struct BeamView {
  int K, T, cap, max_candidates, pos;  // rows; positions of an owner row; ids of a token row; finished sequences kept; positions the parents hold
  int cstride;                         // offers per row in cand_token / cand_logprob
  const int32_t* cand_token;
  const float* cand_logprob;
  const int32_t* own_old;
  int32_t *own_new, *parent;
  float* fin_score;
  int32_t *fin_length, *fin_tokens, *fin_count, *complete, *not_complete;  // not_complete: the launch-wide counter, or null
  const kk_whisper_pick_params* params;
  kk_whisper_pick_state* state;
  int32_t *tokens, *next;
  bool flag_rows;  // row mode: the rows' state.ended carries the group's complete flag (the poll reads it with the plain rows' flags)
};

// OpenAI's BeamSearchDecoder.update on one window, by one workgroup of 256 threads; the parents hold v.pos positions, v.own_old is read, v.own_new written.
// The walk's order is total -- score descending, parent slot ascending, rank within the parent ascending -- so every thread computes its candidate's
// place by counting, and thread 0 walks the sorted list.
__device__ __forceinline__ void beam_select_body(const BeamView& v, const int* s_row) {
  __shared__ kk_whisper_pick_state par[KK_WHISPER_MAX_GROUP];
  __shared__ float c_score[BEAM_N], c_lp[BEAM_N];
  __shared__ int c_tok[BEAM_N], order[BEAM_N];
  __shared__ int s_cand[KK_WHISPER_MAX_GROUP], f_cand[BEAM_FIN], f_slot[BEAM_FIN], n_new, s_done;
  const int tid = threadIdx.x, K = v.K, C = K + 1, n = K * C, T = v.T, cap = v.cap, pos = v.pos;
  const int eot = v.params->eot, tb = v.params->timestamp_begin;
  const int32_t* own_old = v.own_old;
  int32_t* own_new = v.own_new;
  kk_whisper_pick_state* state = v.state;
  int32_t *tokens = v.tokens, *next = v.next;
  __syncthreads();  // s_row is filled
  if (tid < K) par[tid] = state[s_row[tid]];
  if (tid < n) order[tid] = -1;
  __syncthreads();
  const int count = par[0].count;  // the rows of a window step together
  if (tid < n) {
    const int j = tid / C;
    const long long at = (long long)s_row[j] * v.cstride + (tid - j * C);
    const int t = v.cand_token[at];
    const float lp = v.cand_logprob[at];
    const float s = par[j].sum_logprob + lp;
    // at the first sampled position the rows of a window are one prefix: slot 0 offers for all
    const bool valid = t >= 0 && (count > 0 || j == 0) && par[j].sum_logprob != -INFINITY && s == s;
    c_tok[tid] = valid ? t : -1;
    c_score[tid] = valid ? s : -INFINITY;
    c_lp[tid] = lp;
  }
  __syncthreads();
  if (tid < n) {
    const bool mv = c_tok[tid] >= 0;
    const float ms = c_score[tid];
    int place = 0;
    for (int u = 0; u < n; ++u) {
      const bool uv = c_tok[u] >= 0;
      const float us = c_score[u];
      place += uv != mv ? uv : (uv && us != ms ? us > ms : u < tid);  // valid ones first, by score, then by (parent, rank) = the index
    }
    order[place] = tid;
  }
  __syncthreads();
  if (tid == 0) {
    int saved = 0, nf = 0, fc = *v.fin_count;
    fc = fc < 0 ? 0 : fc;  // (a store that was never reset: nothing is written outside it)
    for (int idx = 0; idx < n && saved < K; ++idx) {
      const int c = order[idx];
      if (c < 0 || c_tok[c] < 0) break;  // the offers are used up
      if (c_tok[c] != eot) {
        s_cand[saved++] = c;
      } else if (fc < v.max_candidates && nf < BEAM_FIN) {  // finished, in descending score, while there is room
        f_cand[nf] = c;
        f_slot[nf++] = fc++;
      }
    }
    for (int k = saved; k < K; ++k) s_cand[k] = -1;  // dead slots
    n_new = nf;
    *v.fin_count = fc;
    if (fc >= v.max_candidates && !*v.complete) {
      *v.complete = 1;
      if (v.not_complete) atomicSub(v.not_complete, 1);
    }
    s_done = fc >= v.max_candidates;
  }
  __syncthreads();
  if (tid < K) {  // the child's pick state from the PARENT's
    const int c = s_cand[tid], row = s_row[tid];
    kk_whisper_pick_state N = par[c >= 0 ? c / C : tid];
    int tok = eot;
    if (c >= 0) {
      tok = c_tok[c];
      N.sum_logprob = c_score[c];
      N.last_logprob = c_lp[c];
      if (tok >= tb) N.last_timestamp = tok;
    } else {
      N.sum_logprob = -INFINITY;
      N.last_logprob = 0.f;
    }
    N.penultimate = N.last;
    N.last = tok;
    N.ended = v.flag_rows ? s_done : 0;
    N.count = count + 1;
    state[row] = N;
    next[row] = tok;
    v.parent[row] = c >= 0 ? s_row[c / C] : -1;
    if (count >= 0 && count < cap) tokens[(long long)row * cap + count] = tok;
  }
  auto owner_of = [&](int row, int p) -> int {  // the physical row that holds position p of `row`, kept inside the window whatever the table holds
    const int o = p >= 0 && p < T ? own_old[(long long)row * T + p] : row;
    bool inside = false;
    for (int k = 0; k < K; ++k) inside = inside || o == s_row[k];
    return inside ? o : row;
  };
  for (int e = tid; e < K * T; e += 256) {  // what the parent has is inherited; the positions from `pos` on are the row's own
    const int k = e / T, p = e - k * T, c = s_cand[k];
    own_new[(long long)s_row[k] * T + p] = c >= 0 && p < pos ? owner_of(s_row[c / C], p) : s_row[k];
  }
  const int len = count < 0 ? 0 : (count < cap ? count : cap);
  for (int f = 0; f < n_new; ++f) {  // the finished sequences, materialised now: their rows are overwritten from the next step on
    const int c = f_cand[f], prow = s_row[c / C];
    int32_t* dst = v.fin_tokens + (long long)f_slot[f] * cap;
    for (int i = tid; i < len; i += 256) dst[i] = tokens[(long long)owner_of(prow, pos - count + i) * cap + i];
    if (tid == 0) {
      v.fin_score[f_slot[f]] = c_score[c];
      v.fin_length[f_slot[f]] = len;
    }
  }
}

// window mode: window w = blockIdx.x, rows w K .. w K + K - 1; owner tables: b.owner[flip] is read, b.owner[flip ^ 1] written
__global__ __launch_bounds__(256) void beam_select_kernel(kk_whisper_beam_bufs b, int flip, int pos, const kk_whisper_pick_params* params, kk_whisper_pick_state* state,
                                                          int32_t* tokens, int32_t* next) {
  __shared__ int s_row[KK_WHISPER_MAX_GROUP];
  const int w = blockIdx.x, K = b.beam_size;
  if (threadIdx.x < K) s_row[threadIdx.x] = w * K + threadIdx.x;
  const long long f0 = (long long)w * b.max_candidates;
  const BeamView v{K, b.n_ctx, b.cap, b.max_candidates, pos, K + 1, b.cand_token, b.cand_logprob, b.owner[flip & 1], b.owner[(flip & 1) ^ 1], b.parent,
                   b.fin_score + f0, b.fin_length + f0, b.fin_tokens + f0 * b.cap, b.fin_count + w, b.complete + w, b.not_complete, params, state, tokens, next, false};
  beam_select_body(v, s_row);
}

// row mode: block j is the beam group led by decoder row sel.leader[j], its rows by slot in sel.rows[j], at ITS position and flip; the group's params
// are its leader's, its finished stores (BEAM_FIN sequences of T ids) are indexed by the leader row
__global__ __launch_bounds__(256) void rows_select_kernel(KKGroupSel sel, KKGroupBufs g, int T, const kk_whisper_pick_params* params, kk_whisper_pick_state* state,
                                                          int32_t* tokens, int32_t* next) {
  __shared__ int s_row[KK_WHISPER_MAX_GROUP];
  const int j = blockIdx.x, K = sel.K[j], lead = sel.leader[j], flip = sel.flip[j] & 1;
  if (threadIdx.x < K) s_row[threadIdx.x] = sel.rows[j][threadIdx.x];
  const long long f0 = (long long)lead * BEAM_FIN;
  const BeamView v{K, T, T, sel.max_candidates[j], sel.pos[j], BEAM_C, g.cand_token, g.cand_logprob, flip ? g.owner[1] : g.owner[0], flip ? g.owner[0] : g.owner[1],
                   g.parent, g.fin_score + f0, g.fin_length + f0, g.fin_tokens + f0 * T, g.fin_count + lead, g.complete + lead, nullptr, params + lead, state, tokens,
                   next, true};
  beam_select_body(v, s_row);
}

// a beam group's admission (one block): owner[0] of its K rows is identity, nothing finished, not complete
__global__ __launch_bounds__(256) void rows_group_reset_kernel(KKGroupRows rows, int K, int T, KKGroupBufs g) {
  for (int e = threadIdx.x; e < K * T; e += 256) {
    const int row = rows.row[e / T];
    g.owner[0][(long long)row * T + e % T] = row;
  }
  if (threadIdx.x == 0) {
    g.fin_count[rows.row[0]] = 0;
    g.complete[rows.row[0]] = 0;
  }
}

// the per-row index arrays of a forward call: row r = (b, s) sits at position pos + s of item b.  item_cross (a grouped state, else null): the window
// whose cross K/V row b reads, b / n_group
__global__ void text_rows_kernel(int B, int S, int pos, int n_text_ctx, int n_audio_ctx, int n_group, int* item, int* item_cross, int* posr, int* len_self,
                                 int* len_cross, int* cache_row) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= B * S) return;
  const int b = r / S, p = pos + r % S;
  item[r] = b;
  if (item_cross) item_cross[r] = b / n_group;
  posr[r] = p;
  len_self[r] = p + 1;
  len_cross[r] = n_audio_ctx;
  cache_row[r] = b * n_text_ctx + p;
}

// Row mode's plan: the same arrays, and the rows' tokens, from a table of items that travels as the launch's argument.  Item i covers the flat rows
// first[i] .. first[i] + count[i] - 1: decoder row row[i] at positions pos[i] + s, fed from offset from[i] + s of the row's initial-token store, or
// (from[i] < 0, count 1) with the token the row's last pick chose.
__global__ void text_plan_kernel(KKRowItems t, int R, int n_text_ctx, int n_audio_ctx, const int32_t* init, const int32_t* next, int* item, int* item_cross,
                                 int* posr, int* len_self, int* len_cross, int* cache_row, int32_t* tok) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  int i = 0;
  while (i + 1 < t.n && r >= t.first[i + 1]) ++i;
  const int s = r - t.first[i], row = t.row[i], p = t.pos[i] + s;
  item[r] = row;
  if (item_cross) item_cross[r] = t.cross[i];  // a group's rows read their leader's slice, as item / n_group in text_rows_kernel
  posr[r] = p;
  len_self[r] = p + 1;
  len_cross[r] = n_audio_ctx;
  cache_row[r] = row * n_text_ctx + p;
  tok[r] = t.from[i] >= 0 ? init[(long long)row * n_text_ctx + t.from[i] + s] : next[row];
}

// The owner table of a round that steps a beam group, [R][T] for attn_rows<OWNED>: flat row r = blockIdx.y of item i reads position p in the
// row that table t.own[i] of its decoder row names, or (t.own[i] < 0: a plain row, a prefill) in its own slot
__global__ __launch_bounds__(256) void text_plan_owner_kernel(KKRowItems t, int T, const int32_t* own0, const int32_t* own1, int* table) {
  const int r = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= T) return;
  int i = 0;
  while (i + 1 < t.n && r >= t.first[i + 1]) ++i;
  const int row = t.row[i], f = t.own[i];
  table[(long long)r * T + p] = f < 0 ? row : (f & 1 ? own1 : own0)[(long long)row * T + p];
}

// rows sel.src[j] of x to row j of out (the rows whose logits a row-mode round wants, made contiguous for the final LayerNorm)
__global__ __launch_bounds__(256) void gather_rows_kernel(KKRowGather sel, const float* x, int D, float* out) {
  const float* s = x + (long long)sel.src[blockIdx.x] * D;
  for (int c = threadIdx.x; c < D; c += 256) out[(long long)blockIdx.x * D + c] = s[c];
}
}  // namespace

// ====================================================================================================== the launchers of kk_kernels.h (no checks)
size_t kk_whisper_attn_scratch_floats(int R, int heads, int T_rows) { return (size_t)R * heads * attn_nsplit(T_rows) * ATTN_REC; }

int kk_launch_whisper_attn_rows(hipStream_t st, bool owned, int R, int heads, const float* q, const bf16_t* kv, int k_off, int v_off, int items, int T_rows,
                                int ld, const int* table, const int* len, float* out, float* scratch) {
  const int ns = attn_nsplit(T_rows);
  const auto kernel = owned ? attn_rows_kernel<true> : attn_rows_kernel<false>;
  for (int r0 = 0; r0 < R; r0 += 32768) {  // grid.z limit
    const int n = R - r0 < 32768 ? R - r0 : 32768;
    float* sc = scratch + (size_t)r0 * heads * ns * ATTN_REC;
    hipLaunchKernelGGL(kernel, dim3(ns, heads, n), dim3(64), 0, st, q + (size_t)r0 * heads * 64, kv, k_off, v_off, (long long)T_rows * ld, ld, T_rows, items,
                       table + (owned ? (size_t)r0 * T_rows : (size_t)r0), len + r0, heads, sc, ns);
    KK_CHECK_LAUNCH();
    hipLaunchKernelGGL(attn_merge_kernel, dim3(heads, n), dim3(64), 0, st, sc, ns, heads, len + r0, out + (size_t)r0 * heads * 64);
    KK_CHECK_LAUNCH();
  }
  return 0;
}

int kk_launch_whisper_linear_rows(hipStream_t st, const KKLinRows& a) {
  hipLaunchKernelGGL(linear_rows_kernel, dim3((a.N + 15) / 16), dim3(64 * LIN_WAVES), 0, st, a);
  KK_CHECK_LAUNCH();
  return 0;
}

const char* kk_whisper_q_refusal(int K, int group, int bits) {
  if (bits != 4 && bits != 8) return "bits is not 4 or 8";
  if (group != 32 && group != 64 && group != 128) return "group size is not 32, 64 or 128";
  if (K < group || K % group != 0) return "the input width is not a multiple of the group size";
  return nullptr;
}

int kk_launch_whisper_linear_rows_q(hipStream_t st, const KKLinRows& a, const uint32_t* words, const float2* pairs, int group, int bits) {
  const LinQ q{words, pairs, q_gshift(group)};
  if (bits == 8) hipLaunchKernelGGL(linear_rows_q_kernel<8>, dim3((a.N + 15) / 16), dim3(64 * LIN_WAVES), 0, st, a, q);
  else hipLaunchKernelGGL(linear_rows_q_kernel<4>, dim3((a.N + 15) / 16), dim3(64 * LIN_WAVES), 0, st, a, q);
  KK_CHECK_LAUNCH();
  return 0;
}

int kk_launch_whisper_embed(hipStream_t st, int R, int D, const int* tok, const int* pos, const bf16_t* table, int n_vocab, const float* positions, int n_ctx,
                            float* out) {
  hipLaunchKernelGGL(embed_kernel, dim3(R), dim3(256), 0, st, tok, pos, table, n_vocab, positions, n_ctx, D, out);
  KK_CHECK_LAUNCH();
  return 0;
}

int kk_launch_whisper_embed_q(hipStream_t st, int R, int D, const int* tok, const int* pos, const uint32_t* words, const float2* pairs, int group, int bits,
                              int n_vocab, const float* positions, int n_ctx, float* out) {
  if (bits == 8) hipLaunchKernelGGL(embed_q_kernel<8>, dim3(R), dim3(256), 0, st, tok, pos, words, pairs, group, n_vocab, positions, n_ctx, D, out);
  else hipLaunchKernelGGL(embed_q_kernel<4>, dim3(R), dim3(256), 0, st, tok, pos, words, pairs, group, n_vocab, positions, n_ctx, D, out);
  KK_CHECK_LAUNCH();
  return 0;
}

int kk_launch_whisper_text_rows(hipStream_t st, int B, int S, int pos, int n_text_ctx, int n_audio_ctx, int n_group, int* item, int* item_cross, int* posr,
                                int* len_self, int* len_cross, int* cache_row) {
  hipLaunchKernelGGL(text_rows_kernel, dim3((B * S + 255) / 256), dim3(256), 0, st, B, S, pos, n_text_ctx, n_audio_ctx, n_group, item, item_cross, posr, len_self,
                     len_cross, cache_row);
  KK_CHECK_LAUNCH();
  return 0;
}

int kk_launch_whisper_text_plan(hipStream_t st, const KKRowItems& t, int R, int n_text_ctx, int n_audio_ctx, const int32_t* init, const int32_t* next, int* item,
                                int* item_cross, int* posr, int* len_self, int* len_cross, int* cache_row, int32_t* tok) {
  hipLaunchKernelGGL(text_plan_kernel, dim3((R + 255) / 256), dim3(256), 0, st, t, R, n_text_ctx, n_audio_ctx, init, next, item, item_cross, posr, len_self, len_cross,
                     cache_row, tok);
  KK_CHECK_LAUNCH();
  return 0;
}

int kk_launch_whisper_text_plan_owner(hipStream_t st, const KKRowItems& t, int R, int n_text_ctx, const int32_t* own0, const int32_t* own1, int* table) {
  hipLaunchKernelGGL(text_plan_owner_kernel, dim3((n_text_ctx + 255) / 256, R), dim3(256), 0, st, t, n_text_ctx, own0, own1, table);
  KK_CHECK_LAUNCH();
  return 0;
}

int kk_launch_whisper_rows_select(hipStream_t st, int n, const KKGroupSel& sel, const KKGroupBufs& g, int n_text_ctx, const kk_whisper_pick_params* params,
                                  kk_whisper_pick_state* state, int32_t* tokens, int32_t* next) {
  hipLaunchKernelGGL(rows_select_kernel, dim3(n), dim3(256), 0, st, sel, g, n_text_ctx, params, state, tokens, next);
  KK_CHECK_LAUNCH();
  return 0;
}

int kk_launch_whisper_rows_group_reset(hipStream_t st, const KKGroupRows& rows, int K, int n_text_ctx, const KKGroupBufs& g) {
  hipLaunchKernelGGL(rows_group_reset_kernel, dim3(1), dim3(256), 0, st, rows, K, n_text_ctx, g);
  KK_CHECK_LAUNCH();
  return 0;
}

int kk_launch_whisper_gather_rows(hipStream_t st, int n, const KKRowGather& sel, const float* x, int D, float* out) {
  hipLaunchKernelGGL(gather_rows_kernel, dim3(n), dim3(256), 0, st, sel, x, D, out);
  KK_CHECK_LAUNCH();
  return 0;
}

int kk_launch_whisper_pick_rows(hipStream_t st, int n, const KKPickSel& sel, const float* logits, long long ldl, const kk_whisper_pick_params* params,
                                const uint32_t* suppress, int words, const PickDraw* draws, kk_whisper_pick_state* state, int32_t* tokens, int cap, int32_t* next,
                                int32_t* cand_token, float* cand_logprob) {
  hipLaunchKernelGGL(pick_rows_kernel, dim3(n), dim3(1024), 0, st, sel, logits, ldl, params, suppress, words, draws, state, tokens, cap, next, cand_token,
                     cand_logprob);
  KK_CHECK_LAUNCH();
  return 0;
}

// ============================================================================================================================ kk_op_* entries
extern "C" size_t kk_op_whisper_attn_rows_scratch_bytes(int R, int heads, int T_rows) {
  if (R < 1 || heads < 1 || T_rows < 1) return 0;
  return kk_whisper_attn_scratch_floats(R, heads, T_rows) * sizeof(float);
}

namespace {
// the one body of kk_op_whisper_attn_rows (`table`: item [R]) and kk_op_whisper_attn_rows_owned (`table`: owner [R][T_rows])
template <bool OWNED>
int op_attn_rows(const char* who, void* stream, int R, int heads, const float* q, const void* kv, int k_off, int v_off, int items, int T_rows, int ld,
                 const int32_t* table, const int32_t* len, float* out, void* scratch, size_t scratch_bytes) {
  if (!q || !kv || !table || !len || !out || !scratch) return kk_failf("%s: null argument", who);
  if (R < 1 || heads < 1 || items < 1 || T_rows < 1) return kk_failf("%s: bad argument (need R, heads, items, T_rows >= 1)", who);
  if (k_off < 0 || v_off < 0 || k_off % 8 != 0 || v_off % 8 != 0 || ld % 8 != 0 || k_off + heads * 64 > ld || v_off + heads * 64 > ld)
    return kk_failf("%s: k_off / v_off / ld must be multiples of 8 with `heads` heads of 64 channels inside a row", who);
  if (((uintptr_t)kv & 15) || ((uintptr_t)q & 15) || ((uintptr_t)scratch & 15)) return kk_failf("%s: q, kv and scratch must be 16-byte aligned", who);
  if (scratch_bytes < kk_op_whisper_attn_rows_scratch_bytes(R, heads, T_rows)) return kk_failf("%s: scratch too small", who);
  // the only entries that look at device data: the row table decides what memory is read, so it is checked here (the handle's forward, which
  // makes its own tables, calls the launcher and never synchronises)
  const size_t per = OWNED ? (size_t)T_rows : 1;
  std::vector<int32_t> hv((size_t)R * per), hl((size_t)R);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(hv.data(), table, hv.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(hl.data(), len, (size_t)R * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return kk_failf("%s: reading the row table failed", who);
  for (int r = 0; r < R; ++r) {
    if (hl[r] < 1 || hl[r] > T_rows) return kk_failf("%s: len[%d] = %d is outside [1, %d]", who, r, hl[r], T_rows);
    if constexpr (OWNED) {
      for (int j = 0; j < hl[r]; ++j)
        if (hv[r * per + j] < 0 || hv[r * per + j] >= items) return kk_failf("%s: owner[%d][%d] = %d is outside [0, %d)", who, r, j, hv[r * per + j], items);
    } else if (hv[r] < 0 || hv[r] >= items) {
      return kk_failf("%s: item[%d] = %d is outside [0, %d)", who, r, hv[r], items);
    }
  }
  return kk_launch_whisper_attn_rows(st, OWNED, R, heads, q, (const bf16_t*)kv, k_off, v_off, items, T_rows, ld, table, len, out, (float*)scratch);
}
}  // namespace

extern "C" int kk_op_whisper_attn_rows(void* stream, int R, int heads, const float* q, const void* kv, int k_off, int v_off, int items, int T_rows, int ld,
                                       const int32_t* item, const int32_t* len, float* out, void* scratch, size_t scratch_bytes) {
  return op_attn_rows<false>("kk_op_whisper_attn_rows", stream, R, heads, q, kv, k_off, v_off, items, T_rows, ld, item, len, out, scratch, scratch_bytes);
}

extern "C" int kk_op_whisper_attn_rows_owned(void* stream, int R, int heads, const float* q, const void* kv, int k_off, int v_off, int items, int T_rows, int ld,
                                             const int32_t* owner, const int32_t* len, float* out, void* scratch, size_t scratch_bytes) {
  return op_attn_rows<true>("kk_op_whisper_attn_rows_owned", stream, R, heads, q, kv, k_off, v_off, items, T_rows, ld, owner, len, out, scratch, scratch_bytes);
}

namespace {
// the argument checks of kk_op_whisper_linear_rows and kk_op_whisper_linear_rows_q, in the order both make them.  The entry's own: `null_arg` (its
// operands), `refusal` (the quantised format's, or null) and `misaligned` with the wording of its alignment rule
int check_linear_rows(const char* who, const KKLinRows& a, bool null_arg, const char* refusal, bool misaligned, const char* alignment) {
  if (null_arg || (!a.out && !a.ob)) return kk_failf("%s: null argument", who);
  if (a.M < 1 || a.M > 16) return kk_failf("%s: 1 <= M <= 16 rows per call", who);
  if (a.N < 1 || a.K < 32 || a.K % 32 != 0) return kk_failf("%s: N >= 1 and K a multiple of 32", who);
  if (refusal) return kk_failf("%s: %s (bits 4 or 8, group size 32, 64 or 128 dividing K)", who, refusal);
  if (a.act != KK_ACT_NONE && a.act != KK_ACT_GELU) return kk_failf("%s: act must be none (0) or GELU (2)", who);
  if (a.ldx < a.K || a.ldx % 4 != 0 || misaligned) return kk_failf("%s: %s, ldx >= K, ldx %% 4 == 0", who, alignment);
  if ((a.out && a.ldo < a.N) || (a.res && a.ldr < a.N) || (a.ob && (a.ldb < a.N || a.nrows < 1))) return kk_failf("%s: a row pitch is smaller than N", who);
  return 0;
}
}  // namespace

extern "C" int kk_op_whisper_linear_rows(void* stream, int M, int N, int K, const float* x, long long ldx, const void* w, const float* bias, int act,
                                         const float* res, long long ldr, float* out, long long ldo, void* out_bf16, long long ld_bf16, const int32_t* rows_bf16,
                                         int nrows_bf16) {
  KKLinRows a{x, ldx, (const bf16_t*)w, bias, res, ldr, out, ldo, (bf16_t*)out_bf16, ld_bf16, rows_bf16, nrows_bf16, M, N, K, act};
  KK_TRY(check_linear_rows("kk_op_whisper_linear_rows", a, !x || !w, nullptr, ((uintptr_t)x & 15) || ((uintptr_t)w & 15), "x and w must be 16-byte aligned"));
  return kk_launch_whisper_linear_rows((hipStream_t)stream, a);
}

extern "C" int kk_op_whisper_embed(void* stream, int R, int D, const int32_t* tok, const int32_t* pos, const void* table_bf16, int n_vocab, const float* positions,
                                   int n_ctx, float* out) {
  if (!tok || !pos || !table_bf16 || !positions || !out) return kk_fail("kk_op_whisper_embed: null argument");
  if (R < 1 || D < 1 || n_vocab < 1 || n_ctx < 1) return kk_fail("kk_op_whisper_embed: bad argument");
  return kk_launch_whisper_embed((hipStream_t)stream, R, D, tok, pos, (const bf16_t*)table_bf16, n_vocab, positions, n_ctx, out);
}

extern "C" int kk_op_whisper_linear_rows_q(void* stream, int M, int N, int K, const float* x, long long ldx, const uint32_t* words, const float* pairs,
                                           int group_size, int bits, const float* bias, int act, const float* res, long long ldr, float* out, long long ldo,
                                           void* out_bf16, long long ld_bf16, const int32_t* rows_bf16, int nrows_bf16) {
  KKLinRows a{x, ldx, nullptr, bias, res, ldr, out, ldo, (bf16_t*)out_bf16, ld_bf16, rows_bf16, nrows_bf16, M, N, K, act};
  KK_TRY(check_linear_rows("kk_op_whisper_linear_rows_q", a, !x || !words || !pairs, kk_whisper_q_refusal(K, group_size, bits),
                           ((uintptr_t)x & 15) || ((uintptr_t)words & 7) || ((uintptr_t)pairs & 7), "x must be 16-byte, words and pairs 8-byte aligned"));
  return kk_launch_whisper_linear_rows_q((hipStream_t)stream, a, words, (const float2*)pairs, group_size, bits);
}

extern "C" int kk_op_whisper_embed_q(void* stream, int R, int D, const int32_t* tok, const int32_t* pos, const uint32_t* words, const float* pairs, int group_size,
                                     int bits, int n_vocab, const float* positions, int n_ctx, float* out) {
  if (!tok || !pos || !words || !pairs || !positions || !out) return kk_fail("kk_op_whisper_embed_q: null argument");
  if (R < 1 || D < 1 || n_vocab < 1 || n_ctx < 1) return kk_fail("kk_op_whisper_embed_q: bad argument");
  if (const char* why = kk_whisper_q_refusal(D, group_size, bits)) return kk_failf("kk_op_whisper_embed_q: %s (bits 4 or 8, group size 32, 64 or 128 dividing D)", why);
  if (((uintptr_t)words & 3) || ((uintptr_t)pairs & 7)) return kk_fail("kk_op_whisper_embed_q: words must be 4-byte and pairs 8-byte aligned");
  return kk_launch_whisper_embed_q((hipStream_t)stream, R, D, tok, pos, words, (const float2*)pairs, group_size, bits, n_vocab, positions, n_ctx, out);
}

extern "C" int kk_op_whisper_pick(void* stream, int B, const float* logits, long long ldl, const kk_whisper_pick_params* params, const uint32_t* suppress,
                                  kk_whisper_pick_state* state, int32_t* tokens, int cap, int32_t* next, int32_t* not_ended) {
  if (!logits || !params || !state || !tokens || !next || !not_ended) return kk_fail("kk_op_whisper_pick: null argument");
  if (B < 1 || cap < 1 || ldl < 1) return kk_fail("kk_op_whisper_pick: bad argument");
  hipLaunchKernelGGL(pick_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, logits, ldl, params, suppress, state, tokens, cap, next, not_ended);
  KK_CHECK_LAUNCH();
  return 0;
}

extern "C" int kk_op_whisper_pick_sampled(void* stream, int B, const float* logits, long long ldl, const kk_whisper_pick_params* params, const uint32_t* suppress,
                                          float temperature, uint64_t seed, const uint32_t* streams, kk_whisper_pick_state* state, int32_t* tokens, int cap,
                                          int32_t* next, int32_t* not_ended) {
  if (!logits || !params || !streams || !state || !tokens || !next || !not_ended) return kk_fail("kk_op_whisper_pick_sampled: null argument");
  if (B < 1 || cap < 1 || ldl < 1) return kk_fail("kk_op_whisper_pick_sampled: bad argument");
  const float inv_t = 1.0f / temperature;
  if (!(temperature > 0.f) || !std::isfinite(temperature) || !std::isfinite(inv_t))
    return kk_fail("kk_op_whisper_pick_sampled: temperature must be finite and > 0 (temperature 0 is kk_op_whisper_pick)");
  hipLaunchKernelGGL(pick_sampled_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, logits, ldl, params, suppress, inv_t, seed, streams, state, tokens, cap, next,
                     not_ended);
  KK_CHECK_LAUNCH();
  return 0;
}

extern "C" int kk_op_whisper_pick_reset(void* stream, int B, kk_whisper_pick_state* state, int32_t* not_ended) {
  if (!state || !not_ended || B < 1) return kk_fail("kk_op_whisper_pick_reset: bad argument");
  hipLaunchKernelGGL(pick_reset_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, state, B, not_ended);
  KK_CHECK_LAUNCH();
  return 0;
}

extern "C" int kk_op_whisper_beam_topk(void* stream, int B, int beam_size, const float* logits, long long ldl, const kk_whisper_pick_params* params,
                                       const uint32_t* suppress, const kk_whisper_pick_state* state, int32_t* cand_token, float* cand_logprob) {
  if (!logits || !params || !state || !cand_token || !cand_logprob) return kk_fail("kk_op_whisper_beam_topk: null argument");
  if (B < 1 || ldl < 1) return kk_fail("kk_op_whisper_beam_topk: bad argument");
  if (beam_size < 1 || beam_size > KK_WHISPER_MAX_GROUP) return kk_failf("kk_op_whisper_beam_topk: beam_size = %d is outside [1, %d]", beam_size, KK_WHISPER_MAX_GROUP);
  hipLaunchKernelGGL(beam_topk_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, logits, ldl, params, suppress, state, beam_size + 1, cand_token, cand_logprob);
  KK_CHECK_LAUNCH();
  return 0;
}

namespace {
int check_beam_bufs(const char* who, const kk_whisper_beam_bufs* b) {
  if (!b) return kk_failf("%s: null argument", who);
  if (b->n_audio < 1 || b->n_ctx < 1 || b->cap < 1) return kk_failf("%s: bad argument (need n_audio, n_ctx, cap >= 1)", who);
  if (b->beam_size < 1 || b->beam_size > KK_WHISPER_MAX_GROUP) return kk_failf("%s: beam_size = %d is outside [1, %d]", who, b->beam_size, KK_WHISPER_MAX_GROUP);
  if (b->max_candidates < 1 || b->max_candidates > BEAM_FIN) return kk_failf("%s: max_candidates = %d is outside [1, %d]", who, b->max_candidates, BEAM_FIN);
  if (!b->cand_token || !b->cand_logprob || !b->owner[0] || !b->owner[1] || !b->parent || !b->fin_score || !b->fin_length || !b->fin_tokens || !b->fin_count ||
      !b->complete || !b->not_complete)
    return kk_failf("%s: a null buffer", who);
  return 0;
}
}  // namespace

extern "C" int kk_op_whisper_beam_reset(void* stream, const kk_whisper_beam_bufs* bufs) {
  KK_TRY(check_beam_bufs("kk_op_whisper_beam_reset", bufs));
  const long long n = (long long)bufs->n_audio * bufs->beam_size * bufs->n_ctx;
  hipLaunchKernelGGL(beam_reset_kernel, dim3((unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024)), dim3(256), 0, (hipStream_t)stream, *bufs);
  KK_CHECK_LAUNCH();
  return 0;
}

extern "C" int kk_op_whisper_beam_select(void* stream, const kk_whisper_beam_bufs* bufs, int flip, int pos, const kk_whisper_pick_params* params,
                                         kk_whisper_pick_state* state, int32_t* tokens, int32_t* next) {
  const char* who = "kk_op_whisper_beam_select";
  KK_TRY(check_beam_bufs(who, bufs));
  if (!params || !state || !tokens || !next) return kk_failf("%s: null argument", who);
  if (flip != 0 && flip != 1) return kk_failf("%s: flip must be 0 or 1", who);
  if (pos < 0 || pos > bufs->n_ctx) return kk_failf("%s: pos = %d is outside [0, n_ctx = %d]", who, pos, bufs->n_ctx);
  hipLaunchKernelGGL(beam_select_kernel, dim3(bufs->n_audio), dim3(256), 0, (hipStream_t)stream, *bufs, flip, pos, params, state, tokens, next);
  KK_CHECK_LAUNCH();
  return 0;
}
