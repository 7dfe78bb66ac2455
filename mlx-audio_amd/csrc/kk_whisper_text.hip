// Whisper, text side (gfx950): the decode-step kernels and the text decoder behind a handle.  Restates TextDecoder
// (mlx_audio/stt/models/whisper/whisper.py:202-248, blocks :140-168, attention :90-137) and the token selection of decoding.py:255-395; DESIGN 8g.
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
//
// ---- groups -------------------------------------------------------------------------------------------------------------------------------
//   A window state may carry n_group decoder rows per window (best_of): the cross K/V is projected and kept once per WINDOW, the self K/V, pick state
//   and token stores once per row, and the row-table kernel writes a second table item_cross[r] = item[r] / n_group that the cross-attention reads.
//   n_group = 1 is set_audio: one table, the launches and arguments of before.
//
// ---- beam search ----------------------------------------------------------------------------------------------------------------------------
//   On a grouped state with n_group = beam_size: a step is the forward plus beam_topk (a row's K + 1 best tokens behind the pick's filters) and beam_select
//   (one workgroup per window: OpenAI's BeamSearchDecoder.update on the window's K (K + 1) candidates).  The self K/V is never moved: an owner table
//   [row][position] names the physical row that holds each position of a beam, select rewrites it from the parents' rows (two copies, swapped every step),
//   and the step's self-attention is attn_rows<OWNED>, which reads key j of row r in item owner[r][j].
//
// ---- row mode (the end of this file) ---------------------------------------------------------------------------------------------------
//   Rows with their own window, position, pick parameters and lifetime in a second state buffer.  A round is the window's launch sequence behind
//   text_plan_kernel, which fills the per-row index arrays and tokens from a table of items passed as the launch's argument.
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
inline size_t attn_scratch_floats(int R, int heads, int T_rows) { return (size_t)R * heads * attn_nsplit(T_rows) * ATTN_REC; }

// OWNED: `item` is the owner table [R][T_rows]
template <bool OWNED = false>
int launch_attn_rows(hipStream_t st, int R, int heads, const float* q, const bf16_t* kv, int k_off, int v_off, int items, int T_rows, int ld, const int* item,
                     const int* len, float* out, float* scratch) {
  const int ns = attn_nsplit(T_rows);
  for (int r0 = 0; r0 < R; r0 += 32768) {  // grid.z limit
    const int n = R - r0 < 32768 ? R - r0 : 32768;
    float* sc = scratch + (size_t)r0 * heads * ns * ATTN_REC;
    hipLaunchKernelGGL(attn_rows_kernel<OWNED>, dim3(ns, heads, n), dim3(64), 0, st, q + (size_t)r0 * heads * 64, kv, k_off, v_off, (long long)T_rows * ld, ld, T_rows,
                       items, item + (OWNED ? (size_t)r0 * T_rows : (size_t)r0), len + r0, heads, sc, ns);
    KK_CHECK_LAUNCH();
    hipLaunchKernelGGL(attn_merge_kernel, dim3(heads, n), dim3(64), 0, st, sc, ns, heads, len + r0, out + (size_t)r0 * heads * 64);
    KK_CHECK_LAUNCH();
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------------------- linear
struct LinRows {
  const float* x;
  long long ldx;
  const bf16_t* w;
  const float* bias;
  const float* res;
  long long ldr;
  float* out;
  long long ldo;
  bf16_t* ob;
  long long ldb;
  const int* rows;  // destination row of x row m in the bf16 store
  int nrows;        // rows the store has; a destination outside [0, nrows) is not written
  int M, N, K, act;
};

constexpr int LIN_WAVES = 16;  // waves of a workgroup = slices of K, summed in wave order

// the end of a linear_rows workgroup (bf16 and quantised weights alike): the waves' partial tiles are added in wave order, then bias, GELU, residual
// and the fp32 / bf16 stores.  acc: the wave's D[m = 4 g + r][n = lr]
__device__ __forceinline__ void lin_finish(const LinRows& a, float (&red)[LIN_WAVES][16][17], const f32x4 acc, int n0) {
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

__global__ __launch_bounds__(64 * LIN_WAVES) void linear_rows_kernel(LinRows a) {
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

int launch_linear_rows(hipStream_t st, const LinRows& a) {
  hipLaunchKernelGGL(linear_rows_kernel, dim3((a.N + 15) / 16), dim3(64 * LIN_WAVES), 0, st, a);
  KK_CHECK_LAUNCH();
  return 0;
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
__global__ __launch_bounds__(64 * LIN_WAVES) void linear_rows_q_kernel(LinRows a, LinQ q) {
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
// why a quantised [N][K] matrix cannot stay packed, or null: the formats linear_rows_q / embed_q read
const char* q_refusal(int K, int group, int bits) {
  if (bits != 4 && bits != 8) return "bits is not 4 or 8";
  if (group != 32 && group != 64 && group != 128) return "group size is not 32, 64 or 128";
  if (K < group || K % group != 0) return "the input width is not a multiple of the group size";
  return nullptr;
}

// (a.w is not read)
int launch_linear_rows_q(hipStream_t st, const LinRows& a, const uint32_t* words, const float2* pairs, int group, int bits) {
  const LinQ q{words, pairs, q_gshift(group)};
  if (bits == 8) hipLaunchKernelGGL(linear_rows_q_kernel<8>, dim3((a.N + 15) / 16), dim3(64 * LIN_WAVES), 0, st, a, q);
  else hipLaunchKernelGGL(linear_rows_q_kernel<4>, dim3((a.N + 15) / 16), dim3(64 * LIN_WAVES), 0, st, a, q);
  KK_CHECK_LAUNCH();
  return 0;
}

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

int launch_embed_q(hipStream_t st, int R, int D, const int* tok, const int* pos, const uint32_t* words, const float2* pairs, int group, int bits, int n_vocab,
                   const float* positions, int n_ctx, float* out) {
  if (bits == 8) hipLaunchKernelGGL(embed_q_kernel<8>, dim3(R), dim3(256), 0, st, tok, pos, words, pairs, group, n_vocab, positions, n_ctx, D, out);
  else hipLaunchKernelGGL(embed_q_kernel<4>, dim3(R), dim3(256), 0, st, tok, pos, words, pairs, group, n_vocab, positions, n_ctx, D, out);
  KK_CHECK_LAUNCH();
  return 0;
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
constexpr int BEAM_FIN = 2 * KK_WHISPER_MAX_GROUP;             // finished sequences a window keeps, at most

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

// what a sampled pick adds to a row's arguments: 1 / temperature, the Philox key and the row's stream id
struct PickDraw {
  float inv_t;
  uint64_t seed;
  uint32_t stream;
};
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

// per-row: block j picks for decoder row sel.row[j] on logits row sel.logit[j], with that row's params, bitmask (`words` words each), state and store
struct PickSel {
  int row[KK_WHISPER_MAX_ROWS], logit[KK_WHISPER_MAX_ROWS];
};
__global__ __launch_bounds__(1024) void pick_rows_kernel(PickSel sel, const float* logits, long long ldl, const kk_whisper_pick_params* params,
                                                         const uint32_t* suppress, int words, kk_whisper_pick_state* state, int32_t* tokens, int cap, int32_t* next) {
  __shared__ Osm sh[16];
  const int r = sel.row[blockIdx.x];
  pick_row<PICK_GREEDY>(logits + (long long)sel.logit[blockIdx.x] * ldl, params[r], suppress + (long long)r * words, state + r, tokens + (long long)r * cap, cap, next + r,
                  nullptr, sh);
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

// Window w = blockIdx.x, rows w K .. w K + K - 1, whose parents hold `pos` positions; owner tables: b.owner[flip] is read, b.owner[flip ^ 1] written.
// The walk's order is total -- score descending, parent row ascending, rank within the parent ascending -- so every thread computes its candidate's
// place by counting, and thread 0 walks the sorted list.
__global__ __launch_bounds__(256) void beam_select_kernel(kk_whisper_beam_bufs b, int flip, int pos, const kk_whisper_pick_params* params, kk_whisper_pick_state* state,
                                                          int32_t* tokens, int32_t* next) {
  __shared__ kk_whisper_pick_state par[KK_WHISPER_MAX_GROUP];
  __shared__ float c_score[BEAM_N], c_lp[BEAM_N];
  __shared__ int c_tok[BEAM_N], order[BEAM_N];
  __shared__ int s_cand[KK_WHISPER_MAX_GROUP], f_cand[BEAM_FIN], f_slot[BEAM_FIN], n_new;
  const int w = blockIdx.x, tid = threadIdx.x, K = b.beam_size, C = K + 1, n = K * C, row0 = w * K, T = b.n_ctx, cap = b.cap;
  const int eot = params->eot, tb = params->timestamp_begin;
  const int32_t* own_old = b.owner[flip & 1];
  int32_t* own_new = b.owner[(flip & 1) ^ 1];
  if (tid < K) par[tid] = state[row0 + tid];
  if (tid < n) order[tid] = -1;
  __syncthreads();
  const int count = par[0].count;  // the rows of a window step together
  if (tid < n) {
    const int j = tid / C;
    const int t = b.cand_token[(long long)row0 * C + tid];
    const float lp = b.cand_logprob[(long long)row0 * C + tid];
    const float s = par[j].sum_logprob + lp;
    // at the first sampled position the rows of a window are one prefix: row 0 offers for all
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
    int saved = 0, nf = 0, fc = b.fin_count[w];
    fc = fc < 0 ? 0 : fc;  // (a store that was never reset: nothing is written outside it)
    for (int idx = 0; idx < n && saved < K; ++idx) {
      const int c = order[idx];
      if (c < 0 || c_tok[c] < 0) break;  // the offers are used up
      if (c_tok[c] != eot) {
        s_cand[saved++] = c;
      } else if (fc < b.max_candidates && nf < BEAM_FIN) {  // finished, in descending score, while there is room
        f_cand[nf] = c;
        f_slot[nf++] = fc++;
      }
    }
    for (int k = saved; k < K; ++k) s_cand[k] = -1;  // dead slots
    n_new = nf;
    b.fin_count[w] = fc;
    if (fc >= b.max_candidates && !b.complete[w]) {
      b.complete[w] = 1;
      atomicSub(b.not_complete, 1);
    }
  }
  __syncthreads();
  if (tid < K) {  // the child's pick state from the PARENT's
    const int c = s_cand[tid], row = row0 + tid;
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
    N.ended = 0;
    N.count = count + 1;
    state[row] = N;
    next[row] = tok;
    b.parent[row] = c >= 0 ? row0 + c / C : -1;
    if (count >= 0 && count < cap) tokens[(long long)row * cap + count] = tok;
  }
  auto owner_of = [&](int row, int p) -> int {  // the physical row that holds position p of `row`, kept inside the window whatever the table holds
    const int o = p >= 0 && p < T ? own_old[(long long)row * T + p] : row;
    return o >= row0 && o < row0 + K ? o : row;
  };
  for (int e = tid; e < K * T; e += 256) {  // what the parent has is inherited; the positions from `pos` on are the row's own
    const int k = e / T, p = e - k * T, c = s_cand[k];
    own_new[(long long)(row0 + k) * T + p] = c >= 0 && p < pos ? owner_of(row0 + c / C, p) : row0 + k;
  }
  const int len = count < 0 ? 0 : (count < cap ? count : cap);
  for (int f = 0; f < n_new; ++f) {  // the finished sequences, materialised now: their rows are overwritten from the next step on
    const int c = f_cand[f], prow = row0 + c / C;
    int32_t* dst = b.fin_tokens + ((long long)w * b.max_candidates + f_slot[f]) * cap;
    for (int i = tid; i < len; i += 256) dst[i] = tokens[(long long)owner_of(prow, pos - count + i) * cap + i];
    if (tid == 0) {
      b.fin_score[w * b.max_candidates + f_slot[f]] = c_score[c];
      b.fin_length[w * b.max_candidates + f_slot[f]] = len;
    }
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
struct RowItems {
  int n;
  int row[KK_WHISPER_MAX_ROWS], pos[KK_WHISPER_MAX_ROWS], count[KK_WHISPER_MAX_ROWS], from[KK_WHISPER_MAX_ROWS], first[KK_WHISPER_MAX_ROWS];
};
__global__ void text_plan_kernel(RowItems t, int R, int n_text_ctx, int n_audio_ctx, const int32_t* init, const int32_t* next, int* item, int* posr, int* len_self,
                                 int* len_cross, int* cache_row, int32_t* tok) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  int i = 0;
  while (i + 1 < t.n && r >= t.first[i + 1]) ++i;
  const int s = r - t.first[i], row = t.row[i], p = t.pos[i] + s;
  item[r] = row;
  posr[r] = p;
  len_self[r] = p + 1;
  len_cross[r] = n_audio_ctx;
  cache_row[r] = row * n_text_ctx + p;
  tok[r] = t.from[i] >= 0 ? init[(long long)row * n_text_ctx + t.from[i] + s] : next[row];
}

// rows sel.src[j] of x to row j of out (the rows whose logits a row-mode round wants, made contiguous for the final LayerNorm)
struct RowGather {
  int src[2 * KK_WHISPER_MAX_ROWS];
};
__global__ __launch_bounds__(256) void gather_rows_kernel(RowGather sel, const float* x, int D, float* out) {
  const float* s = x + (long long)sel.src[blockIdx.x] * D;
  for (int c = threadIdx.x; c < D; c += 256) out[(long long)blockIdx.x * D + c] = s[c];
}
}  // namespace

// ============================================================================================================================ kk_op_* entries
extern "C" size_t kk_op_whisper_attn_rows_scratch_bytes(int R, int heads, int T_rows) {
  if (R < 1 || heads < 1 || T_rows < 1) return 0;
  return attn_scratch_floats(R, heads, T_rows) * sizeof(float);
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
  return launch_attn_rows<OWNED>(st, R, heads, q, (const bf16_t*)kv, k_off, v_off, items, T_rows, ld, table, len, out, (float*)scratch);
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

extern "C" int kk_op_whisper_linear_rows(void* stream, int M, int N, int K, const float* x, long long ldx, const void* w, const float* bias, int act,
                                         const float* res, long long ldr, float* out, long long ldo, void* out_bf16, long long ld_bf16, const int32_t* rows_bf16,
                                         int nrows_bf16) {
  if (!x || !w || (!out && !out_bf16)) return kk_fail("kk_op_whisper_linear_rows: null argument");
  if (M < 1 || M > 16) return kk_fail("kk_op_whisper_linear_rows: 1 <= M <= 16 rows per call");
  if (N < 1 || K < 32 || K % 32 != 0) return kk_fail("kk_op_whisper_linear_rows: N >= 1 and K a multiple of 32");
  if (act != KK_ACT_NONE && act != KK_ACT_GELU) return kk_fail("kk_op_whisper_linear_rows: act must be none (0) or GELU (2)");
  if (ldx < K || ldx % 4 != 0 || ((uintptr_t)x & 15) || ((uintptr_t)w & 15)) return kk_fail("kk_op_whisper_linear_rows: x and w must be 16-byte aligned, ldx >= K, ldx % 4 == 0");
  if ((out && ldo < N) || (res && ldr < N) || (out_bf16 && (ld_bf16 < N || nrows_bf16 < 1))) return kk_fail("kk_op_whisper_linear_rows: a row pitch is smaller than N");
  LinRows a{x, ldx, (const bf16_t*)w, bias, res, ldr, out, ldo, (bf16_t*)out_bf16, ld_bf16, rows_bf16, nrows_bf16, M, N, K, act};
  return launch_linear_rows((hipStream_t)stream, a);
}

extern "C" int kk_op_whisper_embed(void* stream, int R, int D, const int32_t* tok, const int32_t* pos, const void* table_bf16, int n_vocab, const float* positions,
                                   int n_ctx, float* out) {
  if (!tok || !pos || !table_bf16 || !positions || !out) return kk_fail("kk_op_whisper_embed: null argument");
  if (R < 1 || D < 1 || n_vocab < 1 || n_ctx < 1) return kk_fail("kk_op_whisper_embed: bad argument");
  hipLaunchKernelGGL(embed_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, tok, pos, (const bf16_t*)table_bf16, n_vocab, positions, n_ctx, D, out);
  KK_CHECK_LAUNCH();
  return 0;
}

extern "C" int kk_op_whisper_linear_rows_q(void* stream, int M, int N, int K, const float* x, long long ldx, const uint32_t* words, const float* pairs,
                                           int group_size, int bits, const float* bias, int act, const float* res, long long ldr, float* out, long long ldo,
                                           void* out_bf16, long long ld_bf16, const int32_t* rows_bf16, int nrows_bf16) {
  if (!x || !words || !pairs || (!out && !out_bf16)) return kk_fail("kk_op_whisper_linear_rows_q: null argument");
  if (M < 1 || M > 16) return kk_fail("kk_op_whisper_linear_rows_q: 1 <= M <= 16 rows per call");
  if (N < 1 || K < 32 || K % 32 != 0) return kk_fail("kk_op_whisper_linear_rows_q: N >= 1 and K a multiple of 32");
  if (const char* why = q_refusal(K, group_size, bits)) return kk_failf("kk_op_whisper_linear_rows_q: %s (bits 4 or 8, group size 32, 64 or 128 dividing K)", why);
  if (act != KK_ACT_NONE && act != KK_ACT_GELU) return kk_fail("kk_op_whisper_linear_rows_q: act must be none (0) or GELU (2)");
  if (ldx < K || ldx % 4 != 0 || ((uintptr_t)x & 15) || ((uintptr_t)words & 7) || ((uintptr_t)pairs & 7))
    return kk_fail("kk_op_whisper_linear_rows_q: x must be 16-byte, words and pairs 8-byte aligned, ldx >= K, ldx % 4 == 0");
  if ((out && ldo < N) || (res && ldr < N) || (out_bf16 && (ld_bf16 < N || nrows_bf16 < 1))) return kk_fail("kk_op_whisper_linear_rows_q: a row pitch is smaller than N");
  LinRows a{x, ldx, nullptr, bias, res, ldr, out, ldo, (bf16_t*)out_bf16, ld_bf16, rows_bf16, nrows_bf16, M, N, K, act};
  return launch_linear_rows_q((hipStream_t)stream, a, words, (const float2*)pairs, group_size, bits);
}

extern "C" int kk_op_whisper_embed_q(void* stream, int R, int D, const int32_t* tok, const int32_t* pos, const uint32_t* words, const float* pairs, int group_size,
                                     int bits, int n_vocab, const float* positions, int n_ctx, float* out) {
  if (!tok || !pos || !words || !pairs || !positions || !out) return kk_fail("kk_op_whisper_embed_q: null argument");
  if (R < 1 || D < 1 || n_vocab < 1 || n_ctx < 1) return kk_fail("kk_op_whisper_embed_q: bad argument");
  if (const char* why = q_refusal(D, group_size, bits)) return kk_failf("kk_op_whisper_embed_q: %s (bits 4 or 8, group size 32, 64 or 128 dividing D)", why);
  if (((uintptr_t)words & 3) || ((uintptr_t)pairs & 7)) return kk_fail("kk_op_whisper_embed_q: words must be 4-byte and pairs 8-byte aligned");
  return launch_embed_q((hipStream_t)stream, R, D, tok, pos, words, (const float2*)pairs, group_size, bits, n_vocab, positions, n_ctx, out);
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

// ================================================================================================================================ the handle
enum { TW_BF16 = 0, TW_Q8 = 8, TW_Q4 = 4 };  // a matrix's storage; the packed ones by their bits
struct TLin {  // a Linear: bf16 [N][K] dense at `w` of wdev, or (fmt != TW_BF16) the checkpoint's words at `qw` of qdev with its (scale, bias)
               // pairs at `qp` of pdev, quantised in groups of `group`; fp32 bias [N] at `b` of fdev
  size_t w = 0, b = 0, qw = 0, qp = 0;
  int N = 0, K = 0, fmt = TW_BF16, group = 0;
  bool bias = false;
};
struct TQHost {  // a quantised matrix as the checkpoint holds it (kk_whisper_text_load_quantized)
  int O = 0, I = 0, group = 0, bits = 0;
  std::vector<uint32_t> words;
  std::vector<float> scales, biases;
};
struct TLayer {
  TLin q, k, v, out, cq, ckv, cout, mlp1, mlp2;
  size_t attn_ln_w = 0, attn_ln_b = 0, cross_ln_w = 0, cross_ln_b = 0, mlp_ln_w = 0, mlp_ln_b = 0;
};

struct kk_whisper_text {
  kk_whisper_text_config cfg;
  std::map<std::string, HostTensor> host;
  std::map<std::string, TQHost> qhost;
  bool finalized = false;
  bf16_t* wdev = nullptr;  // every bf16 matrix, once: the blocks' Linears and the token embedding [V][D]
  uint32_t* qdev = nullptr;  // the packed matrices' words
  float2* pdev = nullptr;    // and their (scale, bias) pairs
  size_t matrix_bytes = 0, total_bytes = 0;  // device bytes of the matrices / of every weight
  int n_packed = 0, n_bf16 = 0;
  std::vector<std::string> fallbacks;  // "name\treason" of every quantised matrix that was dequantised into a bf16 one
  float* fdev = nullptr;   // biases, LayerNorm parameters, the learned positions
  TLin emb;
  std::vector<TLayer> layers;
  size_t ln_w = 0, ln_b = 0, pos = 0;
  // the window in flight (set_audio): the caller's state buffer, its batch and the rows' common position
  char* state = nullptr;
  int B = 0, at = 0;
  int n_audio = 0, n_group = 1;  // B = n_audio * n_group rows; the n_group rows of a window read ONE cross K/V slice (set_audio_groups)
  bool sampling = false;         // sample_setup: pick launches the sampled kernel until the next pick_setup
  float temperature = 0.f;
  uint64_t seed = 0;
  const float* last_logits = nullptr;  // the last forward's last-position logits [B][last_ld], in the caller's memory
  long long last_ld = 0;
  // beam search (beam_setup): until the next pick_setup, pick runs top-k + select on the caller's beam state and a forward of S = 1 reads
  // the self K/V through the owner table owner[beam_flip]
  bool picking = false, beam = false;  // pick_setup was called on this window; beam_setup after it
  char* beam_state = nullptr;
  int beam_cands = 0, beam_flip = 0, beam_picks = 0, beam_begin = 0;  // max_candidates, the current table, picks so far, the first sampled position
  // row mode (rows_open), beside the window: the caller's second state buffer and what the host knows of every row
  struct Row {
    bool admitted = false;
    int n_init = 0;      // initial tokens uploaded at admission
    int logit = -1;      // the row of the last rows_forward's logits_out that holds this row's last position, -1: none
  };
  char* rows_state = nullptr;
  std::vector<Row> rows;
  const float* rows_logits = nullptr;  // the last rows_forward's logits_out
};

namespace {
int check_text_cfg(const kk_whisper_text_config& c) {
  if (c.n_vocab < 1 || c.n_text_ctx < 1 || c.n_text_layer < 1 || c.n_text_head < 1 || c.n_audio_ctx < 1) return kk_fail("kk_whisper_text_create: bad dimensions");
  if (c.n_text_state != 64 * c.n_text_head) return kk_fail("kk_whisper_text_create: the head dimension n_text_state / n_text_head must be 64");
  if (c.n_text_state % 128 != 0 || c.n_text_state > 2048) return kk_fail("kk_whisper_text_create: n_text_state must be a multiple of 128, at most 2048");
  if (c.n_audio_state != c.n_text_state) return kk_fail("kk_whisper_text_create: n_audio_state must equal n_text_state");
  return 0;
}

struct TextState {  // the caller's state buffer
  bf16_t *cross, *self;  // K | V: cross [layer][n_audio][ctx][2 D], one slice per WINDOW; self [layer][B][ctx][2 D], one per row
  kk_whisper_pick_params* params;
  uint32_t* suppress;
  kk_whisper_pick_state* rows;
  int32_t *tokens, *next, *not_ended;
  uint32_t* streams;  // [B] stream ids of a sampled pick (sample_setup); behind everything the greedy path lays out
};
void plan_state(const kk_whisper_text_config& c, int n_audio, int B, Workspace& ws, TextState& s) {
  const size_t D = c.n_text_state, L = c.n_text_layer;
  s.cross = (bf16_t*)ws.raw(L * n_audio * c.n_audio_ctx * 2 * D * 2);
  s.self = (bf16_t*)ws.raw(L * B * c.n_text_ctx * 2 * D * 2);
  s.params = (kk_whisper_pick_params*)ws.raw(sizeof(kk_whisper_pick_params));
  s.suppress = (uint32_t*)ws.raw(((size_t)c.n_vocab + 31) / 32 * 4);
  s.rows = (kk_whisper_pick_state*)ws.raw((size_t)B * sizeof(kk_whisper_pick_state));
  s.tokens = (int32_t*)ws.raw((size_t)B * c.n_text_ctx * 4);
  s.next = (int32_t*)ws.raw((size_t)B * 4);
  s.not_ended = (int32_t*)ws.raw(4);
  s.streams = (uint32_t*)ws.raw((size_t)B * 4);
}
// the caller's beam state: what a beam search keeps beside the grouped window state of n_audio windows of K rows
void plan_beam(const kk_whisper_text_config& c, int n_audio, int K, int max_candidates, Workspace& ws, kk_whisper_beam_bufs& b) {
  const size_t B = (size_t)n_audio * K, T = c.n_text_ctx, F = (size_t)n_audio * max_candidates;
  b.n_audio = n_audio;
  b.beam_size = K;
  b.max_candidates = max_candidates;
  b.n_ctx = b.cap = c.n_text_ctx;
  b.reserved = 0;
  b.cand_token = (int32_t*)ws.raw(B * (K + 1) * 4);
  b.cand_logprob = (float*)ws.raw(B * (K + 1) * 4);
  b.owner[0] = (int32_t*)ws.raw(B * T * 4);
  b.owner[1] = (int32_t*)ws.raw(B * T * 4);
  b.parent = (int32_t*)ws.raw(B * 4);
  b.fin_score = (float*)ws.raw(F * 4);
  b.fin_length = (int32_t*)ws.raw(F * 4);
  b.fin_tokens = (int32_t*)ws.raw(F * T * 4);
  b.fin_count = (int32_t*)ws.raw((size_t)n_audio * 4);
  b.complete = (int32_t*)ws.raw((size_t)n_audio * 4);
  b.not_complete = (int32_t*)ws.raw(4);
}
struct TextWork {
  float *x, *ln, *q, *att, *h, *scratch;
  int *item, *posr, *len_self, *len_cross, *cache_row;
  bf16_t* feat;
  int* item_cross;  // a grouped state's second row table
};
void plan_work(const kk_whisper_text_config& c, int B, int S, Workspace& ws, TextWork& p) {
  const size_t D = c.n_text_state, R = (size_t)B * S;
  const int Tmax = c.n_audio_ctx > c.n_text_ctx ? c.n_audio_ctx : c.n_text_ctx;
  p.x = (float*)ws.raw(R * D * 4);
  p.ln = (float*)ws.raw(R * D * 4);
  p.q = (float*)ws.raw(R * D * 4);
  p.att = (float*)ws.raw(R * D * 4);
  p.h = (float*)ws.raw(R * 4 * D * 4);
  p.scratch = (float*)ws.raw(attn_scratch_floats((int)R, c.n_text_head, Tmax) * 4);
  p.item = (int*)ws.raw(R * 4);
  p.posr = (int*)ws.raw(R * 4);
  p.len_self = (int*)ws.raw(R * 4);
  p.len_cross = (int*)ws.raw(R * 4);
  p.cache_row = (int*)ws.raw(R * 4);
  p.feat = (bf16_t*)ws.raw((size_t)B * c.n_audio_ctx * D * 2);  // set_audio only
  p.item_cross = (int*)ws.raw(R * 4);
}
int bind(Workspace& ws, void* mem, size_t bytes) {
  ws.base = (char*)(((uintptr_t)mem + 255) & ~(uintptr_t)255);
  const size_t skip = (size_t)(ws.base - (char*)mem);
  ws.cap = bytes > skip ? bytes - skip : 0;
  return 0;
}
}  // namespace

extern "C" int kk_whisper_text_create(const kk_whisper_text_config* cfg, kk_whisper_text** out) {
  if (!cfg || !out) return kk_fail("kk_whisper_text_create: null argument");
  KK_TRY(check_text_cfg(*cfg));
  kk_whisper_text* m = new kk_whisper_text();
  m->cfg = *cfg;
  *out = m;
  return 0;
}

extern "C" void kk_whisper_text_destroy(kk_whisper_text* m) {
  if (!m) return;
  if (m->wdev) (void)hipFree(m->wdev);
  if (m->qdev) (void)hipFree(m->qdev);
  if (m->pdev) (void)hipFree(m->pdev);
  if (m->fdev) (void)hipFree(m->fdev);
  delete m;
}

extern "C" int kk_whisper_text_load_tensor(kk_whisper_text* m, const char* name, const int64_t* shape, int ndim, const float* data) {
  if (!m || !name || !shape || !data || ndim < 1) return kk_fail("kk_whisper_text_load_tensor: bad argument");
  if (m->finalized) return kk_fail("kk_whisper_text_load_tensor: model already finalized");
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
  HostTensor& t = m->host[name];
  t.d.assign(data, data + n);
  t.shape.assign(shape, shape + ndim);
  m->qhost.erase(name);
  return 0;
}

extern "C" int kk_whisper_text_load_quantized(kk_whisper_text* m, const char* name, const int64_t* shape, const uint32_t* words, const float* scales,
                                              const float* biases, int group_size, int bits) {
  if (!m || !name || !shape || !words || !scales || !biases) return kk_fail("kk_whisper_text_load_quantized: bad argument");
  if (m->finalized) return kk_fail("kk_whisper_text_load_quantized: model already finalized");
  if (bits != 2 && bits != 4 && bits != 8)
    return kk_fail("kk_whisper_text_load_quantized: bits must be 2, 4 or 8 (values of a word in bits [j bits, (j + 1) bits))");
  const int64_t O = shape[0], I = shape[1];
  if (O < 1 || I < 1 || O > (1 << 30) || I > (1 << 30) || group_size < 1 || I % group_size != 0 || (I * bits) % 32 != 0)
    return kk_failf("kk_whisper_text_load_quantized: %s: shape / group size", name);
  TQHost& t = m->qhost[name];
  t.O = (int)O; t.I = (int)I; t.group = group_size; t.bits = bits;
  t.words.assign(words, words + (size_t)O * (size_t)(I * bits / 32));
  t.scales.assign(scales, scales + (size_t)O * (size_t)(I / group_size));
  t.biases.assign(biases, biases + (size_t)O * (size_t)(I / group_size));
  m->host.erase(name);
  return 0;
}

namespace {
// the checkpoint's own arithmetic on the host: w = fp32(q) * scale + bias, two roundings (quant.dequantize_affine; dequantize_host of kk_csm.hip)
void text_dequantize(const TQHost& t, std::vector<float>& out) {
  const int per = 32 / t.bits, wpr = t.I / per, ngrp = t.I / t.group;
  const uint32_t mask = (1u << t.bits) - 1u;
  out.resize((size_t)t.O * t.I);
  for (int o = 0; o < t.O; ++o)
    for (int i = 0; i < t.I; ++i) {
      const float qf = (float)((t.words[(size_t)o * wpr + i / per] >> ((i % per) * t.bits)) & mask);
      volatile float prod = qf * t.scales[(size_t)o * ngrp + i / t.group];  // (rounded to fp32 before the add whatever the compiler's contraction rule)
      out[(size_t)o * t.I + i] = prod + t.biases[(size_t)o * ngrp + i / t.group];
    }
}
}  // namespace

extern "C" int kk_whisper_text_finalize(kk_whisper_text* m, void* stream) {
  if (!m) return kk_fail("kk_whisper_text_finalize: null model");
  if (m->finalized) return kk_fail("kk_whisper_text_finalize: already finalized");
  const kk_whisper_text_config& c = m->cfg;
  const int D = c.n_text_state, V = c.n_vocab;
  hipStream_t st = (hipStream_t)stream;
  size_t wn = 0, fn = 0, qn = 0, pn = 0;
  m->n_packed = m->n_bf16 = 0;
  m->fallbacks.clear();
  // `qname`: the one tensor this matrix is made of, which decides its storage if it arrived quantised (empty: a stacked matrix, always bf16)
  auto plan = [&](TLin& l, int N, int K, bool bias, const std::string& qname) {
    l.N = N; l.K = K; l.bias = bias; l.fmt = TW_BF16;
    const auto it = qname.empty() ? m->qhost.end() : m->qhost.find(qname);
    if (it != m->qhost.end() && it->second.O == N && it->second.I == K) {  // (a misshapen one is refused below)
      const TQHost& t = it->second;
      if (const char* why = q_refusal(K, t.group, t.bits)) {
        m->fallbacks.push_back(qname + "\t" + why);
      } else {
        l.fmt = t.bits; l.group = t.group;
        l.qw = qn; qn += ((size_t)N * (K / 32 * t.bits) + 63) & ~(size_t)63;
        l.qp = pn; pn += ((size_t)N * (K / t.group) + 63) & ~(size_t)63;
      }
    }
    if (l.fmt == TW_BF16) { l.w = wn; wn += ((size_t)N * K + 63) & ~(size_t)63; }
    ++(l.fmt == TW_BF16 ? m->n_bf16 : m->n_packed);
    if (bias) { l.b = fn; fn += ((size_t)N + 63) & ~(size_t)63; }
  };
  auto planv = [&](size_t& off, size_t n) { off = fn; fn += (n + 63) & ~(size_t)63; };
  m->layers.resize(c.n_text_layer);
  for (int li = 0; li < c.n_text_layer; ++li) {
    TLayer& L = m->layers[li];
    const std::string p = "decoder.blocks." + std::to_string(li) + ".";
    plan(L.q, D, D, true, p + "attn.query.weight"); plan(L.k, D, D, false, p + "attn.key.weight"); plan(L.v, D, D, true, p + "attn.value.weight");
    plan(L.out, D, D, true, p + "attn.out.weight"); plan(L.cq, D, D, true, p + "cross_attn.query.weight");
    // cross key | value as ONE [2 D][D] Linear (the key's half of the bias is zero); set_audio runs it on the bf16 conv kernel, so it is always bf16
    plan(L.ckv, 2 * D, D, true, "");
    for (const char* part : {"cross_attn.key.weight", "cross_attn.value.weight"})
      if (m->qhost.count(p + part)) m->fallbacks.push_back(p + part + "\tthe stacked cross key | value matrix feeds the bf16 conv kernel");
    plan(L.cout, D, D, true, p + "cross_attn.out.weight");
    plan(L.mlp1, 4 * D, D, true, p + "mlp1.weight"); plan(L.mlp2, D, 4 * D, true, p + "mlp2.weight");
    planv(L.attn_ln_w, D); planv(L.attn_ln_b, D); planv(L.cross_ln_w, D); planv(L.cross_ln_b, D); planv(L.mlp_ln_w, D); planv(L.mlp_ln_b, D);
  }
  plan(m->emb, V, D, false, "decoder.token_embedding.weight");
  planv(m->ln_w, D); planv(m->ln_b, D);
  planv(m->pos, (size_t)c.n_text_ctx * D);

  // everything is checked before anything is allocated
  std::string err;
  auto need = [&](const std::string& name, std::initializer_list<int64_t> shape) -> const HostTensor* {
    auto it = m->host.find(name);
    if (it == m->host.end()) {
      if (err.empty()) err = "missing parameter: " + name;
      return nullptr;
    }
    if (it->second.shape != std::vector<int64_t>(shape)) {
      if (err.empty()) err = "unexpected shape for " + name;
      return nullptr;
    }
    return &it->second;
  };
  std::vector<float> fpack(fn, 0.f);
  auto vecp = [&](size_t off, const std::string& name, int n) {
    if (const HostTensor* t = need(name, {n})) memcpy(&fpack[off], t->d.data(), (size_t)n * 4);
  };
  struct Job { const TLin* l; std::string name; int row0, N; };
  std::vector<Job> jobs;
  auto needw = [&](const std::string& name, int N, int K) {  // a matrix: as floats, or quantised
    const auto it = m->qhost.find(name);
    if (it == m->qhost.end()) need(name, {N, K});
    else if ((it->second.O != N || it->second.I != K) && err.empty()) err = "unexpected shape for " + name;
  };
  auto lin = [&](const TLin& l, const std::string& p, int row0, int N, bool bias) {
    needw(p + ".weight", N, l.K);
    if (bias) vecp(l.b + row0, p + ".bias", N);
    jobs.push_back(Job{&l, p + ".weight", row0, N});
  };
  for (int li = 0; li < c.n_text_layer; ++li) {
    TLayer& L = m->layers[li];
    const std::string p = "decoder.blocks." + std::to_string(li) + ".";
    lin(L.q, p + "attn.query", 0, D, true); lin(L.k, p + "attn.key", 0, D, false); lin(L.v, p + "attn.value", 0, D, true); lin(L.out, p + "attn.out", 0, D, true);
    lin(L.cq, p + "cross_attn.query", 0, D, true); lin(L.ckv, p + "cross_attn.key", 0, D, false); lin(L.ckv, p + "cross_attn.value", D, D, true);
    lin(L.cout, p + "cross_attn.out", 0, D, true);
    lin(L.mlp1, p + "mlp1", 0, 4 * D, true); lin(L.mlp2, p + "mlp2", 0, D, true);
    vecp(L.attn_ln_w, p + "attn_ln.weight", D); vecp(L.attn_ln_b, p + "attn_ln.bias", D);
    vecp(L.cross_ln_w, p + "cross_attn_ln.weight", D); vecp(L.cross_ln_b, p + "cross_attn_ln.bias", D);
    vecp(L.mlp_ln_w, p + "mlp_ln.weight", D); vecp(L.mlp_ln_b, p + "mlp_ln.bias", D);
  }
  needw("decoder.token_embedding.weight", V, D);
  jobs.push_back(Job{&m->emb, "decoder.token_embedding.weight", 0, V});
  vecp(m->ln_w, "decoder.ln.weight", D); vecp(m->ln_b, "decoder.ln.bias", D);
  if (const HostTensor* t = need("decoder.positional_embedding", {c.n_text_ctx, D})) memcpy(&fpack[m->pos], t->d.data(), t->d.size() * 4);
  if (!err.empty()) return kk_failf("kk_whisper_text_finalize: %s", err.c_str());

  if (hipMalloc((void**)&m->wdev, wn * sizeof(bf16_t)) != hipSuccess || hipMalloc((void**)&m->fdev, fn * sizeof(float)) != hipSuccess ||
      (qn && (hipMalloc((void**)&m->qdev, qn * sizeof(uint32_t)) != hipSuccess || hipMalloc((void**)&m->pdev, pn * sizeof(float2)) != hipSuccess)))
    return kk_fail("kk_whisper_text_finalize: hipMalloc failed");
  m->matrix_bytes = wn * sizeof(bf16_t) + qn * sizeof(uint32_t) + pn * sizeof(float2);
  m->total_bytes = m->matrix_bytes + fn * sizeof(float);
  // one matrix at a time, and its host copy dropped -- a large checkpoint is never held twice.  A packed matrix: the checkpoint's words as they are and
  // its scales and biases interleaved.  A bf16 one: dequantised first if it arrived quantised, then rounded to nearest even.
  std::vector<uint16_t> wpack;
  std::vector<float> deq, pairs;
  for (const Job& j : jobs) {
    const auto qi = m->qhost.find(j.name);
    bool ok = true;
    if (j.l->fmt != TW_BF16) {
      const TQHost& t = qi->second;
      const size_t np = t.scales.size();
      pairs.resize(2 * np);
      for (size_t i = 0; i < np; ++i) { pairs[2 * i] = t.scales[i]; pairs[2 * i + 1] = t.biases[i]; }
      ok = hipMemcpyAsync(m->qdev + j.l->qw, t.words.data(), t.words.size() * 4, hipMemcpyHostToDevice, st) == hipSuccess &&
           hipMemcpyAsync(m->pdev + j.l->qp, pairs.data(), np * sizeof(float2), hipMemcpyHostToDevice, st) == hipSuccess;
    } else {
      if (qi != m->qhost.end()) text_dequantize(qi->second, deq);
      const float* src = qi != m->qhost.end() ? deq.data() : m->host[j.name].d.data();
      const size_t n = (size_t)j.N * j.l->K;
      wpack.resize(n);
      for (size_t i = 0; i < n; ++i) wpack[i] = f32_to_bf16_rne(src[i]);
      ok = hipMemcpyAsync((uint16_t*)m->wdev + j.l->w + (size_t)j.row0 * j.l->K, wpack.data(), n * 2, hipMemcpyHostToDevice, st) == hipSuccess;
    }
    if (!ok || hipStreamSynchronize(st) != hipSuccess) return kk_fail("kk_whisper_text_finalize: upload failed");
    m->host.erase(j.name);
    m->qhost.erase(j.name);
  }
  if (hipMemcpyAsync(m->fdev, fpack.data(), fn * 4, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return kk_fail("kk_whisper_text_finalize: upload failed");
  m->host.clear();
  m->qhost.clear();
  m->finalized = true;
  return 0;
}

extern "C" int kk_whisper_text_weight_info(const kk_whisper_text* m, size_t* matrix_bytes, size_t* total_bytes, int* n_packed, int* n_bf16, int* n_fallback) {
  if (!m || !m->finalized) return kk_fail("kk_whisper_text_weight_info: needs a finalized model");
  if (matrix_bytes) *matrix_bytes = m->matrix_bytes;
  if (total_bytes) *total_bytes = m->total_bytes;
  if (n_packed) *n_packed = m->n_packed;
  if (n_bf16) *n_bf16 = m->n_bf16;
  if (n_fallback) *n_fallback = (int)m->fallbacks.size();
  return 0;
}

extern "C" const char* kk_whisper_text_weight_fallback(const kk_whisper_text* m, int i) {
  return m && i >= 0 && i < (int)m->fallbacks.size() ? m->fallbacks[i].c_str() : "";
}

extern "C" size_t kk_whisper_text_state_bytes_groups(const kk_whisper_text* m, int n_audio, int n_group) {
  if (!m || n_audio < 1 || n_group < 1 || n_group > KK_WHISPER_MAX_GROUP) return 0;
  Workspace ws;
  TextState s;
  plan_state(m->cfg, n_audio, n_audio * n_group, ws, s);
  return ws.used + 256;
}

extern "C" size_t kk_whisper_text_state_bytes(const kk_whisper_text* m, int B) { return kk_whisper_text_state_bytes_groups(m, B, 1); }

extern "C" size_t kk_whisper_text_workspace_bytes(const kk_whisper_text* m, int B, int S) {
  if (!m || B < 1 || S < 1) return 0;
  Workspace ws;
  TextWork p;
  plan_work(m->cfg, B, S, ws, p);
  return ws.used + 256;
}

namespace {
// the one body of set_audio (n_group 1) and set_audio_groups: n_audio windows, n_group decoder rows on each window's cross K/V
int text_set_audio(const char* who, kk_whisper_text* m, void* stream, int n_audio, int n_group, const float* audio_features, void* state, size_t state_bytes,
                   void* workspace, size_t workspace_bytes) {
  if (!m || !audio_features || !state || !workspace || n_audio < 1) return kk_failf("%s: bad argument", who);
  if (n_group < 1 || n_group > KK_WHISPER_MAX_GROUP) return kk_failf("%s: n_group = %d is outside [1, %d]", who, n_group, KK_WHISPER_MAX_GROUP);
  if (!m->finalized) return kk_failf("%s: model not finalized", who);
  const kk_whisper_text_config& c = m->cfg;
  const int D = c.n_text_state, ctx = c.n_audio_ctx, B = n_audio * n_group;
  hipStream_t st = (hipStream_t)stream;
  Workspace ss, ws;
  bind(ss, state, state_bytes);
  bind(ws, workspace, workspace_bytes);
  TextState s;
  TextWork p;
  plan_state(c, n_audio, B, ss, s);
  plan_work(c, B, 1, ws, p);
  if (ss.oom) return kk_failf("%s: state buffer too small", who);
  if (ws.oom) return kk_failf("%s: workspace too small", who);
  KK_TRY(kk_launch_convert(audio_features, KK_F32, (long long)ctx * D, D, p.feat, KK_BF16, (long long)ctx * D, D, D, ctx, n_audio, st));  // rounded once
  for (int li = 0; li < c.n_text_layer; ++li) {  // whisper.py:114-116, once per window: key | value of every layer on the bf16 MFMA kernel
    const TLin& l = m->layers[li].ckv;
    KKMfmaArgs g;
    memset(&g, 0, sizeof g);
    g.x = p.feat; g.xbs = (long long)ctx * D; g.ldx = D; g.w = m->wdev + l.w; g.CinP = D; g.CoutP = 2 * D; g.Cin = D;
    g.bias = m->fdev + l.b; g.out = s.cross + (size_t)li * n_audio * ctx * 2 * D; g.obs = (long long)ctx * 2 * D; g.ldo = 2 * D;
    g.Cout = 2 * D; g.Kw = 1; g.mode = KK_CONV; g.stride = 1; g.pad = 0; g.dil = 1; g.Q = ctx; g.Lo_rows = ctx;
    g.lin = KKLen{nullptr, 0, ctx}; g.lout = KKLen{nullptr, 0, ctx};
    g.in_slope = 1.0f; g.scale = 1.0f; g.act = KK_ACT_NONE;
    KK_TRY(kk_launch_conv_mfma(g, n_audio, KK_BF16, st));
  }
  m->state = (char*)state;
  m->B = B;
  m->n_audio = n_audio;
  m->n_group = n_group;
  m->sampling = m->picking = m->beam = false;
  m->at = 0;
  m->last_logits = nullptr;
  return 0;
}
}  // namespace

extern "C" int kk_whisper_text_set_audio(kk_whisper_text* m, void* stream, int B, const float* audio_features, void* state, size_t state_bytes, void* workspace,
                                         size_t workspace_bytes) {
  return text_set_audio("kk_whisper_text_set_audio", m, stream, B, 1, audio_features, state, state_bytes, workspace, workspace_bytes);
}

extern "C" int kk_whisper_text_set_audio_groups(kk_whisper_text* m, void* stream, int n_audio, int n_group, const float* audio_features, void* state,
                                                size_t state_bytes, void* workspace, size_t workspace_bytes) {
  return text_set_audio("kk_whisper_text_set_audio_groups", m, stream, n_audio, n_group, audio_features, state, state_bytes, workspace, workspace_bytes);
}

extern "C" int kk_whisper_text_position(const kk_whisper_text* m) { return m && m->state ? m->at : -1; }

extern "C" int kk_whisper_text_rewind(kk_whisper_text* m, int position) {
  if (!m || !m->state) return kk_fail("kk_whisper_text_rewind: set_audio first");
  if (position < 0 || position > m->at) return kk_failf("kk_whisper_text_rewind: position %d is outside [0, %d]", position, m->at);
  m->at = position;  // the self K/V behind it is overwritten by the next forward; the cross K/V of the window stays
  m->last_logits = nullptr;
  return 0;
}

namespace {
struct QkCapture {  // the capturing forward: raw cross-attention scores of the listed (layer, head) pairs, pair p into qk_out[b][p][s][n_keys]
  const int32_t* pairs;  // host [n_pairs][2]
  int n_pairs, n_keys;
  float* qk_out;
};

// The layer loop and the logits of a forward over R flat rows whose index arrays (p.item, p.posr, p.len_self, p.len_cross, p.cache_row) and embedded
// tokens (p.x) are in place.  `items` slots of n_text_ctx / n_audio_ctx positions per layer in the self / cross stores: the batch of the window, or the
// rows of row mode -- the launches are the same.
struct TextPass {
  kk_whisper_text* m;
  hipStream_t st;
  int items, items_cross;  // slots of the self store (one per row) and of the cross store (one per window)
  bf16_t* self;
  const bf16_t* cross;
  const int* item_cross;   // per flat row, the cross slot it reads (the row's own slot when every row has its window)
  const TextWork& p;
  const int* owner = nullptr;  // a beam's step: the owner table [row][n_text_ctx] the self-attention reads its keys through (null: the row's own slot)

  // a Linear over `rows` rows, 16 at a time (S = 1: one launch, every weight byte read once for the batch)
  int lin(const TLin& l, int n0, int N, const float* x, long long ldx, int rows, int act, const float* res, float* out, long long ldo, bf16_t* ob,
          const int* dst) const {
    const int D = m->cfg.n_text_state;
    for (int r0 = 0; r0 < rows; r0 += 16) {
      LinRows a{x + (long long)r0 * ldx, ldx, m->wdev + l.w + (size_t)n0 * l.K, l.bias ? m->fdev + l.b + n0 : nullptr, res ? res + (long long)r0 * ldo : nullptr, ldo,
                out ? out + (long long)r0 * ldo : nullptr, ldo, ob, 2 * D, dst ? dst + r0 : nullptr, items * m->cfg.n_text_ctx, rows - r0 < 16 ? rows - r0 : 16, N, l.K,
                act};
      if (l.fmt == TW_BF16) {
        KK_TRY(launch_linear_rows(st, a));
      } else {  // the matrix stayed packed: the same product, the B fragments decoded in registers
        a.w = nullptr;
        KK_TRY(launch_linear_rows_q(st, a, m->qdev + l.qw + (size_t)n0 * (l.K / 32 * l.fmt), m->pdev + l.qp + (size_t)n0 * (l.K / l.group), l.group, l.fmt));
      }
    }
    return 0;
  }
  int ln(size_t w, size_t b, const float* src, long long ldx, int rows) const {
    const int D = m->cfg.n_text_state;
    KKLnArgs a;
    memset(&a, 0, sizeof a);
    a.x = src; a.xbs = 0; a.ldx = (int)ldx; a.out = p.ln; a.obs = 0; a.ldo = D; a.C = D; a.Lmax = rows;
    a.len = KKLen{nullptr, 0, rows}; a.w = m->fdev + w; a.bias = m->fdev + b; a.eps = 1e-5f;
    return kk_launch_layernorm(a, 1, KK_F32, st);
  }
  // cap (window mode only): R = B * S rows, S per item
  int layers(int R, const QkCapture* cap, int B, int S) const {
    const kk_whisper_text_config& c = m->cfg;
    const int D = c.n_text_state, H = c.n_text_head;
    for (int li = 0; li < c.n_text_layer; ++li) {  // whisper.py:157-168
      const TLayer& L = m->layers[li];
      bf16_t* selfc = self + (size_t)li * items * c.n_text_ctx * 2 * D;
      const bf16_t* crossc = cross + (size_t)li * items_cross * c.n_audio_ctx * 2 * D;
      KK_TRY(ln(L.attn_ln_w, L.attn_ln_b, p.x, D, R));
      KK_TRY(lin(L.q, 0, D, p.ln, D, R, KK_ACT_NONE, nullptr, p.q, D, nullptr, nullptr));
      KK_TRY(lin(L.k, 0, D, p.ln, D, R, KK_ACT_NONE, nullptr, nullptr, D, selfc, p.cache_row));      // K and V of the new positions straight into the cache
      KK_TRY(lin(L.v, 0, D, p.ln, D, R, KK_ACT_NONE, nullptr, nullptr, D, selfc + D, p.cache_row));
      if (owner)  // causal: row (b, s) sees pos + s + 1 keys
        KK_TRY(launch_attn_rows<true>(st, R, H, p.q, selfc, 0, D, items, c.n_text_ctx, 2 * D, owner, p.len_self, p.att, p.scratch));
      else
        KK_TRY(launch_attn_rows(st, R, H, p.q, selfc, 0, D, items, c.n_text_ctx, 2 * D, p.item, p.len_self, p.att, p.scratch));
      KK_TRY(lin(L.out, 0, D, p.att, D, R, KK_ACT_NONE, p.x, p.x, D, nullptr, nullptr));
      KK_TRY(ln(L.cross_ln_w, L.cross_ln_b, p.x, D, R));
      KK_TRY(lin(L.cq, 0, D, p.ln, D, R, KK_ACT_NONE, nullptr, p.q, D, nullptr, nullptr));
      if (cap) {  // this layer's listed heads, 32 to a launch, each into the slot of its pair
        KKQkSel sel;
        sel.n = 0;
        for (int pi = 0; pi <= cap->n_pairs; ++pi) {
          if (pi < cap->n_pairs && cap->pairs[2 * pi] == li) {
            sel.head[sel.n] = cap->pairs[2 * pi + 1];
            sel.slot[sel.n++] = pi;
          }
          if (sel.n == 32 || (pi == cap->n_pairs && sel.n > 0)) {
            KK_TRY(kk_launch_whisper_qk_rows(st, p.q, crossc, (long long)c.n_audio_ctx * 2 * D, 2 * D, H, B, S, cap->n_keys, sel, cap->qk_out,
                                             (long long)S * cap->n_keys, (long long)cap->n_pairs * S * cap->n_keys, cap->n_keys));
            sel.n = 0;
          }
        }
      }
      KK_TRY(launch_attn_rows(st, R, H, p.q, crossc, 0, D, items_cross, c.n_audio_ctx, 2 * D, item_cross, p.len_cross, p.att, p.scratch));
      KK_TRY(lin(L.cout, 0, D, p.att, D, R, KK_ACT_NONE, p.x, p.x, D, nullptr, nullptr));
      KK_TRY(ln(L.mlp_ln_w, L.mlp_ln_b, p.x, D, R));
      KK_TRY(lin(L.mlp1, 0, 4 * D, p.ln, D, R, KK_ACT_GELU, nullptr, p.h, 4 * D, nullptr, nullptr));
      KK_TRY(lin(L.mlp2, 0, D, p.h, 4 * D, R, KK_ACT_NONE, p.x, p.x, D, nullptr, nullptr));
    }
    return 0;
  }
  // token + position of `R` rows into p.x, from the bf16 table or the packed one
  int embed(int R, const int32_t* tok, const int* posr) const {
    const kk_whisper_text_config& c = m->cfg;
    const TLin& e = m->emb;
    if (e.fmt != TW_BF16)
      return launch_embed_q(st, R, c.n_text_state, tok, posr, m->qdev + e.qw, m->pdev + e.qp, e.group, e.fmt, c.n_vocab, m->fdev + m->pos, c.n_text_ctx, p.x);
    hipLaunchKernelGGL(embed_kernel, dim3(R), dim3(256), 0, st, tok, posr, m->wdev + e.w, c.n_vocab, m->fdev + m->pos, c.n_text_ctx, c.n_text_state, p.x);
    KK_CHECK_LAUNCH();
    return 0;
  }
  // decoder.ln and the tied embedding as the output Linear (whisper.py:247-248) on `rows` rows of x at pitch ldx
  int logits(const float* x, long long ldx, int rows, float* out) const {
    const int D = m->cfg.n_text_state, V = m->cfg.n_vocab;
    KK_TRY(ln(m->ln_w, m->ln_b, x, ldx, rows));
    return lin(m->emb, 0, V, p.ln, D, rows, KK_ACT_NONE, nullptr, out, V, nullptr, nullptr);
  }
};

// the one layer loop behind kk_whisper_text_forward and kk_whisper_text_forward_qk (cap == null: nothing is captured, the launches are those of the plain forward)
int text_forward(const char* who, kk_whisper_text* m, void* stream, int B, int S, const int32_t* tokens, float* logits_out, int all_positions, void* workspace,
                 size_t workspace_bytes, const QkCapture* cap) {
  if (!m || !logits_out || !workspace || B < 1 || S < 1) return kk_failf("%s: bad argument", who);
  if (!m->state || B != m->B) return kk_failf("%s: set_audio first, with the same B", who);
  const kk_whisper_text_config& c = m->cfg;
  if (m->at + S > c.n_text_ctx) return kk_failf("%s: position %d + %d tokens exceeds n_text_ctx = %d", who, m->at, S, c.n_text_ctx);
  const int D = c.n_text_state, V = c.n_vocab, R = B * S;
  hipStream_t st = (hipStream_t)stream;
  Workspace ss, ws;
  bind(ss, m->state, (size_t)-1 / 2);
  bind(ws, workspace, workspace_bytes);
  TextState s;
  TextWork p;
  plan_state(c, m->n_audio, B, ss, s);
  plan_work(c, B, S, ws, p);
  if (ws.oom) return kk_failf("%s: workspace too small", who);
  if (cap && m->n_group != 1) return kk_failf("%s: the window was set with n_group = %d; the capturing forward runs on a plain set_audio state", who, m->n_group);
  int* item_cross = m->n_group > 1 ? p.item_cross : nullptr;  // n_group 1: the row's own slot, one table as before
  const int* owner = nullptr;
  if (m->beam && m->beam_picks > 0) {  // before the first select every row holds its own keys
    if (S != 1) return kk_failf("%s: a beam that has stepped takes one position at a time", who);
    Workspace bs;
    bind(bs, m->beam_state, (size_t)-1 / 2);
    kk_whisper_beam_bufs bb;
    plan_beam(c, m->n_audio, m->n_group, m->beam_cands, bs, bb);
    owner = bb.owner[m->beam_flip];
  }
  if (!tokens) {  // the step after a pick: the tokens it chose
    if (S != 1) return kk_failf("%s: tokens may be null only for S = 1 (the tokens of the last pick)", who);
    tokens = s.next;
  }
  hipLaunchKernelGGL(text_rows_kernel, dim3((R + 255) / 256), dim3(256), 0, st, B, S, m->at, c.n_text_ctx, c.n_audio_ctx, m->n_group, p.item, item_cross, p.posr,
                     p.len_self, p.len_cross, p.cache_row);
  KK_CHECK_LAUNCH();
  const TextPass run{m, st, B, m->n_audio, s.self, s.cross, item_cross ? item_cross : p.item, p, owner};
  KK_TRY(run.embed(R, tokens, p.posr));
  KK_TRY(run.layers(R, cap, B, S));
  if (all_positions) {
    KK_TRY(run.logits(p.x, D, R, logits_out));
    m->last_logits = logits_out + (size_t)(S - 1) * V;  // the last position of item b is S rows after that of item b - 1
    m->last_ld = (long long)S * V;
  } else {
    KK_TRY(run.logits(p.x + (size_t)(S - 1) * D, (long long)S * D, B, logits_out));  // the last position of every item
    m->last_logits = logits_out;
    m->last_ld = V;
  }
  m->at += S;
  return 0;
}
}  // namespace

extern "C" int kk_whisper_text_forward(kk_whisper_text* m, void* stream, int B, int S, const int32_t* tokens, float* logits_out, int all_positions,
                                       void* workspace, size_t workspace_bytes) {
  return text_forward("kk_whisper_text_forward", m, stream, B, S, tokens, logits_out, all_positions, workspace, workspace_bytes, nullptr);
}

extern "C" size_t kk_whisper_text_qk_bytes(const kk_whisper_text* m, int B, int S, int n_pairs, int n_keys) {
  if (!m || B < 1 || S < 1 || n_pairs < 1 || n_keys < 1 || n_keys > m->cfg.n_audio_ctx) return 0;
  return (size_t)B * n_pairs * S * n_keys * sizeof(float);
}

extern "C" int kk_whisper_text_forward_qk(kk_whisper_text* m, void* stream, int B, int S, const int32_t* tokens, float* logits_out, const int32_t* pairs,
                                          int n_pairs, int n_keys, float* qk_out, size_t qk_bytes, void* workspace, size_t workspace_bytes) {
  const char* who = "kk_whisper_text_forward_qk";
  if (!m || !tokens || !pairs || !qk_out || n_pairs < 1) return kk_failf("%s: bad argument", who);
  const kk_whisper_text_config& c = m->cfg;
  if (n_keys < 1 || n_keys > c.n_audio_ctx) return kk_failf("%s: n_keys = %d is outside [1, n_audio_ctx = %d]", who, n_keys, c.n_audio_ctx);
  for (int pi = 0; pi < n_pairs; ++pi)
    if (pairs[2 * pi] < 0 || pairs[2 * pi] >= c.n_text_layer || pairs[2 * pi + 1] < 0 || pairs[2 * pi + 1] >= c.n_text_head)
      return kk_failf("%s: pair %d = (layer %d, head %d) is outside the decoder's %d layers of %d heads", who, pi, pairs[2 * pi], pairs[2 * pi + 1], c.n_text_layer,
                      c.n_text_head);
  if (B < 1 || S < 1 || qk_bytes < kk_whisper_text_qk_bytes(m, B, S, n_pairs, n_keys)) return kk_failf("%s: qk_out too small", who);
  const QkCapture cap{pairs, n_pairs, n_keys, qk_out};
  return text_forward(who, m, stream, B, S, tokens, logits_out, 1, workspace, workspace_bytes, &cap);
}

extern "C" int kk_whisper_text_pick_setup(kk_whisper_text* m, void* stream, const kk_whisper_pick_params* params, const uint32_t* suppress) {
  if (!m || !params) return kk_fail("kk_whisper_text_pick_setup: null argument");
  if (!m->state) return kk_fail("kk_whisper_text_pick_setup: set_audio first");
  const kk_whisper_text_config& c = m->cfg;
  if (params->n_vocab != c.n_vocab) return kk_fail("kk_whisper_text_pick_setup: params.n_vocab differs from the model's");
  if (params->eot < 0 || params->eot >= c.n_vocab || params->timestamp_begin < 0 || params->timestamp_begin > c.n_vocab)
    return kk_fail("kk_whisper_text_pick_setup: token ids outside the vocabulary");
  hipStream_t st = (hipStream_t)stream;
  Workspace ss;
  bind(ss, m->state, (size_t)-1 / 2);
  TextState s;
  plan_state(c, m->n_audio, m->B, ss, s);
  const size_t words = ((size_t)c.n_vocab + 31) / 32;
  if (hipMemcpyAsync(s.params, params, sizeof *params, hipMemcpyHostToDevice, st) != hipSuccess) return kk_fail("kk_whisper_text_pick_setup: upload failed");
  if ((suppress ? hipMemcpyAsync(s.suppress, suppress, words * 4, hipMemcpyHostToDevice, st) : hipMemsetAsync(s.suppress, 0, words * 4, st)) != hipSuccess)
    return kk_fail("kk_whisper_text_pick_setup: upload failed");
  if (hipStreamSynchronize(st) != hipSuccess) return kk_fail("kk_whisper_text_pick_setup: stream sync failed");  // the host arrays may go away
  m->sampling = m->beam = false;
  m->picking = true;
  return kk_op_whisper_pick_reset(stream, m->B, s.rows, s.not_ended);
}

extern "C" int kk_whisper_text_sample_setup(kk_whisper_text* m, void* stream, float temperature, uint64_t seed, const uint32_t* streams) {
  const char* who = "kk_whisper_text_sample_setup";
  if (!m || !streams) return kk_failf("%s: null argument", who);
  if (!m->state) return kk_failf("%s: set_audio first", who);
  if (!(temperature > 0.f) || !std::isfinite(temperature) || !std::isfinite(1.0f / temperature))
    return kk_failf("%s: temperature must be finite and > 0 (temperature 0 is the greedy pick: leave this call out)", who);
  hipStream_t st = (hipStream_t)stream;
  Workspace ss;
  bind(ss, m->state, (size_t)-1 / 2);
  TextState s;
  plan_state(m->cfg, m->n_audio, m->B, ss, s);
  if (hipMemcpyAsync(s.streams, streams, (size_t)m->B * 4, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return kk_failf("%s: upload failed", who);  // synchronised: the host array may go away
  m->sampling = true;
  m->temperature = temperature;
  m->seed = seed;
  return 0;
}

extern "C" int kk_whisper_text_pick(kk_whisper_text* m, void* stream) {
  if (!m) return kk_fail("kk_whisper_text_pick: null model");
  if (!m->state || !m->last_logits) return kk_fail("kk_whisper_text_pick: no logits: run forward first");
  Workspace ss;
  bind(ss, m->state, (size_t)-1 / 2);
  TextState s;
  plan_state(m->cfg, m->n_audio, m->B, ss, s);
  if (m->beam) {
    Workspace bs;
    bind(bs, m->beam_state, (size_t)-1 / 2);
    kk_whisper_beam_bufs bb;
    plan_beam(m->cfg, m->n_audio, m->n_group, m->beam_cands, bs, bb);
    if (m->beam_picks == 0) m->beam_begin = m->at;
    KK_TRY(kk_op_whisper_beam_topk(stream, m->B, m->n_group, m->last_logits, m->last_ld, s.params, s.suppress, s.rows, bb.cand_token, bb.cand_logprob));
    KK_TRY(kk_op_whisper_beam_select(stream, &bb, m->beam_flip, m->at, s.params, s.rows, s.tokens, s.next));
    m->beam_flip ^= 1;
    ++m->beam_picks;
    return 0;
  }
  if (m->sampling)
    return kk_op_whisper_pick_sampled(stream, m->B, m->last_logits, m->last_ld, s.params, s.suppress, m->temperature, m->seed, s.streams, s.rows, s.tokens,
                                      m->cfg.n_text_ctx, s.next, s.not_ended);
  return kk_op_whisper_pick(stream, m->B, m->last_logits, m->last_ld, s.params, s.suppress, s.rows, s.tokens, m->cfg.n_text_ctx, s.next, s.not_ended);
}

extern "C" int kk_whisper_text_not_ended(kk_whisper_text* m, void* stream, int32_t* out) {
  if (!m || !out) return kk_fail("kk_whisper_text_not_ended: null argument");
  if (!m->state) return kk_fail("kk_whisper_text_not_ended: set_audio first");
  Workspace ss;
  bind(ss, m->state, (size_t)-1 / 2);
  TextState s;
  plan_state(m->cfg, m->n_audio, m->B, ss, s);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(out, s.not_ended, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return kk_fail("kk_whisper_text_not_ended: read failed");
  return 0;
}

extern "C" int kk_whisper_text_read(kk_whisper_text* m, void* stream, int32_t* tokens, int cap, kk_whisper_pick_state* rows) {
  if (!m || !tokens || !rows || cap < 1) return kk_fail("kk_whisper_text_read: bad argument");
  if (!m->state) return kk_fail("kk_whisper_text_read: set_audio first");
  Workspace ss;
  bind(ss, m->state, (size_t)-1 / 2);
  TextState s;
  plan_state(m->cfg, m->n_audio, m->B, ss, s);
  hipStream_t st = (hipStream_t)stream;
  const int n = cap < m->cfg.n_text_ctx ? cap : m->cfg.n_text_ctx;
  if (hipMemcpy2DAsync(tokens, (size_t)cap * 4, s.tokens, (size_t)m->cfg.n_text_ctx * 4, (size_t)n * 4, m->B, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(rows, s.rows, (size_t)m->B * sizeof *rows, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return kk_fail("kk_whisper_text_read: read failed");
  return 0;
}

// ---- beam search on a grouped window state ---------------------------------------------------------------------------------------------
extern "C" size_t kk_whisper_text_beam_state_bytes(const kk_whisper_text* m, int n_audio, int beam_size, int max_candidates) {
  if (!m || n_audio < 1 || beam_size < 1 || beam_size > KK_WHISPER_MAX_GROUP || max_candidates < 1 || max_candidates > BEAM_FIN) return 0;
  Workspace ws;
  kk_whisper_beam_bufs b;
  plan_beam(m->cfg, n_audio, beam_size, max_candidates, ws, b);
  return ws.used + 256;
}

extern "C" int kk_whisper_text_beam_setup(kk_whisper_text* m, void* stream, int beam_size, int max_candidates, void* beam_state, size_t bytes) {
  const char* who = "kk_whisper_text_beam_setup";
  if (!m || !beam_state) return kk_failf("%s: null argument", who);
  if (!m->state) return kk_failf("%s: set_audio_groups first", who);
  if (!m->picking) return kk_failf("%s: pick_setup first", who);
  if (beam_size != m->n_group) return kk_failf("%s: beam_size = %d, but the window was set with n_group = %d", who, beam_size, m->n_group);
  if (max_candidates < 1 || max_candidates > BEAM_FIN) return kk_failf("%s: max_candidates = %d is outside [1, %d]", who, max_candidates, BEAM_FIN);
  Workspace bs;
  bind(bs, beam_state, bytes);
  kk_whisper_beam_bufs bb;
  plan_beam(m->cfg, m->n_audio, beam_size, max_candidates, bs, bb);
  if (bs.oom) return kk_failf("%s: beam state buffer too small", who);
  KK_TRY(kk_op_whisper_beam_reset(stream, &bb));
  m->beam_state = (char*)beam_state;
  m->beam_cands = max_candidates;
  m->beam_flip = m->beam_picks = m->beam_begin = 0;
  m->beam = true;
  m->sampling = false;
  return 0;
}

namespace {
int beam_bound(const char* who, const kk_whisper_text* m, kk_whisper_beam_bufs& bb) {
  if (!m) return kk_failf("%s: null model", who);
  if (!m->state || !m->beam) return kk_failf("%s: no beam: kk_whisper_text_beam_setup first", who);
  Workspace bs;
  bind(bs, m->beam_state, (size_t)-1 / 2);
  plan_beam(m->cfg, m->n_audio, m->n_group, m->beam_cands, bs, bb);
  return 0;
}
}  // namespace

extern "C" int kk_whisper_text_beam_not_complete(kk_whisper_text* m, void* stream, int32_t* out) {
  const char* who = "kk_whisper_text_beam_not_complete";
  kk_whisper_beam_bufs bb;
  KK_TRY(beam_bound(who, m, bb));
  if (!out) return kk_failf("%s: null argument", who);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(out, bb.not_complete, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return kk_failf("%s: read failed", who);
  return 0;
}

extern "C" int kk_whisper_text_beam_read(kk_whisper_text* m, void* stream, int cap, int32_t* fin_count, float* fin_score, int32_t* fin_length, int32_t* fin_tokens,
                                         int32_t* live_tokens, float* live_sum, int32_t* live_length) {
  const char* who = "kk_whisper_text_beam_read";
  kk_whisper_beam_bufs bb;
  KK_TRY(beam_bound(who, m, bb));
  if (!fin_count || !fin_score || !fin_length || !fin_tokens || !live_tokens || !live_sum || !live_length || cap < 1) return kk_failf("%s: bad argument", who);
  Workspace ss;
  bind(ss, m->state, (size_t)-1 / 2);
  TextState s;
  plan_state(m->cfg, m->n_audio, m->B, ss, s);
  hipStream_t st = (hipStream_t)stream;
  const int T = m->cfg.n_text_ctx, B = m->B, n = cap < T ? cap : T;
  const size_t F = (size_t)m->n_audio * m->beam_cands;
  std::vector<int32_t> tok((size_t)B * T), own((size_t)B * T);
  std::vector<kk_whisper_pick_state> rows(B);
  if (hipMemcpyAsync(fin_count, bb.fin_count, (size_t)m->n_audio * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(fin_score, bb.fin_score, F * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(fin_length, bb.fin_length, F * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpy2DAsync(fin_tokens, (size_t)cap * 4, bb.fin_tokens, (size_t)T * 4, (size_t)n * 4, F, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(tok.data(), s.tokens, tok.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(own.data(), bb.owner[m->beam_flip], own.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(rows.data(), s.rows, (size_t)B * sizeof(kk_whisper_pick_state), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return kk_failf("%s: read failed", who);
  for (int b = 0; b < B; ++b) {  // a live row's tokens lie where its ancestors wrote them: token i in the row that owns position beam_begin + i
    const int len = rows[b].count < 0 ? 0 : (rows[b].count < n ? rows[b].count : n);
    live_sum[b] = rows[b].sum_logprob;
    live_length[b] = len;
    for (int i = 0; i < len; ++i) {
      const int p = m->beam_begin + i;
      int o = p < T ? own[(size_t)b * T + p] : b;
      if (o < 0 || o >= B) o = b;
      live_tokens[(size_t)b * cap + i] = tok[(size_t)o * T + i];
    }
  }
  return 0;
}

// ================================================================================================================================== row mode
// A second state beside the window's: max_rows decoder rows on the same weights, each with its own cross and self K/V, position (the caller's),
// pick parameters, bitmask, pick state, token stores and two kept logits rows.  A round (rows_forward) is the window's layer loop over any mix of
// prefill and step rows; what differs is the plan kernel in front of it and the per-row pick behind it.  DESIGN 8i.
namespace {
struct RowsState {  // the caller's row-mode state buffer
  bf16_t *cross, *self;  // [layer][max_rows][ctx][2 D]: K | V, the window's layout with the rows as its batch
  kk_whisper_pick_params* params;  // [max_rows]
  uint32_t* suppress;              // [max_rows][words]
  kk_whisper_pick_state* rows;     // [max_rows]; .ended is the row's flag
  int32_t *tokens, *init, *next, *not_ended;  // sampled [max_rows][n_text_ctx], initial [max_rows][n_text_ctx], [max_rows], the reset kernel's counter
  float* kept;                     // [max_rows][2][n_vocab]
};
inline size_t mask_words(const kk_whisper_text_config& c) { return ((size_t)c.n_vocab + 31) / 32; }
void plan_rows_state(const kk_whisper_text_config& c, int N, Workspace& ws, RowsState& s) {
  const size_t D = c.n_text_state, L = c.n_text_layer;
  s.cross = (bf16_t*)ws.raw(L * N * c.n_audio_ctx * 2 * D * 2);
  s.self = (bf16_t*)ws.raw(L * N * c.n_text_ctx * 2 * D * 2);
  s.params = (kk_whisper_pick_params*)ws.raw((size_t)N * sizeof(kk_whisper_pick_params));
  s.suppress = (uint32_t*)ws.raw((size_t)N * mask_words(c) * 4);
  s.rows = (kk_whisper_pick_state*)ws.raw((size_t)N * sizeof(kk_whisper_pick_state));
  s.tokens = (int32_t*)ws.raw((size_t)N * c.n_text_ctx * 4);
  s.init = (int32_t*)ws.raw((size_t)N * c.n_text_ctx * 4);
  s.next = (int32_t*)ws.raw((size_t)N * 4);
  s.not_ended = (int32_t*)ws.raw(4);
  s.kept = (float*)ws.raw((size_t)N * 2 * c.n_vocab * 4);
}
struct RowsWork {
  TextWork t;    // t.feat: ONE window (rows_admit)
  int32_t* tok;  // [R]
};
void plan_rows_work(const kk_whisper_text_config& c, int R, Workspace& ws, RowsWork& p) {
  plan_work(c, 1, R, ws, p.t);  // B = 1, S = R: R flat rows and one window of features
  p.tok = (int32_t*)ws.raw((size_t)R * 4);
}
int rows_bound(const char* who, const kk_whisper_text* m, RowsState& s) {
  if (!m) return kk_failf("%s: null model", who);
  if (!m->rows_state) return kk_failf("%s: row mode not opened (kk_whisper_text_rows_open first)", who);
  Workspace ss;
  bind(ss, m->rows_state, (size_t)-1 / 2);
  plan_rows_state(m->cfg, (int)m->rows.size(), ss, s);
  return 0;
}
int rows_check_row(const char* who, const kk_whisper_text* m, int row, bool admitted) {
  const int N = (int)m->rows.size();
  if (row < 0 || row >= N) return kk_failf("%s: row %d is outside [0, max_rows = %d)", who, row, N);
  if (admitted && !m->rows[row].admitted) return kk_failf("%s: row %d was never admitted", who, row);
  return 0;
}
}  // namespace

extern "C" size_t kk_whisper_text_rows_state_bytes(const kk_whisper_text* m, int max_rows) {
  if (!m || max_rows < 1 || max_rows > KK_WHISPER_MAX_ROWS) return 0;
  Workspace ws;
  RowsState s;
  plan_rows_state(m->cfg, max_rows, ws, s);
  return ws.used + 256;
}

extern "C" size_t kk_whisper_text_rows_workspace_bytes(const kk_whisper_text* m, int max_round_rows, int max_items) {
  if (!m || max_round_rows < 1 || max_items < 1 || max_items > KK_WHISPER_MAX_ROWS) return 0;
  Workspace ws;
  RowsWork p;
  plan_rows_work(m->cfg, max_round_rows, ws, p);
  return ws.used + 256;
}

extern "C" int kk_whisper_text_rows_open(kk_whisper_text* m, void* stream, int max_rows, void* state, size_t state_bytes) {
  const char* who = "kk_whisper_text_rows_open";
  if (!m || !state) return kk_failf("%s: null argument", who);
  if (!m->finalized) return kk_failf("%s: model not finalized", who);
  if (max_rows < 1 || max_rows > KK_WHISPER_MAX_ROWS) return kk_failf("%s: max_rows = %d is outside [1, %d]", who, max_rows, KK_WHISPER_MAX_ROWS);
  Workspace ss;
  bind(ss, state, state_bytes);
  RowsState s;
  plan_rows_state(m->cfg, max_rows, ss, s);
  if (ss.oom) return kk_failf("%s: state buffer too small", who);
  KK_TRY(kk_op_whisper_pick_reset(stream, max_rows, s.rows, s.not_ended));  // every row's flag reads 0 before its first admission
  m->rows_state = (char*)state;
  m->rows.assign(max_rows, kk_whisper_text::Row());
  m->rows_logits = nullptr;
  return 0;
}

extern "C" int kk_whisper_text_rows_admit(kk_whisper_text* m, void* stream, int row, const float* audio_features, const int32_t* tokens, int n,
                                          const kk_whisper_pick_params* params, const uint32_t* suppress, void* workspace, size_t workspace_bytes) {
  const char* who = "kk_whisper_text_rows_admit";
  RowsState s;
  KK_TRY(rows_bound(who, m, s));
  KK_TRY(rows_check_row(who, m, row, false));
  if (!audio_features || !tokens || !params || !workspace) return kk_failf("%s: null argument", who);
  const kk_whisper_text_config& c = m->cfg;
  if (n < 1 || n > c.n_text_ctx) return kk_failf("%s: %d initial tokens are outside [1, n_text_ctx = %d]", who, n, c.n_text_ctx);
  if (params->n_vocab != c.n_vocab) return kk_failf("%s: params.n_vocab differs from the model's", who);
  if (params->eot < 0 || params->eot >= c.n_vocab || params->timestamp_begin < 0 || params->timestamp_begin > c.n_vocab)
    return kk_failf("%s: token ids outside the vocabulary", who);
  const int D = c.n_text_state, ctx = c.n_audio_ctx, N = (int)m->rows.size();
  hipStream_t st = (hipStream_t)stream;
  Workspace ws;
  bind(ws, workspace, workspace_bytes);
  RowsWork p;
  plan_rows_work(c, 1, ws, p);
  if (ws.oom) return kk_failf("%s: workspace too small", who);
  m->rows[row].admitted = false;  // a failure below leaves the row unusable, not half new
  m->rows[row].logit = -1;
  KK_TRY(kk_launch_convert(audio_features, KK_F32, (long long)ctx * D, D, p.t.feat, KK_BF16, (long long)ctx * D, D, D, ctx, 1, st));  // rounded once
  for (int li = 0; li < c.n_text_layer; ++li) {  // set_audio's launch with B = 1, into this row's slice of every layer
    const TLin& l = m->layers[li].ckv;
    KKMfmaArgs g;
    memset(&g, 0, sizeof g);
    g.x = p.t.feat; g.xbs = (long long)ctx * D; g.ldx = D; g.w = m->wdev + l.w; g.CinP = D; g.CoutP = 2 * D; g.Cin = D;
    g.bias = m->fdev + l.b; g.out = s.cross + ((size_t)li * N + row) * ctx * 2 * D; g.obs = (long long)ctx * 2 * D; g.ldo = 2 * D;
    g.Cout = 2 * D; g.Kw = 1; g.mode = KK_CONV; g.stride = 1; g.pad = 0; g.dil = 1; g.Q = ctx; g.Lo_rows = ctx;
    g.lin = KKLen{nullptr, 0, ctx}; g.lout = KKLen{nullptr, 0, ctx};
    g.in_slope = 1.0f; g.scale = 1.0f; g.act = KK_ACT_NONE;
    KK_TRY(kk_launch_conv_mfma(g, 1, KK_BF16, st));
  }
  const size_t words = mask_words(c);
  uint32_t* mask = s.suppress + (size_t)row * words;
  if (hipMemcpyAsync(s.init + (size_t)row * c.n_text_ctx, tokens, (size_t)n * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(s.params + row, params, sizeof *params, hipMemcpyHostToDevice, st) != hipSuccess ||
      (suppress ? hipMemcpyAsync(mask, suppress, words * 4, hipMemcpyHostToDevice, st) : hipMemsetAsync(mask, 0, words * 4, st)) != hipSuccess)
    return kk_failf("%s: upload failed", who);
  if (hipStreamSynchronize(st) != hipSuccess) return kk_failf("%s: stream sync failed", who);  // the host arrays may go away
  KK_TRY(kk_op_whisper_pick_reset(stream, 1, s.rows + row, s.not_ended));
  m->rows[row].admitted = true;
  m->rows[row].n_init = n;
  return 0;
}

extern "C" int kk_whisper_text_rows_forward(kk_whisper_text* m, void* stream, const kk_whisper_rows_item* items, int n_items, const int32_t* out_rows, int n_out,
                                            float* logits_out, void* workspace, size_t workspace_bytes) {
  const char* who = "kk_whisper_text_rows_forward";
  RowsState s;
  KK_TRY(rows_bound(who, m, s));
  if (!items || !out_rows || !logits_out || !workspace) return kk_failf("%s: null argument", who);
  if (n_items < 1 || n_items > KK_WHISPER_MAX_ROWS) return kk_failf("%s: %d items are outside [1, %d]", who, n_items, KK_WHISPER_MAX_ROWS);
  const kk_whisper_text_config& c = m->cfg;
  const int D = c.n_text_state, V = c.n_vocab, N = (int)m->rows.size();
  // everything is checked on the host before anything is launched: the table decides what memory the round reads and writes
  RowItems t;
  memset(&t, 0, sizeof t);
  t.n = n_items;
  long long R = 0;
  unsigned seen = 0;
  for (int i = 0; i < n_items; ++i) {
    const kk_whisper_rows_item& it = items[i];
    KK_TRY(rows_check_row(who, m, it.row, true));
    if (seen >> it.row & 1u) return kk_failf("%s: row %d appears twice in one round", who, it.row);
    seen |= 1u << it.row;
    if (it.count < 1 || it.pos < 0 || (long long)it.pos + it.count > c.n_text_ctx)
      return kk_failf("%s: item %d: position %d + %d tokens exceeds n_text_ctx = %d", who, i, it.pos, it.count, c.n_text_ctx);
    if (it.from < -1) return kk_failf("%s: item %d: from = %d (an offset of the initial tokens, or -1 for the last pick's token)", who, i, it.from);
    if (it.from == -1 && it.count != 1) return kk_failf("%s: item %d: from = -1 (the last pick's token) needs count 1, not %d", who, i, it.count);
    if (it.from == -1 && m->rows[it.row].logit != -2) return kk_failf("%s: item %d: row %d has no picked token to step on", who, i, it.row);
    if (it.from >= 0 && (long long)it.from + it.count > m->rows[it.row].n_init)
      return kk_failf("%s: item %d: from %d + %d tokens is beyond row %d's %d initial tokens", who, i, it.from, it.count, it.row, m->rows[it.row].n_init);
    if (it.keep < -1 || it.keep >= it.count || (it.keep >= 0 && (it.slot < 0 || it.slot > 1)))
      return kk_failf("%s: item %d: keep = %d must be -1 or an offset below count, slot 0 or 1", who, i, it.keep);
    t.row[i] = it.row; t.pos[i] = it.pos; t.count[i] = it.count; t.from[i] = it.from; t.first[i] = (int)R;
    R += it.count;
  }
  Workspace ws;
  bind(ws, workspace, workspace_bytes);
  RowsWork p;
  plan_rows_work(c, (int)R, ws, p);
  if (ws.oom) return kk_failf("%s: workspace too small for R = %lld rows", who, R);
  if (n_out < 1 || n_out > 2 * n_items || n_out > R) return kk_failf("%s: n_out = %d is outside [1, min(2 n_items, R)]", who, n_out);
  std::vector<int> where((size_t)R, -1);  // flat row -> its row of logits_out
  bool identity = n_out == R;
  RowGather sel;
  memset(&sel, 0, sizeof sel);
  for (int j = 0; j < n_out; ++j) {
    if (out_rows[j] < 0 || out_rows[j] >= R) return kk_failf("%s: out_rows[%d] = %d is outside [0, R = %lld)", who, j, out_rows[j], R);
    if (where[out_rows[j]] >= 0) return kk_failf("%s: out_rows lists flat row %d twice", who, out_rows[j]);
    where[out_rows[j]] = j;
    sel.src[j] = out_rows[j];
    identity = identity && out_rows[j] == j;
  }
  for (int i = 0; i < n_items; ++i)
    if (items[i].keep >= 0 && where[t.first[i] + items[i].keep] < 0) return kk_failf("%s: item %d: the kept position is not in out_rows", who, i);

  hipStream_t st = (hipStream_t)stream;
  for (auto& r : m->rows)
    if (r.logit >= 0) r.logit = -1;
  m->rows_logits = logits_out;
  hipLaunchKernelGGL(text_plan_kernel, dim3(((int)R + 255) / 256), dim3(256), 0, st, t, (int)R, c.n_text_ctx, c.n_audio_ctx, s.init, s.next, p.t.item, p.t.posr,
                     p.t.len_self, p.t.len_cross, p.t.cache_row, p.tok);
  KK_CHECK_LAUNCH();
  const TextPass run{m, st, N, N, s.self, s.cross, p.t.item, p.t};
  KK_TRY(run.embed((int)R, p.tok, p.t.posr));
  KK_TRY(run.layers((int)R, nullptr, 0, 0));
  const float* x = p.t.x;
  if (!identity) {  // a round of steps wants every row: nothing to gather
    hipLaunchKernelGGL(gather_rows_kernel, dim3(n_out), dim3(256), 0, st, sel, p.t.x, D, p.t.q);
    KK_CHECK_LAUNCH();
    x = p.t.q;
  }
  KK_TRY(run.logits(x, D, n_out, logits_out));
  for (int i = 0; i < n_items; ++i) {
    const kk_whisper_rows_item& it = items[i];
    kk_whisper_text::Row& r = m->rows[it.row];
    const int last = where[t.first[i] + it.count - 1];
    r.logit = last >= 0 ? last : -1;
    if (it.keep >= 0 && hipMemcpyAsync(s.kept + ((size_t)it.row * 2 + it.slot) * V, logits_out + (size_t)where[t.first[i] + it.keep] * V, (size_t)V * 4,
                                       hipMemcpyDeviceToDevice, st) != hipSuccess)
      return kk_failf("%s: keeping a logits row failed", who);
  }
  return 0;
}

extern "C" int kk_whisper_text_rows_pick(kk_whisper_text* m, void* stream, const int32_t* rows, int n) {
  const char* who = "kk_whisper_text_rows_pick";
  RowsState s;
  KK_TRY(rows_bound(who, m, s));
  if (!rows) return kk_failf("%s: null argument", who);
  if (n < 1 || n > KK_WHISPER_MAX_ROWS) return kk_failf("%s: %d rows are outside [1, %d]", who, n, KK_WHISPER_MAX_ROWS);
  PickSel sel;
  memset(&sel, 0, sizeof sel);
  unsigned seen = 0;
  for (int j = 0; j < n; ++j) {
    KK_TRY(rows_check_row(who, m, rows[j], true));
    if (seen >> rows[j] & 1u) return kk_failf("%s: row %d appears twice", who, rows[j]);
    seen |= 1u << rows[j];
    if (m->rows[rows[j]].logit < 0 || !m->rows_logits) return kk_failf("%s: row %d has no logits of its last position from the last round", who, rows[j]);
    sel.row[j] = rows[j];
    sel.logit[j] = m->rows[rows[j]].logit;
  }
  const kk_whisper_text_config& c = m->cfg;
  hipLaunchKernelGGL(pick_rows_kernel, dim3(n), dim3(1024), 0, (hipStream_t)stream, sel, m->rows_logits, (long long)c.n_vocab, s.params, s.suppress,
                     (int)mask_words(c), s.rows, s.tokens, c.n_text_ctx, s.next);
  KK_CHECK_LAUNCH();
  for (int j = 0; j < n; ++j) m->rows[rows[j]].logit = -2;  // picked: the row can step on its token, and is not picked twice on the same logits
  return 0;
}

extern "C" int kk_whisper_text_rows_flags(kk_whisper_text* m, void* stream, int32_t* ended) {
  const char* who = "kk_whisper_text_rows_flags";
  RowsState s;
  KK_TRY(rows_bound(who, m, s));
  if (!ended) return kk_failf("%s: null argument", who);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpy2DAsync(ended, 4, &s.rows[0].ended, sizeof(kk_whisper_pick_state), 4, m->rows.size(), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return kk_failf("%s: read failed", who);
  return 0;
}

extern "C" int kk_whisper_text_rows_read(kk_whisper_text* m, void* stream, int row, int32_t* tokens, int cap, kk_whisper_pick_state* state, float* kept) {
  const char* who = "kk_whisper_text_rows_read";
  RowsState s;
  KK_TRY(rows_bound(who, m, s));
  KK_TRY(rows_check_row(who, m, row, true));
  if (!tokens || !state || cap < 1) return kk_failf("%s: bad argument", who);
  const kk_whisper_text_config& c = m->cfg;
  hipStream_t st = (hipStream_t)stream;
  const int n = cap < c.n_text_ctx ? cap : c.n_text_ctx;
  if (hipMemcpyAsync(tokens, s.tokens + (size_t)row * c.n_text_ctx, (size_t)n * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(state, s.rows + row, sizeof *state, hipMemcpyDeviceToHost, st) != hipSuccess ||
      (kept && hipMemcpyAsync(kept, s.kept + (size_t)row * 2 * c.n_vocab, (size_t)2 * c.n_vocab * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) ||
      hipStreamSynchronize(st) != hipSuccess)
    return kk_failf("%s: read failed", who);
  return 0;
}

extern "C" int kk_whisper_text_rows_set_token(kk_whisper_text* m, void* stream, int row, int index, const int32_t* token) {
  const char* who = "kk_whisper_text_rows_set_token";
  RowsState s;
  KK_TRY(rows_bound(who, m, s));
  KK_TRY(rows_check_row(who, m, row, true));
  if (!token) return kk_failf("%s: null argument", who);
  if (index < 0 || index >= m->rows[row].n_init) return kk_failf("%s: index %d is outside row %d's %d initial tokens", who, index, row, m->rows[row].n_init);
  if (hipMemcpyAsync(s.init + (size_t)row * m->cfg.n_text_ctx + index, token, 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
    return kk_failf("%s: copy failed", who);
  return 0;
}
