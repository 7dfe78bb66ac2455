// The device code of the CSM frame generator apart from the sampler (kk_csm_sample.hip) and the cache attention (kk_attn_cache.hip), with its launchers,
// the fragment packers and the raw entry points the tests call; kk_csm.hip is the handle that launches it through kk_kernels.h.
//   glue: embedding sums and gathers, RMSNorm, SwiGLU, row copies, the device position, the cache shift, the K / V run copy;
//   Linears: the skinny GEMM of fp32 weights (+ reduce), the matrix-core GEMV of a fragment pack (kk_csm_gemvm.h; + the split-K combine), the prompt GEMM.
#include <math.h>
#include <string.h>

#include "../../include/kokoro_hip.h"
#include "kk_common.h"
#include "kk_host.h"
#include "kk_kernels.h"

namespace {

#include "kk_csm_gemvm.h"

// kk_csm_debug_timestamps: in-kernel wall-clock marks (100 MHz) of the instrumented kernels, 8 words per launch in launch order:
// [class id, earliest workgroup start, latest workgroup end, workgroup 0 after its input loads, workgroup 0's start / shader clock at start / end / shader
// clock at end]; null in production
unsigned long long* g_ts = nullptr;
int g_ts_cap = 0, g_ts_next = 0;
unsigned long long* ts_slot() { return (g_ts && g_ts_next < g_ts_cap) ? g_ts + 8 * (size_t)g_ts_next++ : nullptr; }

// ------------------------------------------------------------------------------------------------------------- kernels
// h[b][s][:] = sum_j mask[b][s][j] * emb_j(tokens[b][s][j]),  j < n_cb: audio_embeddings[token + j*V], j = n_cb: text_embeddings
__global__ __launch_bounds__(256) void embed_sum_kernel(const int* tokens, const float* mask, const float* audio, const float* text, int ncb, int V, int TV,
                                                        int D, float* h) {
  // grid (row = b * S + s, column block of 256).  The row's ids and masks go to LDS first so that the 33 embedding loads of a column do not wait on 33
  // dependent id loads (the first form walked them one L2 round trip at a time: 60-130 us for the 8 rows of a single-token frame); the loads of 16
  // code books are in flight together, the sum stays in code-book order.
  __shared__ int tk_s[72];
  __shared__ float mk_s[72];
  const long long row = blockIdx.x;
  const int c = blockIdx.y * 256 + threadIdx.x;
  if ((int)threadIdx.x <= ncb) {
    const int j = threadIdx.x;
    tk_s[j] = j < ncb ? clamp_id(tokens[row * (ncb + 1) + j], V) + j * V : clamp_id(tokens[row * (ncb + 1) + j], TV);
    mk_s[j] = mask[row * (ncb + 1) + j];
  }
  __syncthreads();
  if (c >= D) return;
  float acc = 0.f;
  for (int j0 = 0; j0 <= ncb; j0 += 16) {
    float v[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      const int j = j0 + jj <= ncb ? j0 + jj : ncb;
      v[jj] = (j < ncb ? audio : text)[(long long)tk_s[j] * D + c];
    }
#pragma unroll
    for (int jj = 0; jj < 16; ++jj)
      if (j0 + jj <= ncb) acc += v[jj] * mk_s[j0 + jj];
  }
  h[row * D + c] = acc;
}

// rows of audio_embeddings for code book `cb`: out[b][pos][:] = audio[(codes[b] + cb*V)][:]   (out row pitch = rows*D per item)
__global__ __launch_bounds__(256) void embed_audio_kernel(const int* codes, int cstride, const float* audio, int cb, int V, int D, float* out, int rows,
                                                          int pos) {
  const int b = blockIdx.x;
  const float* e = audio + ((long long)clamp_id(codes[(long long)b * cstride], V) + (long long)cb * V) * D;
  for (int c = threadIdx.x; c < D; c += 256) out[((long long)b * rows + pos) * D + c] = e[c];
}

__global__ __launch_bounds__(256) void copy_rows_kernel(const float* src, long long sbs, float* dst, long long dbs, int D) {
  const int b = blockIdx.x;
  for (int c = threadIdx.x; c < D; c += 256) dst[(long long)b * dbs + c] = src[(long long)b * sbs + c];
}

// RMSNorm over the last axis, fp32: x * rsqrt(mean(x^2) + eps) * w
__global__ __launch_bounds__(256) void rmsnorm_kernel(const float* x, const float* w, int D, float eps, float* out) {
  __shared__ float red[4];
  const long long row = blockIdx.x;
  const float* xr = x + row * D;
  float ss = 0.f;
  for (int c = threadIdx.x; c < D; c += 256) ss = __builtin_fmaf(xr[c], xr[c], ss);
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
  __syncthreads();
  const float tot = (red[0] + red[1]) + (red[2] + red[3]);
  const float r = 1.0f / sqrtf(tot / (float)D + eps);
  for (int c = threadIdx.x; c < D; c += 256) out[row * D + c] = xr[c] * r * w[c];
}

__global__ void advance_pos_kernel(int* pos, int by) { *pos += by; }

// kk_csm_shift_caches: the window [pad[b], P) of every live row moves by `delta` slots, in every layer, K (blockIdx.z even) and V (odd).
// Source and destination overlap whenever |delta| is smaller than the row's length, so the walk is ordered PER THREAD: a thread owns one
// 16-byte column of the row (rowf4 = KV hd / 4 of them, 64 neighbours per workgroup: a slot is read and written in 1 KiB pieces) and moves it
// slot by slot in the safe direction -- ascending for a move down, descending for a move up --, eight slots per trip, all eight loads in
// front of the eight stores.  A store lands on a slot this thread has already read (or outside the window), and no other thread touches the
// column, so no barrier or bounce buffer is needed.  P and pad are read from device memory; they are updated behind this kernel in stream order.
// The host has checked that every live window stays inside [0, max_pos); the same test here turns a violation into a no-op for that row.
__global__ __launch_bounds__(64) void shift_cache_kernel(float* kc, float* vc, int maxB, int max_pos, int rowf4, const int* pos_dev, const int* pad,
                                                         int delta) {
  const int c = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y, layer = blockIdx.z >> 1;
  if (c >= rowf4) return;
  const int hi = *pos_dev, lo = pad[b];
  if (lo >= hi || lo < 0 || lo + delta < 0 || hi + delta > max_pos) return;  // parked / empty row, or a window that would leave the cache
  float4* base = (float4*)((blockIdx.z & 1) ? vc : kc) + ((long long)layer * maxB + b) * max_pos * rowf4 + c;
  float4 r[8];
  if (delta < 0) {
    for (int s = lo; s < hi; s += 8) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (s + i < hi) r[i] = base[(long long)(s + i) * rowf4];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (s + i < hi) base[(long long)(s + i + delta) * rowf4] = r[i];
    }
  } else {
    for (int s = hi - 1; s >= lo; s -= 8) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (s - i >= lo) r[i] = base[(long long)(s - i) * rowf4];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (s - i >= lo) base[(long long)(s - i + delta) * rowf4] = r[i];
    }
  }
}

// One contiguous run of seg4 16-byte columns per (layer, K | V) from one K / V store to another, every layer's K and V in one launch: blockIdx.y =
// 2 layer + (0 K, 1 V); only the layer pitches of the two sides differ.  Three callers, which have added row and first slot to a cache's pointers:
//   kk_csm_admit_prefixed  a compact prefix buffer ([layer][K|V][n][KV hd] fp32: K base buf, V base buf + n KV hd, layer pitch 2 n KV hd) goes under a
//                          stream's suffix, into n slots of ONE cache row;
//   kk_csm_prefix_capture  the mirror: the first n slots of ONE live row leave for a new prefix buffer;
//   kk_csm_admit_transfer  the window of ONE live row of another generator's cache goes into as many slots of ONE row of this one (max_batch * max_pos of
//                          the two need not match).  A key is stored rotated by its stream's own position, so every one of these moves is a plain copy.
// A workgroup owns 16 KiB of the run (eight 2 KiB slot rows at CSM-1B's geometry), a thread four columns 4 KiB apart -- every wave instruction moves
// 1 KiB of consecutive bytes --, the four loads are issued ahead of the four stores, the tail is checked.  Default cache policy on both sides: a prefix is
// read again by the next admission (10 MB at n = 160 stay in the last-level cache) and the row is read right behind by the suffix block's attention.  It
// reads nothing outside the source runs and writes nothing outside the destination's.
__global__ __launch_bounds__(256) void kv_runs_copy_kernel(const float* skc, const float* svc, long long src_pitch4, float* kc, float* vc,
                                                           long long dst_pitch4, long long seg4) {
  const int z = blockIdx.y;
  const float4* s = (const float4*)((z & 1) ? svc : skc) + (long long)(z >> 1) * src_pitch4;
  float4* d = (float4*)((z & 1) ? vc : kc) + (long long)(z >> 1) * dst_pitch4;
  const long long i0 = (long long)blockIdx.x * 1024 + threadIdx.x;
  float4 r[4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (i0 + 256 * u < seg4) r[u] = s[i0 + 256 * u];
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (i0 + 256 * u < seg4) d[i0 + 256 * u] = r[u];
}

// silu(gate) * up, gu [rows][2I] -> [rows][I]
__global__ __launch_bounds__(256) void swiglu_kernel(const float* gu, int I, long long n, float* out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const long long r = e / I;
  const int c = (int)(e - r * I);
  const float g = gu[r * 2 * I + c], u = gu[r * 2 * I + I + c];
  out[e] = (g / (1.0f + expf(-g))) * u;
}

// Skinny GEMM for the single-token steps (M = B rows <= 16): out[m][n] = sum_k x[m][k] W[k][n].  The grid is (column blocks) x (KS
// slices of K): every thread streams ONE column (fp32 weights) or TWO adjacent columns (bf16 weights, one 4-byte load) of its K slice
// with coalesced row reads, 16 loads in flight; the slices' partial sums are added in slice order by the second kernel
// (deterministic, residual fused).  The rows are held as PACKED PAIRS: xs[k][m] keeps the M activations of one k adjacent, so a
// weight meets rows (2i, 2i+1) in one v_pk_fma_f32 -- MT/2 packed FMAs per weight (MT = 8 or 16 rows, a template parameter).  The
// first version issued 16 predicated scalar FMAs per weight whatever M was and was VALU-bound (K*N*16 lane-FMAs: 13.6 us for the
// backbone's gate|up matrix against a 13 us HBM floor in bf16), which is why halving the weight bytes did not pay before.
// `GATED`: x is the gate|up pair of a SwiGLU MLP ([M][2K]) and the staged input is silu(gate) * up (the stand-alone swiglu kernel of
// the single-token step disappears).
constexpr int SK_MAXM = KK_CSM_SKINNY_MAXM, SK_KC = 256;
typedef float sk2f __attribute__((ext_vector_type(2)));
template <int MT, bool BF16W, bool GATED>
__global__ __launch_bounds__(256) void skinny_gemm_kernel(const float* x, int M, int K, const void* wv_, int ldw, int N, int kchunk, float* part) {
  constexpr int NC = BF16W ? 2 : 1;  // columns per thread
  constexpr int MP = MT / 2;         // row pairs
  __shared__ __attribute__((aligned(16))) float xs[SK_KC][MT];
  const int n = (blockIdx.x * 256 + threadIdx.x) * NC, ks = blockIdx.y;
  const int k0 = ks * kchunk, k1 = min(K, k0 + kchunk);
  sk2f acc[NC][MP];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int i = 0; i < MP; ++i) acc[c][i] = sk2f{0.f, 0.f};
  for (int kb = k0; kb < k1; kb += SK_KC) {
    const int kn = min(SK_KC, k1 - kb);
    __syncthreads();
    for (int e = threadIdx.x; e < MT * kn; e += 256) {
      const int m = e / kn, k = e - m * kn;  // consecutive threads read consecutive k of one row
      float v = 0.f;
      if (m < M) {
        if (GATED) {
          const float g = x[(long long)m * 2 * K + kb + k], u = x[(long long)m * 2 * K + K + kb + k];
          v = g / (1.0f + expf(-g)) * u;
        } else {
          v = x[(long long)m * K + kb + k];
        }
      }
      xs[k][m] = v;
    }
    __syncthreads();
    if (n < N) {
      const unsigned* wp = BF16W ? (const unsigned*)((const uint16_t*)wv_ + (long long)kb * ldw + n) : (const unsigned*)((const float*)wv_ + (long long)kb * ldw + n);
      const long long ldq = BF16W ? (ldw >> 1) : ldw;  // row pitch in 4-byte words
      auto fma_k = [&](unsigned wbits, int k) {
        const sk2f* xr = (const sk2f*)&xs[k][0];
        if (BF16W) {
          const float w0 = __uint_as_float(wbits << 16), w1 = __uint_as_float(wbits & 0xffff0000u);
#pragma unroll
          for (int i = 0; i < MP; ++i) {
            const sk2f xv = xr[i];
            acc[0][i] = __builtin_elementwise_fma(xv, sk2f{w0, w0}, acc[0][i]);
            acc[NC - 1][i] = __builtin_elementwise_fma(xv, sk2f{w1, w1}, acc[NC - 1][i]);
          }
        } else {
          const float w0 = __uint_as_float(wbits);
#pragma unroll
          for (int i = 0; i < MP; ++i) acc[0][i] = __builtin_elementwise_fma(xr[i], sk2f{w0, w0}, acc[0][i]);
        }
      };
      int k = 0;
      for (; k + 16 <= kn; k += 16) {  // 16 independent loads in flight per thread
        unsigned wv[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) wv[j] = wp[(long long)(k + j) * ldq];
#pragma unroll
        for (int j = 0; j < 16; ++j) fma_k(wv[j], k + j);
      }
      for (; k < kn; ++k) fma_k(wp[(long long)k * ldq], k);
    }
  }
  if (n < N) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (n + c >= N) continue;
#pragma unroll
      for (int i = 0; i < MP; ++i) {
        // slices of one output element are contiguous
        if (2 * i < M) part[((long long)(2 * i) * N + n + c) * gridDim.y + ks] = acc[c][i].x;
        if (2 * i + 1 < M) part[((long long)(2 * i + 1) * N + n + c) * gridDim.y + ks] = acc[c][i].y;
      }
    }
  }
}

__global__ __launch_bounds__(256) void skinny_reduce_kernel(const float* part, int KS, int M, int N, const float* res, float* out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)M * N) return;
  const float* p = part + e * KS;
  float v = 0.f;
  int ks = 0;
  if ((KS & 3) == 0) {
    for (; ks < KS; ks += 4) {
      const float4 q = *(const float4*)(p + ks);
      v += q.x; v += q.y; v += q.z; v += q.w;  // slice order
    }
  }
  for (; ks < KS; ++ks) v += p[ks];
  if (res) v += res[e];
  out[e] = v;
}


// ---------------------------------------------------------------------------------------------------------------------------------------
// h[m][n] += sum over the K slices of a split-K launch (slice order): the combine of the deep down projections
__global__ __launch_bounds__(256) void combine_slices_kernel(const float* part, int KS, long long pss, long long n, float* h, unsigned long long* ts) {
  ts_begin(ts, 2);
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  // all slices are requested at once (a plain loop is KS dependent L2 round trips); KS <= 16 (KKCsmWeight::ks)
  float v[16];
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) v[ks] = part[(long long)(ks < KS ? ks : 0) * pss + e];
  const float h0 = h[e];
  float t = 0.f;
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) t += ks < KS ? v[ks] : 0.f;
  h[e] = h0 + t;
  ts_end(ts);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// gemmp_kernel (round 3): the PROMPT block's Linear layers (M = B x S rows, hundreds to thousands) on the matrix cores, from the same bf16
// fragment pack and with the same exact three-way bf16 split of the fp32 input as gemvm_kernel -- out[M][N] = x[M][K] W (+ res) in
// fp32 arithmetic on bf16 weights.  Round 2 ran the prompt through the library's generic fp32 conv kernel (64 launches, 37 ms for a
// 64-token prompt at B = 8).  A workgroup (4 waves) owns 64 rows x 64 columns (four 16-column sub-blocks, whatever the pack's nsub) and
// walks K in 32-row chunks: the A operands of a chunk (4 row tiles x 3 terms x 1 KiB) are split on the way from global memory into a
// double-buffered LDS tile while the matrix instructions of the previous chunk run; wave w multiplies row tile w with all four
// B fragments (16-byte loads, one chunk ahead).  The three terms of a row accumulate into the SAME accumulator (x1 W + x2 W + x3 W), so a
// row's result depends on nothing but its own input row: the prompt block is batch-invariant.
struct GPArgs {
  const float* x; long long xrs;
  const void* w;
  int K, N, M, nsub;
  const float* res; long long rrs;
  float* out; long long ors;
  const float2* wp; int gmagic, fmt;  // quantised fragment packs (kk_csm_gemvm.h): pairs, wf_group_magic(group), KK_WF_*
};
// FMT: the B fragments arrive as bf16, or as the quantised integers + one (scale, bias) pair per lane, decoded to bf16 in registers ahead of a
// chunk's matrix instructions (every wave decodes the four fragments it multiplies)
template <int FMT>
__global__ __launch_bounds__(256) void gemmp_kernel(GPArgs a) {
  // RT row tiles of 16 per workgroup (one per wave), KC 32-row K chunks per barrier.  Measured, prefill of 190 positions, RT x KC: 30.7 / 31.1 /
  // 33.9 / 36.3 ms for 4 x 2 / 4 x 1 / 8 x 2 / 8 x 1 -- the split arithmetic redone per column tile, not the tile shape, is what is left
  constexpr int RT = 4, KC = 2;
  constexpr int NIT = RT / 4;      // row tiles per wave
  constexpr int NLD = RT / 2;      // float4 loads per thread and chunk: (16 RT rows) x (8 quads of 4 k) / 256 threads
  constexpr int KOP = 384, FRAGB = 4 * KOP;  // k-octet pitch in bytes (256 of data: the two k octets a wave's 8-byte writes touch share no bank), fragment bytes
  constexpr int CHB = RT * 3 * FRAGB;        // one chunk's A operands: [row tile][term][k octet][16 rows][8 bf16]
  extern __shared__ __attribute__((aligned(16))) unsigned char abuf[];  // [2 buffers][KC chunks][CHB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * (16 * RT), sb0 = blockIdx.x * 4, nch = a.K >> 5;
  typedef typename WFrag<FMT>::Q u32x4;  // (a lane's fragment: 16 bytes of bf16, or 8 / 4 bytes of integers)
  // B fragment of (chunk c, global sub-block sb): block sb / nsub, sub sb % nsub of the pack [block][chunk][sub][lane]
  const int nsbt = (a.N + 15) >> 4;
  const u32x4* bp[4];
  const float2* pp[4];  // pairs of (group g, sub-block sb): [block][group][sub][16 columns]
  const int ngrp = FMT == KK_WF_BF16 ? 0 : wf_group(nch, a.gmagic);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int sb = sb0 + s < nsbt ? sb0 + s : nsbt - 1;  // (a sub-block past the end repeats the last one; its columns are not stored)
    bp[s] = (const u32x4*)a.w + ((long long)(sb / a.nsub) * nch * a.nsub + sb % a.nsub) * 64 + lane;
    pp[s] = FMT == KK_WF_BF16 ? nullptr : a.wp + ((long long)(sb / a.nsub) * ngrp * a.nsub + sb % a.nsub) * 16 + (lane & 15);
  }
  const long long bstep = (long long)a.nsub * 64;  // per chunk
  const long long pstep = (long long)a.nsub * 16;  // per group
  // A staging: thread (row tid / 8 + 32 it, quad tid % 8) takes 4 consecutive k of its row: the 8 lanes of a row read one whole 128-byte line
  // (a thread per (row, k octet) read 64 different lines per wave instruction: the first form of this kernel was bound by exactly that)
  const int aq = tid & 7, ar0 = tid >> 3;
  const float* arow[NLD];
  int aoff[NLD];
#pragma unroll
  for (int it = 0; it < NLD; ++it) {
    const int rl = ar0 + 32 * it, row = m0 + rl;
    arow[it] = a.x + (long long)(row < a.M ? row : a.M - 1) * a.xrs + aq * 4;
    aoff[it] = (rl >> 4) * 3 * FRAGB + (aq >> 1) * KOP + (rl & 15) * 16 + (aq & 1) * 8;
  }
  float4 g[KC][NLD];
  u32x4 b[KC][4], bn[KC][4];
  float2 pb[FMT == KK_WF_BF16 ? 1 : KC][4] = {}, pbn[FMT == KK_WF_BF16 ? 1 : KC][4] = {};
  // (a chunk index past the end is clamped: the loads stay unconditional, the extra operands are never multiplied)
  auto load_ab = [&](int c0, u32x4 (&bd)[KC][4], float2 (&pd)[FMT == KK_WF_BF16 ? 1 : KC][4]) __attribute__((always_inline)) {
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      const int c = c0 + kc < nch ? c0 + kc : nch - 1;
#pragma unroll
      for (int it = 0; it < NLD; ++it) g[kc][it] = *(const float4*)(arow[it] + 32 * c);
#pragma unroll
      for (int s = 0; s < 4; ++s) bd[kc][s] = *(bp[s] + (long long)c * bstep);
      if constexpr (FMT != KK_WF_BF16) {
        const int gq = wf_group(c, a.gmagic);
#pragma unroll
        for (int s = 0; s < 4; ++s) pd[kc][s] = *(pp[s] + (long long)gq * pstep);
      }
    }
  };
  auto store_a = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int kc = 0; kc < KC; ++kc)
#pragma unroll
      for (int it = 0; it < NLD; ++it) {
        const float t[4] = {g[kc][it].x, g[kc][it].y, g[kc][it].z, g[kc][it].w};
        unsigned x1[2], x2[2], x3[2];
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          const float a0 = t[e], a1 = t[e + 1];
          const float b0 = a0 - __uint_as_float(__float_as_uint(a0) & 0xffff0000u), b1 = a1 - __uint_as_float(__float_as_uint(a1) & 0xffff0000u);
          const float c0 = b0 - __uint_as_float(__float_as_uint(b0) & 0xffff0000u), c1 = b1 - __uint_as_float(__float_as_uint(b1) & 0xffff0000u);
          x1[e >> 1] = __builtin_amdgcn_perm(__float_as_uint(a1), __float_as_uint(a0), 0x07060302u);
          x2[e >> 1] = __builtin_amdgcn_perm(__float_as_uint(b1), __float_as_uint(b0), 0x07060302u);
          x3[e >> 1] = __builtin_amdgcn_perm(__float_as_uint(c1), __float_as_uint(c0), 0x07060302u);
        }
        unsigned char* d = abuf + (buf * KC + kc) * CHB + aoff[it];
        *(uint2*)d = make_uint2(x1[0], x1[1]);
        *(uint2*)(d + FRAGB) = make_uint2(x2[0], x2[1]);
        *(uint2*)(d + 2 * FRAGB) = make_uint2(x3[0], x3[1]);
      }
  };
  kk_f32x4 acc[NIT][4];
#pragma unroll
  for (int mi = 0; mi < NIT; ++mi)
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[mi][s] = kk_f32x4{0.f, 0.f, 0.f, 0.f};
  load_ab(0, b, pb);
  store_a(0);
  __syncthreads();
  const int rdoff = (lane >> 4) * KOP + (lane & 15) * 16;
  int buf = 0;
  for (int c = 0; c < nch; c += KC, buf ^= 1) {
    load_ab(c + KC, bn, pbn);  // the next step's operands: in flight under this step's matrix instructions
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      if (c + kc < nch) {
        kk_bf16x8 bf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) bf[s] = wf_decode(b[kc][s], pb[FMT == KK_WF_BF16 ? 0 : kc][s]);
#pragma unroll
        for (int mi = 0; mi < NIT; ++mi)
#pragma unroll
          for (int t = 0; t < 3; ++t) {
            const kk_bf16x8 af = *(const kk_bf16x8*)(abuf + (buf * KC + kc) * CHB + ((NIT * wave + mi) * 3 + t) * FRAGB + rdoff);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[mi][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf[s], acc[mi][s], 0, 0, 0);
          }
      }
    }
    store_a(buf ^ 1);
#pragma unroll
    for (int kc = 0; kc < KC; ++kc)
#pragma unroll
      for (int s = 0; s < 4; ++s) b[kc][s] = bn[kc][s];
    if constexpr (FMT != KK_WF_BF16) {
#pragma unroll
      for (int kc = 0; kc < KC; ++kc)
#pragma unroll
        for (int s = 0; s < 4; ++s) pb[kc][s] = pbn[kc][s];
    }
    __syncthreads();
  }
#pragma unroll
  for (int mi = 0; mi < NIT; ++mi)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int n = (sb0 + s) * 16 + (lane & 15);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long row = m0 + (NIT * wave + mi) * 16 + 4 * (lane >> 4) + i;
        if (row < a.M && n < a.N) {
          float v = acc[mi][s][i];
          if (a.res) v += a.res[row * a.rrs + n];
          a.out[row * a.ors + n] = v;
        }
      }
    }
}
// one launch of the prompt GEMM (64-row tiles)
int launch_gemmp(const GPArgs& g, hipStream_t st) {
  const size_t lds = (size_t)2 * 2 * 4 * 3 * 1536;  // [2 buffers][KC chunks][RT row tiles][3 terms][1536-byte fragments]
  static KKDevOnce attr;
  if (attr.first()) {
    (void)hipFuncSetAttribute((const void*)gemmp_kernel<KK_WF_BF16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipFuncSetAttribute((const void*)gemmp_kernel<KK_WF_Q8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipFuncSetAttribute((const void*)gemmp_kernel<KK_WF_Q4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr.done();
  }
  if (g.fmt != KK_WF_BF16 && !g.wp) return kk_fail("kk_csm: internal: quantised prompt GEMM without pairs");
  const dim3 grid((g.N + 63) / 64, (g.M + 63) / 64);
  if (g.fmt == KK_WF_Q8) hipLaunchKernelGGL(gemmp_kernel<KK_WF_Q8>, grid, dim3(256), lds, st, g);
  else if (g.fmt == KK_WF_Q4) hipLaunchKernelGGL(gemmp_kernel<KK_WF_Q4>, grid, dim3(256), lds, st, g);
  else hipLaunchKernelGGL(gemmp_kernel<KK_WF_BF16>, grid, dim3(256), lds, st, g);
  KK_CHECK_LAUNCH();
  return 0;
}
// the prompt GEMM of a packed matrix (bf16 or quantised fragments)
static void gemmp_weights(GPArgs& g, const KKCsmWeight& w) {
  g.w = w.wm; g.nsub = w.nsub; g.fmt = w.fmt; g.wp = w.wp; g.gmagic = w.fmt != KK_WF_BF16 ? wf_group_magic(w.group) : 0;
}

// The skinny GEMM's K slices (fp32 weights, single-token steps): ~4 workgroups per CU (measured: fewer, longer slices are slower -- the kernel is
// latency-bound); depends on the matrix only
static void skinny_plan(int K, int N, int* KS_out, int* kchunk_out) {
  const int nblk256 = kk_cdiv(N, 256);
  int KS = 1024 / nblk256;
  int maxks = kk_cdiv(K, 32);
  if (maxks > 128) maxks = 128;  // deep, narrow matrices (down projections: K = 8192, N = 1024 / 2048) need the slices to fill the chip
  KS = KS < 1 ? 1 : (KS > maxks ? maxks : KS);
  const int kchunk = kk_cdiv(kk_cdiv(K, KS), 32) * 32;
  *KS_out = kk_cdiv(K, kchunk);
  *kchunk_out = kchunk;
}
// out[m][:] = x[m] W (+ res[m]) for Mtot contiguous rows, in launches of <= 16 rows; part: KS * 16 * N floats
static int launch_skinny(const float* x, int Mtot, int K, int N, const float* w, int ldw, int KS, int kchunk, const float* res, float* out, float* part,
                         hipStream_t st) {
  const int nblk = kk_cdiv(N, 256);
  for (int m0 = 0; m0 < Mtot; m0 += SK_MAXM) {
    const int M = Mtot - m0 < SK_MAXM ? Mtot - m0 : SK_MAXM;
    const float* xin = x + (size_t)m0 * K;
    const dim3 g(nblk, KS), t(256);
#define SK_GO(MT) hipLaunchKernelGGL((skinny_gemm_kernel<MT, false, false>), g, t, 0, st, xin, M, K, (const void*)w, ldw, N, kchunk, part)
    // MT depends on the rows per launch only through "fits in 8": a row's arithmetic is the same in both instantiations
    if (M <= 8) SK_GO(8); else SK_GO(16);
#undef SK_GO
    KK_CHECK_LAUNCH();
    const float* resp = res ? res + (size_t)m0 * N : nullptr;
    float* outp = out + (size_t)m0 * N;
    hipLaunchKernelGGL(skinny_reduce_kernel, dim3((unsigned)(((long long)M * N + 255) / 256)), dim3(256), 0, st, part, KS, M, N, resp, outp);
    KK_CHECK_LAUNCH();
  }
  return 0;
}

// the matrix-core GEMV: one launch for all rows (grid z = 8-row chunks); KS must be the pack's w.ks
int launch_gemvm(const KKCsmWeight& w, int pro, int epi, FGArgs a, int Mtot, hipStream_t st) {
  a.w = w.wm; a.K = w.Cin; a.N = w.Cout; a.M = Mtot; a.kper = w.Cin / w.ks;
  a.wp = w.wp; a.gmagic = w.fmt != KK_WF_BF16 ? wf_group_magic(w.group) : 0;
  if (w.fmt != KK_WF_BF16 && (!w.wp || !wf_group_ok(w.Cin, w.group))) return kk_fail("kk_csm: internal: quantised GEMV without pairs / group size");
  a.ts = ts_slot(); a.ts_id = (w.Cout << 4) | (pro << 2) | epi;
  const int CB = 16 * w.nsub, nblk = (w.Cout + CB - 1) / CB, kper = w.Cin / w.ks;
  const size_t lds = gm_lds_bytes(w.nsub, kper);
  if (!gm_slice_fits(w.nsub, kper)) return kk_fail("kk_csm: internal: matrix-core GEMV: K slice too long for LDS");
  // PRO 3 reads an item's non-last rows from ONE x row per item (x + item * xrs): items of 1 or 2 rows only (the depth decoder's first step)
  if (pro == 3 && a.rows != 1 && a.rows != 2) return kk_fail("kk_csm: internal: matrix-core GEMV: item rows");
  const dim3 grid(nblk, w.ks, (Mtot + 7) / 8);
  const int rounds = (kper / 32 + 31) / 32;  // straight-line rounds of 4 chunks x 8 waves (K slice <= 1024: one)
#define GM_GO2(FMT, NSUB, PRO, EPI, RD)                                                                                                       \
  do {                                                                                                                                        \
    static KKDevOnce attr;                                                                                                                    \
    if (attr.first()) {                                                                                                                       \
      (void)hipFuncSetAttribute((const void*)gemvm_kernel<FMT, NSUB, PRO, EPI, RD>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);  \
      attr.done();                                                                                                                            \
    }                                                                                                                                         \
    hipLaunchKernelGGL((gemvm_kernel<FMT, NSUB, PRO, EPI, RD>), grid, dim3(512), lds, st, a);                                                 \
  } while (0)
#define GM_GO1(NSUB, PRO, EPI, RD)                                          \
  do {                                                                      \
    if (w.fmt == KK_WF_Q8) GM_GO2(KK_WF_Q8, NSUB, PRO, EPI, RD);            \
    else if (w.fmt == KK_WF_Q4) GM_GO2(KK_WF_Q4, NSUB, PRO, EPI, RD);       \
    else GM_GO2(KK_WF_BF16, NSUB, PRO, EPI, RD);                            \
  } while (0)
#define GM_GO(NSUB, PRO, EPI)                                              \
  do {                                                                      \
    if (rounds == 1) GM_GO1(NSUB, PRO, EPI, 1);                             \
    else if (rounds == 2) GM_GO1(NSUB, PRO, EPI, 2);                        \
    else GM_GO1(NSUB, PRO, EPI, 3);                                         \
  } while (0)
#define GM_PE(NSUB)                                                         \
  do {                                                                       \
    if (pro == 1 && epi == 0) GM_GO(NSUB, 1, 0);                             \
    else if (pro == 0 && epi == 1) GM_GO(NSUB, 0, 1);                        \
    else if (pro == 2 && epi == 1) GM_GO(NSUB, 2, 1);                        \
    else if (pro == 2 && epi == 2) GM_GO(NSUB, 2, 2);                        \
    else if (pro == 3 && epi == 0) GM_GO(NSUB, 3, 0);                        \
    else if (pro == 0 && epi == 0) GM_GO(NSUB, 0, 0);                        \
    else return kk_fail("kk_csm: internal: fused GEMV form");                \
  } while (0)
  if (w.nsub == 4) GM_PE(4); else if (w.nsub == 2) GM_PE(2); else GM_PE(1);
#undef GM_PE
#undef GM_GO
#undef GM_GO1
#undef GM_GO2
  KK_CHECK_LAUNCH();
  return 0;
}

// the single-token GEMV of a bf16 matrix: `a` carries everything but the weights; KS = w.ks split-K slices (epi 2) or one (any other epi)
int launch_gemv(const KKCsmWeight& w, int pro, int epi, FGArgs a, int Mtot, hipStream_t st) {
  if (!w.wm || !w.nsub) return kk_fail("kk_csm: internal: GEMV without a fragment pack");
  if ((epi == 2) != (w.ks > 1)) return kk_fail("kk_csm: internal: split-K form");
  return launch_gemvm(w, pro, epi, a, Mtot, st);
}

// h[m][:] += x[m] W for M rows of N = w.Cout contiguous floats: EPI 1 in place, or for a split-K pack (w.ks > 1) the slices of an EPI 2 launch
// into `part` ([ks][M][N]) and one combine (h += sum of the slices, slice order)
int gemv_accumulate(const KKCsmWeight& w, int pro, FGArgs g, int M, float* h, float* part, hipStream_t st) {
  if (w.ks > 1) {  // deep projection: K slices over workgroups, then one small combine
    g.out = part; g.ors = w.Cout; g.pss = (long long)M * w.Cout;
    KK_TRY(launch_gemv(w, pro, 2, g, M, st));
    const long long n = (long long)M * w.Cout;
    hipLaunchKernelGGL(combine_slices_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, w.ks, n, n, h, ts_slot());
    KK_CHECK_LAUNCH();
    return 0;
  }
  g.res = h; g.rrs = w.Cout; g.out = h; g.ors = w.Cout;
  return launch_gemv(w, pro, 1, g, M, st);
}

}  // namespace

// ---- what the handle launches (kk_kernels.h)
int kk_launch_csm_embed_sum(hipStream_t st, const int* tokens, const float* mask, const float* audio, const float* text, int ncb, int V, int TV, int D, int rows,
                            float* h) {
  if (ncb > 71) return kk_fail("kk_csm: more than 71 code books");
  hipLaunchKernelGGL(embed_sum_kernel, dim3(rows, (D + 255) / 256), dim3(256), 0, st, tokens, mask, audio, text, ncb, V, TV, D, h);
  KK_CHECK_LAUNCH();
  return 0;
}
int kk_launch_csm_embed_audio(hipStream_t st, const int* codes, int cstride, const float* audio, int cb, int V, int D, float* out, int rows, int pos, int B) {
  hipLaunchKernelGGL(embed_audio_kernel, dim3(B), dim3(256), 0, st, codes, cstride, audio, cb, V, D, out, rows, pos);
  KK_CHECK_LAUNCH();
  return 0;
}
int kk_launch_csm_copy_rows(hipStream_t st, const float* src, long long sbs, float* dst, long long dbs, int D, int B) {
  hipLaunchKernelGGL(copy_rows_kernel, dim3(B), dim3(256), 0, st, src, sbs, dst, dbs, D);
  KK_CHECK_LAUNCH();
  return 0;
}
int kk_launch_csm_rmsnorm(hipStream_t st, const float* x, const float* w, int D, float eps, float* out, int rows) {
  hipLaunchKernelGGL(rmsnorm_kernel, dim3(rows), dim3(256), 0, st, x, w, D, eps, out);
  KK_CHECK_LAUNCH();
  return 0;
}
int kk_launch_csm_swiglu(hipStream_t st, const float* gu, int I, long long n, float* out) {
  hipLaunchKernelGGL(swiglu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, gu, I, n, out);
  KK_CHECK_LAUNCH();
  return 0;
}
int kk_launch_csm_advance_pos(hipStream_t st, int* pos, int by) {
  hipLaunchKernelGGL(advance_pos_kernel, dim3(1), dim3(1), 0, st, pos, by);
  KK_CHECK_LAUNCH();
  return 0;
}
int kk_launch_csm_shift_cache(hipStream_t st, float* kc, float* vc, int maxB, int max_pos, int rowf4, int layers, const int* pos_dev, const int* pad, int delta) {
  hipLaunchKernelGGL(shift_cache_kernel, dim3((rowf4 + 63) / 64, maxB, 2 * layers), dim3(64), 0, st, kc, vc, maxB, max_pos, rowf4, pos_dev, pad, delta);
  KK_CHECK_LAUNCH();
  return 0;
}
int kk_launch_csm_kv_runs(const float* src_k, const float* src_v, long long src_pitch4, float* dst_k, float* dst_v, long long dst_pitch4, long long seg4,
                          int layers, hipStream_t stream) {
  hipLaunchKernelGGL(kv_runs_copy_kernel, dim3((unsigned)((seg4 + 1023) / 1024), 2 * layers), dim3(256), 0, stream, src_k, src_v, src_pitch4, dst_k, dst_v,
                     dst_pitch4, seg4);
  KK_CHECK_LAUNCH();
  return 0;
}
size_t kk_csm_skinny_floats(int K, int N) {
  int KS, kchunk;
  skinny_plan(K, N, &KS, &kchunk);
  return (size_t)KS * SK_MAXM * N;
}
int kk_launch_csm_skinny(hipStream_t st, const KKCsmWeight& w, const float* x, int Mtot, const float* res, float* out, float* part) {
  int KS, kchunk;
  skinny_plan(w.Cin, w.Cout, &KS, &kchunk);
  return launch_skinny(x, Mtot, w.Cin, w.Cout, w.w, w.ldw, KS, kchunk, res, out, part, st);
}
int kk_launch_csm_gemm_prompt(hipStream_t st, const KKCsmWeight& w, const float* x, long long xrs, int M, const float* res, long long rrs, float* out, long long ors) {
  GPArgs g;
  memset(&g, 0, sizeof g);
  g.x = x; g.xrs = xrs; g.K = w.Cin; g.N = w.Cout; g.M = M;
  gemmp_weights(g, w);
  g.res = res; g.rrs = rrs; g.out = out; g.ors = ors;
  return launch_gemmp(g, st);
}
// the caller's part of the GEMV's arguments; launch_gemvm adds the weights, the shape and the timestamp slot
static FGArgs fg_args(const KKCsmGemv& c) {
  FGArgs a;
  memset(&a, 0, sizeof a);
  a.x = c.x; a.xrs = c.xrs; a.nw = c.nw; a.eps = c.eps; a.codes = c.codes; a.cstride = c.cstride; a.cb = c.cb; a.V = c.V; a.rows = c.rows; a.emb = c.emb;
  a.gather_out = c.gather_out; a.res = c.res; a.rrs = c.rrs; a.out = c.out; a.ors = c.ors;
  return a;
}
int kk_launch_csm_gemv(hipStream_t st, const KKCsmWeight& w, int pro, int epi, const KKCsmGemv& a, int Mtot) { return launch_gemv(w, pro, epi, fg_args(a), Mtot, st); }
int kk_launch_csm_gemv_accumulate(hipStream_t st, const KKCsmWeight& w, int pro, const KKCsmGemv& a, int M, float* h, float* part) {
  return gemv_accumulate(w, pro, fg_args(a), M, h, part, st);
}
bool kk_csm_group_ok(int K, int group) { return wf_group_ok(K, group); }
unsigned long long* kk_csm_ts_slot() { return ts_slot(); }
const void* kk_csm_ts_buffer() { return g_ts; }

// ------------------------------------------------------------------------------------------------------------- host
// The fragment pack of a K x N matrix: *nsub = 0 if it gets none.  Split-K for the deep projections (K >= 4096 in slices of 1024 rows), then
// the widest column block (16 * nsub) that still gives ~200 workgroups; both depend on the matrix only, never on the batch.  (Measured: 2
// instead of 4 sub-blocks for gate|up, i.e. 32-column blocks and more workgroups, cost +0.09 ms per frame.)  Only packs the GEMV can run:
// split-K only where the step launches the matrix in that form (`split_ok`: the down projections), and a K slice too long for the launcher
// takes more slices there, or leaves the matrix without a pack elsewhere (its stack then runs on the fp32 path, stack_can_step).
void kk_csm_frag_plan(int K, int N, bool split_ok, int* ks_out, int* nsub_out) {
  *ks_out = 1; *nsub_out = 0;
  if (K < 32 || K % 32 != 0 || N < 1) return;
  int ks = 1;
  if (split_ok) {
    ks = (K >= 4096 && K % 1024 == 0) ? (K / 1024 > 16 ? 16 : K / 1024) : 1;
    while (ks > 1 && (K % ks != 0 || (K / ks) % 32 != 0)) --ks;
    for (int s = ks; !gm_slice_fits(4, K / ks) && s <= 16; ++s)
      if (K % s == 0 && (K / s) % 32 == 0) ks = s;
  }
  if (!gm_slice_fits(4, K / ks)) return;
  const int nb16 = (N + 15) / 16;
  *ks_out = ks;
  *nsub_out = nb16 * ks / 4 >= 192 ? 4 : (nb16 * ks / 2 >= 192 ? 2 : 1);
}
size_t kk_csm_frag_elems(int K, int N, int nsub) { return (size_t)((N + 16 * nsub - 1) / (16 * nsub)) * K * 16 * nsub; }
// w [K][ldw] fp32 -> out [N / (16 nsub)][K / 32][nsub][64 lanes][8] bf16 (RNE): lane L of chunk c, sub-block s holds k = 32 c + 8 (L / 16) + j,
// n = 16 s + L % 16 of its column block; the columns that pad N to whole blocks are zero
void kk_csm_frag_pack_rows(const float* w, int K, int N, long long ldw, int nsub, uint16_t* out) {
  const int CBm = 16 * nsub, nblk = (N + CBm - 1) / CBm, nchunk = K / 32;
  for (int i = 0; i < K; ++i) {
    const int c = i >> 5, kq = (i & 31) >> 3, j = i & 7;
    for (int o = 0; o < nblk * CBm; ++o) {
      uint32_t u = 0;
      if (o < N) memcpy(&u, &w[(size_t)i * ldw + o], 4);
      const int nbk = o / CBm, sb = (o % CBm) >> 4, L = kq * 16 + (o & 15);
      out[((((size_t)nbk * nchunk + c) * nsub + sb) * 64 + L) * 8 + j] = (uint16_t)kk_csm_bf16_round(u);
    }
  }
}

// ---- quantised fragment packs (kk_csm_gemvm.h: KK_WF_Q8 / KK_WF_Q4)
size_t kk_csm_qfrag_q_bytes(int K, int N, int nsub, int bits) { return kk_csm_frag_elems(K, N, nsub) * (size_t)bits / 8; }
size_t kk_csm_qfrag_pair_bytes(int K, int N, int nsub, int group) { return kk_csm_frag_elems(K, N, nsub) / (size_t)group * 8; }
// One nn.Linear part (words [O][K bits / 32], scales / biases [O][K / group]: output column n0 + o) into the packs of a K x N matrix; `q` and
// `pairs` must be zero-filled before the first part (the columns that pad N to whole blocks stay q = 0, scale = bias = 0: they decode to +0).
//   q:     [N / (16 nsub)][K / 32][nsub][64 lanes] x 8 values of `bits` bits, value j in bits [j bits, (j + 1) bits) of the lane's 8 / 4 bytes
//          (lane L: k = 32 c + 8 (L / 16) + j, n = 16 s + L % 16, as in frag_pack)
//   pairs: [N / (16 nsub)][K / group][nsub][16 columns] float2 (scale, bias)
void kk_csm_qfrag_pack_part(const uint32_t* words, const float* scales, const float* biases, int O, int n0, int K, int nsub, int group, int bits, uint8_t* q,
                            float* pairs) {
  const int CBm = 16 * nsub, nchunk = K / 32, ngrp = K / group, per = 32 / bits, wpr = K / per;
  const uint32_t mask = (1u << bits) - 1u;
  for (int o = 0; o < O; ++o) {
    const int n = n0 + o, nbk = n / CBm, sb = (n % CBm) >> 4;
    for (int g = 0; g < ngrp; ++g) {
      float* pr = pairs + ((((size_t)nbk * ngrp + g) * nsub + sb) * 16 + (n & 15)) * 2;
      pr[0] = scales[(size_t)o * ngrp + g];
      pr[1] = biases[(size_t)o * ngrp + g];
    }
    for (int i = 0; i < K; ++i) {
      const uint32_t v = (words[(size_t)o * wpr + i / per] >> ((i % per) * bits)) & mask;
      const int c = i >> 5, L = ((i & 31) >> 3) * 16 + (n & 15), j = i & 7;
      const size_t lane = (((size_t)nbk * nchunk + c) * nsub + sb) * 64 + L;
      if (bits == 8) q[lane * 8 + j] = (uint8_t)v;
      else q[lane * 4 + (j >> 1)] |= (uint8_t)(v << (4 * (j & 1)));
    }
  }
}

// ---- the kernels of the frame step on their own (tests): each entry point runs the launcher the frame runs, on caller-owned buffers
extern "C" int kk_csm_frag_choice(int K, int N, int split_ok, int32_t* ks, int32_t* nsub) {
  if (!ks || !nsub) return kk_fail("kk_csm_frag_choice: null argument");
  int k = 1, s = 0;
  kk_csm_frag_plan(K, N, split_ok != 0, &k, &s);
  *ks = k; *nsub = s;
  return 0;
}

extern "C" int kk_csm_frag_pack(const float* w, int K, int N, int nsub, uint16_t* out) {
  if (!w || !out || K < 32 || K % 32 != 0 || N < 1 || (nsub != 1 && nsub != 2 && nsub != 4)) return kk_fail("kk_csm_frag_pack: bad argument");
  kk_csm_frag_pack_rows(w, K, N, N, nsub, out);
  return 0;
}

extern "C" int kk_csm_qfrag_bytes(int K, int N, int nsub, int group_size, int bits, size_t* q_bytes, size_t* pair_bytes) {
  if (K < 32 || K % 32 != 0 || N < 1 || (nsub != 1 && nsub != 2 && nsub != 4) || (bits != 4 && bits != 8) || !wf_group_ok(K, group_size))
    return kk_fail("kk_csm_qfrag_bytes: bad argument");
  if (q_bytes) *q_bytes = kk_csm_qfrag_q_bytes(K, N, nsub, bits);
  if (pair_bytes) *pair_bytes = kk_csm_qfrag_pair_bytes(K, N, nsub, group_size);
  return 0;
}

extern "C" int kk_csm_qfrag_pack(const uint32_t* words, const float* scales, const float* biases, int K, int N, int nsub, int group_size, int bits,
                                 void* q_out, float* pairs_out) {
  if (!words || !scales || !biases || !q_out || !pairs_out || K < 32 || K % 32 != 0 || N < 1 || (nsub != 1 && nsub != 2 && nsub != 4) ||
      (bits != 4 && bits != 8) || !wf_group_ok(K, group_size))
    return kk_fail("kk_csm_qfrag_pack: bad argument");
  memset(q_out, 0, kk_csm_qfrag_q_bytes(K, N, nsub, bits));
  memset(pairs_out, 0, kk_csm_qfrag_pair_bytes(K, N, nsub, group_size));
  kk_csm_qfrag_pack_part(words, scales, biases, N, 0, K, nsub, group_size, bits, (uint8_t*)q_out, pairs_out);
  return 0;
}

static int op_csm_gemv(const char* who, KKCsmWeight& w, void* stream, int pro, int epi, int ks, int nsub, int K, int N, int M, const float* x, long long xrs,
                       const float* nw, float eps, const int32_t* codes, int cstride, int cb, int V, int rows, const float* emb, float* gather_out,
                       const float* res, long long rrs, float* out, long long ors, float* part);

extern "C" int kk_op_csm_gemv(void* stream, int pro, int epi, int ks, int nsub, int K, int N, int M, const void* w_frag, const float* x, long long xrs,
                              const float* nw, float eps, const int32_t* codes, int cstride, int cb, int V, int rows, const float* emb, float* gather_out,
                              const float* res, long long rrs, float* out, long long ors, float* part) {
  KKCsmWeight w;
  w.wm = (const uint16_t*)w_frag;
  return op_csm_gemv("kk_op_csm_gemv", w, stream, pro, epi, ks, nsub, K, N, M, x, xrs, nw, eps, codes, cstride, cb, V, rows, emb, gather_out, res, rrs, out, ors,
                     part);
}

extern "C" int kk_op_csm_gemv_q(void* stream, int pro, int epi, int ks, int nsub, int K, int N, int M, const void* q_frag, const void* pairs, int group_size,
                                int bits, const float* x, long long xrs, const float* nw, float eps, const int32_t* codes, int cstride, int cb, int V, int rows,
                                const float* emb, float* gather_out, const float* res, long long rrs, float* out, long long ors, float* part) {
  if (!pairs || (bits != 4 && bits != 8) || K < 32 || !wf_group_ok(K, group_size)) return kk_fail("kk_op_csm_gemv_q: pairs / bits / group size");
  KKCsmWeight w;
  w.wm = (const uint16_t*)q_frag; w.wp = (const float2*)pairs; w.fmt = bits == 8 ? KK_WF_Q8 : KK_WF_Q4; w.group = group_size;
  return op_csm_gemv("kk_op_csm_gemv_q", w, stream, pro, epi, ks, nsub, K, N, M, x, xrs, nw, eps, codes, cstride, cb, V, rows, emb, gather_out, res, rrs, out,
                     ors, part);
}

static int op_csm_gemv(const char* who, KKCsmWeight& w, void* stream, int pro, int epi, int ks, int nsub, int K, int N, int M, const float* x, long long xrs,
                       const float* nw, float eps, const int32_t* codes, int cstride, int cb, int V, int rows, const float* emb, float* gather_out,
                       const float* res, long long rrs, float* out, long long ors, float* part) {
  (void)who;
  const void* w_frag = w.wm;
  if (!w_frag || !out || M < 1 || N < 1 || K < 32 || K % 32 != 0 || (nsub != 1 && nsub != 2 && nsub != 4)) return kk_fail("kk_op_csm_gemv: bad argument");
  if (ks < 1 || ks > 16 || K % ks != 0 || (K / ks) % 32 != 0 || !gm_slice_fits(nsub, K / ks)) return kk_fail("kk_op_csm_gemv: K slices do not fit this K");
  if (pro < 0 || pro > 3 || epi < 0 || epi > 2 || (epi == 2) != (ks > 1)) return kk_fail("kk_op_csm_gemv: form");
  const bool gathered = (pro == 1 && codes) || pro == 3;
  if ((!x && !(pro == 1 && codes)) || (x && (xrs < (pro == 2 ? 2LL * K : (long long)K) || xrs % 4 != 0))) return kk_fail("kk_op_csm_gemv: input rows");
  if (gathered && (!codes || !emb || V < 1 || cb < 0 || cstride < 1)) return kk_fail("kk_op_csm_gemv: gathered rows");
  if (pro == 1 && !nw) return kk_fail("kk_op_csm_gemv: norm weight");
  if (epi == 1 && (!res || rrs < N)) return kk_fail("kk_op_csm_gemv: residual");
  if (ors < N || (epi == 2 && (ors != N || res || !part))) return kk_fail("kk_op_csm_gemv: output");
  w.Cin = K; w.Cout = N; w.nsub = nsub; w.ks = ks;
  FGArgs g;
  memset(&g, 0, sizeof g);
  g.x = x; g.xrs = xrs; g.nw = nw; g.eps = eps;
  g.codes = codes; g.cstride = cstride; g.cb = cb; g.V = V; g.rows = rows; g.emb = emb; g.gather_out = gather_out;
  g.res = res; g.rrs = rrs; g.out = out; g.ors = ors;
  if (ks > 1) return gemv_accumulate(w, pro, g, M, out, part, (hipStream_t)stream);
  return launch_gemv(w, pro, epi, g, M, (hipStream_t)stream);
}

extern "C" int kk_op_csm_gemm_prompt(void* stream, int K, int N, int M, int nsub, const void* w_frag, const float* x, long long xrs, const float* res,
                                     long long rrs, float* out, long long ors) {
  if (!w_frag || !x || !out || M < 1 || N < 1 || K < 32 || K % 32 != 0 || (nsub != 1 && nsub != 2 && nsub != 4) || xrs < K || xrs % 4 != 0 || ors < N ||
      (res && rrs < N))
    return kk_fail("kk_op_csm_gemm_prompt: bad argument");
  GPArgs g;
  memset(&g, 0, sizeof g);
  g.x = x; g.xrs = xrs; g.w = w_frag; g.K = K; g.N = N; g.M = M; g.nsub = nsub;
  g.res = res; g.rrs = rrs; g.out = out; g.ors = ors;
  return launch_gemmp(g, (hipStream_t)stream);
}

extern "C" int kk_op_csm_gemm_prompt_q(void* stream, int K, int N, int M, int nsub, const void* q_frag, const void* pairs, int group_size, int bits,
                                       const float* x, long long xrs, const float* res, long long rrs, float* out, long long ors) {
  if (!q_frag || !pairs || !x || !out || M < 1 || N < 1 || K < 32 || K % 32 != 0 || (nsub != 1 && nsub != 2 && nsub != 4) || xrs < K || xrs % 4 != 0 || ors < N ||
      (res && rrs < N) || (bits != 4 && bits != 8) || !wf_group_ok(K, group_size))
    return kk_fail("kk_op_csm_gemm_prompt_q: bad argument");
  GPArgs g;
  memset(&g, 0, sizeof g);
  g.x = x; g.xrs = xrs; g.w = q_frag; g.K = K; g.N = N; g.M = M; g.nsub = nsub;
  g.wp = (const float2*)pairs; g.gmagic = wf_group_magic(group_size); g.fmt = bits == 8 ? KK_WF_Q8 : KK_WF_Q4;
  g.res = res; g.rrs = rrs; g.out = out; g.ors = ors;
  return launch_gemmp(g, (hipStream_t)stream);
}

extern "C" int kk_op_csm_linear_skinny(void* stream, int K, int N, int M, const float* w, int ldw, const float* x, const float* res, float* out, float* scratch,
                                       size_t scratch_floats) {
  if (!w || !x || !out || !scratch || K < 1 || N < 1 || M < 1 || ldw < N) return kk_fail("kk_op_csm_linear_skinny: bad argument");
  int KS, kchunk;
  skinny_plan(K, N, &KS, &kchunk);
  if ((size_t)KS * SK_MAXM * N > scratch_floats) return kk_failf("kk_op_csm_linear_skinny: scratch needs %zu floats", (size_t)KS * SK_MAXM * N);
  return launch_skinny(x, M, K, N, w, ldw, KS, kchunk, res, out, scratch, (hipStream_t)stream);
}

extern "C" int kk_csm_debug_timestamps(unsigned long long* buf, int capacity) {
  g_ts = buf;
  g_ts_cap = buf ? capacity : 0;
  g_ts_next = 0;
  return 0;
}
