// Whisper, token timestamps from cross-attention (gfx950): the raw scores of selected heads, the alignment matrix and the dynamic time warping of
// mlx_audio/stt/models/whisper/timing.py:19-100, 143-157 and whisper.py:125-130; DESIGN 8h.
//
// The invariant of kk_whisper_text_kernels.hip holds here too: an item's (a row's) bits depend on that item's inputs alone.  Reduction orders are fixed,
// nothing is accumulated with floating-point atomics, and every loop bound is a function of the sizes, never of the data.
//
// ---- qk_rows: out[sel][row][key] = 64^-0.5 q . k, the score half of attn_rows ---------------------------------------------------------------
//   grid (64-key tile, selected head, item x chunk of QK_ROWS rows), one wave per workgroup.  Lane (kg = lane >> 3, ch = lane & 7) holds channels
//   8 ch .. 8 ch + 7 of the keys k0 + 8 j + kg, j = 0 .. 7, loaded ONCE and kept in registers for the chunk's rows.  Per row: the lane's 8-term fma
//   chain (q fp32, k bf16 from the store), xor-butterflies 1, 2, 4, one multiply by 0.125; lane (kg, ch) stores key k0 + 8 ch + kg, so a wave
//   writes 64 consecutive floats.  Keys at or past n_keys are not loaded and not stored.
//
// ---- align_matrix: softmax -> per-column standardisation over the rows -> median filter along the columns -> mean over the heads --------------
//   Heads are taken in groups of `group`; a group's softmax weights live in the workspace [B][group][rows][cols] (it does not grow with the
//   number of heads), and the filtered values are ADDED to the output head by head, in list order, across the groups: the running sum in
//   memory is the same fp32 sequence whatever the group size.  The last group divides by the number of heads.
//     softmax   one workgroup of 256 per (row, head): maximum, exp and sum (per-thread strided shares, xor-butterflies, the 4 waves in wave order)
//     colstats  one thread per (head, column): mean = sum / n over the rows in row order, variance = sum (w - mean)^2 / n (two passes, ddof 0),
//               then (w - mean) / sqrt(variance) written in place.  No guard against a zero deviation: inf and NaN flow through.
//     median    one thread per (row, column): the reflect-padded window, width 7 on a 16-exchange sorting network, other widths by rank counting.
//               A window that holds a NaN gives NaN.  n_frames <= width / 2 skips the filter (timing.py:22-24).
//
// ---- dtw: one wave per item ------------------------------------------------------------------------------------------------------------------
//   Bands of 64 rows; in a band lane l owns row 64 band + l and handles column t - l at step t, so cost[i-1][j] is the neighbour lane's value of the
//   step before (one lane shift per step, no barrier) and cost[i-1][j-1] is what the shift delivered one step earlier.  Lane 0's neighbour is the
//   previous band's last row, kept in LDS (one float per column, updated in place: lane 63 writes column t - 63 while lane 0 reads column t).
//   x is read 16 steps ahead into registers.  The trace is packed 2 bits per cell, 16 columns to a word, each lane writing its own row's words.
//   The backtrace is a second launch, one lane per item: at most n_rows + n_cols steps from (N, M) with the borders of timing.py:51-52, a trace word
//   re-read only when the row or the word changes; it fills the path from the back of the output arrays, and the wave then moves it to the front.
#include "kk_host.h"
#include "../../include/kokoro_hip.h"

#include <math.h>

namespace {
constexpr int QK_ROWS = 8;         // query rows per workgroup of qk_rows (the K tile is loaded once for them)
constexpr int ALIGN_GROUP = 8;     // heads per group of align_matrix when the caller passes 0
constexpr int DTW_MAX_COLS = 15360;  // the LDS row of dtw: 60 KB

__device__ __forceinline__ float bf_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(unsigned w) { return __uint_as_float(w & 0xFFFF0000u); }

// ------------------------------------------------------------------------------------------------------------------------------ qk_rows
__global__ __launch_bounds__(64) void qk_rows_kernel(const float* q, const bf16_t* k, long long item_stride, int ld, int heads, int rows, int n_keys, KKQkSel sel,
                                                     float* out, long long stride_slot, long long stride_item, long long ldo, int chunks) {
  const int lane = threadIdx.x, kg = lane >> 3, ch = lane & 7;
  const int k0 = blockIdx.x * 64, j = blockIdx.y, item = blockIdx.z / chunks, r0 = (blockIdx.z % chunks) * QK_ROWS;
  const int h = sel.head[j];
  const bf16_t* base = k + (long long)item * item_stride + h * 64 + ch * 8;
  uint4 kr[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int key = k0 + 8 * u + kg;
    kr[u] = uint4{0u, 0u, 0u, 0u};
    if (key < n_keys) kr[u] = *(const uint4*)(base + (long long)key * ld);
  }
  const int mykey = k0 + 8 * ch + kg;
  float* o = out + (long long)sel.slot[j] * stride_slot + (long long)item * stride_item + mykey;
  for (int rr = 0; rr < QK_ROWS; ++rr) {
    const int r = r0 + rr;
    if (r >= rows) break;  // (uniform)
    const float* qp = q + (((long long)item * rows + r) * heads + h) * 64 + ch * 8;
    const float4 qa = *(const float4*)qp, qb = *(const float4*)(qp + 4);
    float mine = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      float d = qa.x * bf_lo(kr[u].x);
      d = __builtin_fmaf(qa.y, bf_hi(kr[u].x), d);
      d = __builtin_fmaf(qa.z, bf_lo(kr[u].y), d);
      d = __builtin_fmaf(qa.w, bf_hi(kr[u].y), d);
      d = __builtin_fmaf(qb.x, bf_lo(kr[u].z), d);
      d = __builtin_fmaf(qb.y, bf_hi(kr[u].z), d);
      d = __builtin_fmaf(qb.z, bf_lo(kr[u].w), d);
      d = __builtin_fmaf(qb.w, bf_hi(kr[u].w), d);
      d += __shfl_xor(d, 1);
      d += __shfl_xor(d, 2);
      d += __shfl_xor(d, 4);
      mine = u == ch ? d : mine;
    }
    if (mykey < n_keys) o[(long long)r * ldo] = mine * 0.125f;  // 64^-0.5
  }
}

// ------------------------------------------------------------------------------------------------------------------------- align_matrix
struct AlignArgs {
  const float* qk;  // [B][heads][rows][ld_in] by strides
  long long stride_b, stride_h;
  int ld_in;
  const int *n_rows, *n_frames;  // device [B]
  int rows_max, cols_max;
  float qk_scale;
  float* w;  // workspace [B][group][rows_max][cols_max]
  int group;
  float* out;  // [B][rows_max][ld_out]
  int ld_out;
  int h0, hn, n_heads;  // this launch: heads h0 .. h0 + hn - 1 of n_heads
  int width;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void align_softmax_kernel(AlignArgs a) {
  __shared__ float sh[4];
  const int r = blockIdx.x, g = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int n = clampi(a.n_rows[b], 0, a.rows_max), F = clampi(a.n_frames[b], 0, a.cols_max);
  if (r >= n || F < 1) return;  // (uniform)
  const float* x = a.qk + (long long)b * a.stride_b + (long long)(a.h0 + g) * a.stride_h + (long long)r * a.ld_in;
  float* w = a.w + (((long long)b * a.group + g) * a.rows_max + r) * a.cols_max;
  float m = -INFINITY;
  for (int c = tid; c < F; c += 256) m = fmaxf(m, x[c] * a.qk_scale);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((tid & 63) == 0) sh[tid >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  __syncthreads();
  float s = 0.f;
  for (int c = tid; c < F; c += 256) {
    const float e = expf(x[c] * a.qk_scale - m);
    w[c] = e;
    s += e;
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
  if ((tid & 63) == 0) sh[tid >> 6] = s;
  __syncthreads();
  s = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  for (int c = tid; c < F; c += 256) w[c] = w[c] / s;  // each thread re-reads what it wrote
}

__global__ __launch_bounds__(64) void align_colstats_kernel(AlignArgs a) {
  const int c = blockIdx.x * 64 + threadIdx.x, g = blockIdx.y, b = blockIdx.z;
  const int n = clampi(a.n_rows[b], 0, a.rows_max), F = clampi(a.n_frames[b], 0, a.cols_max);
  if (c >= F || n < 1) return;
  float* w = a.w + ((long long)b * a.group + g) * a.rows_max * a.cols_max + c;
  const long long ld = a.cols_max;
  float s = 0.f;
  for (int r = 0; r < n; ++r) s += w[r * ld];
  const float mean = s / (float)n;
  float ss = 0.f;
  for (int r = 0; r < n; ++r) {
    const float d = w[r * ld] - mean;
    ss = __builtin_fmaf(d, d, ss);
  }
  const float sd = sqrtf(ss / (float)n);
  for (int r = 0; r < n; ++r) w[r * ld] = (w[r * ld] - mean) / sd;
}

#define KK_CSWAP(x, y)             \
  do {                             \
    const float lo__ = fminf(x, y); \
    y = fmaxf(x, y);               \
    x = lo__;                      \
  } while (0)

__device__ __forceinline__ float median7(float v0, float v1, float v2, float v3, float v4, float v5, float v6) {  // 16 exchanges, 6 layers
  KK_CSWAP(v0, v6); KK_CSWAP(v2, v3); KK_CSWAP(v4, v5);
  KK_CSWAP(v0, v2); KK_CSWAP(v1, v4); KK_CSWAP(v3, v6);
  KK_CSWAP(v0, v1); KK_CSWAP(v2, v5); KK_CSWAP(v3, v4);
  KK_CSWAP(v1, v2); KK_CSWAP(v4, v6);
  KK_CSWAP(v2, v3); KK_CSWAP(v4, v5);
  KK_CSWAP(v1, v2); KK_CSWAP(v3, v4); KK_CSWAP(v5, v6);
  return v3;
}

__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// the median of the reflect-padded window of `width` around column c of a row of F values (F > width / 2); a window that holds a NaN gives NaN
template <int W7>
__device__ __forceinline__ float window_median(const float* w, int c, int F, int width) {
  const int pad = width >> 1;
  bool nan = false;
  float med = 0.f;
  if (W7) {
    float v[7];
#pragma unroll
    for (int u = 0; u < 7; ++u) {
      v[u] = w[reflect(c - 3 + u, F)];
      nan |= v[u] != v[u];
    }
    med = median7(v[0], v[1], v[2], v[3], v[4], v[5], v[6]);
  } else {
    // rank counting: the element with exactly `pad` others before it (smaller, or equal with a lower index)
    for (int u = 0; u < width; ++u) {
      const float x = w[reflect(c - pad + u, F)];
      nan |= x != x;
      int rank = 0;
      for (int t = 0; t < width; ++t) {
        const float y = w[reflect(c - pad + t, F)];
        rank += (y < x || (y == x && t < u)) ? 1 : 0;
      }
      med = rank == pad ? x : med;
    }
  }
  return nan ? NAN : med;
}

template <int W7>
__global__ __launch_bounds__(256) void align_median_kernel(AlignArgs a) {
  const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y, b = blockIdx.z;
  const int n = clampi(a.n_rows[b], 0, a.rows_max), F = clampi(a.n_frames[b], 0, a.cols_max);
  if (r >= n || c >= F) return;
  const bool filter = a.width > 1 && F > (a.width >> 1);
  float* o = a.out + ((long long)b * a.rows_max + r) * a.ld_out + c;
  float acc = a.h0 == 0 ? 0.f : *o;
  for (int g = 0; g < a.hn; ++g) {  // head order
    const float* w = a.w + (((long long)b * a.group + g) * a.rows_max + r) * a.cols_max;
    acc += filter ? window_median<W7>(w, c, F, a.width) : w[c];
  }
  if (a.h0 + a.hn == a.n_heads) acc = acc / (float)a.n_heads;
  *o = acc;
}

// timing.py:19-44 on its own: rows of n values, n > width / 2
template <int W7>
__global__ __launch_bounds__(256) void median_rows_kernel(const float* x, long long ldx, int n, int width, float* out, long long ldo) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const long long r = blockIdx.y;
  if (c < n) out[r * ldo + c] = window_median<W7>(x + r * ldx, c, n, width);
}

// ---------------------------------------------------------------------------------------------------------------------------------- dtw
struct DtwArgs {
  const float* x;  // [B][rows_max][ld]
  long long xbs;
  int ld, rows_max, cols_max;
  const int *n_rows, *n_cols;  // device [B]
  int negate;
  uint32_t* trace;  // [B][rows_max][trace_ld] words
  int trace_ld;
  int32_t *text_idx, *time_idx;  // [B][cap], cap = rows_max + cols_max
  int32_t *len, *first;          // [B], [B][rows_max]
};

__global__ __launch_bounds__(64) void dtw_kernel(DtwArgs a) {
  extern __shared__ float lastrow[];  // the previous band's last row, cost[64 band][1 .. M]
  const int b = blockIdx.x, lane = threadIdx.x;
  const int N = clampi(a.n_rows[b], 0, a.rows_max), M = clampi(a.n_cols[b], 0, a.cols_max);
  if (N < 1 || M < 1) return;  // (the host entry refuses it)
  const float* xb = a.x + (long long)b * a.xbs;
  uint32_t* tr = a.trace + (long long)b * a.rows_max * a.trace_ld;
  const int nbands = (N + 63) >> 6, nblk = (M + 63 + 15) >> 4;
  for (int band = 0; band < nbands; ++band) {
    const int i0 = band * 64 + lane;  // this lane's row of x
    const bool rowok = i0 < N;
    const float* xr = xb + (long long)(rowok ? i0 : 0) * a.ld;
    uint32_t* trr = tr + (long long)(rowok ? i0 : 0) * a.trace_ld;
    float cur = INFINITY;                     // cost[i][j - 1]; column 0 is inf
    float diag = i0 == 0 ? 0.f : INFINITY;    // cost[i - 1][j - 1]; cost[0][0] = 0
    uint32_t word = 0;
    float xa[16], xn[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int c = u - lane;
      xa[u] = rowok && c >= 0 && c < M ? xr[c] : 0.f;
    }
    for (int blk = 0; blk < nblk; ++blk) {
#pragma unroll
      for (int u = 0; u < 16; ++u) {  // the next 16 steps' x, requested before this block's chain starts
        const int c = (blk + 1) * 16 + u - lane;
        xn[u] = rowok && c >= 0 && c < M ? xr[c] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int c = blk * 16 + u - lane;  // column of x, 0-based
        const bool incol = c >= 0 && c < M;
        float up = __shfl_up(cur, 1);  // cost[i - 1][j]: what the lane above computed one step ago
        if (lane == 0) up = band > 0 && incol ? lastrow[c] : INFINITY;
        if (rowok && incol) {
          const float c0 = diag, c1 = up, c2 = cur;
          float best;
          uint32_t t;
          if (c0 < c1 && c0 < c2) { best = c0; t = 0u; }
          else if (c1 < c0 && c1 < c2) { best = c1; t = 1u; }
          else { best = c2; t = 2u; }
          const float v = a.negate ? -xa[u] : xa[u];
          cur = v + best;
          diag = up;
          word |= t << (2 * (c & 15));
          if ((c & 15) == 15 || c == M - 1) {
            trr[c >> 4] = word;
            word = 0u;
          }
          if (lane == 63) lastrow[c] = cur;
        }
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) xa[u] = xn[u];
    }
  }
}

// the backtrace of one item, a launch of its own behind the sweep (the kernel boundary makes the trace visible): lane 0 walks, the wave moves the path
__global__ __launch_bounds__(64) void dtw_backtrace_kernel(DtwArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int N = clampi(a.n_rows[b], 0, a.rows_max), M = clampi(a.n_cols[b], 0, a.cols_max);
  const int cap = a.rows_max + a.cols_max;
  if (N < 1 || M < 1) {  // (the host entry refuses it)
    if (lane == 0) a.len[b] = 0;
    return;
  }
  const uint32_t* tr = a.trace + (long long)b * a.rows_max * a.trace_ld;
  int32_t* ti = a.text_idx + (long long)b * cap;
  int32_t* tj = a.time_idx + (long long)b * cap;
  int L = 0;
  if (lane == 0) {
    int32_t* first = a.first + (long long)b * a.rows_max;
    int i = N, j = M, wrow = -1, wcol = -1;
    uint32_t w = 0u;
    for (int step = 0; step < N + M; ++step) {
      if (i > 0 || j > 0) {
        const int pos = cap - 1 - L;
        ti[pos] = i - 1;
        tj[pos] = j - 1;
        if (i >= 1) first[i - 1] = j - 1;  // the last write of a row is its first entry in forward order
        int t;
        if (i == 0) t = 2;       // trace[0, :] = 2
        else if (j == 0) t = 1;  // trace[:, 0] = 1
        else {
          if (wrow != i - 1 || wcol != (j - 1) >> 4) {
            wrow = i - 1;
            wcol = (j - 1) >> 4;
            w = tr[(long long)wrow * a.trace_ld + wcol];
          }
          t = (int)((w >> (2 * ((j - 1) & 15))) & 3u);
        }
        if (t == 0) { --i; --j; }
        else if (t == 1) --i;
        else --j;
        ++L;
      }
    }
    a.len[b] = L;
  }
  __threadfence();
  __syncthreads();
  L = __shfl(L, 0);
  const int shift = cap - L;
  if (shift > 0) {
    for (int k0 = 0; k0 < cap; k0 += 64) {  // to the front, ascending: a chunk's sources lie behind everything written so far
      const int k = k0 + lane;
      int vi = 0, vj = 0;
      if (k < L) {
        vi = ti[k + shift];
        vj = tj[k + shift];
      }
      __syncthreads();
      if (k < L) {
        ti[k] = vi;
        tj[k] = vj;
      }
      __syncthreads();
    }
  }
}

inline int align_group(int group, int n_heads) {
  const int g = group > 0 ? group : ALIGN_GROUP;
  return g < n_heads ? g : n_heads;
}
inline int dtw_trace_ld(int cols_max) { return (cols_max + 15) / 16; }
}  // namespace

int kk_launch_whisper_qk_rows(hipStream_t st, const float* q, const bf16_t* k, long long item_stride, int ld, int heads, int items, int rows, int n_keys,
                              const KKQkSel& sel, float* out, long long stride_slot, long long stride_item, long long ldo) {
  const int chunks = (rows + QK_ROWS - 1) / QK_ROWS;
  if ((long long)items * chunks > 65535) return kk_fail("qk_rows: items x ceil(rows / 8) exceeds 65535");
  if (sel.n < 1 || sel.n > 32) return kk_fail("qk_rows: 1 .. 32 heads per launch");
  hipLaunchKernelGGL(qk_rows_kernel, dim3((n_keys + 63) / 64, sel.n, items * chunks), dim3(64), 0, st, q, k, item_stride, ld, heads, rows, n_keys, sel, out,
                     stride_slot, stride_item, ldo, chunks);
  KK_CHECK_LAUNCH();
  return 0;
}

// ============================================================================================================================ kk_op_* entries
extern "C" size_t kk_op_whisper_qk_rows_workspace_bytes(int items, int rows, int n_sel, int n_keys) {
  (void)items; (void)rows; (void)n_sel; (void)n_keys;
  return 0;  // the kernel needs no scratch; the entry exists so that every raw op of this file is sized the same way
}

extern "C" int kk_op_whisper_qk_rows(void* stream, int items, int rows, int heads, const float* q, const void* k, int T_rows, int ld, const int32_t* sel,
                                     int n_sel, int n_keys, float* out, long long ldo) {
  if (!q || !k || !sel || !out) return kk_fail("kk_op_whisper_qk_rows: null argument");
  if (items < 1 || rows < 1 || heads < 1 || T_rows < 1 || n_sel < 1) return kk_fail("kk_op_whisper_qk_rows: bad argument (need items, rows, heads, T_rows, n_sel >= 1)");
  if (n_keys < 1 || n_keys > T_rows) return kk_failf("kk_op_whisper_qk_rows: n_keys = %d is outside [1, %d]", n_keys, T_rows);
  if (ld % 8 != 0 || heads * 64 > ld) return kk_fail("kk_op_whisper_qk_rows: ld must be a multiple of 8 with `heads` heads of 64 channels inside a row");
  if (ldo < n_keys) return kk_fail("kk_op_whisper_qk_rows: ldo is smaller than n_keys");
  if (((uintptr_t)k & 15) || ((uintptr_t)q & 15)) return kk_fail("kk_op_whisper_qk_rows: q and k must be 16-byte aligned");
  for (int j = 0; j < n_sel; ++j)
    if (sel[j] < 0 || sel[j] >= heads) return kk_failf("kk_op_whisper_qk_rows: sel[%d] = %d is outside [0, %d)", j, sel[j], heads);
  const long long R = (long long)items * rows;
  for (int j0 = 0; j0 < n_sel; j0 += 32) {
    KKQkSel s;
    memset(&s, 0, sizeof s);
    s.n = n_sel - j0 < 32 ? n_sel - j0 : 32;
    for (int j = 0; j < s.n; ++j) {
      s.head[j] = sel[j0 + j];
      s.slot[j] = j0 + j;
    }
    KK_TRY(kk_launch_whisper_qk_rows((hipStream_t)stream, q, (const bf16_t*)k, (long long)T_rows * ld, ld, heads, items, rows, n_keys, s, out, R * ldo,
                                     (long long)rows * ldo, ldo));
  }
  return 0;
}

namespace {
// the device row / column counts of a raw entry, read back and checked (the entry synchronises, like kk_op_whisper_attn_rows)
int check_counts(const char* who, hipStream_t st, int B, const int32_t* n_rows, int rows_max, const int32_t* n_cols, int cols_max) {
  std::vector<int32_t> hv(2 * (size_t)B);
  if (hipMemcpyAsync(hv.data(), n_rows, (size_t)B * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(hv.data() + B, n_cols, (size_t)B * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return kk_failf("%s: reading the row and column counts failed", who);
  for (int b = 0; b < B; ++b) {
    if (hv[b] < 1 || hv[b] > rows_max) return kk_failf("%s: n_rows[%d] = %d is outside [1, %d]", who, b, hv[b], rows_max);
    if (hv[B + b] < 1 || hv[B + b] > cols_max) return kk_failf("%s: n_cols[%d] = %d is outside [1, %d]", who, b, hv[B + b], cols_max);
  }
  return 0;
}
}  // namespace

extern "C" size_t kk_op_whisper_align_matrix_workspace_bytes(int B, int n_heads, int rows_max, int cols_max, int group) {
  if (B < 1 || n_heads < 1 || rows_max < 1 || cols_max < 1 || group < 0) return 0;
  return (size_t)B * align_group(group, n_heads) * rows_max * cols_max * sizeof(float);
}

extern "C" int kk_op_whisper_align_matrix(void* stream, int B, int n_heads, const float* qk, long long stride_b, long long stride_h, int ld_in, const int32_t* n_rows,
                                          int rows_max, const int32_t* n_frames, int cols_max, float qk_scale, int medfilt_width, int group, float* out, int ld_out,
                                          void* workspace, size_t workspace_bytes) {
  const char* who = "kk_op_whisper_align_matrix";
  if (!qk || !n_rows || !n_frames || !out || !workspace) return kk_failf("%s: null argument", who);
  if (B < 1 || n_heads < 1 || group < 0) return kk_failf("%s: bad argument (need B, n_heads >= 1, group >= 0)", who);
  if (B > 65535 || rows_max > 65535) return kk_failf("%s: B and rows_max are limited to 65535", who);
  if (rows_max < 1 || cols_max < 1) return kk_failf("%s: n_rows >= 1 and n_cols >= 1 (rows_max = %d, cols_max = %d)", who, rows_max, cols_max);
  if (ld_in < cols_max || ld_out < cols_max) return kk_failf("%s: cols_max = %d exceeds a leading dimension (%d in, %d out)", who, cols_max, ld_in, ld_out);
  if (stride_h < (long long)rows_max * ld_in) return kk_failf("%s: rows_max = %d rows of %d do not fit the head stride", who, rows_max, ld_in);
  if (medfilt_width < 1 || medfilt_width > 31 || medfilt_width % 2 == 0) return kk_failf("%s: medfilt_width = %d must be odd and within 1 .. 31", who, medfilt_width);
  if (workspace_bytes < kk_op_whisper_align_matrix_workspace_bytes(B, n_heads, rows_max, cols_max, group)) return kk_failf("%s: workspace too small", who);
  hipStream_t st = (hipStream_t)stream;
  KK_TRY(check_counts(who, st, B, n_rows, rows_max, n_frames, cols_max));
  AlignArgs a;
  memset(&a, 0, sizeof a);
  a.qk = qk; a.stride_b = stride_b; a.stride_h = stride_h; a.ld_in = ld_in; a.n_rows = n_rows; a.n_frames = n_frames; a.rows_max = rows_max; a.cols_max = cols_max;
  a.qk_scale = qk_scale; a.w = (float*)workspace; a.group = align_group(group, n_heads); a.out = out; a.ld_out = ld_out; a.n_heads = n_heads; a.width = medfilt_width;
  for (int h0 = 0; h0 < n_heads; h0 += a.group) {
    a.h0 = h0;
    a.hn = n_heads - h0 < a.group ? n_heads - h0 : a.group;
    hipLaunchKernelGGL(align_softmax_kernel, dim3(rows_max, a.hn, B), dim3(256), 0, st, a);
    KK_CHECK_LAUNCH();
    hipLaunchKernelGGL(align_colstats_kernel, dim3((cols_max + 63) / 64, a.hn, B), dim3(64), 0, st, a);
    KK_CHECK_LAUNCH();
    if (medfilt_width == 7) hipLaunchKernelGGL(align_median_kernel<1>, dim3((cols_max + 255) / 256, rows_max, B), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(align_median_kernel<0>, dim3((cols_max + 255) / 256, rows_max, B), dim3(256), 0, st, a);
    KK_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int kk_op_whisper_median_filter(void* stream, long long rows, int n, const float* x, long long ldx, int width, float* out, long long ldo) {
  const char* who = "kk_op_whisper_median_filter";
  if (!x || !out) return kk_failf("%s: null argument", who);
  if (rows < 1 || n < 1 || ldx < n || ldo < n) return kk_failf("%s: bad argument (need rows, n >= 1 and row pitches of at least n)", who);
  if (width < 1 || width > 31 || width % 2 == 0) return kk_failf("%s: width = %d must be odd and within 1 .. 31", who, width);
  if (n <= width / 2) return kk_failf("%s: %d values are no longer than the padding %d (timing.py:22-24 returns the input)", who, n, width / 2);
  hipStream_t st = (hipStream_t)stream;
  for (long long r0 = 0; r0 < rows; r0 += 65535) {  // grid.y limit
    const int nr = (int)(rows - r0 < 65535 ? rows - r0 : 65535);
    if (width == 7) hipLaunchKernelGGL(median_rows_kernel<1>, dim3((n + 255) / 256, nr), dim3(256), 0, st, x + r0 * ldx, ldx, n, width, out + r0 * ldo, ldo);
    else hipLaunchKernelGGL(median_rows_kernel<0>, dim3((n + 255) / 256, nr), dim3(256), 0, st, x + r0 * ldx, ldx, n, width, out + r0 * ldo, ldo);
    KK_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" size_t kk_op_whisper_dtw_workspace_bytes(int B, int rows_max, int cols_max) {
  if (B < 1 || rows_max < 1 || cols_max < 1) return 0;
  return (size_t)B * rows_max * dtw_trace_ld(cols_max) * sizeof(uint32_t);
}

extern "C" int kk_op_whisper_dtw(void* stream, int B, const float* x, long long stride_b, int ld, const int32_t* n_rows, int rows_max, const int32_t* n_cols,
                                 int cols_max, int negate, int32_t* text_indices, int32_t* time_indices, int32_t* length, int32_t* first_cols, void* workspace,
                                 size_t workspace_bytes) {
  const char* who = "kk_op_whisper_dtw";
  if (!x || !n_rows || !n_cols || !text_indices || !time_indices || !length || !first_cols || !workspace) return kk_failf("%s: null argument", who);
  if (B < 1) return kk_failf("%s: bad argument (need B >= 1)", who);
  if (rows_max < 1 || cols_max < 1) return kk_failf("%s: n_rows >= 1 and n_cols >= 1 (rows_max = %d, cols_max = %d)", who, rows_max, cols_max);
  if (ld < cols_max) return kk_failf("%s: cols_max = %d exceeds the leading dimension %d", who, cols_max, ld);
  if (stride_b < (long long)rows_max * ld) return kk_failf("%s: rows_max = %d rows of %d do not fit the item stride", who, rows_max, ld);
  if (cols_max > DTW_MAX_COLS) return kk_failf("%s: at most %d columns (one row of costs is kept in LDS)", who, DTW_MAX_COLS);
  if (workspace_bytes < kk_op_whisper_dtw_workspace_bytes(B, rows_max, cols_max)) return kk_failf("%s: workspace too small", who);
  hipStream_t st = (hipStream_t)stream;
  KK_TRY(check_counts(who, st, B, n_rows, rows_max, n_cols, cols_max));
  DtwArgs a;
  memset(&a, 0, sizeof a);
  a.x = x; a.xbs = stride_b; a.ld = ld; a.rows_max = rows_max; a.cols_max = cols_max; a.n_rows = n_rows; a.n_cols = n_cols; a.negate = negate ? 1 : 0;
  a.trace = (uint32_t*)workspace; a.trace_ld = dtw_trace_ld(cols_max); a.text_idx = text_indices; a.time_idx = time_indices; a.len = length; a.first = first_cols;
  hipLaunchKernelGGL(dtw_kernel, dim3(B), dim3(64), (size_t)cols_max * sizeof(float), st, a);
  KK_CHECK_LAUNCH();
  hipLaunchKernelGGL(dtw_backtrace_kernel, dim3(B), dim3(64), 0, st, a);
  KK_CHECK_LAUNCH();
  return 0;
}
