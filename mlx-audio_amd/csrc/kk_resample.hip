// Row-mode polyphase FIR resampler (ABI minor 10): the sample-rate edge of CSM serving.  One object holds `max_rows` independent
// streams, each with its own ratio L / M, position and lifetime; ONE launch per step serves every row that takes part.
//   y[n] = sum_j h[n M + half - j L] x[j]      (scipy.signal.resample_poly(x, L, M) with its defaults; the taps come from the caller)
// Output n reads the T inputs j0 - T + 1 .. j0, j0 = (n M + half) / L, with the taps of phase p = (n M + half) % L: tab[p][t] = h[p + t L]
// meets x[j0 - t].  A thread runs ONE fmaf chain from 0.0f over those T products in ascending input order, whether an input is a fed sample,
// a zero in front of the clip or a zero behind it -- multiply, never skip -- so an output's bits depend on its index and the clip alone,
// never on the slicing of the steps or on the other rows.
// PCM formats (ABI minor 11): a row reads f32, s16le, mu-law or A-law samples and writes any of the four.  x and y are byte
// buffers; a row's samples are decoded as they are staged into the LDS window and into the carried history (both stay fp32, and a decoded
// sample is exact in fp32), and the store encodes the chain's result.  The format is uniform per workgroup: the branch sits around the
// staging and the store, never in the tap loop.  pcm_convert_rows_kernel is the same edge for rows at the model's own rate.
#include "../../include/kokoro_hip.h"
#include "kk_host.h"
#include "kk_pcm.h"

static_assert(PCM_F32 == KK_PCM_F32 && PCM_S16LE == KK_PCM_S16LE && PCM_MULAW == KK_PCM_MULAW && PCM_ALAW == KK_PCM_ALAW, "kk_pcm.h and kokoro_hip.h disagree");

#define RS_B 256          // outputs (= threads) per workgroup
#define RS_WIN 4096       // floats of the input window one pass holds in LDS; a wider window takes several passes over the same chain
#define RS_MAX_RATIO 320  // max(L, M): half <= 3200, 2 half + 1 <= 6401 taps
#define RS_TAB_LDS 7168   // L (T | 1) <= 6401 + 319 + 320
#define RS_TAB_DEV 6784   // L T <= 6401 + 319, rounded up to 64
#define RS_HCAP 6404      // T <= 6401 carried inputs per history buffer
#define RS_MAX_ROWS 64    // the per-step table travels as a launch argument

struct RsRow {  // device descriptor of one row, written by kk_resampler_set_row
  int L, M, half, T;
  int in_fmt, out_fmt;  // KK_PCM_*: what the row's new samples are stored as, and its outputs
  const float* tab;     // [L][T] fp32, phase-major
  float* hist;          // [2][RS_HCAP]: the last T inputs, double buffered (a step reads one and writes the other: no order between workgroups)
  long long cnt[2][2];  // [buffer][inputs consumed, outputs emitted], double buffered with hist
};

struct RsStep {
  int n_in, n_out;
  int flags;  // bit 0: the row takes part; bit 1: the buffer this step reads
};
struct RsSteps {
  RsStep s[RS_MAX_ROWS];
};

// element r of [carried history (T) | the step's new samples (n_in) | zeros]; r < 0 only in the alignment slack of a window, which no tap reads
__device__ static inline float rs_cat(const float* hist, const float* x, int T, int n_in, int r) {
  if (r < 0) return 0.f;
  if (r < T) return hist[r];
  r -= T;
  return r < n_in ? x[r] : 0.f;
}
// ... whose new samples are stored as `fmt`
__device__ static inline float rs_cat_fmt(const float* hist, const char* x, int fmt, int T, int n_in, int r) {
  if (r < 0) return 0.f;
  if (r < T) return hist[r];
  r -= T;
  return r < n_in ? pcm_load(x, fmt, r) : 0.f;
}

// One pass of the window for a row of 2-byte (G = 8) or 1-byte (G = 16) samples: a thread decodes the G samples of one 16-byte load.
// q + G <= RS_WIN, since q < cn <= RS_WIN and both q and RS_WIN are multiples of G.
template <int G>
__device__ static inline void rs_stage(float* win_s, const float* hist, const char* xb, int fmt, int T, int n_in, int c0, int cn, int tid) {
  for (int q = tid * G; q < cn; q += RS_B * G) {
    const int xi = c0 + q - T;  // a multiple of G: the load is 16-byte aligned
    float v[G];
    if (xi >= 0 && xi + G - 1 < n_in) {
      pcm_decode16<G>(fmt, *(const uint4*)(xb + (long long)xi * (16 / G)), v);
    } else {
#pragma unroll
      for (int k = 0; k < G; ++k) v[k] = rs_cat_fmt(hist, xb, fmt, T, n_in, c0 + q + k);
    }
#pragma unroll
    for (int k = 0; k < G; k += 4) *(float4*)(win_s + q + k) = make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
  }
}

// x, y: bytes, with row pitches ldx, ldy in bytes; a row's n_in and n_out count samples of its own formats
__global__ __launch_bounds__(RS_B) void resample_rows_kernel(RsRow* rows, RsSteps steps, const char* x, long long ldx, char* y, long long ldy) {
  __shared__ float tab_s[RS_TAB_LDS];
  __shared__ __attribute__((aligned(16))) float win_s[RS_WIN];
  const int row = blockIdx.y, tid = threadIdx.x;
  const RsStep st = steps.s[row];
  if (!(st.flags & 1)) return;  // a row that sits out: nothing of it is read
  const int o0 = blockIdx.x * RS_B;
  if (blockIdx.x > 0 && o0 >= st.n_out) return;
  const int par = (st.flags >> 1) & 1, n_in = st.n_in;
  const int L = rows[row].L, M = rows[row].M, half = rows[row].half, T = rows[row].T;
  const int in_fmt = rows[row].in_fmt, out_fmt = rows[row].out_fmt;
  const float* tab = rows[row].tab;
  const float* hist = rows[row].hist + par * RS_HCAP;
  const long long consumed = rows[row].cnt[par][0], emitted = rows[row].cnt[par][1];
  const char* xb = x + row * ldx;
  const float* xr = (const float*)xb;
  if (blockIdx.x == 0) {  // the carry: the last T of [history | new samples] and the counts, into the other buffer
    float* hnew = rows[row].hist + (par ^ 1) * RS_HCAP;
    if (in_fmt == PCM_F32)
      for (int i = tid; i < T; i += RS_B) hnew[i] = rs_cat(hist, xr, T, n_in, n_in + i);
    else
      for (int i = tid; i < T; i += RS_B) hnew[i] = rs_cat_fmt(hist, xb, in_fmt, T, n_in, n_in + i);
    if (tid == 0) {
      rows[row].cnt[par ^ 1][0] = consumed + n_in;
      rows[row].cnt[par ^ 1][1] = emitted + st.n_out;
    }
    if (st.n_out == 0) return;
  }
  const int Ts = T | 1;  // odd pitch: the phases of adjacent outputs scatter over the table
  for (int e = tid; e < L * T; e += RS_B) {
    const int p = e / T;
    tab_s[p * Ts + (e - p * T)] = tab[e];
  }
  const int nb = min(RS_B, st.n_out - o0);
  const bool live = tid < nb;
  // this thread's output, and the window of the workgroup: indices into [history | new | zeros], whose element 0 is input consumed - T
  const long long num = (emitted + o0 + (live ? tid : 0)) * M + half, j0 = num / L;
  const int rlo = (int)(j0 + 1 - consumed);  // >= 1: an output whose first input lay before the history was ready a step earlier
  const float* tp = tab_s + (int)(num - j0 * L) * Ts;
  const int wlo = (int)(((emitted + o0) * M + half) / L + 1 - consumed);
  const int whi = (int)(((emitted + o0 + nb - 1) * M + half) / L - consumed) + T;  // the last output's last input, inclusive
  const int G = 16 / pcm_bytes(in_fmt);  // the samples of one 16-byte load: 4, 8 or 16
  int a = wlo - T;  // window starts are moved down to a sample index that is a multiple of G: 16-byte loads of x
  a -= ((a % G) + G) % G;
  float acc = 0.f;
  for (int c0 = a + T; c0 <= whi; c0 += RS_WIN) {
    const int cn = min(RS_WIN, whi - c0 + 1);
    if (in_fmt == PCM_F32) {
      for (int q = tid * 4; q < cn; q += RS_B * 4) {
        const int xi = c0 + q - T;
        float4 v;
        if (xi >= 0 && xi + 3 < n_in) {
          v = *(const float4*)(xr + xi);
        } else {
          v.x = rs_cat(hist, xr, T, n_in, c0 + q);
          v.y = rs_cat(hist, xr, T, n_in, c0 + q + 1);
          v.z = rs_cat(hist, xr, T, n_in, c0 + q + 2);
          v.w = rs_cat(hist, xr, T, n_in, c0 + q + 3);
        }
        *(float4*)(win_s + q) = v;
      }
    } else if (in_fmt == PCM_S16LE) {
      rs_stage<8>(win_s, hist, xb, in_fmt, T, n_in, c0, cn, tid);
    } else {
      rs_stage<16>(win_s, hist, xb, in_fmt, T, n_in, c0, cn, tid);
    }
    __syncthreads();
    if (live) {
      const int i1 = min(T, c0 + cn - rlo);
      for (int i = max(0, c0 - rlo); i < i1; ++i) acc = fmaf(tp[T - 1 - i], win_s[rlo + i - c0], acc);
    }
    __syncthreads();
  }
  if (live) {
    char* yb = y + row * ldy;
    if (out_fmt == PCM_F32) ((float*)yb)[o0 + tid] = acc;
    else pcm_store(yb, out_fmt, o0 + tid, acc);
  }
}

// ---- rows at the model's own rate: no ratio, no state --------------------------------------------------------------------------------------
#define PCM_MAX_ROWS 64
struct PcmRows {  // the launch-argument table, like RsSteps
  int in_fmt[PCM_MAX_ROWS], out_fmt[PCM_MAX_ROWS], n[PCM_MAX_ROWS];
};

// y[row][i] = encode(decode(x[row][i])), i < n[row].  A thread owns the G samples of one 16-byte load of its row's input format (4, 8 or 16)
// and stores them four at a time (16, 8 or 4 bytes); a row's last, partial group goes element by element.  A row with n = 0 is never read.
template <int G>
__device__ static inline void pcm_convert_group(const char* xb, int fi, char* yb, int fo, int n) {
  const long long base = ((long long)blockIdx.x * 256 + threadIdx.x) * G;
  if (base >= n) return;
  if (base + G > n) {
    for (long long i = base; i < n; ++i) pcm_store(yb, fo, i, pcm_load(xb, fi, i));
    return;
  }
  float v[G];
  const uint4 w = *(const uint4*)(xb + base * (16 / G));
  if constexpr (G == 4) {
    v[0] = __uint_as_float(w.x), v[1] = __uint_as_float(w.y), v[2] = __uint_as_float(w.z), v[3] = __uint_as_float(w.w);
  } else {
    pcm_decode16<G>(fi, w, v);
  }
#pragma unroll
  for (int k = 0; k < G; k += 4) {  // base + k is a multiple of 4: the stores are aligned to their own size
    if (fo == PCM_F32) {
      *(float4*)(yb + (base + k) * 4) = make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
    } else if (fo == PCM_S16LE) {
      uint2 o;
      o.x = pcm_encode_bits(fo, v[k]) | (pcm_encode_bits(fo, v[k + 1]) << 16);
      o.y = pcm_encode_bits(fo, v[k + 2]) | (pcm_encode_bits(fo, v[k + 3]) << 16);
      *(uint2*)(yb + (base + k) * 2) = o;
    } else {
      *(unsigned*)(yb + base + k) = pcm_encode_bits(fo, v[k]) | (pcm_encode_bits(fo, v[k + 1]) << 8) | (pcm_encode_bits(fo, v[k + 2]) << 16) |
                                    (pcm_encode_bits(fo, v[k + 3]) << 24);
    }
  }
}

__global__ __launch_bounds__(256) void pcm_convert_rows_kernel(PcmRows t, const char* x, long long ldx, char* y, long long ldy) {
  const int row = blockIdx.y, n = t.n[row], fi = t.in_fmt[row], fo = t.out_fmt[row];
  const char* xb = x + row * ldx;
  char* yb = y + row * ldy;
  if (fi == PCM_F32) pcm_convert_group<4>(xb, fi, yb, fo, n);
  else if (fi == PCM_S16LE) pcm_convert_group<8>(xb, fi, yb, fo, n);
  else pcm_convert_group<16>(xb, fi, yb, fo, n);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
struct kk_resampler {
  int max_rows = 0, max_in = 0;
  RsRow* d_rows = nullptr;
  float* d_tab = nullptr;   // [max_rows][RS_TAB_DEV]
  float* d_hist = nullptr;  // [max_rows][2][RS_HCAP]
  char* pin = nullptr;      // [max_rows] x (RsRow | RS_TAB_DEV floats): what kk_resampler_set_row uploads
  struct Row {
    bool set = false, flushed = false;
    int L = 0, M = 0, half = 0, T = 0, par = 0;
    int in_fmt = KK_PCM_F32, out_fmt = KK_PCM_F32;
    long long consumed = 0, emitted = 0;
    hipEvent_t ev = nullptr;  // behind the row's last upload: its staging block is reused only after it
  };
  std::vector<Row> rows;
};

static const size_t RS_PIN = sizeof(RsRow) + RS_TAB_DEV * sizeof(float);

static long long rs_ready(long long N, int L, int M, int half) {
  const long long a = N * L - 1 - half;
  return a < 0 ? 0 : a / M + 1;
}
static long long rs_out_len(long long N, int L, int M) { return (N * L + M - 1) / M; }

extern "C" int kk_resampler_block_outputs(void) { return RS_B; }

extern "C" void kk_resampler_destroy(kk_resampler* r) {
  if (!r) return;
  for (auto& w : r->rows)
    if (w.ev) {
      (void)hipEventSynchronize(w.ev);
      (void)hipEventDestroy(w.ev);
    }
  if (r->d_rows) (void)hipFree(r->d_rows);
  if (r->d_tab) (void)hipFree(r->d_tab);
  if (r->d_hist) (void)hipFree(r->d_hist);
  if (r->pin) (void)hipHostFree(r->pin);
  delete r;
}

extern "C" int kk_resampler_create(int max_rows, int max_in_per_step, kk_resampler** out) {
  const char* who = "kk_resampler_create";
  if (!out) return kk_failf("%s: null out", who);
  *out = nullptr;
  if (max_rows < 1 || max_rows > RS_MAX_ROWS) return kk_failf("%s: max_rows %d is outside [1, %d]", who, max_rows, RS_MAX_ROWS);
  if (max_in_per_step < 1) return kk_failf("%s: max_in_per_step must be >= 1", who);
  kk_resampler* r = new kk_resampler;
  r->max_rows = max_rows;
  r->max_in = max_in_per_step;
  r->rows.resize(max_rows);
  bool ok = hipMalloc((void**)&r->d_rows, sizeof(RsRow) * max_rows) == hipSuccess &&
            hipMalloc((void**)&r->d_tab, sizeof(float) * RS_TAB_DEV * max_rows) == hipSuccess &&
            hipMalloc((void**)&r->d_hist, sizeof(float) * 2 * RS_HCAP * max_rows) == hipSuccess &&
            hipHostMalloc((void**)&r->pin, RS_PIN * max_rows, hipHostMallocDefault) == hipSuccess;
  for (auto& w : r->rows) ok = ok && hipEventCreateWithFlags(&w.ev, hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    kk_resampler_destroy(r);
    return kk_failf("%s: allocation failed", who);
  }
  *out = r;
  return 0;
}

static int rs_set_row(const char* who, kk_resampler* r, void* stream, int row, int L, int M, const float* taps, int T, int in_fmt, int out_fmt) {
  if (!r) return kk_failf("%s: null resampler", who);
  if (row < 0 || row >= r->max_rows) return kk_failf("%s: row %d is outside [0, %d)", who, row, r->max_rows);
  if (!pcm_known(in_fmt) || !pcm_known(out_fmt)) return kk_failf("%s: unknown format %d -> %d (KK_PCM_*)", who, in_fmt, out_fmt);
  if (L < 1 || M < 1 || L > RS_MAX_RATIO || M > RS_MAX_RATIO) return kk_failf("%s: L = %d, M = %d: both must be in [1, %d]", who, L, M, RS_MAX_RATIO);
  const int half = 10 * (L > M ? L : M);
  if (!taps || T != (2 * half + L) / L) return kk_failf("%s: T = %d, the taps of %d / %d are [%d][%d]", who, T, L, M, L, (2 * half + L) / L);
  hipStream_t st = (hipStream_t)stream;
  kk_resampler::Row& w = r->rows[row];
  if (hipEventSynchronize(w.ev) != hipSuccess) return kk_failf("%s: the row's last upload failed", who);  // (long done, but for two calls in a row)
  char* pin = r->pin + RS_PIN * row;
  RsRow d;
  memset(&d, 0, sizeof d);
  d.L = L, d.M = M, d.half = half, d.T = T;
  d.in_fmt = in_fmt, d.out_fmt = out_fmt;
  d.tab = r->d_tab + (size_t)RS_TAB_DEV * row;
  d.hist = r->d_hist + (size_t)2 * RS_HCAP * row;
  memcpy(pin, &d, sizeof d);
  memcpy(pin + sizeof d, taps, sizeof(float) * L * T);
  w.set = false;
  if (hipMemcpyAsync(r->d_rows + row, pin, sizeof d, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync((void*)d.tab, pin + sizeof d, sizeof(float) * L * T, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(d.hist, 0, sizeof(float) * 2 * RS_HCAP, st) != hipSuccess || hipEventRecord(w.ev, st) != hipSuccess)
    return kk_failf("%s: upload failed", who);
  w.set = true, w.flushed = false;
  w.L = L, w.M = M, w.half = half, w.T = T, w.par = 0, w.consumed = 0, w.emitted = 0;
  w.in_fmt = in_fmt, w.out_fmt = out_fmt;
  return 0;
}

extern "C" int kk_resampler_set_row(kk_resampler* r, void* stream, int row, int L, int M, const float* taps, int T) {
  return rs_set_row("kk_resampler_set_row", r, stream, row, L, M, taps, T, KK_PCM_F32, KK_PCM_F32);
}

extern "C" int kk_resampler_set_row_fmt(kk_resampler* r, void* stream, int row, int L, int M, const float* taps, int T, int in_fmt, int out_fmt) {
  return rs_set_row("kk_resampler_set_row_fmt", r, stream, row, L, M, taps, T, in_fmt, out_fmt);
}

// x, y and their pitches in bytes.  bytes: the call is kk_resampler_step_fmt; else kk_resampler_step, whose rows must all be f32 -> f32.
static int rs_step(const char* who, bool bytes, kk_resampler* r, void* stream, const char* x, long long ldx, const int32_t* n_in, const int32_t* flush,
                   char* y, long long ldy, int32_t* n_out) {
  if (!r || !n_in || !flush || !n_out) return kk_failf("%s: null argument", who);
  RsSteps steps;
  memset(&steps, 0, sizeof steps);
  long long most = -1;
  for (int b = 0; b < r->max_rows; ++b) {  // every refusal before anything is launched or changed
    n_out[b] = 0;
    if (n_in[b] < 0) return kk_failf("%s: row %d: n_in = %d", who, b, n_in[b]);
    if (n_in[b] == 0 && !flush[b]) continue;  // the row sits out
    const kk_resampler::Row& w = r->rows[b];
    if (!w.set) return kk_failf("%s: row %d has no ratio (kk_resampler_set_row)", who, b);
    if (w.flushed) return kk_failf("%s: row %d was flushed: its stream has ended (kk_resampler_set_row starts the next)", who, b);
    if (n_in[b] > r->max_in) return kk_failf("%s: row %d: %d samples, the resampler was created for %d per step", who, b, n_in[b], r->max_in);
    if (!bytes && (w.in_fmt != KK_PCM_F32 || w.out_fmt != KK_PCM_F32))
      return kk_failf("%s: row %d reads format %d and writes format %d: the f32 entry takes f32 rows only (kk_resampler_step_fmt)", who, b, w.in_fmt, w.out_fmt);
    const int bi = pcm_bytes(w.in_fmt), bo = pcm_bytes(w.out_fmt);
    if ((long long)n_in[b] * bi > ldx) return kk_failf("%s: row %d: %d samples in a row of %lld", who, b, n_in[b], ldx / bi);
    const long long N = w.consumed + n_in[b];
    const long long n = (flush[b] ? rs_out_len(N, w.L, w.M) : rs_ready(N, w.L, w.M, w.half)) - w.emitted;
    if (n * bo > ldy) return kk_failf("%s: row %d: %lld outputs in a row of %lld", who, b, n, ldy / bo);
    steps.s[b].n_in = n_in[b];
    steps.s[b].n_out = (int)n;
    steps.s[b].flags = 1 | (w.par << 1);
    if (n > most) most = n;
  }
  if (most < 0) return 0;  // no row takes part
  if (!x || !y || ldx % 16 || ((uintptr_t)x & 15))
    return kk_failf(bytes ? "%s: x must be 16-byte aligned with a row pitch that is a multiple of 16 bytes" : "%s: x must be 16-byte aligned with a row pitch that is a multiple of 4", who);
  if (bytes && (ldy % 16 || ((uintptr_t)y & 15))) return kk_failf("%s: y must be 16-byte aligned with a row pitch that is a multiple of 16 bytes", who);
  const dim3 grid((unsigned)(most > 0 ? (most + RS_B - 1) / RS_B : 1), (unsigned)r->max_rows);
  hipLaunchKernelGGL(resample_rows_kernel, grid, dim3(RS_B), 0, (hipStream_t)stream, r->d_rows, steps, x, ldx, y, ldy);
  KK_CHECK_LAUNCH();
  for (int b = 0; b < r->max_rows; ++b) {
    if (!(steps.s[b].flags & 1)) continue;
    kk_resampler::Row& w = r->rows[b];
    w.consumed += steps.s[b].n_in;
    w.emitted += steps.s[b].n_out;
    w.par ^= 1;
    w.flushed = flush[b] != 0;
    n_out[b] = steps.s[b].n_out;
  }
  return 0;
}

extern "C" int kk_resampler_step(kk_resampler* r, void* stream, const float* x, long long ldx, const int32_t* n_in, const int32_t* flush, float* y,
                                 long long ldy, int32_t* n_out) {
  return rs_step("kk_resampler_step", false, r, stream, (const char*)x, ldx * 4, n_in, flush, (char*)y, ldy * 4, n_out);
}

extern "C" int kk_resampler_step_fmt(kk_resampler* r, void* stream, const void* x, long long ldx_bytes, const int32_t* n_in, const int32_t* flush, void* y,
                                     long long ldy_bytes, int32_t* n_out) {
  if (ldx_bytes < 0 || ldy_bytes < 0) return kk_fail("kk_resampler_step_fmt: a negative row pitch");
  return rs_step("kk_resampler_step_fmt", true, r, stream, (const char*)x, ldx_bytes, n_in, flush, (char*)y, ldy_bytes, n_out);
}

extern "C" int kk_pcm_convert_rows(void* stream, int rows, const void* x, long long ldx_bytes, const int32_t* in_fmt, void* y, long long ldy_bytes,
                                   const int32_t* out_fmt, const int32_t* n) {
  const char* who = "kk_pcm_convert_rows";
  if (rows < 1 || rows > PCM_MAX_ROWS) return kk_failf("%s: rows %d is outside [1, %d]", who, rows, PCM_MAX_ROWS);
  if (!in_fmt || !out_fmt || !n) return kk_failf("%s: null argument", who);
  PcmRows t;
  memset(&t, 0, sizeof t);
  long long groups = 0;
  for (int b = 0; b < rows; ++b) {  // every refusal before the launch
    if (n[b] < 0) return kk_failf("%s: row %d: n = %d", who, b, n[b]);
    if (n[b] == 0) continue;  // the row sits out: its formats are not read either
    if (!pcm_known(in_fmt[b]) || !pcm_known(out_fmt[b])) return kk_failf("%s: row %d: unknown format %d -> %d (KK_PCM_*)", who, b, in_fmt[b], out_fmt[b]);
    const int bi = pcm_bytes(in_fmt[b]), bo = pcm_bytes(out_fmt[b]);
    if ((long long)n[b] * bi > ldx_bytes) return kk_failf("%s: row %d: %d samples in a row of %lld", who, b, n[b], ldx_bytes / bi);
    if ((long long)n[b] * bo > ldy_bytes) return kk_failf("%s: row %d: %d samples into a row of %lld", who, b, n[b], ldy_bytes / bo);
    t.in_fmt[b] = in_fmt[b], t.out_fmt[b] = out_fmt[b], t.n[b] = n[b];
    const long long g = ((long long)n[b] * bi + 15) / 16;
    if (g > groups) groups = g;
  }
  if (groups == 0) return 0;  // no row takes part
  if (!x || !y || ldx_bytes % 16 || ldy_bytes % 16 || ((uintptr_t)x & 15) || ((uintptr_t)y & 15))
    return kk_failf("%s: x and y must be 16-byte aligned with row pitches that are multiples of 16 bytes", who);
  const dim3 grid((unsigned)((groups + 255) / 256), (unsigned)rows);
  hipLaunchKernelGGL(pcm_convert_rows_kernel, grid, dim3(256), 0, (hipStream_t)stream, t, (const char*)x, ldx_bytes, (char*)y, ldy_bytes);
  KK_CHECK_LAUNCH();
  return 0;
}

extern "C" int kk_op_pcm_convert(void* stream, const void* x, int in_fmt, void* y, int out_fmt, int n) {
  if (n < 1) return kk_fail("kk_op_pcm_convert: n must be >= 1");
  const int32_t fi = in_fmt, fo = out_fmt, nn = n;
  const long long big = (long long)1 << 40;  // one row: the pitches only bound n, and the caller vouches for x [n] and y [n]
  return kk_pcm_convert_rows(stream, 1, x, big, &fi, y, big, &fo, &nn);
}

extern "C" int kk_op_resample(void* stream, const float* x, int N, int L, int M, const float* taps, int T, float* y) {
  if (N < 1) return kk_fail("kk_op_resample: N must be >= 1");
  kk_resampler* r = nullptr;
  KK_TRY(kk_resampler_create(1, N, &r));
  const int32_t n_in = N, flush = 1;
  int32_t n_out = 0;
  int rc = kk_resampler_set_row(r, stream, 0, L, M, taps, T);
  if (rc == 0) rc = kk_resampler_step(r, stream, x, ((long long)N + 3) / 4 * 4, &n_in, &flush, y, rs_out_len(N, L > 0 ? L : 1, M > 0 ? M : 1), &n_out);
  if (rc == 0 && hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc = kk_fail("kk_op_resample: stream sync failed");
  kk_resampler_destroy(r);
  return rc;
}
