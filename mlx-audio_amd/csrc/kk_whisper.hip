// Whisper, audio side (gfx950): the log-mel front end, a long-sequence non-causal attention kernel and the audio encoder behind a handle.
// Restates mlx_audio/stt/models/whisper/audio.py:41-82 (log_mel_spectrogram) and whisper.py:171-199 (AudioEncoder); DESIGN 8f.
//
// ---- log-mel (fp32) -------------------------------------------------------------------------------------------------------------------
//   logmel_frames_kernel: one workgroup per (frame, row).  The 400 windowed samples of the frame go to LDS (reflect padding of 200 at both
//   ends of the row's n + padding samples, samples >= n are the zero padding and are never read), thread k < 201 walks them in index order
//   with the twiddle cos / sin[(i k) mod 400] from the host's float64 table (four interleaved fmaf chains per part, combined in a fixed
//   order), the 201 powers go back to LDS and thread m < n_mels sums its filter row over the bins in index order.  log10(max(., 1e-10)) is
//   stored, and the frame's maximum goes to partial[b][frame].
//   logmel_finish_kernel: every workgroup takes the maximum of the row's partials (a maximum does not depend on order), then clamps at
//   max - 8 and maps (. + 4) / 4.  Rows of the output past the row's frame count are zeros.
//   A row's bits depend on its own samples alone: no sum crosses a row, a frame or a workgroup.
//   logmel_spans_kernel / logmel_spans_finish_kernel: the same frame body (logmel_frame) behind the resampler's fmaf chains, for spans
//   of sample buffers at another rate -- see the comment above them.
//
// ---- attention (bf16, v_mfma_f32_16x16x32_bf16) ------------------------------------------------------------------------------------------
//   One workgroup = 64 query rows of one (item, head), 4 waves of 16 query rows; keys walked in tiles of 64 through LDS in index order.
//   Scores are computed TRANSPOSED, S^T = K Q^T (A = key rows from LDS, B = the wave's query fragment, held in registers for the whole walk):
//   the accumulator then has the query on the lane (lane & 15) and keys 16 c + 4 (lane >> 4) + r in register r of block c, so the softmax
//   of a query is a reduction over a lane's 16 registers and lanes l, l ^ 16, l ^ 32, and the probabilities, rounded to bf16 in place, ARE the
//   B fragment of O^T = V^T P^T (B[k][col = query]): the two 16-key blocks 2 s, 2 s + 1 form k-step s, with k = 8 g + j standing for key
//   32 s + 16 (j >> 2) + 4 g + (j & 3).  The A operand takes V^T in that same key order: V is transposed while it is staged (Vt[d][key], two keys
//   per 32-bit LDS write), and a lane reads keys 32 s + 4 g .. + 3 and 32 s + 16 + 4 g .. + 3 of its d row as two 8-byte reads.
//   Running maximum and sum in fp32 per query; scale and log2(e) folded into one multiply, exp2 from v_exp_f32.  Keys >= T get a score of
//   -inf by SELECT and their V rows are staged as zeros (0 x NaN would poison the row); query rows >= T are computed from row T - 1 and
//   not stored.  LDS: K tile [64][72] bf16 (144-byte rows: the 16-byte fragment reads of 16 consecutive rows fall on distinct bank groups),
//   Vt [64][68].
#include "kk_host.h"
#include "../../include/kokoro_hip.h"

#include <math.h>

namespace {
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NFFT = 400, HOP = 160, NBIN = 201, RPAD = 200;

// ------------------------------------------------------------------------------------------------------------------------------ log-mel
// The arithmetic of one frame, from its 400 windowed samples in fr (staged by the caller, no barrier yet) to its n_mels log values: the twiddles
// go to LDS, the DFT, the filter bank and log10 run as described above.  orow: where the frame's values go, or null for a frame that only enters
// the row's maximum.  Returns the frame's maximum (valid in thread 0).  Every thread of the workgroup calls it.
__device__ static inline float logmel_frame(float* fr, float* tc, float* ts, float* pw, float* wmax, int n_mels, const float* cs, const float* fbT,
                                            float* orow, int tid) {
  for (int i = tid; i < NFFT; i += 256) {
    tc[i] = cs[i];
    ts[i] = cs[NFFT + i];
  }
  __syncthreads();
  if (tid < NBIN) {
    const int k = tid;
    float re[4] = {0.f, 0.f, 0.f, 0.f}, im[4] = {0.f, 0.f, 0.f, 0.f};
    int idx = 0;  // (i k) mod 400
    for (int i = 0; i < NFFT; i += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float v = fr[i + u];
        re[u] = __builtin_fmaf(v, tc[idx], re[u]);
        im[u] = __builtin_fmaf(v, ts[idx], im[u]);
        idx += k;
        idx = idx >= NFFT ? idx - NFFT : idx;
      }
    }
    const float r = (re[0] + re[1]) + (re[2] + re[3]), q = (im[0] + im[1]) + (im[2] + im[3]);
    pw[k] = __builtin_fmaf(r, r, q * q);
  }
  __syncthreads();
  float lg = -INFINITY;
  if (tid < n_mels) {
    float acc = 0.f;
    for (int k = 0; k < NBIN; ++k) acc = __builtin_fmaf(pw[k], fbT[k * n_mels + tid], acc);
    lg = acc > 1e-10f ? log10f(acc) : -10.0f;  // log10(max(mel, 1e-10)); the floor itself is exactly -10
    if (orow) orow[tid] = lg;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lg = fmaxf(lg, __shfl_xor(lg, o));
  if ((tid & 63) == 0) wmax[tid >> 6] = lg;
  __syncthreads();
  return fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
}

// max(., row maximum - 8), (. + 4) / 4
__device__ static inline float logmel_scale(float v, float lo) { return (fmaxf(v, lo) + 4.0f) * 0.25f; }

// the maximum of partial[0 .. F) in every thread of the workgroup
__device__ static inline float logmel_row_max(const float* partial, int F, float* wmax, int tid) {
  float mx = -INFINITY;
  for (int f = tid; f < F; f += 256) mx = fmaxf(mx, partial[f]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if ((tid & 63) == 0) wmax[tid >> 6] = mx;
  __syncthreads();
  return fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
}

__global__ __launch_bounds__(256) void logmel_frames_kernel(const float* x, long long ldx, const int* n, int padding, int n_mels, const float* window,
                                                            const float* cs, const float* fbT, float* partial, float* out, int F_rows) {
  __shared__ float fr[NFFT];
  __shared__ float tc[NFFT], ts[NFFT];
  __shared__ float pw[NBIN + 3];
  __shared__ float wmax[4];
  const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int nb = n[b], N = nb + padding, F = N / HOP;
  float* orow = out + ((long long)b * F_rows + f) * n_mels;
  if (f >= F) {  // (uniform) past the row's frames: zeros
    if (tid < n_mels) orow[tid] = 0.f;
    if (tid == 0) partial[(long long)b * F_rows + f] = -INFINITY;
    return;
  }
  const float* xb = x + (long long)b * ldx;
  for (int i = tid; i < NFFT; i += 256) {
    int j = f * HOP + i - RPAD;
    j = j < 0 ? -j : j;
    j = j >= N ? 2 * (N - 1) - j : j;
    j = j < 0 ? 0 : j;  // (only a row shorter than the reflect padding, which the callers refuse)
    const float v = j < nb ? xb[j] : 0.f;  // [n, N) is the zero padding: never read
    fr[i] = v * window[i];
  }
  const float mx = logmel_frame(fr, tc, ts, pw, wmax, n_mels, cs, fbT, orow, tid);
  if (tid == 0) partial[(long long)b * F_rows + f] = mx;
}

__global__ __launch_bounds__(256) void logmel_finish_kernel(const int* n, int padding, int n_mels, const float* partial, float* out, int F_rows) {
  __shared__ float wmax[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int F = (n[b] + padding) / HOP;
  const float lo = logmel_row_max(partial + (long long)b * F_rows, F, wmax, tid) - 8.0f;
  const long long total = (long long)F * n_mels;
  float* ob = out + (long long)b * F_rows * n_mels;
  for (long long e = (long long)blockIdx.x * 2048 + tid; e < (long long)(blockIdx.x + 1) * 2048 && e < total; e += 256)
    ob[e] = logmel_scale(ob[e], lo);
}

// ---- a span of a sample buffer becomes a Whisper window --------------------------------------------------------------------
//   Row r: the n samples of its span (a flat buffer from `pos` on, or the ring of kk_ring.hip, sample i at (pos + i) % ring_len) are resampled
//   L / M to 16 kHz (n16 = ceil(n L / M) samples), log_mel with padding = 160 W runs over them and the first W frames are the window.
//   logmel_spans_kernel: one workgroup per (frame, row).  The frame's 16 kHz samples q0 .. q1 (at most 400; reflected indices of frames 0 and 1
//   fall inside the same run) are recomputed here: the source samples they read, (q0 M + half) / L - T + 1 .. (q1 M + half) / L, go to LDS with
//   the ring's wrap resolved and ZEROS wherever the index is outside [0, n) -- the buffer is never read there -- and thread q runs kk_resample.hip's
//   one fmaf chain from 0.0f over the T taps of its phase in ascending input order.  L == M: the samples are taken as they are.  Then the
//   frame body above.  A frame whose 400 samples are all padding (160 f - 200 >= n16; with W >= 3 every frame that sees a sample exists and the reflection at the clip's end never
//   reaches back to a sample) is the floor -10 in every bin: written, not computed.  Frames W and W + 1 may still see the clip's tail: they
//   are computed for the maximum and not stored; later ones are silent, and a silent frame cannot raise a maximum that frame 0 already
//   holds at >= -10.
//   logmel_spans_finish_kernel: the maximum over the row's W + 2 partials, the clamp and the scale over its W stored frames.
constexpr int SP_WIN = 1536, SP_TAB = 512, SP_EXTRA = 2;
struct KKMelSpans {  // by value: the rows may lie in different allocations
  const float* buf[KK_WHISPER_MAX_ROWS];
  long long pos[KK_WHISPER_MAX_ROWS];  // flat: the span's first element; ring: its stream position
  int ring_len[KK_WHISPER_MAX_ROWS], n[KK_WHISPER_MAX_ROWS], n16[KK_WHISPER_MAX_ROWS];
};

__global__ __launch_bounds__(256) void logmel_spans_kernel(KKMelSpans t, int W, int L, int M, int half, int T, const float* tab, int n_mels,
                                                           const float* window, const float* cs, const float* fbT, float* partial, float* out) {
  __shared__ float fr[NFFT];
  __shared__ float tc[NFFT], ts[NFFT];
  __shared__ float pw[NBIN + 3];
  __shared__ float wmax[4];
  __shared__ float seg[NFFT];
  __shared__ float win_s[SP_WIN];
  __shared__ float tab_s[SP_TAB];
  const int f = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  const int n = t.n[r], n16 = t.n16[r];
  float* orow = f < W ? out + ((long long)r * W + f) * n_mels : nullptr;
  float* prow = partial + (long long)r * (W + SP_EXTRA);
  const int lo = f * HOP - RPAD;
  if (lo >= n16) {  // (uniform) all padding: the floor
    if (orow && tid < n_mels) orow[tid] = -10.0f;
    if (tid == 0) prow[f] = -10.0f;
    return;
  }
  const int q0 = lo < 0 ? 0 : lo, q1 = min(max(lo + NFFT - 1, -lo), n16 - 1);  // the 16 kHz samples the frame reads (frame 0 reflects -200 to 200)
  const int cnt = q1 - q0 + 1;
  const long long s0 = L == M ? q0 : ((long long)q0 * M + half) / L - T + 1;  // source index of win_s[0]
  const int sn = L == M ? cnt : (int)(((long long)q1 * M + half) / L - s0) + 1;  // <= SP_WIN: the host has checked the ratio
  {
    const float* buf = t.buf[r];
    const long long pos = t.pos[r];
    const int ring = t.ring_len[r];
    const long long base = ring ? pos % ring : pos;
    for (int e = tid; e < sn; e += 256) {
      const long long i = s0 + e;
      float v = 0.f;  // outside the span: a zero that is multiplied, from a slot that is never read
      if (i >= 0 && i < n) {
        long long a = base + i;
        if (ring && a >= ring) a -= ring;  // i < n <= ring_len
        v = buf[a];
      }
      win_s[e] = v;
    }
  }
  const int Ts = T | 1;
  if (L != M)
    for (int e = tid; e < L * T; e += 256) {
      const int p = e / T;
      tab_s[p * Ts + (e - p * T)] = tab[e];
    }
  __syncthreads();
  for (int e = tid; e < cnt; e += 256) {
    if (L == M) {
      seg[e] = win_s[e];
    } else {
      const long long num = (long long)(q0 + e) * M + half, j0 = num / L;
      const float* tp = tab_s + (int)(num - j0 * L) * Ts;
      const float* wp = win_s + (int)(j0 - T + 1 - s0);
      float acc = 0.f;
      for (int i = 0; i < T; ++i) acc = fmaf(tp[T - 1 - i], wp[i], acc);
      seg[e] = acc;
    }
  }
  __syncthreads();
  for (int i = tid; i < NFFT; i += 256) {
    int j = lo + i;
    j = j < 0 ? -j : j;  // (the reflection at the padded clip's end stays inside the zero padding)
    const float v = j < n16 ? seg[j - q0] : 0.f;
    fr[i] = v * window[i];
  }
  const float mx = logmel_frame(fr, tc, ts, pw, wmax, n_mels, cs, fbT, orow, tid);
  if (tid == 0) prow[f] = mx;
}

__global__ __launch_bounds__(256) void logmel_spans_finish_kernel(int W, int n_mels, const float* partial, float* out) {
  __shared__ float wmax[4];
  const int r = blockIdx.y, tid = threadIdx.x;
  const float lo = logmel_row_max(partial + (long long)r * (W + SP_EXTRA), W + SP_EXTRA, wmax, tid) - 8.0f;
  const long long total = (long long)W * n_mels;
  float* ob = out + (long long)r * total;
  for (long long e = (long long)blockIdx.x * 2048 + tid; e < (long long)(blockIdx.x + 1) * 2048 && e < total; e += 256)
    ob[e] = logmel_scale(ob[e], lo);
}

// ---------------------------------------------------------------------------------------------------------------------------- attention
constexpr int AQ = 64, AK = 64, KLD = 72, VLD = 68;

__global__ __launch_bounds__(256) void attention_long_kernel(const bf16_t* qkv, long long bs, int ld, int T, int heads, bf16_t* out, long long obs,
                                                             int ldo) {
  __shared__ __attribute__((aligned(16))) bf16_t Ks[AK * KLD];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[64 * VLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z, q0 = blockIdx.x * AQ;
  const int hs = heads * 64, t_hi = T - 1;
  const bf16_t* base = qkv + (long long)b * bs;

  // the wave's query fragment: B[k = d][col = query], lane (lr, g) holds d = 32 ks + 8 g .. + 7 of query lr
  const int qrow = q0 + wave * 16 + lr;
  const bf16_t* qp = base + (long long)(qrow < t_hi ? qrow : t_hi) * ld + h * 64 + 8 * g;
  const bf16x8 qf0 = *(const bf16x8*)qp, qf1 = *(const bf16x8*)(qp + 32);

  // staging: thread (kp, ch) moves 8 channels of keys 2 kp and 2 kp + 1 of K and of V
  const int kp = tid >> 3, ch = tid & 7;
  uint4 kr0, kr1, vr0, vr1;
  auto load_tile = [&](int k0) __attribute__((always_inline)) {
    const int r0 = k0 + 2 * kp < t_hi ? k0 + 2 * kp : t_hi, r1 = k0 + 2 * kp + 1 < t_hi ? k0 + 2 * kp + 1 : t_hi;
    const bf16_t* kb = base + hs + h * 64 + ch * 8;
    kr0 = *(const uint4*)(kb + (long long)r0 * ld);
    kr1 = *(const uint4*)(kb + (long long)r1 * ld);
    vr0 = *(const uint4*)(kb + hs + (long long)r0 * ld);
    vr1 = *(const uint4*)(kb + hs + (long long)r1 * ld);
  };
  auto store_tile = [&](int k0) __attribute__((always_inline)) {
    *(uint4*)(Ks + (2 * kp) * KLD + ch * 8) = kr0;
    *(uint4*)(Ks + (2 * kp + 1) * KLD + ch * 8) = kr1;
    const unsigned m0 = k0 + 2 * kp < T ? 0xFFFFFFFFu : 0u, m1 = k0 + 2 * kp + 1 < T ? 0xFFFFFFFFu : 0u;  // V rows past T: exact zeros
    const unsigned a[4] = {vr0.x & m0, vr0.y & m0, vr0.z & m0, vr0.w & m0}, c[4] = {vr1.x & m1, vr1.y & m1, vr1.z & m1, vr1.w & m1};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      *(unsigned*)(Vt + (ch * 8 + 2 * w) * VLD + 2 * kp) = (a[w] & 0xFFFFu) | (c[w] << 16);
      *(unsigned*)(Vt + (ch * 8 + 2 * w + 1) * VLD + 2 * kp) = (a[w] >> 16) | (c[w] & 0xFFFF0000u);
    }
  };

  float m = -1e30f, l = 0.f;  // running maximum (log2 domain) and this lane's share of the running sum, of query lr
  f32x4 o[4];                 // O^T[d = 16 db + 4 g + r][query lr]
#pragma unroll
  for (int db = 0; db < 4; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float sc = 0.125f * 1.4426950408889634f;  // 64^-0.5 log2(e)
  const int ntile = (T + AK - 1) / AK;
  load_tile(0);
  for (int it = 0; it < ntile; ++it) {
    const int k0 = it * AK;
    __syncthreads();  // the previous tile's readers are done
    store_tile(k0);
    __syncthreads();
    if (it + 1 < ntile) load_tile(k0 + AK);  // lands while this tile is computed

    f32x4 s[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bf16_t* kf = Ks + (16 * c + lr) * KLD + 8 * g;
      s[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)kf, qf0, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      s[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(kf + 32), qf1, s[c], 0, 0, 0);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float t = k0 + 16 * c + 4 * g + r < T ? s[c][r] * sc : -INFINITY;
        s[c][r] = t;
        mx = fmaxf(mx, t);
      }
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
    for (int db = 0; db < 4; ++db) {
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
    bf16_t* op = out + (long long)b * obs + (long long)qrow * ldo + h * 64 + 4 * g;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      const bf16x4 w = {(bf16_t)(o[db][0] * inv), (bf16_t)(o[db][1] * inv), (bf16_t)(o[db][2] * inv), (bf16_t)(o[db][3] * inv)};
      *(bf16x4*)(op + 16 * db) = w;
    }
  }
}

int launch_attention_long(hipStream_t st, int B, const void* qkv, long long bs, int ld, int T, int heads, void* out, long long obs, int ldo) {
  dim3 grid((T + AQ - 1) / AQ, heads, B);
  hipLaunchKernelGGL(attention_long_kernel, grid, dim3(256), 0, st, (const bf16_t*)qkv, bs, ld, T, heads, (bf16_t*)out, obs, ldo);
  KK_CHECK_LAUNCH();
  return 0;
}
}  // namespace

extern "C" int kk_op_log_mel(void* stream, int B, const float* x, long long ldx, const int32_t* n, int padding, int n_mels, const float* window,
                             const float* cos_sin, const float* fbT, float* partial, float* out, int F_rows) {
  if (!x || !n || !window || !cos_sin || !fbT || !partial || !out) return kk_fail("kk_op_log_mel: null argument");
  if (B < 1 || F_rows < 1 || padding < 0 || ldx < 1) return kk_fail("kk_op_log_mel: bad argument");
  if (n_mels != 80 && n_mels != 128) return kk_fail("kk_op_log_mel: n_mels must be 80 or 128");
  hipLaunchKernelGGL(logmel_frames_kernel, dim3(F_rows, B), dim3(256), 0, (hipStream_t)stream, x, ldx, n, padding, n_mels, window, cos_sin, fbT, partial,
                     out, F_rows);
  KK_CHECK_LAUNCH();
  const long long total = (long long)F_rows * n_mels;
  hipLaunchKernelGGL(logmel_finish_kernel, dim3((unsigned)((total + 2047) / 2048), B), dim3(256), 0, (hipStream_t)stream, n, padding, n_mels, partial,
                     out, F_rows);
  KK_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------------- mel windows
// The windows of a transcription round: row r is `size[r]` frames of its file's spectrogram from frame first[r] on, then zeros up to W
// frames.  A frame is n_mels floats (320 or 512 bytes), so a window is a run of 16-byte words in both the source and the output: thread t of
// block x moves words 1024 x + t + 256 u, u = 0 .. 3, all four requested before the first is stored.  No arithmetic.
namespace {
struct KKMelWindows {  // by value: the rows may lie in different allocations
  const float* src[KK_WHISPER_MAX_ROWS];
  int first[KK_WHISPER_MAX_ROWS], size[KK_WHISPER_MAX_ROWS];
};
__global__ __launch_bounds__(256) void mel_windows_kernel(KKMelWindows t, int W, int n_mels, float* out) {
  const int r = blockIdx.y, q = n_mels / 4;  // q: 16-byte words per frame
  const long long total = (long long)W * q, have = (long long)t.size[r] * q;
  const f32x4* src = (const f32x4*)t.src[r] + (long long)t.first[r] * q;
  f32x4* dst = (f32x4*)out + (long long)r * total;
  const long long base = (long long)blockIdx.x * 1024 + threadIdx.x;
  f32x4 v[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long long i = base + 256 * u;
    v[u] = i < have ? src[i] : f32x4{0.f, 0.f, 0.f, 0.f};  // (i < have <= total: never past the file's frames, which the host has checked)
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long long i = base + 256 * u;
    if (i < total) dst[i] = v[u];
  }
}
}  // namespace

extern "C" int kk_op_mel_windows(void* stream, int R, const float* const* src, const int32_t* frames, const int32_t* first, const int32_t* size, int W, int n_mels,
                                 float* out) {
  const char* who = "kk_op_mel_windows";
  if (!src || !frames || !first || !size || !out) return kk_failf("%s: null argument", who);
  if (R < 1 || R > KK_WHISPER_MAX_ROWS) return kk_failf("%s: R = %d is outside [1, %d]", who, R, KK_WHISPER_MAX_ROWS);
  if (W < 1) return kk_failf("%s: W = %d must be >= 1", who, W);
  if (n_mels != 80 && n_mels != 128) return kk_failf("%s: n_mels must be 80 or 128", who);
  if ((uintptr_t)out & 15) return kk_failf("%s: out must be 16-byte aligned", who);
  KKMelWindows t;
  memset(&t, 0, sizeof t);
  for (int r = 0; r < R; ++r) {
    if (size[r] < 0 || size[r] > W) return kk_failf("%s: row %d: size = %d is outside [0, W = %d]", who, r, size[r], W);
    if (first[r] < 0 || frames[r] < 0 || (long long)first[r] + size[r] > frames[r])
      return kk_failf("%s: row %d: frames %d .. %lld are outside the source's %d", who, r, first[r], (long long)first[r] + size[r], frames[r]);
    if (size[r] > 0 && (!src[r] || ((uintptr_t)src[r] & 15))) return kk_failf("%s: row %d: the source must be a 16-byte aligned device pointer", who, r);
    t.src[r] = src[r];
    t.first[r] = first[r];
    t.size[r] = size[r];
  }
  const long long total = (long long)W * (n_mels / 4);
  hipLaunchKernelGGL(mel_windows_kernel, dim3((unsigned)((total + 1023) / 1024), R), dim3(256), 0, (hipStream_t)stream, t, W, n_mels, out);
  KK_CHECK_LAUNCH();
  return 0;
}

extern "C" int kk_op_log_mel_spans(void* stream, int R, const float* const* buf, const int64_t* buf_len, const int32_t* ring_len, const int64_t* pos,
                                   const int32_t* n, int W, int L, int M, const float* tab, int T, int n_mels, const float* window, const float* cos_sin,
                                   const float* fbT, float* partial, float* out) {
  const char* who = "kk_op_log_mel_spans";
  if (!buf || !buf_len || !ring_len || !pos || !n || !window || !cos_sin || !fbT || !partial || !out) return kk_failf("%s: null argument", who);
  if (R < 1 || R > KK_WHISPER_MAX_ROWS) return kk_failf("%s: R = %d is outside [1, %d]", who, R, KK_WHISPER_MAX_ROWS);
  if (W < 3 || W > (1 << 20)) return kk_failf("%s: W = %d is outside [3, 2^20]", who, W);
  if (n_mels != 80 && n_mels != 128) return kk_failf("%s: n_mels must be 80 or 128", who);
  if (L < 1 || M < 1) return kk_failf("%s: L = %d, M = %d: both must be >= 1", who, L, M);
  int half = 0;
  if (L == M) {
    L = M = 1, T = 0;
  } else {
    half = 10 * (L > M ? L : M);
    if (!tab || T != (2 * half + L) / L) return kk_failf("%s: T = %d, the taps of %d / %d are [%d][%d]", who, T, L, M, L, (2 * half + L) / L);
    if ((long long)L * (T | 1) > SP_TAB || ((long long)(NFFT - 1) * M) / L + T + 2 > SP_WIN)
      return kk_failf("%s: the ratio %d / %d is not served: its phase table or a frame's source samples do not fit the workgroup's LDS", who, L, M);
  }
  KKMelSpans t;
  memset(&t, 0, sizeof t);
  for (int r = 0; r < R; ++r) {
    if (!buf[r]) return kk_failf("%s: row %d: null buffer", who, r);
    if (n[r] < 1) return kk_failf("%s: row %d: n = %d must be >= 1", who, r, n[r]);
    const long long n16 = ((long long)n[r] * L + M - 1) / M;
    if (n16 > (long long)W * HOP) return kk_failf("%s: row %d: %d samples are %lld at 16 kHz, a window holds %lld", who, r, n[r], n16, (long long)W * HOP);
    if (pos[r] < 0) return kk_failf("%s: row %d: a negative position", who, r);
    if (ring_len[r] < 0) return kk_failf("%s: row %d: a negative ring length", who, r);
    if (ring_len[r] ? (n[r] > ring_len[r] || buf_len[r] < ring_len[r]) : (pos[r] + n[r] > buf_len[r]))
      return kk_failf("%s: row %d: the span [%lld, + %d) does not lie in its buffer of %lld (ring %d)", who, r, (long long)pos[r], n[r], (long long)buf_len[r],
                      ring_len[r]);
    t.buf[r] = buf[r];
    t.pos[r] = pos[r];
    t.ring_len[r] = ring_len[r];
    t.n[r] = n[r];
    t.n16[r] = (int)n16;
  }
  hipLaunchKernelGGL(logmel_spans_kernel, dim3(W + SP_EXTRA, R), dim3(256), 0, (hipStream_t)stream, t, W, L, M, half, T, tab, n_mels, window, cos_sin, fbT,
                     partial, out);
  KK_CHECK_LAUNCH();
  const long long total = (long long)W * n_mels;
  hipLaunchKernelGGL(logmel_spans_finish_kernel, dim3((unsigned)((total + 2047) / 2048), R), dim3(256), 0, (hipStream_t)stream, W, n_mels, partial, out);
  KK_CHECK_LAUNCH();
  return 0;
}

extern "C" int kk_op_attention_long(void* stream, int B, const void* qkv, int ld, int T_rows, int T, int heads, void* out, int ldo) {
  if (!qkv || !out) return kk_fail("kk_op_attention_long: null argument");
  if (B < 1 || heads < 1 || T < 1 || T > T_rows) return kk_fail("kk_op_attention_long: bad argument (need B, heads >= 1 and 1 <= T <= T_rows)");
  if (ld < 3 * heads * 64) return kk_fail("kk_op_attention_long: ld is smaller than q | k | v of `heads` heads of 64 channels");
  if (ldo < heads * 64) return kk_fail("kk_op_attention_long: ldo is smaller than `heads` heads of 64 channels");
  if (ld % 8 != 0 || ldo % 4 != 0 || ((uintptr_t)qkv & 15) || ((uintptr_t)out & 7))
    return kk_fail("kk_op_attention_long: qkv must be 16-byte aligned with ld % 8 == 0, out 8-byte aligned with ldo % 4 == 0");
  return launch_attention_long((hipStream_t)stream, B, qkv, (long long)T_rows * ld, ld, T, heads, out, (long long)T_rows * ldo, ldo);
}

// ------------------------------------------------------------------------------------------------------------------------------ encoder
struct WLin {  // a Linear / convolution packed for the bf16 MFMA kernel: bf16 [Kw][CoutP][CinP] at `w`, fp32 bias [CoutP] at `b`
  size_t w = 0, b = 0;
  int Kw = 1, CinP = 0, CoutP = 0, Cin = 0;
};
struct WLayer {
  WLin qkv, out, mlp1, mlp2;
  size_t attn_ln_w = 0, attn_ln_b = 0, mlp_ln_w = 0, mlp_ln_b = 0;
};

struct kk_whisper {
  kk_whisper_config cfg;
  std::map<std::string, HostTensor> host;
  bool finalized = false;
  bf16_t* wdev = nullptr;  // every packed matrix
  float* fdev = nullptr;   // biases, LayerNorm parameters, the position table
  WLin conv1, conv2;
  std::vector<WLayer> layers;
  size_t ln_post_w = 0, ln_post_b = 0, pos = 0;
};

namespace {
int check_cfg(const kk_whisper_config& c) {
  if (c.n_mels != 80 && c.n_mels != 128) return kk_fail("kk_whisper_create: n_mels must be 80 or 128");
  if (c.n_audio_ctx < 1 || c.n_audio_layer < 1 || c.n_audio_head < 1) return kk_fail("kk_whisper_create: bad dimensions");
  if (c.n_audio_state != 64 * c.n_audio_head) return kk_fail("kk_whisper_create: the head dimension n_audio_state / n_audio_head must be 64");
  if (c.n_audio_state % 128 != 0 || c.n_audio_state > 2048) return kk_fail("kk_whisper_create: n_audio_state must be a multiple of 128, at most 2048");
  return 0;
}
}  // namespace

extern "C" int kk_whisper_create(const kk_whisper_config* cfg, kk_whisper** out) {
  if (!cfg || !out) return kk_fail("kk_whisper_create: null argument");
  KK_TRY(check_cfg(*cfg));
  kk_whisper* m = new kk_whisper();
  m->cfg = *cfg;
  *out = m;
  return 0;
}

extern "C" void kk_whisper_destroy(kk_whisper* m) {
  if (!m) return;
  if (m->wdev) (void)hipFree(m->wdev);
  if (m->fdev) (void)hipFree(m->fdev);
  delete m;
}

extern "C" int kk_whisper_load_tensor(kk_whisper* m, const char* name, const int64_t* shape, int ndim, const float* data) {
  return kk_host_load_tensor("kk_whisper_load_tensor", m ? &m->host : nullptr, m && m->finalized, name, shape, ndim, data);
}

extern "C" int kk_whisper_finalize(kk_whisper* m, void* stream) {
  if (!m) return kk_fail("kk_whisper_finalize: null model");
  if (m->finalized) return kk_fail("kk_whisper_finalize: already finalized");
  const kk_whisper_config& c = m->cfg;
  const int D = c.n_audio_state, M = c.n_mels, ctx = c.n_audio_ctx;
  hipStream_t st = (hipStream_t)stream;
  // plan
  size_t wn = 0, fn = 0;
  auto plan = [&](WLin& l, int Kw, int CoutP, int CinP, int Cin) {
    l.Kw = Kw; l.CoutP = CoutP; l.CinP = CinP; l.Cin = Cin;
    l.w = wn; wn += (size_t)Kw * CoutP * CinP;
    l.b = fn; fn += (size_t)CoutP;
  };
  auto planv = [&](size_t& off, size_t n) { off = fn; fn += (n + 63) & ~(size_t)63; };
  plan(m->conv1, 3, D, 128, M);
  plan(m->conv2, 2, D, 2 * D, 2 * D);  // the stride-2 k 3 convolution as a k 2 convolution over PAIRS of rows, see kk_whisper_encode
  m->layers.resize(c.n_audio_layer);
  for (auto& L : m->layers) {
    plan(L.qkv, 1, 3 * D, D, D);
    plan(L.out, 1, D, D, D);
    plan(L.mlp1, 1, 4 * D, D, D);
    plan(L.mlp2, 1, D, 4 * D, 4 * D);
    planv(L.attn_ln_w, D); planv(L.attn_ln_b, D); planv(L.mlp_ln_w, D); planv(L.mlp_ln_b, D);
  }
  planv(m->ln_post_w, D); planv(m->ln_post_b, D);
  planv(m->pos, (size_t)ctx * D);
  if (hipMalloc((void**)&m->wdev, wn * sizeof(bf16_t)) != hipSuccess || hipMalloc((void**)&m->fdev, fn * sizeof(float)) != hipSuccess)
    return kk_fail("kk_whisper_finalize: hipMalloc failed");

  std::string err;
  std::vector<float> fpack(fn, 0.f);
  std::vector<uint16_t> wpack;
  // one matrix at a time: pack (round to nearest even), copy, drop the host copy -- a large checkpoint is never held twice
  auto flush = [&](const WLin& l) -> int {
    if (hipMemcpyAsync((uint16_t*)m->wdev + l.w, wpack.data(), wpack.size() * 2, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return kk_fail("kk_whisper_finalize: upload failed");
    return 0;
  };
  auto vecp = [&](size_t off, const std::string& name, int n) {
    if (const HostTensor* t = kk_host_want(m->host, name, {n}, err)) memcpy(&fpack[off], t->d.data(), (size_t)n * 4);
  };
  // rows [o0, o0 + N) of a Linear's pack from an [N][K] matrix
  auto lin_rows = [&](const WLin& l, const std::string& name, int o0, int N, int K) {
    const HostTensor* t = kk_host_want(m->host, name, {N, K}, err);
    if (!t) return;
    for (int o = 0; o < N; ++o)
      for (int i = 0; i < K; ++i) wpack[(size_t)(o0 + o) * l.CinP + i] = f32_to_bf16_rne(t->d[(size_t)o * K + i]);
    m->host.erase(name);
  };
  {  // conv1: MLX layout [O][K][I] -> [tap][O][128]
    wpack.assign((size_t)3 * D * 128, 0);
    if (const HostTensor* t = kk_host_want(m->host, "encoder.conv1.weight", {D, 3, M}, err))
      for (int o = 0; o < D; ++o)
        for (int k = 0; k < 3; ++k)
          for (int i = 0; i < M; ++i) wpack[((size_t)k * D + o) * 128 + i] = f32_to_bf16_rne(t->d[((size_t)o * 3 + k) * M + i]);
    vecp(m->conv1.b, "encoder.conv1.bias", D);
    KK_TRY(flush(m->conv1));
  }
  {  // conv2 over row pairs (x[2p] | x[2p + 1]): out[q] = [0 | W0] pair[q - 1] + [W1 | W2] pair[q]
    wpack.assign((size_t)2 * D * 2 * D, 0);
    if (const HostTensor* t = kk_host_want(m->host, "encoder.conv2.weight", {D, 3, D}, err))
      for (int o = 0; o < D; ++o)
        for (int i = 0; i < D; ++i) {
          const float* w = &t->d[(size_t)o * 3 * D + i];
          wpack[((size_t)0 * D + o) * 2 * D + D + i] = f32_to_bf16_rne(w[0]);
          wpack[((size_t)1 * D + o) * 2 * D + i] = f32_to_bf16_rne(w[D]);
          wpack[((size_t)1 * D + o) * 2 * D + D + i] = f32_to_bf16_rne(w[2 * D]);
        }
    m->host.erase("encoder.conv2.weight");
    vecp(m->conv2.b, "encoder.conv2.bias", D);
    KK_TRY(flush(m->conv2));
  }
  for (int li = 0; li < c.n_audio_layer; ++li) {
    WLayer& L = m->layers[li];
    const std::string p = "encoder.blocks." + std::to_string(li) + ".";
    wpack.assign((size_t)3 * D * D, 0);
    lin_rows(L.qkv, p + "attn.query.weight", 0, D, D);
    lin_rows(L.qkv, p + "attn.key.weight", D, D, D);
    lin_rows(L.qkv, p + "attn.value.weight", 2 * D, D, D);
    vecp(L.qkv.b, p + "attn.query.bias", D);  // the key has no bias: its third stays zero
    vecp(L.qkv.b + 2 * D, p + "attn.value.bias", D);
    KK_TRY(flush(L.qkv));
    wpack.assign((size_t)D * D, 0);
    lin_rows(L.out, p + "attn.out.weight", 0, D, D);
    vecp(L.out.b, p + "attn.out.bias", D);
    KK_TRY(flush(L.out));
    wpack.assign((size_t)4 * D * D, 0);
    lin_rows(L.mlp1, p + "mlp1.weight", 0, 4 * D, D);
    vecp(L.mlp1.b, p + "mlp1.bias", 4 * D);
    KK_TRY(flush(L.mlp1));
    lin_rows(L.mlp2, p + "mlp2.weight", 0, D, 4 * D);
    vecp(L.mlp2.b, p + "mlp2.bias", D);
    KK_TRY(flush(L.mlp2));
    vecp(L.attn_ln_w, p + "attn_ln.weight", D); vecp(L.attn_ln_b, p + "attn_ln.bias", D);
    vecp(L.mlp_ln_w, p + "mlp_ln.weight", D); vecp(L.mlp_ln_b, p + "mlp_ln.bias", D);
  }
  vecp(m->ln_post_w, "encoder.ln_post.weight", D);
  vecp(m->ln_post_b, "encoder.ln_post.bias", D);
  if (!err.empty()) return kk_failf("kk_whisper_finalize: %s", err.c_str());
  {  // sinusoids(n_ctx, n_state), whisper.py:81-87, in fp32: sin | cos of t * exp(-log(10000) / (D/2 - 1) * j)
    const int half = D / 2;
    const float inc = (float)(log(10000.0) / (half - 1));
    for (int j = 0; j < half; ++j) {
      const float inv = expf(-inc * (float)j);
      for (int t = 0; t < ctx; ++t) {
        const float a = (float)t * inv;
        fpack[m->pos + (size_t)t * D + j] = sinf(a);
        fpack[m->pos + (size_t)t * D + half + j] = cosf(a);
      }
    }
  }
  if (hipMemcpyAsync(m->fdev, fpack.data(), fn * 4, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return kk_fail("kk_whisper_finalize: upload failed");
  m->host.clear();
  m->finalized = true;
  return 0;
}

namespace {
struct EncPlan {
  bf16_t *melb, *c1, *lnb, *qkv, *att, *h;
  float *x, *lnf;
};
void plan_encode(const kk_whisper_config& c, int B, Workspace& ws, EncPlan& p) {
  const size_t D = c.n_audio_state, ctx = c.n_audio_ctx, rows = (size_t)B * ctx;
  p.melb = (bf16_t*)ws.raw(rows * 2 * 128 * 2);
  p.c1 = (bf16_t*)ws.raw(rows * 2 * D * 2);
  p.x = (float*)ws.raw(rows * D * 4);
  p.lnf = (float*)ws.raw(rows * D * 4);
  p.lnb = (bf16_t*)ws.raw(rows * D * 2);
  p.qkv = (bf16_t*)ws.raw(rows * 3 * D * 2);
  p.att = (bf16_t*)ws.raw(rows * D * 2);
  p.h = (bf16_t*)ws.raw(rows * 4 * D * 2);
}
}  // namespace

extern "C" size_t kk_whisper_encode_workspace_bytes(const kk_whisper* m, int B) {
  if (!m || B < 1) return 0;
  Workspace ws;
  EncPlan p;
  plan_encode(m->cfg, B, ws, p);
  return ws.used + 256;
}

extern "C" int kk_whisper_encode(kk_whisper* m, void* stream, int B, const float* mel, void* workspace, size_t workspace_bytes, float* out) {
  if (!m || !mel || !workspace || !out || B < 1) return kk_fail("kk_whisper_encode: bad argument");
  if (!m->finalized) return kk_fail("kk_whisper_encode: model not finalized");
  const kk_whisper_config& c = m->cfg;
  const int D = c.n_audio_state, M = c.n_mels, ctx = c.n_audio_ctx, H = c.n_audio_head;
  hipStream_t st = (hipStream_t)stream;
  Workspace ws;
  ws.base = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  ws.cap = workspace_bytes - (size_t)(ws.base - (char*)workspace);
  EncPlan p;
  plan_encode(c, B, ws, p);
  if (ws.oom) return kk_fail("kk_whisper_encode: workspace too small");

  // one Linear / convolution on the bf16 MFMA kernel: out = act(x W + bias) (+ res), rows dense
  auto conv = [&](const WLin& l, const bf16_t* x, int ldx, int rows_in, int rows_out, int pad, int act, const void* res, long long rbs, void* o,
                  int ldo, int out_dtype) -> int {
    KKMfmaArgs g;
    memset(&g, 0, sizeof g);
    g.x = x; g.xbs = (long long)rows_in * ldx; g.ldx = ldx; g.w = m->wdev + l.w; g.CinP = l.CinP; g.CoutP = l.CoutP; g.Cin = l.Cin;
    g.bias = m->fdev + l.b; g.out = o; g.obs = (long long)rows_out * ldo; g.ldo = ldo; g.res = res; g.rbs = rbs; g.ldr = ldo;
    g.Cout = l.CoutP; g.Kw = l.Kw; g.mode = KK_CONV; g.stride = 1; g.pad = pad; g.dil = 1; g.Q = rows_out; g.Lo_rows = rows_out;
    g.lin = KKLen{nullptr, 0, rows_in}; g.lout = KKLen{nullptr, 0, rows_out};
    g.in_slope = 1.0f; g.scale = 1.0f; g.act = act;
    return kk_launch_conv_mfma(g, B, out_dtype, st);
  };
  // LayerNorm of the fp32 stream, then one rounding to bf16 for the matrix cores
  auto ln = [&](size_t w, size_t b, float* dst) -> int {
    KKLnArgs a;
    memset(&a, 0, sizeof a);
    a.x = p.x; a.xbs = (long long)ctx * D; a.ldx = D; a.out = dst; a.obs = a.xbs; a.ldo = D; a.C = D; a.Lmax = ctx;
    a.len = KKLen{nullptr, 0, ctx}; a.w = m->fdev + w; a.bias = m->fdev + b; a.eps = 1e-5f;
    return kk_launch_layernorm(a, B, KK_F32, st);
  };
  auto ln_bf16 = [&](size_t w, size_t b) -> int {
    KK_TRY(ln(w, b, p.lnf));
    return kk_launch_convert(p.lnf, KK_F32, (long long)ctx * D, D, p.lnb, KK_BF16, (long long)ctx * D, D, D, ctx, B, st);
  };

  // stem (whisper.py:190-193).  mel fp32 [B][2 ctx][n_mels] -> bf16 rows of 128 channels (the pad channels are masked by the kernel)
  KK_TRY(kk_launch_convert(mel, KK_F32, (long long)2 * ctx * M, M, p.melb, KK_BF16, (long long)2 * ctx * 128, 128, M, 2 * ctx, B, st));
  KK_TRY(conv(m->conv1, p.melb, 128, 2 * ctx, 2 * ctx, 1, KK_ACT_GELU, nullptr, 0, p.c1, D, KK_BF16));
  // conv2 (k 3, stride 2, pad 1) on the stride-1 kernel: conv1's rows taken in pairs [ctx][2 D], out[q] = [0 | W0] pair[q - 1] + [W1 | W2] pair[q];
  // the positions are the epilogue's residual (the same table for every item: item stride 0), the sum is the fp32 stream
  KK_TRY(conv(m->conv2, p.c1, 2 * D, ctx, ctx, 1, KK_ACT_GELU, m->fdev + m->pos, 0, p.x, D, KK_F32));
  for (const WLayer& L : m->layers) {  // whisper.py:157-168
    KK_TRY(ln_bf16(L.attn_ln_w, L.attn_ln_b));
    KK_TRY(conv(L.qkv, p.lnb, D, ctx, ctx, 0, KK_ACT_NONE, nullptr, 0, p.qkv, 3 * D, KK_BF16));
    KK_TRY(launch_attention_long(st, B, p.qkv, (long long)ctx * 3 * D, 3 * D, ctx, H, p.att, (long long)ctx * D, D));
    KK_TRY(conv(L.out, p.att, D, ctx, ctx, 0, KK_ACT_NONE, p.x, (long long)ctx * D, p.x, D, KK_F32));
    KK_TRY(ln_bf16(L.mlp_ln_w, L.mlp_ln_b));
    KK_TRY(conv(L.mlp1, p.lnb, D, ctx, ctx, 0, KK_ACT_GELU, nullptr, 0, p.h, 4 * D, KK_BF16));
    KK_TRY(conv(L.mlp2, p.h, 4 * D, ctx, ctx, 0, KK_ACT_NONE, p.x, (long long)ctx * D, p.x, D, KK_F32));
  }
  KK_TRY(ln(m->ln_post_w, m->ln_post_b, out));  // ln_post straight into the caller's fp32 output
  return 0;
}
