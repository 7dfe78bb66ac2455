// The sampler family of the CSM frame generator (kk_csm.hip is the handle that launches it): make_sampler of the reference on the device --
// arg-max, top-k by radix select, the whole-vocabulary top-p / min-p form, the per-row table form -- with injected or Philox uniforms, and the raw entry
// points the tests call (kk_op_csm_sample*, kk_op_csm_uniforms).
#include <math.h>

#include <vector>

#include "../../include/kokoro_hip.h"
#include "kk_common.h"
#include "kk_host.h"
#include "kk_kernels.h"
#include "kk_philox.h"

namespace {

// Where a sampling launch takes its uniform from: the injected array (priority), or Philox4x32-10 keyed by the device seed on the counter
// (stream id << 32 | position, code book) -- nothing in it depends on the batch layout, so a stream draws the same numbers alone, in a ragged
// batch or in another slot.  position = *pos + pos_add - pad[b]: the frame being generated, counted in the item's own tokens.
// The fields are KKCsmSampleSrc's (kk_kernels.h), which the handle fills; the kernels keep an argument type of this file.
struct SampleSrc : KKCsmSampleSrc {
  SampleSrc() = default;
  SampleSrc(const KKCsmSampleSrc& a) : KKCsmSampleSrc(a) {}
};
__device__ __forceinline__ float sample_uniform(const SampleSrc& a, int b) {
  if (a.u) return a.u[(long long)b * a.ustride];
  const uint32_t sid = a.sid ? (uint32_t)a.sid[b] : (uint32_t)b;
  const int p = (a.pos ? a.pos[(long long)b * a.pos_stride] : 0) + a.pos_add - (a.pad ? a.pad[b] : 0);
  uint32_t r[4];
  philox4(a.seed[(long long)b * a.seed_stride], ((uint64_t)sid << 32) | (uint32_t)p, (uint32_t)a.cb, r);
  return philox_unit(r[0]);
}
__global__ __launch_bounds__(256) void sample_uniforms_kernel(SampleSrc a, int B, int ncb, float* out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * ncb) return;
  a.cb = e % ncb;
  out[e] = sample_uniform(a, e / ncb);
}
struct SampleCfg : KKCsmSampleCfg {  // kk_csm_sampler as the kernels read it (kokoro_hip.h states the rule)
  SampleCfg() = default;
  SampleCfg(const KKCsmSampleCfg& a) : KKCsmSampleCfg(a) {}
};

// one workgroup per item: argmax (temp == 0 or no uniforms) or inverse CDF over the top_k logits in descending order
// (ties: lower index first) of softmax(logit / temp) with the uniform of item b (sample_uniform).
// Round-based selection (the fallback of sample_select_kernel below): every thread keeps its V / 256 logits and their running maximum in registers; a round is one wave-shuffle argmax, one
// LDS exchange between the four waves (double-buffered: one barrier per round) and a re-scan by the single thread that owned the
// winner -- ~0.3 us per round instead of a scan of all V logits from LDS plus an eight-level LDS tree (90 -> ~15 us for top-50).
template <int NPER>
__device__ void sample_rounds(float (&v)[NPER], int V, float temp, int top_k, const SampleSrc& src, int* out, int ostride) {
  __shared__ float wv[2][4];
  __shared__ int wi[2][4];
  __shared__ float topv[64];
  __shared__ int topi[64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < NPER; ++i)
    if (v[i] > bv) { bv = v[i]; bi = tid + 256 * i; }  // ascending index: the lower index wins a tie
  const bool greedy = (src.u == nullptr && src.seed == nullptr) || temp == 0.f;
  const int k = greedy ? 1 : (top_k < 64 ? (top_k < V ? top_k : V) : 64);
  for (int r = 0; r < k; ++r) {
    float cv = bv;
    int ci = bi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(cv, o);
      const int oi = __shfl_xor(ci, o);
      if (ov > cv || (ov == cv && oi < ci)) { cv = ov; ci = oi; }
    }
    if (lane == 0) { wv[r & 1][wave] = cv; wi[r & 1][wave] = ci; }
    __syncthreads();
    float gv = wv[r & 1][0];
    int gi = wi[r & 1][0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float ov = wv[r & 1][w];
      const int oi = wi[r & 1][w];
      if (ov > gv || (ov == gv && oi < gi)) { gv = ov; gi = oi; }
    }
    if (tid == 0) { topv[r] = gv; topi[r] = gi; }
    if (gi != 0x7fffffff && (gi & 255) == tid) {  // the owner retires the winner and re-scans its own logits
      bv = -INFINITY;
      bi = 0x7fffffff;
#pragma unroll
      for (int i = 0; i < NPER; ++i) {
        if (i == (gi >> 8)) v[i] = -INFINITY;
        if (v[i] > bv) { bv = v[i]; bi = tid + 256 * i; }
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    int pick = topi[0];
    if (!greedy) {
      __shared__ float c[64];  // (LDS, not a private array: scratch memory would be set up for every dispatch of the kernel)
      const float z0 = topv[0] / temp;
      float run = 0.f;
      for (int r = 0; r < k; ++r) {
        run += expf(topv[r] / temp - z0);
        c[r] = run;
      }
      const float target = sample_uniform(src, b) * run;
      int j = 0;
      while (j < k - 1 && c[j] < target) ++j;
      pick = topi[j];
    }
    out[(long long)b * ostride] = (unsigned)pick < (unsigned)V ? pick : 0;  // (a row of NaNs wins no round: still a valid row of the next launch's gather)
  }
}
// Top-k by radix SELECT instead of k rounds of arg-max (rounds are serial: 50 x ~1.3 us however they are organised -- a 256-thread
// barrier per round or a 12-shuffle chain per round in one wave).  Logits become order-preserving 32-bit keys in registers; four 8-bit
// histogram passes (LDS atomics, one wave scans the 256 bins from the top) find the key of the k-th largest logit; every logit >= that key
// is a candidate (k of them plus ties of the k-th); ONE wave sorts the <= 64 candidates (bitonic, value descending, index ascending on
// ties: the oracle's order) and the softmax / inverse-CDF tail is the old one.  More than 64 candidates (a wall of exactly equal logits)
// falls back to the round-based kernel.  Same picks as before, bit for bit.
__device__ __forceinline__ unsigned sk_key(float f) {
  const unsigned bits = __float_as_uint(f);
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
__device__ __forceinline__ float sk_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// The bodies of the sampling kernels as device functions: sample_select_kernel / sample_full_kernel (settings as launch arguments) and
// sample_rows_kernel (settings from the row's table entry) run the SAME source, so with -ffp-contract=off the same arithmetic and the same picks.
// arg-max (lower index on ties): the key order is the float order, so one max over (key, ~index) does it -- no histogram
template <int NPER>
__device__ __forceinline__ void sample_argmax_body(const unsigned (&key)[NPER], int V, int* out, int ostride) {
  __shared__ unsigned long long wbest[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long best = 0ull;
#pragma unroll
  for (int i = 0; i < NPER; ++i) {
    const int j = tid + 256 * i;
    const unsigned long long c = j < V ? (((unsigned long long)key[i] << 32) | (unsigned)(0x7fffffff - j)) : 0ull;
    best = c > best ? c : best;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(best, o);
    best = t > best ? t : best;
  }
  if (lane == 0) wbest[wave] = best;
  __syncthreads();
  if (tid == 0) {
    unsigned long long g = wbest[0];
    for (int w = 1; w < 4; ++w) g = wbest[w] > g ? wbest[w] : g;
    out[(long long)b * ostride] = 0x7fffffff - (int)(unsigned)(g & 0xffffffffull);
  }
}
template <int NPER>
__device__ __forceinline__ void sample_select_body(const float* logits, int V, float temp, int top_k, const SampleSrc& src, int* out, int ostride) {
  __shared__ unsigned hist[256];
  __shared__ unsigned s_prefix, s_krem, s_bin, ccount;
  __shared__ unsigned ckey[64];
  __shared__ int cidx[64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned key[NPER];
#pragma unroll
  for (int i = 0; i < NPER; ++i) {
    const int j = tid + 256 * i;
    key[i] = j < V ? sk_key(logits[(long long)b * V + j]) : 0u;
  }
  const bool greedy = (src.u == nullptr && src.seed == nullptr) || temp == 0.f;
  const int k = greedy ? 1 : (top_k < 64 ? (top_k < V ? top_k : V) : 64);
  if (greedy) {
    sample_argmax_body<NPER>(key, V, out, ostride);
    return;
  }
  unsigned prefix = 0u, mask = 0u, krem = (unsigned)k;
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0u;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NPER; ++i)
      if (tid + 256 * i < V && (key[i] & mask) == prefix) atomicAdd(&hist[(key[i] >> shift) & 255u], 1u);
    __syncthreads();
    if (wave == 0) {  // lane l owns bins 255 - 4l .. 252 - 4l: ascending lanes walk the digits from the top
      const unsigned c0 = hist[255 - 4 * lane], c1 = hist[254 - 4 * lane], c2 = hist[253 - 4 * lane], c3 = hist[252 - 4 * lane];
      const unsigned sum = c0 + c1 + c2 + c3;
      unsigned inc = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
      }
      const unsigned exc = inc - sum;
      if (exc < krem && krem <= inc) {  // exactly one lane: the digit that holds the krem-th largest of the surviving keys
        const unsigned r = krem - exc;
        unsigned bin, above;
        if (r <= c0) { bin = 255 - 4 * lane; above = exc; }
        else if (r <= c0 + c1) { bin = 254 - 4 * lane; above = exc + c0; }
        else if (r <= c0 + c1 + c2) { bin = 253 - 4 * lane; above = exc + c0 + c1; }
        else { bin = 252 - 4 * lane; above = exc + c0 + c1 + c2; }
        s_prefix = prefix | (bin << shift);
        s_krem = krem - above;
        s_bin = hist[bin];
      }
    }
    __syncthreads();
    prefix = s_prefix;
    krem = s_krem;
    mask |= 255u << shift;
    // every key >= prefix (lower digits zero) is a candidate: the k - krem keys above the chosen digit and the s_bin keys that share it.  Once
    // they fit the 64-entry sort the remaining digits need not be resolved (typically after two passes: 16 bits separate the top-50 of 2051 logits)
    if ((unsigned)k - krem + s_bin <= 64u) break;
  }
  if (tid == 0) ccount = 0u;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NPER; ++i)
    if (tid + 256 * i < V && key[i] >= prefix) {
      const unsigned p = atomicAdd(&ccount, 1u);
      if (p < 64u) { ckey[p] = key[i]; cidx[p] = tid + 256 * i; }
    }
  __syncthreads();
  const unsigned nc = ccount;
  if (nc > 64u) {  // block-uniform: a wall of equal logits -- the round-based selection handles any input
    float v[NPER];
#pragma unroll
    for (int i = 0; i < NPER; ++i) v[i] = tid + 256 * i < V ? sk_unkey(key[i]) : -INFINITY;
    sample_rounds<NPER>(v, V, temp, top_k, src, out, ostride);
    return;
  }
  if (wave != 0) return;
  unsigned kk = lane < (int)nc ? ckey[lane] : 0u;
  int ii = lane < (int)nc ? cidx[lane] : 0x7fffffff;
#pragma unroll
  for (int size = 2; size <= 64; size <<= 1)
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const unsigned ok = __shfl_xor(kk, stride);
      const int oi = __shfl_xor(ii, stride);
      const bool other_first = ok > kk || (ok == kk && oi < ii);  // `other` precedes `mine` in the wanted order
      const bool want_first = ((lane & stride) == 0) == ((lane & size) == 0 || size == 64);  // this lane keeps the earlier element
      if (other_first == want_first) { kk = ok; ii = oi; }
    }
  // lane r holds the r-th candidate.  The cumulative sums run in candidate order (the oracle's cumsum) on values read lane by lane
  // (v_readlane with a uniform index): the whole wave walks the same scalar chain, no scratch array, no LDS round trips
  const float tv = sk_unkey(kk);
  auto lane_f = [](float v, int l) __attribute__((always_inline)) { return __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(v), l)); };
  const float t0 = lane_f(tv, 0);
  const float e = (!greedy && lane < k) ? expf(tv / temp - t0 / temp) : 0.f;
  int pick = __builtin_amdgcn_readlane(ii, 0);
  if (!greedy) {
    float run = 0.f;
    for (int r = 0; r < k; ++r) run += lane_f(e, r);
    const float target = sample_uniform(src, b) * run;
    int j = 0;
    float c = lane_f(e, 0);
    while (j < k - 1 && c < target) {
      ++j;
      c += lane_f(e, j);
    }
    pick = __builtin_amdgcn_readlane(ii, __builtin_amdgcn_readfirstlane(j));
  }
  if (lane == 0) out[(long long)b * ostride] = (unsigned)pick < (unsigned)V ? pick : 0;
}
template <int NPER>
__global__ __launch_bounds__(256) void sample_select_kernel(const float* logits, int V, float temp, int top_k, SampleSrc src, int* out, int ostride) {
  sample_select_body<NPER>(logits, V, temp, top_k, src, out, ostride);
}

// The full make_sampler family on the WHOLE vocabulary (top_k = 0 / >= V / > 64, top_p, min_p): one 256-thread workgroup per item.
//   1. (order-preserving key, ~index) pairs of all V logits in LDS (NaN reads as -inf), bitonic sort descending: the order is (logit
//      descending, index ascending), the order of sample_select_kernel and of the oracle;
//   2. thread t owns the N / 256 consecutive sorted positions t N / 256 ..: it sums p-weights exp(l - l_max) and draw weights
//      exp((l - l_max) / temp) over them in order, one fixed-tree block scan (wave shuffles, then the four wave totals in wave order) gives
//      every thread the sums in front of its positions and Z -- no atomics anywhere, the same inputs give the same pick in every slot;
//   3. the cuts: the first sorted position whose mass in front is not < top_p Z, the first whose weight is not >= min_p (p_max's weight
//      is 1), each by a block minimum; n = min(n_k, n_p, max(n_m, min_keep));
//   4. c[n - 1] from its owner, target = u c[n - 1], the first position j < n with c[j] >= target by a block minimum (n - 1 if none).
// Dynamic LDS: N pairs of 8 bytes (64 KiB at N = 8192) + 64 bytes of exchange; no scratch.
__device__ __forceinline__ int sf_block_min(int v, int* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int t = __shfl_xor(v, o);
    v = t < v ? t : v;
  }
  __syncthreads();  // (sh may still be read from the previous use)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const int a = sh[0] < sh[1] ? sh[0] : sh[1], b = sh[2] < sh[3] ? sh[2] : sh[3];
  return a < b ? a : b;
}
template <int N>
__device__ __forceinline__ void sample_full_body(unsigned long long* sf_lds, const float* logits, int V, const SampleCfg& cfg, const SampleSrc& src, int* out,
                                                 int ostride) {
  unsigned long long* sk = sf_lds;
  float* shf = (float*)(sf_lds + N);  // [8]: wave totals of the two scans
  int* shi = (int*)(shf + 8);         // [4] block minimum; [4] c[n - 1]
  constexpr int PER = N / 256;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < N; i += 256) {
    unsigned long long e = 0ull;  // padding sorts behind every logit (the smallest key of a number is that of -inf, 0x007fffff)
    if (i < V) {
      float l = logits[(long long)b * V + i];
      if (!(l == l)) l = -INFINITY;
      if (l == 0.f) l = 0.f;  // -0 and +0 are one logit: a tie, decided by the index (their keys would differ)
      e = ((unsigned long long)sk_key(l) << 32) | (unsigned)(0xffffffffu - (unsigned)i);
    }
    sk[i] = e;
  }
  for (int size = 2; size <= N; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = tid; t < N / 2; t += 256) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const unsigned long long x = sk[i], y = sk[j];
        if ((x < y) == ((i & size) == 0)) { sk[i] = y; sk[j] = x; }  // descending blocks where bit `size` of i is clear (all of them in the last merge)
      }
    }
  __syncthreads();
  const float lmax = sk_unkey((unsigned)(sk[0] >> 32));
  const float temp = cfg.temp;
  // weight of sorted position j at temperature 1 / temp; l == l_max counts as distance 0 (so a row of -inf, or +inf on top, stays finite)
  auto dist = [&](int j) __attribute__((always_inline)) {
    const float l = sk_unkey((unsigned)(sk[j] >> 32));
    return l == lmax ? 0.f : l - lmax;
  };
  const int j0 = tid * PER;
  float s1 = 0.f, sT = 0.f;
  for (int i = 0; i < PER; ++i)
    if (j0 + i < V) {
      const float d = dist(j0 + i);
      s1 += expf(d);
      sT += expf(d / temp);
    }
  float i1 = s1, iT = sT;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t1 = __shfl_up(i1, o), tT = __shfl_up(iT, o);
    if (lane >= o) { i1 += t1; iT += tT; }
  }
  if (lane == 63) { shf[wave] = i1; shf[4 + wave] = iT; }
  float off1 = __shfl_up(i1, 1), offT = __shfl_up(iT, 1);
  if (lane == 0) { off1 = 0.f; offT = 0.f; }
  __syncthreads();
  float base1 = 0.f, baseT = 0.f, Z = 0.f;
  for (int w = 0; w < 4; ++w) {
    if (w < wave) { base1 += shf[w]; baseT += shf[4 + w]; }
    Z += shf[w];
  }
  off1 = base1 + off1;
  offT = baseT + offT;
  const bool use_p = cfg.top_p > 0.f && cfg.top_p < 1.f, use_m = cfg.min_p > 0.f;
  int np = V, nm = V;
  if (use_p || use_m) {
    const float cut = cfg.top_p * Z;
    float run = off1;
    for (int i = 0; i < PER; ++i) {
      const int j = j0 + i;
      if (j < V) {
        const float w = expf(dist(j));
        if (use_p && !(run < cut) && j < np) np = j;
        if (use_m && !(w >= cfg.min_p) && j < nm) nm = j;
        run += w;
      }
    }
    if (use_p) np = sf_block_min(np, shi);
    if (use_m) nm = sf_block_min(nm, shi);
  }
  if (nm < cfg.min_keep) nm = cfg.min_keep;
  int n = (cfg.top_k > 0 && cfg.top_k < V) ? cfg.top_k : V;
  n = np < n ? np : n;
  n = nm < n ? nm : n;
  n = n < 1 ? 1 : (n > V ? V : n);
  float* ctot = (float*)(shi + 4);
  if ((n - 1) / PER == tid) {
    float run = offT;
    for (int i = 0; i < PER; ++i)
      if (j0 + i < n) run += expf(dist(j0 + i) / temp);
    *ctot = run;
  }
  __syncthreads();
  const float target = sample_uniform(src, b) * *ctot;
  int first = n - 1;
  {
    float run = offT;
    for (int i = 0; i < PER; ++i) {
      const int j = j0 + i;
      if (j < n) {
        run += expf(dist(j) / temp);
        if (run >= target && j < first) first = j;
      }
    }
  }
  first = sf_block_min(first, shi);
  if (tid == 0) {
    const unsigned idx = 0xffffffffu - (unsigned)(sk[first] & 0xffffffffull);
    out[(long long)b * ostride] = idx < (unsigned)V ? (int)idx : 0;  // always a valid row of the next launch's embedding gather
  }
}
template <int N>
__global__ __launch_bounds__(256) void sample_full_kernel(const float* logits, int V, SampleCfg cfg, SampleSrc src, int* out, int ostride) {
  extern __shared__ unsigned long long sf_lds[];
  sample_full_body<N>(sf_lds, logits, V, cfg, src, out, ostride);
}

// The sampler with its settings PER ROW: one table entry per cache row (kk_csm_set_row_sampler), read by the row's workgroup, which then takes --
// block-uniformly -- exactly the branch launch_sample would have chosen for that entry, through the bodies above.  One launch per code book serves a
// batch whose rows mix greedy, top-k and top-p / min-p streams, and nothing of the entry is a launch argument: a captured frame step replays
// unchanged when a row's sampler changes.  An all-zero entry (a parked or never-set row) has temp == 0: arg-max, a code in [0, V).
struct RowSampler {  // 32 bytes
  float temp;
  int top_k;
  float top_p, min_p;
  int min_keep, pad_;
  unsigned long long seed;  // Philox seed of the row's stream (SampleSrc::seed_stride = 4)
};
static_assert(sizeof(RowSampler) == 32, "RowSampler is 32 bytes");
__global__ void set_row_sampler_kernel(RowSampler* table, int row, RowSampler e) { table[row] = e; }

__device__ __forceinline__ int rs_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float rs_uniform(float v) { return __uint_as_float((unsigned)__builtin_amdgcn_readfirstlane((int)__float_as_uint(v))); }
// NPER: the select path's logits per thread (V <= 256 NPER); N: the full path's sort size (V <= N).  Every workgroup reserves the full path's
// dynamic LDS (8 N + 64 bytes), whichever branch it takes; the select path's small arrays stay static next to it.
template <int NPER, int N>
__global__ __launch_bounds__(256) void sample_rows_kernel(const float* logits, int V, const RowSampler* table, SampleSrc src, int* out, int ostride) {
  extern __shared__ unsigned long long sf_lds[];
  const RowSampler* e = table + blockIdx.x;
  SampleCfg cfg;  // the entry is one value for the workgroup: held in scalar registers like the launch arguments it replaces
  cfg.temp = rs_uniform(e->temp); cfg.top_k = rs_uniform(e->top_k); cfg.top_p = rs_uniform(e->top_p); cfg.min_p = rs_uniform(e->min_p);
  cfg.min_keep = rs_uniform(e->min_keep);
  const bool greedy = (src.u == nullptr && src.seed == nullptr) || cfg.temp == 0.f;  // launch_sample's rule, word for word
  const bool filters = (cfg.top_p > 0.f && cfg.top_p < 1.f) || cfg.min_p > 0.f;
  if (!greedy && (filters || cfg.top_k <= 0 || cfg.top_k > 64)) sample_full_body<N>(sf_lds, logits, V, cfg, src, out, ostride);
  else sample_select_body<NPER>(logits, V, cfg.temp, cfg.top_k, src, out, ostride);
}

template <int N>
int launch_sample_full(const float* logits, int V, const SampleCfg& cfg, const SampleSrc& src, int* out, int ostride, int B, hipStream_t st) {
  const size_t lds = (size_t)N * 8 + 64;
  static KKDevOnce attr;
  if (attr.first()) {
    (void)hipFuncSetAttribute((const void*)sample_full_kernel<N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr.done();
  }
  hipLaunchKernelGGL(sample_full_kernel<N>, dim3(B), dim3(256), lds, st, logits, V, cfg, src, out, ostride);
  KK_CHECK_LAUNCH();
  return 0;
}

// Which kernel draws: argmax, or top_k in 1..64 with top_p / min_p off -> sample_select_kernel (the shipped default, unchanged picks);
// everything else -> sample_full_kernel.
int launch_sample(const float* logits, int V, const SampleCfg& cfg, const SampleSrc& src, int* out, int ostride, int B, hipStream_t st) {
  if (V > 256 * 32) return kk_fail("kk_csm: audio vocabulary larger than 8192 entries");
  const bool greedy = (src.u == nullptr && src.seed == nullptr) || cfg.temp == 0.f;
  const bool filters = (cfg.top_p > 0.f && cfg.top_p < 1.f) || cfg.min_p > 0.f;
  if (!greedy && (filters || cfg.top_k <= 0 || cfg.top_k > 64)) {
    if (V <= 1024) return launch_sample_full<1024>(logits, V, cfg, src, out, ostride, B, st);
    if (V <= 2048) return launch_sample_full<2048>(logits, V, cfg, src, out, ostride, B, st);
    if (V <= 4096) return launch_sample_full<4096>(logits, V, cfg, src, out, ostride, B, st);
    return launch_sample_full<8192>(logits, V, cfg, src, out, ostride, B, st);
  }
  const float temp = cfg.temp;
  const int top_k = cfg.top_k;
  if (V <= 256 * 4) hipLaunchKernelGGL(sample_select_kernel<4>, dim3(B), dim3(256), 0, st, logits, V, temp, top_k, src, out, ostride);
  else if (V <= 256 * 9) hipLaunchKernelGGL(sample_select_kernel<9>, dim3(B), dim3(256), 0, st, logits, V, temp, top_k, src, out, ostride);
  else hipLaunchKernelGGL(sample_select_kernel<32>, dim3(B), dim3(256), 0, st, logits, V, temp, top_k, src, out, ostride);
  KK_CHECK_LAUNCH();
  return 0;
}

template <int NPER, int N>
int launch_sample_rows_t(const float* logits, int V, const RowSampler* table, const SampleSrc& src, int* out, int ostride, int B, hipStream_t st) {
  const size_t lds = (size_t)N * 8 + 64;
  static KKDevOnce attr;
  if (attr.first()) {
    (void)hipFuncSetAttribute((const void*)sample_rows_kernel<NPER, N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr.done();
  }
  hipLaunchKernelGGL((sample_rows_kernel<NPER, N>), dim3(B), dim3(256), lds, st, logits, V, table, src, out, ostride);
  KK_CHECK_LAUNCH();
  return 0;
}
// launch_sample with row b's settings read from table[b]: V picks the pair (NPER of the select path, N of the full path) launch_sample picks one by one
int launch_sample_rows(const float* logits, int V, const RowSampler* table, const SampleSrc& src, int* out, int ostride, int B, hipStream_t st) {
  if (V > 256 * 32) return kk_fail("kk_csm: audio vocabulary larger than 8192 entries");
  if (V <= 1024) return launch_sample_rows_t<4, 1024>(logits, V, table, src, out, ostride, B, st);
  if (V <= 2048) return launch_sample_rows_t<9, 2048>(logits, V, table, src, out, ostride, B, st);
  if (V <= 256 * 9) return launch_sample_rows_t<9, 4096>(logits, V, table, src, out, ostride, B, st);
  if (V <= 4096) return launch_sample_rows_t<32, 4096>(logits, V, table, src, out, ostride, B, st);
  return launch_sample_rows_t<32, 8192>(logits, V, table, src, out, ostride, B, st);
}

}  // namespace

int kk_csm_sampler_cfg(const kk_csm_sampler* sp, KKCsmSampleCfg* c, const char* who) {
  if (!sp) return kk_failf("%s: null sampler", who);
  if (!(sp->temperature >= 0.f) || !(sp->top_p >= 0.f && sp->top_p <= 1.f) || !(sp->min_p >= 0.f && sp->min_p <= 1.f) || sp->min_tokens_to_keep < 1 || sp->top_k < -1)
    return kk_failf("%s: sampler out of range (temperature >= 0, top_p and min_p in [0, 1], min_tokens_to_keep >= 1, top_k >= -1)", who);
  c->temp = sp->temperature; c->top_k = sp->top_k; c->top_p = sp->top_p; c->min_p = sp->min_p; c->min_keep = sp->min_tokens_to_keep;
  return 0;
}
// ---- what the handle launches (kk_kernels.h)
int kk_launch_csm_sample(hipStream_t st, const float* logits, int V, const KKCsmSampleCfg& cfg, const KKCsmSampleSrc& src, int* out, int ostride, int B) {
  return launch_sample(logits, V, cfg, src, out, ostride, B, st);
}
int kk_launch_csm_sample_rows(hipStream_t st, const float* logits, int V, const void* table, KKCsmSampleSrc src, int* out, int ostride, int B) {
  static_assert(sizeof(RowSampler) == KK_CSM_ROW_SAMPLER_BYTES, "the handle sizes the table");
  if (src.seed) { src.seed = &((const RowSampler*)table)->seed; src.seed_stride = (int)(sizeof(RowSampler) / 8); }
  return launch_sample_rows(logits, V, (const RowSampler*)table, src, out, ostride, B, st);
}
int kk_launch_csm_set_row_sampler(hipStream_t st, void* table, int row, const KKCsmSampleCfg& c, unsigned long long seed) {
  RowSampler e;
  e.temp = c.temp; e.top_k = c.top_k; e.top_p = c.top_p; e.min_p = c.min_p; e.min_keep = c.min_keep; e.pad_ = 0; e.seed = seed;
  hipLaunchKernelGGL(set_row_sampler_kernel, dim3(1), dim3(1), 0, st, (RowSampler*)table, row, e);
  KK_CHECK_LAUNCH();
  return 0;
}

// make_sampler(temp, top_k) on its own (tests): logits [B][V] fp32 -> codes [B] int32, uniforms [B] (NULL or temp == 0: argmax)
extern "C" int kk_op_csm_sample(void* stream, int B, int V, const float* logits, float temperature, int top_k, const float* uniforms, int32_t* codes_out) {
  if (!logits || !codes_out || B < 1 || V < 1) return kk_fail("kk_op_csm_sample: bad argument");
  SampleCfg c;
  c.temp = temperature; c.top_k = top_k;
  SampleSrc s;
  s.u = uniforms; s.ustride = 1;
  return launch_sample(logits, V, c, s, codes_out, 1, B, (hipStream_t)stream);
}

// the whole sampler on its own (tests): uniforms [B] have priority; without them and with use_device_rng, Philox on (seed, stream id, pos[b], code
// book 0) -- `seed` is passed by value here and staged in a device word for the launch; pos [B] device int32 or NULL (0)
extern "C" int kk_op_csm_sample_ex(void* stream, int B, int V, const float* logits, const kk_csm_sampler* sampler, const float* uniforms,
                                   const int32_t* stream_ids, const int32_t* pos, int32_t* codes_out) {
  if (!logits || !codes_out || B < 1 || V < 1) return kk_fail("kk_op_csm_sample_ex: bad argument");
  SampleCfg c;
  KK_TRY(kk_csm_sampler_cfg(sampler, &c, "kk_op_csm_sample_ex"));
  SampleSrc s;
  s.u = uniforms; s.ustride = 1;
  unsigned long long* seed_dev = nullptr;
  if (!uniforms && sampler->use_device_rng) {
    if (hipMalloc((void**)&seed_dev, 8) != hipSuccess) return kk_fail("kk_op_csm_sample_ex: hipMalloc failed");
    const unsigned long long sd = sampler->seed;
    if (hipMemcpy(seed_dev, &sd, 8, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(seed_dev); return kk_fail("kk_op_csm_sample_ex: seed upload failed"); }
    s.seed = seed_dev; s.sid = stream_ids; s.pos = pos; s.pos_stride = 1;
  }
  const int rc = launch_sample(logits, V, c, s, codes_out, 1, B, (hipStream_t)stream);
  if (seed_dev) {
    (void)hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(seed_dev);
  }
  return rc;
}

// launch_sample_rows on its own (tests): row b's settings from samplers[b] (HOST array), through a temporary device table.  uniforms [B] have priority;
// without them the launch draws on the device when the entries say so (use_device_rng must agree across the entries: it is a property of the launch)
extern "C" int kk_op_csm_sample_rows(void* stream, int B, int V, const float* logits, const kk_csm_sampler* samplers, const float* uniforms,
                                     const int32_t* stream_ids, const int32_t* pos, int32_t* codes_out) {
  if (!logits || !codes_out || !samplers || B < 1 || V < 1) return kk_fail("kk_op_csm_sample_rows: bad argument");
  std::vector<RowSampler> host((size_t)B);
  for (int b = 0; b < B; ++b) {
    SampleCfg c;
    KK_TRY(kk_csm_sampler_cfg(samplers + b, &c, "kk_op_csm_sample_rows"));
    if ((samplers[b].use_device_rng != 0) != (samplers[0].use_device_rng != 0)) return kk_fail("kk_op_csm_sample_rows: use_device_rng differs between the entries");
    RowSampler& e = host[(size_t)b];
    e.temp = c.temp; e.top_k = c.top_k; e.top_p = c.top_p; e.min_p = c.min_p; e.min_keep = c.min_keep; e.pad_ = 0; e.seed = samplers[b].seed;
  }
  RowSampler* table = nullptr;
  if (hipMalloc((void**)&table, (size_t)B * sizeof(RowSampler)) != hipSuccess) return kk_fail("kk_op_csm_sample_rows: hipMalloc failed");
  if (hipMemcpy(table, host.data(), (size_t)B * sizeof(RowSampler), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(table);
    return kk_fail("kk_op_csm_sample_rows: table upload failed");
  }
  SampleSrc s;
  s.u = uniforms; s.ustride = 1;
  if (!uniforms && samplers[0].use_device_rng) {
    s.seed = &table->seed; s.sid = stream_ids; s.pos = pos; s.pos_stride = 1;
  }
  const int rc = kk_launch_csm_sample_rows((hipStream_t)stream, logits, V, table, s, codes_out, 1, B);
  (void)hipStreamSynchronize((hipStream_t)stream);
  (void)hipFree(table);
  return rc;
}

// the uniforms the sampling kernels draw (sample_uniform): out [B][n_cb] for (seed, stream_ids[b] or b, pos[b] or 0, code book)
extern "C" int kk_op_csm_uniforms(void* stream, int B, int n_cb, uint64_t seed, const int32_t* stream_ids, const int32_t* pos, float* out) {
  if (!out || B < 1 || n_cb < 1) return kk_fail("kk_op_csm_uniforms: bad argument");
  unsigned long long* seed_dev = nullptr;
  if (hipMalloc((void**)&seed_dev, 8) != hipSuccess) return kk_fail("kk_op_csm_uniforms: hipMalloc failed");
  const unsigned long long sd = seed;
  if (hipMemcpy(seed_dev, &sd, 8, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(seed_dev); return kk_fail("kk_op_csm_uniforms: seed upload failed"); }
  SampleSrc s;
  s.seed = seed_dev; s.sid = stream_ids; s.pos = pos; s.pos_stride = 1;
  hipLaunchKernelGGL(sample_uniforms_kernel, dim3((B * n_cb + 255) / 256), dim3(256), 0, (hipStream_t)stream, s, B, n_cb, out);
  const bool ok = hipGetLastError() == hipSuccess;
  (void)hipStreamSynchronize((hipStream_t)stream);
  (void)hipFree(seed_dev);
  return ok ? 0 : kk_fail("kk_op_csm_uniforms: launch failed");
}
