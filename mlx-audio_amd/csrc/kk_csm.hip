// CSM-1B frame generator: SesameModel.generate_frame, mlx_audio/tts/models/sesame/sesame.py:349-395
//   tokens [B][S][n_cb+1] -> masked sum of 33 embeddings -> Llama backbone (KV cache) -> codebook0 head -> sample ->
//   31 x { projection -> Llama depth decoder (fresh cache per frame) -> audio_head[i-1] -> sample -> embed } -> codes [B][n_cb]
// Llama layer (mlx_lm LlamaModel with the reference's Attention, sesame.py:296-299; attention.py:113-195):
//   h += Wo . attn(rope(Wq x), rope(Wk x), Wv x), x = rms(h);   h += Wdown (silu(Wgate x) * Wup x), x = rms(h);   final rms
//   RoPE: interleaved pairs, llama3-scaled frequencies (attention.py:33-110); GQA: query head h reads kv head h / (H / KV);
//   mask: causal inside the new block, every cached key visible (sesame.py:37-48).
// Round 1: fp32, the library's generic conv kernel for every linear (M = B*S rows is tiny in the decode loop), one simple attention
// kernel for both head sizes.  The KV caches are library-owned device memory (kk_csm_setup_caches), like the module-owned caches of
// the reference (sesame.py:320-333).
#include <math.h>
#include <string.h>

#include <atomic>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "../../include/kokoro_hip.h"
#include "kk_common.h"
#include "kk_host.h"
#include "kk_philox.h"

namespace {

#include "kk_csm_gemvm.h"

struct Lin {  // generic-kernel pack [1][Cin][ldw]
  size_t off = 0;
  int Cin = 0, Cout = 0, ldw = 0;
  const float* w = nullptr;
  // bf16 weight mode (kk_csm_set_weight_dtype): the same matrix as bf16 in FRAGMENT order for the matrix-core GEMV (gemvm_kernel) of the
  // single-token steps and the prompt GEMM (gemmp_kernel): [Cout / (16 nsub)][Cin / 32][nsub][64 lanes][8]: a wave
  // load of 1 KiB is one 32 x 16 B operand of v_mfma_f32_16x16x32_bf16 (lane L: k = 32 c + 8 (L / 16) + j, n = 16 s + L % 16)
  size_t moff = 0;
  const uint16_t* wm = nullptr;
  bool has_f32 = true;
  int nsub = 0;  // 0 = no fragment pack (K not a multiple of 32)
  int ks = 1;    // split-K slices of a deep projection (K >= 4096): partial tiles + combine
  // packed storage of a quantised checkpoint (kk_csm_load_quantized): `wm` points at the quantised fragment pack instead (kk_csm_gemvm.h,
  // KK_WF_Q8 / KK_WF_Q4), `wp` at its (scale, bias) pairs; such a matrix has NO fp32 copy (w == nullptr) and no bf16 one
  int fmt = KK_WF_BF16, group = 0;
  size_t qoff = 0, poff = 0;  // byte offsets into kk_csm::packq
  const float2* wp = nullptr;
};
struct LlamaLayer {
  Lin qkv, o, gu, down;
  ArenaVec n1, n2;
};
struct Stack {
  kk_llama_args a;
  std::vector<LlamaLayer> layers;
  ArenaVec norm, rope;  // rope: [max_pos][hd/2][2] cos, sin
  float* kc = nullptr;  // [layers][maxB][max_pos][KV*hd]
  float* vc = nullptr;
  int max_pos = 0, offset = 0;
  int* pos_dev = nullptr;  // backbone only: device copy of `offset` (null: positions are launch constants)
  int* pad_dev = nullptr;  // backbone only: [max_batch] left padding of each item's prompt (kk_csm_set_padding), zeros by default
  size_t layer_pitch = 0;  // floats between two layers of kc / vc; 0: the caches' own max_batch * max_pos * KV * hd (kk_csm_prefix_create sets its buffer's)
};

}  // namespace

struct kk_csm {
  kk_csm_config cfg;
  WeightArena arena;  // fp32 parameters; arena.dev is shared by kk_csm_share copies
  bool finalized = false;
  int wdt = KK_F32;              // weight storage of the single-token steps (KK_F32 / KK_BF16)
  std::vector<uint16_t> packb;   // host staging of the bf16 copies
  uint16_t* devb = nullptr;
  // quantised checkpoint: tensors as loaded; the packed Linears' integer fragment packs + pairs (bytes; shared like devb)
  std::map<std::string, QuantHost> qhost;
  std::vector<uint8_t> packq;
  uint8_t* devq = nullptr;
  bool packed = false;           // kk_csm_finalize's all-or-nothing decision: every Linear of the fast path runs from its quantised pack
  bool q_fallback = false;       // a quantised checkpoint that was dequantised on the host instead (bf16 weight mode)
  std::string q_reason;          // why
  int n_q8 = 0, n_q4 = 0;        // packed Linears per format
  size_t linear_bytes = 0, table_bytes = 0, total_bytes = 0;  // device bytes of the Linears' storage / of the projection table
  Stack bb, dec;
  ArenaVec text_emb, audio_emb;
  Lin proj, c0_head;
  std::vector<Lin> audio_head;
  int max_batch = 0;
  float* dbg_logits = nullptr;  // [n_cb][maxB][V] of the last frame
  float* proj_table = nullptr;  // bf16 weight mode: projection(audio_embeddings) [n_cb * V][decoder hidden], computed once at finalize (weights: shared by kk_csm_share)
  // graph replay of the single-token frame step (kk_csm_set_graph_mode)
  bool graph_mode = false;
  GraphCache graphs{8};  // a kk_csm_share copy starts with an empty cache
  // kk_csm_reset_caches / kk_csm_set_padding take no stream: what they change on the device is applied on the NEXT frame's stream (a
  // synchronous hipMemset / hipMemcpy here would touch the legacy stream and break another thread's graph capture)
  bool reset_pending = false, pad_pending = false;
  std::vector<int32_t> pad_host;  // host mirror of bb.pad_dev ([max_batch] since kk_csm_setup_caches); max_pos = a parked row (kk_csm_park_row)
  int* admit_sid_dev = nullptr;   // kk_csm_admit: the new stream's id where the sampling kernels read it
  int32_t admit_sid_host = 0;
  // device RNG of the sampler (kk_csm_sampler.use_device_rng): the Philox seed in device memory, read by the sampling kernels
  unsigned long long* seed_dev = nullptr;
  unsigned long long seed_host = 0;
  bool seed_valid = false;
  // per-row sampler table (kk_csm_set_row_sampler / kk_csm_generate_frame_rows): [max_batch] entries of 32 bytes (RowSampler), zero = arg-max
  void* row_samplers = nullptr;
  bool row_samplers_zero_pending = false;  // kk_csm_reset_caches_parked takes no stream: zeroed on the next stream that flushes
  unsigned long long weights_id = 0;   // the weight set (kk_csm_finalize; kk_csm_share copies it): what a kk_csm_prefix is tied to
  const kk_csm* weights_of = nullptr;  // kk_csm_share: `dev` / `devb` / `devq` belong to that generator (immutable after finalize), not to this one
  // kk_csm_admit_transfer into THIS generator: the source's stream has finished the admission / this stream has finished the copy.  Created at the
  // first transfer, destroyed with the generator (a kk_csm_share copy starts without them).
  hipEvent_t xfer_ready = nullptr, xfer_done = nullptr;
};

namespace {

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

// kk_csm_admit_prefixed: the K / V of a shared prefix ([layer][K|V][n][KV hd] fp32, compact) go under a stream's suffix -- into the n slots of ONE
// cache row that start at `kc` / `vc` (the caller has added row and first slot), in every layer: blockIdx.y = 2 layer + (0 K, 1 V).  Per (layer,
// K|V) both sides are ONE contiguous run of seg4 = n KV hd / 4 16-byte columns, so this is a plain streaming copy: a workgroup owns 16 KiB of
// the run (eight 2 KiB slot rows at CSM-1B's geometry), a thread four columns 4 KiB apart -- every wave instruction moves 1 KiB of consecutive
// bytes --, the four loads are issued ahead of the four stores.  Default cache policy on both sides: the prefix is read again by the next
// admission (10 MB at n = 160 stay in the last-level cache) and the row is read right behind by the suffix block's attention.
__global__ __launch_bounds__(256) void prefix_restore_kernel(const float4* src, float* kc, float* vc, long long layer_pitch4, long long seg4) {
  const int z = blockIdx.y;
  const float4* s = src + (long long)z * seg4;
  float4* d = (float4*)((z & 1) ? vc : kc) + (long long)(z >> 1) * layer_pitch4;
  const long long i0 = (long long)blockIdx.x * 1024 + threadIdx.x;
  float4 r[4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (i0 + 256 * u < seg4) r[u] = s[i0 + 256 * u];
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (i0 + 256 * u < seg4) d[i0 + 256 * u] = r[u];
}

// kk_csm_prefix_capture: the mirror of prefix_restore_kernel.  The first n slots of ONE live cache row (`kc` / `vc`: the caller has added row and
// first slot) leave for a compact prefix buffer `dst` ([layer][K|V][n][KV hd] fp32), every layer's K and V in one launch: blockIdx.y = 2 layer +
// (0 K, 1 V).  Same work division: 16 KiB per workgroup, four 16-byte columns 4 KiB apart per thread, loads ahead of stores, the tail checked.
// It reads nothing outside the row's window [first slot, first slot + n) and writes nothing but `dst`.
__global__ __launch_bounds__(256) void prefix_capture_kernel(const float* kc, const float* vc, float4* dst, long long layer_pitch4, long long seg4) {
  const int z = blockIdx.y;
  const float4* s = (const float4*)((z & 1) ? vc : kc) + (long long)(z >> 1) * layer_pitch4;
  float4* d = dst + (long long)z * seg4;
  const long long i0 = (long long)blockIdx.x * 1024 + threadIdx.x;
  float4 r[4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (i0 + 256 * u < seg4) r[u] = s[i0 + 256 * u];
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (i0 + 256 * u < seg4) d[i0 + 256 * u] = r[u];
}

// kk_csm_admit_transfer: the window of ONE live row of another generator's cache (`skc` / `svc`: the caller has added row and first slot) goes
// into the same number of slots of ONE row of this generator's (`kc` / `vc`, likewise), every layer's K and V in one launch: blockIdx.y =
// 2 layer + (0 K, 1 V).  A key is stored rotated by its stream's own position, so the move is a plain copy.  Per (layer, K|V) both sides are one
// contiguous run of seg4 16-byte columns; only the layer pitches differ (max_batch * max_pos of the two generators need not match).  The form
// of prefix_restore_kernel: 16 KiB per workgroup, four 16-byte columns 4 KiB apart per thread, loads ahead of stores, the tail checked.  It
// reads nothing outside the source window and writes nothing outside the destination's L slots.
__global__ __launch_bounds__(256) void row_transfer_kernel(const float* skc, const float* svc, long long src_pitch4, float* kc, float* vc,
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

// Where a sampling launch takes its uniform from: the injected array (priority), or Philox4x32-10 keyed by the device seed on the counter
// (stream id << 32 | position, code book) -- nothing in it depends on the batch layout, so a stream draws the same numbers alone, in a ragged
// batch or in another slot.  position = *pos + pos_add - pad[b]: the frame being generated, counted in the item's own tokens.
struct SampleSrc {
  const float* u = nullptr;  // [B] at pitch ustride, or null
  int ustride = 0;
  const unsigned long long* seed = nullptr;  // device; null = no device RNG
  int seed_stride = 0;                       // 64-bit words between the seeds of two items: 0 = one word for the launch, 4 = the row's RowSampler entry
  const int* sid = nullptr;                  // [B] stream ids, null = batch index
  const int* pos = nullptr;                  // device position(s): pos[b * pos_stride]
  int pos_stride = 0, pos_add = 0;
  const int* pad = nullptr;                  // [B] left padding, or null
  int cb = 0;
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
struct SampleCfg {  // kk_csm_sampler as the kernels read it (kokoro_hip.h states the rule)
  float temp = 0.f;
  int top_k = 0;
  float top_p = 0.f, min_p = 0.f;
  int min_keep = 1;
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

// Skinny GEMM for the single-token steps (M = B rows <= 16): out[m][n] = sum_k x[m][k] W[k][n].  The grid is (column blocks) x (KS
// slices of K): every thread streams ONE column (fp32 weights) or TWO adjacent columns (bf16 weights, one 4-byte load) of its K slice
// with coalesced row reads, 16 loads in flight; the slices' partial sums are added in slice order by the second kernel
// (deterministic, residual fused).  The rows are held as PACKED PAIRS: xs[k][m] keeps the M activations of one k adjacent, so a
// weight meets rows (2i, 2i+1) in one v_pk_fma_f32 -- MT/2 packed FMAs per weight (MT = 8 or 16 rows, a template parameter).  The
// first version issued 16 predicated scalar FMAs per weight whatever M was and was VALU-bound (K*N*16 lane-FMAs: 13.6 us for the
// backbone's gate|up matrix against a 13 us HBM floor in bf16), which is why halving the weight bytes did not pay before.
// `GATED`: x is the gate|up pair of a SwiGLU MLP ([M][2K]) and the staged input is silu(gate) * up (the stand-alone swiglu kernel of
// the single-token step disappears).
constexpr int SK_MAXM = 16, SK_KC = 256;
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
  // all slices are requested at once (a plain loop is KS dependent L2 round trips); KS <= 16 (Lin::ks)
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
static void gemmp_weights(GPArgs& g, const Lin& w) {
  g.w = w.wm; g.nsub = w.nsub; g.fmt = w.fmt; g.wp = w.wp; g.gmagic = w.fmt != KK_WF_BF16 ? wf_group_magic(w.group) : 0;
}

// ------------------------------------------------------------------------------------------------------------- host
// fp32 bits -> bf16 bits, round to nearest even (a NaN is truncated)
static inline uint32_t bf16_round(uint32_t u) {
  if ((u & 0x7FFFFFFFu) <= 0x7F800000u) u += 0x7FFFu + ((u >> 16) & 1u);
  return u >> 16;
}

// The fragment pack of a K x N matrix: *nsub = 0 if it gets none.  Split-K for the deep projections (K >= 4096 in slices of 1024 rows), then
// the widest column block (16 * nsub) that still gives ~200 workgroups; both depend on the matrix only, never on the batch.  (Measured: 2
// instead of 4 sub-blocks for gate|up, i.e. 32-column blocks and more workgroups, cost +0.09 ms per frame.)  Only packs the GEMV can run:
// split-K only where the step launches the matrix in that form (`split_ok`: the down projections), and a K slice too long for the launcher
// takes more slices there, or leaves the matrix without a pack elsewhere (its stack then runs on the fp32 path, stack_can_step).
static void frag_choice(int K, int N, bool split_ok, int* ks_out, int* nsub_out) {
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
static size_t frag_elems(int K, int N, int nsub) { return (size_t)((N + 16 * nsub - 1) / (16 * nsub)) * K * 16 * nsub; }
// w [K][ldw] fp32 -> out [N / (16 nsub)][K / 32][nsub][64 lanes][8] bf16 (RNE): lane L of chunk c, sub-block s holds k = 32 c + 8 (L / 16) + j,
// n = 16 s + L % 16 of its column block; the columns that pad N to whole blocks are zero
static void frag_pack(const float* w, int K, int N, long long ldw, int nsub, uint16_t* out) {
  const int CBm = 16 * nsub, nblk = (N + CBm - 1) / CBm, nchunk = K / 32;
  for (int i = 0; i < K; ++i) {
    const int c = i >> 5, kq = (i & 31) >> 3, j = i & 7;
    for (int o = 0; o < nblk * CBm; ++o) {
      uint32_t u = 0;
      if (o < N) memcpy(&u, &w[(size_t)i * ldw + o], 4);
      const int nbk = o / CBm, sb = (o % CBm) >> 4, L = kq * 16 + (o & 15);
      out[((((size_t)nbk * nchunk + c) * nsub + sb) * 64 + L) * 8 + j] = (uint16_t)bf16_round(u);
    }
  }
}

// ---- quantised fragment packs (kk_csm_gemvm.h: KK_WF_Q8 / KK_WF_Q4)
static size_t qfrag_q_bytes(int K, int N, int nsub, int bits) { return frag_elems(K, N, nsub) * (size_t)bits / 8; }
static size_t qfrag_pair_bytes(int K, int N, int nsub, int group) { return frag_elems(K, N, nsub) / (size_t)group * 8; }
// One nn.Linear part (words [O][K bits / 32], scales / biases [O][K / group]: output column n0 + o) into the packs of a K x N matrix; `q` and
// `pairs` must be zero-filled before the first part (the columns that pad N to whole blocks stay q = 0, scale = bias = 0: they decode to +0).
//   q:     [N / (16 nsub)][K / 32][nsub][64 lanes] x 8 values of `bits` bits, value j in bits [j bits, (j + 1) bits) of the lane's 8 / 4 bytes
//          (lane L: k = 32 c + 8 (L / 16) + j, n = 16 s + L % 16, as in frag_pack)
//   pairs: [N / (16 nsub)][K / group][nsub][16 columns] float2 (scale, bias)
static void qfrag_pack_part(const uint32_t* words, const float* scales, const float* biases, int O, int n0, int K, int nsub, int group, int bits, uint8_t* q,
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
// host tensors are erased as soon as they are packed: peak host memory stays near one copy of the 1.6 B parameters
struct Packer {
  kk_csm* m;
  WeightArena& a;  // m->arena
  ArenaVec vec(const std::string& name, size_t n) {
    const ArenaVec r = a.vec(name, n);
    a.host.erase(name);
    return r;
  }
  // nn.Linear weights [O_i][I] stacked along the output axis -> one [I][ldw] pack; `raw`: the source is [I][O] (audio_head);
  // `split_ok`: the single-token step launches this matrix in the split-K form too (the down projections)
  // `keep_f32` = false (packed storage: the audio heads): the fp32 matrix is staged in a scratch vector and only its bf16 pack is kept
  Lin linear(const std::vector<std::string>& names, const std::vector<int>& outs, int I, const float* raw = nullptr, bool split_ok = false,
             bool keep_f32 = true) {
    Lin l;
    int O = 0;
    for (int o : outs) O += o;
    l.Cin = I; l.Cout = O; l.ldw = rup(O, 64);
    std::vector<float> scratch;
    if (keep_f32) l.off = a.alloc((size_t)I * l.ldw);
    else scratch.assign((size_t)I * l.ldw, 0.f);
    l.has_f32 = keep_f32;
    if (keep_f32) m->linear_bytes += (size_t)I * l.ldw * 4;
    int base = 0;
    for (size_t k = 0; k < outs.size(); ++k) {
      const float* src = raw;
      if (!raw) {
        const HostTensor* w = a.get(names[k], (size_t)outs[k] * I);
        if (!w) return l;
        src = w->d.data();
      }
      float* dst = keep_f32 ? &a.pack[l.off] : scratch.data();
      if (raw) {  // [I][O]
        for (int i = 0; i < I; ++i)
          for (int o = 0; o < outs[k]; ++o) dst[(size_t)i * l.ldw + base + o] = src[(size_t)i * outs[k] + o];
      } else {
        for (int o = 0; o < outs[k]; ++o)
          for (int i = 0; i < I; ++i) dst[(size_t)i * l.ldw + base + o] = src[(size_t)o * I + i];
        a.host.erase(names[k]);
      }
      base += outs[k];
    }
    if (m->wdt == KK_BF16) {
      // bf16 weight mode: the matrix IS its bf16 rounding everywhere (the fp32 pack the multi-token prompt block reads holds the rounded
      // values too, so a prompt block and single-token steps multiply by identical weights); lossless for a bf16 checkpoint.
      float* dst = keep_f32 ? &a.pack[l.off] : scratch.data();
      for (size_t e = 0; e < (size_t)I * l.ldw; ++e) {
        uint32_t u;
        memcpy(&u, &dst[e], 4);
        u = bf16_round(u) << 16;
        memcpy(&dst[e], &u, 4);
      }
      int ks = 1, nsub = 0;
      frag_choice(I, O, split_ok, &ks, &nsub);
      if (nsub) {
        l.ks = ks; l.nsub = nsub;
        l.moff = m->packb.size();
        m->packb.resize(l.moff + frag_elems(I, O, nsub));
        frag_pack(dst, I, O, l.ldw, nsub, &m->packb[l.moff]);
        m->linear_bytes += frag_elems(I, O, nsub) * 2;
      }
    }
    return l;
  }
  // the same stacked matrix from QUANTISED parts (kk_csm_load_quantized; csm_can_pack has checked them): integer fragment pack + pairs, nothing else
  Lin qlinear(const std::vector<std::string>& names, const std::vector<int>& outs, int I, bool split_ok = false) {
    Lin l;
    int O = 0;
    for (int o : outs) O += o;
    l.Cin = I; l.Cout = O; l.ldw = rup(O, 64);
    l.has_f32 = false;
    const QuantHost& first = m->qhost.at(names[0]);
    l.fmt = first.bits == 8 ? KK_WF_Q8 : KK_WF_Q4;
    l.group = first.group;
    frag_choice(I, O, split_ok, &l.ks, &l.nsub);
    const size_t qb = qfrag_q_bytes(I, O, l.nsub, first.bits), pb = qfrag_pair_bytes(I, O, l.nsub, l.group);
    l.qoff = (m->packq.size() + 255) & ~(size_t)255;
    l.poff = (l.qoff + qb + 255) & ~(size_t)255;
    m->packq.resize(l.poff + pb, 0);
    int base = 0;
    for (size_t k = 0; k < outs.size(); ++k) {
      const QuantHost& t = m->qhost.at(names[k]);
      qfrag_pack_part(t.words.data(), t.scales.data(), t.biases.data(), outs[k], base, I, l.nsub, l.group, t.bits, &m->packq[l.qoff],
                      (float*)&m->packq[l.poff]);
      m->qhost.erase(names[k]);
      base += outs[k];
    }
    m->linear_bytes += qb + pb;
    (l.fmt == KK_WF_Q8 ? m->n_q8 : m->n_q4) += 1;
    return l;
  }
  Lin any_linear(const std::vector<std::string>& names, const std::vector<int>& outs, int I, bool split_ok = false) {
    return m->packed ? qlinear(names, outs, I, split_ok) : linear(names, outs, I, nullptr, split_ok);
  }
};

// The Linears of the frame step, as pack_stack / kk_csm_finalize stack them: (names, output widths, K, split-K allowed)
struct LinSpec {
  std::vector<std::string> names;
  std::vector<int> outs;
  int I;
  bool split_ok;
};
static void stack_specs(const std::string& name, const kk_llama_args& a, std::vector<LinSpec>& v) {
  const int H = a.num_heads, KV = a.num_kv_heads, hd = a.head_dim, D = a.hidden, I = a.intermediate;
  for (int i = 0; i < a.num_layers; ++i) {
    const std::string p = name + ".layers." + std::to_string(i);
    v.push_back({{p + ".self_attn.q_proj.weight", p + ".self_attn.k_proj.weight", p + ".self_attn.v_proj.weight"}, {H * hd, KV * hd, KV * hd}, D, false});
    v.push_back({{p + ".self_attn.o_proj.weight"}, {D}, H * hd, false});
    v.push_back({{p + ".mlp.gate_proj.weight", p + ".mlp.up_proj.weight"}, {I, I}, D, false});
    v.push_back({{p + ".mlp.down_proj.weight"}, {D}, I, true});
  }
}
// Packed storage is all or nothing (a packed matrix has no fp32 copy for the fallback kernels): every Linear the fast frame path multiplies by
// must arrive quantised in a form the kernels decode and get a fragment pack, and so must the bf16 audio heads.  Empty result = yes; else why not.
static std::string csm_can_pack(const kk_csm* m) {
  const kk_csm_config& c = m->cfg;
  std::vector<LinSpec> v;
  stack_specs("backbone", c.backbone, v);
  stack_specs("decoder", c.decoder, v);
  v.push_back({{"projection.weight"}, {c.decoder.hidden}, c.backbone.hidden, false});
  v.push_back({{"codebook0_head.weight"}, {c.audio_vocab_size}, c.backbone.hidden, false});
  for (const LinSpec& s : v) {
    int O = 0, bits = 0, group = 0;
    for (size_t k = 0; k < s.names.size(); ++k) {
      auto it = m->qhost.find(s.names[k]);
      if (it == m->qhost.end()) return s.names[k] + " is not quantised";
      const QuantHost& t = it->second;
      if (t.O != s.outs[k] || t.I != s.I) return "unexpected shape for " + s.names[k];
      if (k == 0) { bits = t.bits; group = t.group; }
      if (t.bits != bits || t.group != group) return s.names[k] + ": the parts of a stacked matrix differ in bits / group size";
      O += s.outs[k];
    }
    if (bits != 4 && bits != 8) return s.names[0] + ": " + std::to_string(bits) + " bits (the kernels decode 4 and 8)";
    if (!wf_group_ok(s.I, group)) return s.names[0] + ": group size " + std::to_string(group) + " (a multiple of 32 that divides K)";
    int ks = 1, nsub = 0;
    frag_choice(s.I, O, s.split_ok, &ks, &nsub);
    if (!nsub) return s.names[0] + ": no fragment pack for K = " + std::to_string(s.I);
  }
  if (c.audio_num_codebooks > 1) {
    int ks = 1, nsub = 0;
    frag_choice(c.decoder.hidden, c.audio_vocab_size, false, &ks, &nsub);
    if (!nsub) return "audio_head: no fragment pack";
  }
  return "";
}

void llama3_theta(const kk_llama_args& a, std::vector<float>& th) {  // attention.py:33-82, float32 like the reference
  const int half = a.head_dim / 2;
  th.resize(half);
  const double low_w = 8192.0 / 1.0, high_w = 8192.0 / 4.0;
  for (int i = 0; i < half; ++i) {
    const float f = 1.0f / powf(a.rope_theta, (float)(2 * i) / (float)a.head_dim);
    const double wl = 2.0 * M_PI / (double)f;
    double v;
    if (wl < high_w) v = f;
    else if (wl > low_w) v = (double)f / a.rope_factor;
    else {
      const double smooth = (8192.0 / wl - 1.0) / (4.0 - 1.0);
      v = (1.0 - smooth) * (double)f / a.rope_factor + smooth * (double)f;
    }
    th[i] = (float)v;
  }
}

void pack_stack(Packer& P, const std::string& name, Stack& st, int max_pos) {
  const kk_llama_args& a = st.a;
  const int H = a.num_heads, KV = a.num_kv_heads, hd = a.head_dim, D = a.hidden, I = a.intermediate;
  st.layers.resize(a.num_layers);
  for (int i = 0; i < a.num_layers; ++i) {
    const std::string p = name + ".layers." + std::to_string(i);
    LlamaLayer& L = st.layers[i];
    L.n1 = P.vec(p + ".input_layernorm.weight", D);
    L.n2 = P.vec(p + ".post_attention_layernorm.weight", D);
    L.qkv = P.any_linear({p + ".self_attn.q_proj.weight", p + ".self_attn.k_proj.weight", p + ".self_attn.v_proj.weight"}, {H * hd, KV * hd, KV * hd}, D);
    L.o = P.any_linear({p + ".self_attn.o_proj.weight"}, {D}, H * hd);
    L.gu = P.any_linear({p + ".mlp.gate_proj.weight", p + ".mlp.up_proj.weight"}, {I, I}, D);
    L.down = P.any_linear({p + ".mlp.down_proj.weight"}, {D}, I, true);
  }
  st.norm = P.vec(name + ".norm.weight", D);
  std::vector<float> th;
  llama3_theta(a, th);
  st.max_pos = max_pos;
  st.rope.n = (size_t)max_pos * (hd / 2) * 2;
  st.rope.off = P.a.alloc(st.rope.n);
  float* r = &P.a.pack[st.rope.off];
  for (int pos = 0; pos < max_pos; ++pos)
    for (int i = 0; i < hd / 2; ++i) {
      const float ang = (float)pos * th[i];  // einsum in float32 (attention.py:56-58)
      r[((size_t)pos * (hd / 2) + i) * 2] = cosf(ang);
      r[((size_t)pos * (hd / 2) + i) * 2 + 1] = sinf(ang);
    }
}

void resolve(kk_csm* m, Lin& l) {
  l.w = l.has_f32 ? m->arena.dev + l.off : nullptr;
  if (l.fmt != KK_WF_BF16) {
    l.wm = m->devq ? (const uint16_t*)(m->devq + l.qoff) : nullptr;
    l.wp = m->devq ? (const float2*)(m->devq + l.poff) : nullptr;
    return;
  }
  l.wm = (m->devb && l.nsub) ? m->devb + l.moff : nullptr;
}
void resolve(kk_csm* m, ArenaVec& v) { m->arena.resolve(v); }
void resolve(kk_csm* m, Stack& st) {
  for (auto& L : st.layers) { resolve(m, L.qkv); resolve(m, L.o); resolve(m, L.gu); resolve(m, L.down); resolve(m, L.n1); resolve(m, L.n2); }
  resolve(m, st.norm); resolve(m, st.rope);
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

struct Run : Workspace {
  kk_csm* m;
  hipStream_t st;
  int B;
  float* skinny_scratch = nullptr;  // partial sums of the skinny GEMM
  size_t skinny_floats = 0;
  // Which kernel a Linear takes is a function of the block's rows per item (below).  A prompt that is SPLIT into a prefix block and a suffix block
  // (kk_csm_prefix_create / kk_csm_admit_prefixed) must carry the bits of the unsplit block, whose rows all took the prompt kernels:
  //   LIN_PROMPT: a block of <= 2 rows goes where a long block goes (gemmp_kernel on a fragment pack, else the generic fp32 kernel);
  //   LIN_GENERIC: the generic fp32 kernel -- where the last row of a long block goes for the first head (a strided one-row block).
  // Both kernels compute an output row from its input row alone, in an order that does not depend on the row count.
  enum { LIN_AUTO = 0, LIN_PROMPT, LIN_GENERIC };
  int lin_mode = LIN_AUTO;
  Run(kk_csm* m_, hipStream_t st_, int B_, void* ws, size_t ws_bytes) : m(m_), st(st_), B(B_) {
    base = (char*)ws; cap = ws_bytes; dry = ws == nullptr;
  }
  float* f32(size_t n) { return (float*)raw(n * 4); }
  // out[b][row][:] = W x[b][row][:] (+ res); x rows: `rows` per item at pitch `xbs` elements between items
  // `nw` / `xn`: RMSNorm of the result rows, launched right behind.
  int lin(const Lin& w, const float* x, long long xbs, int rows, float* out, long long obs, const float* res, const float* nw = nullptr,
          float* xn = nullptr, float eps = 0.f) {
    if (dry) return 0;
    KKConvArgs a;
    memset(&a, 0, sizeof a);
    a.x = x; a.xbs = xbs; a.ldx = w.Cin; a.w = w.w; a.ldw = w.ldw;
    a.out = out; a.obs = obs; a.ldo = w.Cout;
    if (res) { a.res = res; a.rbs = obs; a.ldr = w.Cout; }
    a.Cin = w.Cin; a.Cout = w.Cout; a.Kw = 1; a.mode = KK_CONV; a.stride = 1; a.dil = 1;
    a.Q = rows; a.Lo_rows = rows; a.lin = KKLen{nullptr, 0, rows}; a.lout = KKLen{nullptr, 0, rows};
    a.in_slope = 1.f; a.scale = 1.f;
    int nb = B;
    if (xbs == (long long)rows * w.Cin && obs == (long long)rows * w.Cout && rows <= 2 && skinny_scratch && w.w && lin_mode == LIN_AUTO) {
      // single-token steps (and the decoder's 2-token first step): the HBM-bound skinny GEMM (every CU streams a slice of W once for up
      // to 16 rows).  The choice depends on the rows PER ITEM only, never on B, so a stream's bits do not depend on its batch.
      const int Mtot = B * rows;
      int KS, kchunk;
      skinny_plan(w.Cin, w.Cout, &KS, &kchunk);
      if ((size_t)KS * SK_MAXM * w.Cout <= skinny_floats) {
        KK_TRY(launch_skinny(x, Mtot, w.Cin, w.Cout, w.w, w.ldw, KS, kchunk, res, out, skinny_scratch, st));
        if (xn) {  // (one workgroup per row summing the slices AND normalising was tried: 17-38 us against 5 + 5 for the two launches)
          hipLaunchKernelGGL(rmsnorm_kernel, dim3(Mtot), dim3(256), 0, st, out, nw, w.Cout, eps, xn);
          KK_CHECK_LAUNCH();
        }
        return 0;
      }
    }
    if (xbs == (long long)rows * w.Cin && obs == (long long)rows * w.Cout && w.wm && w.nsub && (rows > 2 || !w.w || lin_mode == LIN_PROMPT) &&
        lin_mode != LIN_GENERIC) {
      // the prompt block in bf16 weight mode: matrix cores (gemmp_kernel); without a fragment pack, the generic fp32 kernel below.
      // The choice depends on the rows PER ITEM only, never on B: a stream's bits do not depend on its batch.  (A packed quantised matrix has
      // no fp32 copy for the skinny GEMM: its one- and two-row blocks come here too.)
      GPArgs g;
      memset(&g, 0, sizeof g);
      g.x = x; g.xrs = w.Cin; g.K = w.Cin; g.N = w.Cout; g.M = B * rows;
      gemmp_weights(g, w);
      g.res = res; g.rrs = w.Cout; g.out = out; g.ors = w.Cout;
      { const int rc_ = launch_gemmp(g, st); if (rc_ != 0) return rc_; }
      if (xn) {
        hipLaunchKernelGGL(rmsnorm_kernel, dim3(B * rows), dim3(256), 0, st, out, nw, w.Cout, eps, xn);
        KK_CHECK_LAUNCH();
      }
      return 0;
    }
    if (!w.w) return kk_fail("kk_csm: internal: a packed matrix has no fp32 copy for the generic kernel");
    if (xbs == (long long)rows * w.Cin && obs == (long long)rows * w.Cout) {
      // items are contiguous: one launch over B*rows rows, so a weight tile is read once for the whole batch (single-token steps would
      // otherwise re-read every matrix once per item)
      a.Q = a.Lo_rows = B * rows;
      a.lin = a.lout = KKLen{nullptr, 0, B * rows};
      a.xbs = a.obs = a.rbs = 0;
      nb = 1;
    }
    const int rc = kk_launch_conv_generic(a, nb, KK_F32, KK_F32, st);
    if (rc != 0 || !xn) return rc;
    if (obs != (long long)rows * w.Cout) return kk_fail("kk_csm: internal: norm of a strided result");
    hipLaunchKernelGGL(rmsnorm_kernel, dim3(B * rows), dim3(256), 0, st, out, nw, w.Cout, eps, xn);
    KK_CHECK_LAUNCH();
    return 0;
  }
};

// the matrix-core GEMV: one launch for all rows (grid z = 8-row chunks); KS must be the pack's w.ks
int launch_gemvm(const Lin& w, int pro, int epi, FGArgs a, int Mtot, hipStream_t st) {
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
int launch_gemv(const Lin& w, int pro, int epi, FGArgs a, int Mtot, hipStream_t st) {
  if (!w.wm || !w.nsub) return kk_fail("kk_csm: internal: GEMV without a fragment pack");
  if ((epi == 2) != (w.ks > 1)) return kk_fail("kk_csm: internal: split-K form");
  return launch_gemvm(w, pro, epi, a, Mtot, st);
}

// h[m][:] += x[m] W for M rows of N = w.Cout contiguous floats: EPI 1 in place, or for a split-K pack (w.ks > 1) the slices of an EPI 2 launch
// into `part` ([ks][M][N]) and one combine (h += sum of the slices, slice order)
int gemv_accumulate(const Lin& w, int pro, FGArgs g, int M, float* h, float* part, hipStream_t st) {
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

// h [B][S][D] (updated in place) -> out [B][S][D] = final norm; appends S positions to the stack's cache at st.offset
int stack_forward(Run& r, Stack& st, float* h, int S, int offset, float* out) {
  const kk_llama_args& a = st.a;
  const int B = r.B, H = a.num_heads, KV = a.num_kv_heads, hd = a.head_dim, D = a.hidden, I = a.intermediate;
  const int W = (H + 2 * KV) * hd;
  float* x = r.f32((size_t)B * S * D);
  float* qkv = r.f32((size_t)B * S * W);
  float* att = r.f32((size_t)B * S * H * hd);
  float* gu = r.f32((size_t)B * S * 2 * I);
  float* act = r.f32((size_t)B * S * I);
  if (r.oom) return kk_fail("kk_csm: workspace too small");
  if (!r.dry && offset + S > st.max_pos) return kk_fail("kk_csm: sequence exceeds the cache (max_seq_len)");
  // x = RMSNorm(h) of the CURRENT layer's input: stand-alone for layer 0, afterwards produced by the previous down projection's tail
  if (!r.dry) {
    hipLaunchKernelGGL(rmsnorm_kernel, dim3(B * S), dim3(256), 0, r.st, h, st.layers[0].n1.p, D, a.rms_eps, x);
    KK_CHECK_LAUNCH();
  }
  for (int l = 0; l < a.num_layers; ++l) {
    const LlamaLayer& L = st.layers[l];
    const size_t lp = st.layer_pitch ? st.layer_pitch : (size_t)r.m->max_batch * st.max_pos * KV * hd;
    float* kc = st.kc + (size_t)l * lp;
    float* vc = st.vc + (size_t)l * lp;
    KK_TRY(r.lin(L.qkv, x, (long long)S * D, S, qkv, (long long)S * W, nullptr));
    if (!r.dry) {
      if (S == 1 && r.lin_mode == Run::LIN_AUTO)  // single-token step: RoPE + cache append inside the attention kernel
        KK_TRY(attn_single(ATTN_CACHE, qkv, B, H, KV, hd, st.pos_dev, st.pos_dev ? 0 : offset, kc, vc, st.max_pos, st.rope.p, st.pad_dev, att, nullptr, nullptr, r.st));
      else
        KK_TRY(attn_prompt(qkv, B, S, H, KV, hd, st.pos_dev, st.pos_dev ? 0 : offset, kc, vc, st.max_pos, st.rope.p, st.pad_dev, att, r.st));
    }
    // h += o(att); x = RMSNorm(h) (post_attention_layernorm)
    KK_TRY(r.lin(L.o, att, (long long)S * H * hd, S, h, (long long)S * D, h, L.n2.p, x, a.rms_eps));
    KK_TRY(r.lin(L.gu, x, (long long)S * D, S, gu, (long long)S * 2 * I, nullptr));
    // h += down(silu(gate) * up); then the NEXT consumer's norm: the next layer's input_layernorm -> x, or the stack's final norm -> out
    const bool lastl = l + 1 == a.num_layers;
    const float* nw = lastl ? st.norm.p : st.layers[l + 1].n1.p;
    float* xn = lastl ? out : x;
    if (!r.dry) {
      const long long n = (long long)B * S * I;
      hipLaunchKernelGGL(swiglu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, r.st, gu, I, n, act);
      KK_CHECK_LAUNCH();
    }
    KK_TRY(r.lin(L.down, act, (long long)S * I, S, h, (long long)S * D, h, nw, xn, a.rms_eps));
  }
  return 0;
}

// The single-token step of a Llama stack in bf16 weight mode: FIVE launches per layer, no split-K partials, no stand-alone reduce / norm /
// SwiGLU kernels -- qkv = W(rms(h) n1); attention (RoPE + cache append inside for one-row items); h += Wo att; gu = W(rms(h) n2);
// h += Wdown(silu(gate) up).  h [B][rows][D] is updated in place; the consumer applies the final norm (a head's prologue).
bool stack_can_step(const Stack& st) {
  for (const auto& L : st.layers)
    for (const Lin* w : {&L.qkv, &L.o, &L.gu, &L.down})
      if (!w->wm) return false;
  return !st.layers.empty();
}
// `gather` (optional): layer 0 reads its input rows from a table by code instead of from h, and writes them to h (FGArgs codes / cstride / cb / V / emb)
int stack_step(Run& r, Stack& st, float* h, int rows, int offset, const FGArgs* gather = nullptr) {
  const kk_llama_args& a = st.a;
  const int B = r.B, H = a.num_heads, KV = a.num_kv_heads, hd = a.head_dim, D = a.hidden, I = a.intermediate;
  const int W = (H + 2 * KV) * hd, M = B * rows;
  float* qkv = r.f32((size_t)M * W);
  float* att = r.f32((size_t)M * H * hd);
  float* gu = r.f32((size_t)M * 2 * I);
  float* part = r.f32((size_t)16 * M * D);  // partial tiles of a split-K down projection (<= 16 slices)
  float* attp = r.f32((size_t)8 * M * H * (hd + 2));  // key-split partials of the long-cache attention (<= 8 splits)
  if (r.oom) return kk_fail("kk_csm: workspace too small");
  if (r.dry) return 0;
  if (offset + rows > st.max_pos) return kk_fail("kk_csm: sequence exceeds the cache (max_seq_len)");
  for (int l = 0; l < a.num_layers; ++l) {
    const LlamaLayer& L = st.layers[l];
    float* kc = st.kc + (size_t)l * r.m->max_batch * st.max_pos * KV * hd;
    float* vc = st.vc + (size_t)l * r.m->max_batch * st.max_pos * KV * hd;
    FGArgs g;
    memset(&g, 0, sizeof g);
    g.x = h; g.xrs = D; g.nw = L.n1.p; g.eps = a.rms_eps; g.out = qkv; g.ors = W;
    if (l == 0 && gather) { g.codes = gather->codes; g.cstride = gather->cstride; g.cb = gather->cb; g.V = gather->V; g.emb = gather->emb; g.gather_out = h; }
    KK_TRY(launch_gemv(L.qkv, 1, 0, g, M, r.st));
    if (rows == 1) {
      const int form = attn_auto_form(H / KV, st.max_pos);  // (the short-cache kernel is the instrumented one)
      KK_TRY(attn_single(form, qkv, B, H, KV, hd, st.pos_dev, st.pos_dev ? 0 : offset, kc, vc, st.max_pos, st.rope.p, st.pad_dev, att, attp,
                         form == ATTN_STEP ? ts_slot() : nullptr, r.st));
    } else KK_TRY(attn_prompt(qkv, B, rows, H, KV, hd, st.pos_dev, st.pos_dev ? 0 : offset, kc, vc, st.max_pos, st.rope.p, st.pad_dev, att, r.st));
    memset(&g, 0, sizeof g);
    g.x = att; g.xrs = (long long)H * hd; g.res = h; g.rrs = D; g.out = h; g.ors = D;
    KK_TRY(launch_gemv(L.o, 0, 1, g, M, r.st));
    memset(&g, 0, sizeof g);
    g.x = h; g.xrs = D; g.nw = L.n2.p; g.eps = a.rms_eps; g.out = gu; g.ors = 2 * I;
    KK_TRY(launch_gemv(L.gu, 1, 0, g, M, r.st));
    memset(&g, 0, sizeof g);
    g.x = gu; g.xrs = 2 * I;
    KK_TRY(gemv_accumulate(L.down, 2, g, M, h, part, r.st));
  }
  return 0;
}

// `seed`: the device seed of the Philox uniforms, or null (injected uniforms / argmax)
// `own_pos` >= 0 (kk_csm_admit): the frame is the prompt block of ONE stream in a row view of the backbone cache -- its Philox position is that
// constant (the stream's own position, not slot - padding) and the shared slot counter is NOT advanced
// `split` (kk_csm_admit_prefixed): the block is the tail of a longer prompt -- its backbone rows and the first head take the kernels the rows of the
// unsplit block take, whatever S (Run::lin_mode); the depth decoder sees the same shapes either way
int run_frame(Run& r, int S, const int* tokens, const float* mask, const SampleCfg& sc, const float* uniforms, const unsigned long long* seed,
              const int* stream_ids, int* codes, int own_pos = -1, bool split = false, const RowSampler* table = nullptr) {
  kk_csm* m = r.m;
  // the uniform of (item, code book i): uniforms[b][i], or Philox at the position of the frame being generated (slot *pos_dev + S, minus the padding)
  auto src_of = [&](int i) {
    SampleSrc s;
    s.u = uniforms ? uniforms + i : nullptr; s.ustride = m->cfg.audio_num_codebooks;
    s.seed = uniforms ? nullptr : seed; s.sid = stream_ids; s.pos = m->bb.pos_dev; s.pos_stride = 0; s.pos_add = S; s.pad = m->bb.pad_dev; s.cb = i;
    if (own_pos >= 0) { s.pos = nullptr; s.pad = nullptr; s.pos_add = own_pos; }
    if (table && s.seed) { s.seed = &table->seed; s.seed_stride = (int)(sizeof(RowSampler) / 8); }  // table mode: `seed` only says that the launch draws
    return s;
  };
  // the sampling launch of code book i: the settings as launch arguments, or (table mode) row b's from table[b] -- one launch either way
  auto sample = [&](const float* lg, int i, int* out) {
    return table ? launch_sample_rows(lg, m->cfg.audio_vocab_size, table, src_of(i), out, m->cfg.audio_num_codebooks, r.B, r.st)
                 : launch_sample(lg, m->cfg.audio_vocab_size, sc, src_of(i), out, m->cfg.audio_num_codebooks, r.B, r.st);
  };
  const kk_csm_config& c = m->cfg;
  const int B = r.B, ncb = c.audio_num_codebooks, V = c.audio_vocab_size, D = c.backbone.hidden, Dd = c.decoder.hidden;
  const size_t mark = r.used;
  float* h = r.f32((size_t)B * S * D);
  float* hn = r.f32((size_t)B * S * D);
  float* logits = r.f32((size_t)B * V);
  float* curr = r.f32((size_t)B * 2 * D);
  float* pin = r.f32((size_t)B * 2 * Dd);
  float* dn = r.f32((size_t)B * 2 * Dd);
  {  // skinny-GEMM partials: at most 1024 workgroups of 256 columns -> KS * N <= 1024 * 256 (+ slack for the rounding of the K slices)
    r.skinny_floats = (size_t)2 * 1024 * 256 * SK_MAXM;
    r.skinny_scratch = r.f32(r.skinny_floats);
  }
  if (r.oom) return kk_fail("kk_csm_generate_frame: workspace too small");
  if (!r.dry) {
    if (ncb > 71) return kk_fail("kk_csm: more than 71 code books");
    hipLaunchKernelGGL(embed_sum_kernel, dim3(B * S, (D + 255) / 256), dim3(256), 0, r.st, tokens, mask, m->audio_emb.p, m->text_emb.p, ncb, V, c.text_vocab_size, D, h);
    KK_CHECK_LAUNCH();
  }
  const size_t inner = r.used;
  // bf16 weight mode: single-token frames (and every depth-decoder step) run on the fused five-launch layers
  const bool fast = m->wdt == KK_BF16 && stack_can_step(m->bb) && stack_can_step(m->dec) && m->proj.wm && m->c0_head.wm;
  bool heads_fast = fast;
  for (const auto& l : m->audio_head) heads_fast = heads_fast && l.wm;
  const float* last_h;   // the backbone's final-normed last position of every item
  long long last_rs;     // its item pitch
  if (fast && heads_fast && S == 1 && !split) {
    KK_TRY(stack_step(r, m->bb, h, 1, m->bb.offset));
    if (!r.dry) {
      hipLaunchKernelGGL(rmsnorm_kernel, dim3(B), dim3(256), 0, r.st, h, m->bb.norm.p, D, c.backbone.rms_eps, hn);
      KK_CHECK_LAUNCH();
    }
    last_h = hn; last_rs = D;
  } else {
    if (split) r.lin_mode = Run::LIN_PROMPT;
    const int rc_ = stack_forward(r, m->bb, h, S, m->bb.offset, hn);
    r.lin_mode = Run::LIN_AUTO;
    if (rc_ != 0) return rc_;
    last_h = hn ? hn + (size_t)(S - 1) * D : nullptr;  // row S-1 of every item (pitch S*D)
    last_rs = (long long)S * D;
  }
  size_t peak = r.used;
  r.used = inner;  // the stack's scratch is free again
  // the heads write their logits straight into the slot kk_csm_debug_logits reads ([n_cb][maxB][V], first B rows): no copy per code book
  const bool dbg = !r.dry && m->dbg_logits && own_pos < 0;  // (an admission leaves the live rows' debug logits alone)
  if (dbg) logits = m->dbg_logits;
  if (fast && heads_fast) {
    if (!r.dry) {
      FGArgs g;
      memset(&g, 0, sizeof g);
      g.x = last_h; g.xrs = last_rs; g.out = logits; g.ors = V;
      KK_TRY(launch_gemv(m->c0_head, 0, 0, g, B, r.st));
      KK_TRY(sample(logits, 0, codes));
    }
    int rows = 2, dpos = 0;
    for (int i = 1; i < ncb; ++i) {
      r.used = inner;
      // curr = [last_h, embed(0, c0)] for the first step, [embed(i-1, c_{i-1})] afterwards (sesame.py:373-392): gathered by the projection's prologue
      // later steps (one row per item): the projection of an embedding row is a row of the table built at finalize -- no launch; the decoder's first
      // kernel gathers it and materialises the residual stream
      const bool tabled = rows == 1 && m->proj_table && m->dec.layers[0].qkv.wm;
      FGArgs gat;
      memset(&gat, 0, sizeof gat);
      gat.codes = codes + (i - 1); gat.cstride = ncb; gat.cb = i - 1; gat.V = V; gat.emb = m->proj_table;
      if (!r.dry && !tabled) {
        FGArgs g;
        memset(&g, 0, sizeof g);
        g.x = last_h; g.xrs = last_rs; g.codes = codes + (i - 1); g.cstride = ncb; g.cb = i - 1; g.V = V; g.rows = rows; g.emb = m->audio_emb.p;
        g.out = pin; g.ors = Dd;
        KK_TRY(launch_gemv(m->proj, 3, 0, g, B * rows, r.st));
      }
      KK_TRY(stack_step(r, m->dec, pin, rows, dpos, tabled ? &gat : nullptr));
      if (r.used > peak) peak = r.used;
      dpos += rows;
      if (!r.dry) {
        if (dbg) logits = m->dbg_logits + (size_t)i * m->max_batch * V;
        FGArgs g;
        memset(&g, 0, sizeof g);
        g.x = pin + (size_t)(rows - 1) * Dd; g.xrs = (long long)rows * Dd; g.nw = m->dec.norm.p; g.eps = c.decoder.rms_eps; g.out = logits; g.ors = V;
        KK_TRY(launch_gemv(m->audio_head[i - 1], 1, 0, g, B, r.st));
        KK_TRY(sample(logits, i, codes + i));
      }
      rows = 1;
    }
  } else {
  if (split) r.lin_mode = Run::LIN_GENERIC;
  {
    const int rc_ = r.lin(m->c0_head, last_h, last_rs, 1, logits, V, nullptr);
    r.lin_mode = Run::LIN_AUTO;
    if (rc_ != 0) return rc_;
  }
  if (!r.dry) {
    KK_TRY(sample(logits, 0, codes));
    // curr = [last_h, embed_audio(0, c0)]
    hipLaunchKernelGGL(copy_rows_kernel, dim3(B), dim3(256), 0, r.st, last_h, last_rs, curr, (long long)2 * D, D);
    KK_CHECK_LAUNCH();
    hipLaunchKernelGGL(embed_audio_kernel, dim3(B), dim3(256), 0, r.st, codes, ncb, m->audio_emb.p, 0, V, D, curr, 2, 1);
    KK_CHECK_LAUNCH();
  }
  int rows = 2, dpos = 0;
  for (int i = 1; i < ncb; ++i) {
    r.used = inner;
    KK_TRY(r.lin(m->proj, curr, (long long)rows * D, rows, pin, (long long)rows * Dd, nullptr));
    KK_TRY(stack_forward(r, m->dec, pin, rows, dpos, dn));
    if (r.used > peak) peak = r.used;
    dpos += rows;
    const float* dl = dn ? dn + (size_t)(rows - 1) * Dd : nullptr;
    if (dbg) logits = m->dbg_logits + (size_t)i * m->max_batch * V;
    KK_TRY(r.lin(m->audio_head[i - 1], dl, (long long)rows * Dd, 1, logits, V, nullptr));
    if (!r.dry) {
      KK_TRY(sample(logits, i, codes + i));
      hipLaunchKernelGGL(embed_audio_kernel, dim3(B), dim3(256), 0, r.st, codes + i, ncb, m->audio_emb.p, i, V, D, curr, 1, 0);
      KK_CHECK_LAUNCH();
    }
    rows = 1;
  }
  }
  if (!r.dry && own_pos < 0) {
    hipLaunchKernelGGL(advance_pos_kernel, dim3(1), dim3(1), 0, r.st, m->bb.pos_dev, S);
    KK_CHECK_LAUNCH();
  }
  r.used = peak;
  (void)mark;
  return 0;
}

int check_llama(const kk_llama_args& a) {
  if (a.num_layers < 1 || a.num_heads < 1 || a.num_kv_heads < 1 || a.num_heads % a.num_kv_heads != 0) return kk_fail("kk_csm_create: bad head counts");
  if (a.hidden < 1 || a.intermediate < 1) return kk_fail("kk_csm_create: bad sizes");
  if (a.head_dim != 64 && a.head_dim != 128) return kk_fail("kk_csm_create: head_dim must be 64 or 128 (llama-1B / llama-100M, sesame.py:225-273)");
  return 0;
}

}  // namespace

// make_sampler(temp, top_k) on its own (tests): logits [B][V] fp32 -> codes [B] int32, uniforms [B] (NULL or temp == 0: argmax)
extern "C" int kk_op_csm_sample(void* stream, int B, int V, const float* logits, float temperature, int top_k, const float* uniforms, int32_t* codes_out) {
  if (!logits || !codes_out || B < 1 || V < 1) return kk_fail("kk_op_csm_sample: bad argument");
  SampleCfg c;
  c.temp = temperature; c.top_k = top_k;
  SampleSrc s;
  s.u = uniforms; s.ustride = 1;
  return launch_sample(logits, V, c, s, codes_out, 1, B, (hipStream_t)stream);
}

namespace {
int sampler_cfg(const kk_csm_sampler* sp, SampleCfg* c, const char* who) {
  if (!sp) return kk_failf("%s: null sampler", who);
  if (!(sp->temperature >= 0.f) || !(sp->top_p >= 0.f && sp->top_p <= 1.f) || !(sp->min_p >= 0.f && sp->min_p <= 1.f) || sp->min_tokens_to_keep < 1 || sp->top_k < -1)
    return kk_failf("%s: sampler out of range (temperature >= 0, top_p and min_p in [0, 1], min_tokens_to_keep >= 1, top_k >= -1)", who);
  c->temp = sp->temperature; c->top_k = sp->top_k; c->top_p = sp->top_p; c->min_p = sp->min_p; c->min_keep = sp->min_tokens_to_keep;
  return 0;
}
}  // namespace

// the whole sampler on its own (tests): uniforms [B] have priority; without them and with use_device_rng, Philox on (seed, stream id, pos[b], code
// book 0) -- `seed` is passed by value here and staged in a device word for the launch; pos [B] device int32 or NULL (0)
extern "C" int kk_op_csm_sample_ex(void* stream, int B, int V, const float* logits, const kk_csm_sampler* sampler, const float* uniforms,
                                   const int32_t* stream_ids, const int32_t* pos, int32_t* codes_out) {
  if (!logits || !codes_out || B < 1 || V < 1) return kk_fail("kk_op_csm_sample_ex: bad argument");
  SampleCfg c;
  KK_TRY(sampler_cfg(sampler, &c, "kk_op_csm_sample_ex"));
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
    KK_TRY(sampler_cfg(samplers + b, &c, "kk_op_csm_sample_rows"));
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
    s.seed = &table->seed; s.seed_stride = (int)(sizeof(RowSampler) / 8); s.sid = stream_ids; s.pos = pos; s.pos_stride = 1;
  }
  const int rc = launch_sample_rows(logits, V, table, s, codes_out, 1, B, (hipStream_t)stream);
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

// ---- the kernels of the frame step on their own (tests): each entry point runs the launcher the frame runs, on caller-owned buffers
extern "C" int kk_csm_frag_choice(int K, int N, int split_ok, int32_t* ks, int32_t* nsub) {
  if (!ks || !nsub) return kk_fail("kk_csm_frag_choice: null argument");
  int k = 1, s = 0;
  frag_choice(K, N, split_ok != 0, &k, &s);
  *ks = k; *nsub = s;
  return 0;
}

extern "C" int kk_csm_frag_pack(const float* w, int K, int N, int nsub, uint16_t* out) {
  if (!w || !out || K < 32 || K % 32 != 0 || N < 1 || (nsub != 1 && nsub != 2 && nsub != 4)) return kk_fail("kk_csm_frag_pack: bad argument");
  frag_pack(w, K, N, N, nsub, out);
  return 0;
}

extern "C" int kk_csm_qfrag_bytes(int K, int N, int nsub, int group_size, int bits, size_t* q_bytes, size_t* pair_bytes) {
  if (K < 32 || K % 32 != 0 || N < 1 || (nsub != 1 && nsub != 2 && nsub != 4) || (bits != 4 && bits != 8) || !wf_group_ok(K, group_size))
    return kk_fail("kk_csm_qfrag_bytes: bad argument");
  if (q_bytes) *q_bytes = qfrag_q_bytes(K, N, nsub, bits);
  if (pair_bytes) *pair_bytes = qfrag_pair_bytes(K, N, nsub, group_size);
  return 0;
}

extern "C" int kk_csm_qfrag_pack(const uint32_t* words, const float* scales, const float* biases, int K, int N, int nsub, int group_size, int bits,
                                 void* q_out, float* pairs_out) {
  if (!words || !scales || !biases || !q_out || !pairs_out || K < 32 || K % 32 != 0 || N < 1 || (nsub != 1 && nsub != 2 && nsub != 4) ||
      (bits != 4 && bits != 8) || !wf_group_ok(K, group_size))
    return kk_fail("kk_csm_qfrag_pack: bad argument");
  memset(q_out, 0, qfrag_q_bytes(K, N, nsub, bits));
  memset(pairs_out, 0, qfrag_pair_bytes(K, N, nsub, group_size));
  qfrag_pack_part(words, scales, biases, N, 0, K, nsub, group_size, bits, (uint8_t*)q_out, pairs_out);
  return 0;
}

static int op_csm_gemv(const char* who, Lin& w, void* stream, int pro, int epi, int ks, int nsub, int K, int N, int M, const float* x, long long xrs,
                       const float* nw, float eps, const int32_t* codes, int cstride, int cb, int V, int rows, const float* emb, float* gather_out,
                       const float* res, long long rrs, float* out, long long ors, float* part);

extern "C" int kk_op_csm_gemv(void* stream, int pro, int epi, int ks, int nsub, int K, int N, int M, const void* w_frag, const float* x, long long xrs,
                              const float* nw, float eps, const int32_t* codes, int cstride, int cb, int V, int rows, const float* emb, float* gather_out,
                              const float* res, long long rrs, float* out, long long ors, float* part) {
  Lin w;
  w.wm = (const uint16_t*)w_frag;
  return op_csm_gemv("kk_op_csm_gemv", w, stream, pro, epi, ks, nsub, K, N, M, x, xrs, nw, eps, codes, cstride, cb, V, rows, emb, gather_out, res, rrs, out, ors,
                     part);
}

extern "C" int kk_op_csm_gemv_q(void* stream, int pro, int epi, int ks, int nsub, int K, int N, int M, const void* q_frag, const void* pairs, int group_size,
                                int bits, const float* x, long long xrs, const float* nw, float eps, const int32_t* codes, int cstride, int cb, int V, int rows,
                                const float* emb, float* gather_out, const float* res, long long rrs, float* out, long long ors, float* part) {
  if (!pairs || (bits != 4 && bits != 8) || K < 32 || !wf_group_ok(K, group_size)) return kk_fail("kk_op_csm_gemv_q: pairs / bits / group size");
  Lin w;
  w.wm = (const uint16_t*)q_frag; w.wp = (const float2*)pairs; w.fmt = bits == 8 ? KK_WF_Q8 : KK_WF_Q4; w.group = group_size;
  return op_csm_gemv("kk_op_csm_gemv_q", w, stream, pro, epi, ks, nsub, K, N, M, x, xrs, nw, eps, codes, cstride, cb, V, rows, emb, gather_out, res, rrs, out,
                     ors, part);
}

static int op_csm_gemv(const char* who, Lin& w, void* stream, int pro, int epi, int ks, int nsub, int K, int N, int M, const float* x, long long xrs,
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

extern "C" int kk_csm_create(const kk_csm_config* cfg, kk_csm** out) {
  if (!cfg || !out) return kk_fail("kk_csm_create: null argument");
  if (cfg->audio_num_codebooks < 1 || cfg->audio_vocab_size < 1 || cfg->audio_vocab_size > 8192 || cfg->text_vocab_size < 1 || cfg->max_seq_len < 2)
    return kk_fail("kk_csm_create: bad configuration");
  KK_TRY(check_llama(cfg->backbone));
  KK_TRY(check_llama(cfg->decoder));
  kk_csm* m = new kk_csm();
  m->cfg = *cfg;
  m->bb.a = cfg->backbone;
  m->dec.a = cfg->decoder;
  *out = m;
  return 0;
}

// A second generator on the SAME device weights: the packed matrices of a finalized generator are immutable, everything a frame mutates (KV
// caches, positions, padding, logits, captured graphs) is per generator.  Concurrent jobs (own stream / thread each) share one copy of the
// 1.6 B parameters this way.  `m` must outlive the generators made from it.  Call kk_csm_setup_caches on the new one.
extern "C" int kk_csm_share(const kk_csm* m, kk_csm** out) {
  if (!m || !out || !m->finalized) return kk_fail("kk_csm_share: needs a finalized generator");
  kk_csm* c = new (std::nothrow) kk_csm(*m);  // descriptors + resolved device pointers of the weights
  if (!c) return kk_fail("kk_csm_share: out of memory");
  c->weights_of = m->weights_of ? m->weights_of : m;
  for (Stack* s : {&c->bb, &c->dec}) {
    s->kc = s->vc = nullptr;
    s->offset = 0;
    s->pos_dev = s->pad_dev = nullptr;
  }
  c->max_batch = 0;
  c->dbg_logits = nullptr;
  c->seed_dev = nullptr;
  c->admit_sid_dev = nullptr;
  c->row_samplers = nullptr;
  c->row_samplers_zero_pending = false;
  c->seed_valid = false;
  c->reset_pending = c->pad_pending = false;
  c->pad_host.clear();
  c->xfer_ready = c->xfer_done = nullptr;
  *out = c;
  return 0;
}

extern "C" void kk_csm_destroy(kk_csm* m) {
  if (!m) return;
  if (m->arena.dev && !m->weights_of) (void)hipFree(m->arena.dev);
  if (m->devb && !m->weights_of) (void)hipFree(m->devb);
  if (m->devq && !m->weights_of) (void)hipFree(m->devq);
  if (m->proj_table && !m->weights_of) (void)hipFree(m->proj_table);
  for (Stack* s : {&m->bb, &m->dec}) {
    if (s->kc) (void)hipFree(s->kc);
    if (s->vc) (void)hipFree(s->vc);
  }
  if (m->dbg_logits) (void)hipFree(m->dbg_logits);
  if (m->bb.pos_dev) (void)hipFree(m->bb.pos_dev);
  if (m->bb.pad_dev) (void)hipFree(m->bb.pad_dev);
  if (m->seed_dev) (void)hipFree(m->seed_dev);
  if (m->admit_sid_dev) (void)hipFree(m->admit_sid_dev);
  if (m->row_samplers) (void)hipFree(m->row_samplers);
  if (m->xfer_ready) (void)hipEventDestroy(m->xfer_ready);
  if (m->xfer_done) (void)hipEventDestroy(m->xfer_done);
  m->graphs.clear();
  delete m;
}

// Weight storage of the linears in the single-token steps.  KK_DTYPE_BF16: every Linear matrix is rounded to bf16 once (lossless for a
// bf16 checkpoint -- the reference keeps the checkpoint's dtype, tts/utils.py:217-262) and the skinny GEMM streams 2-byte weights (half
// the bytes per frame; the 212 MB depth decoder then fits the 256 MB Infinity Cache across its 31 steps); activations, accumulation,
// KV cache and logits stay fp32.  Call before kk_csm_finalize.
extern "C" int kk_csm_set_weight_dtype(kk_csm* m, int dtype) {
  if (!m) return kk_fail("kk_csm_set_weight_dtype: null model");
  if (m->finalized) return kk_fail("kk_csm_set_weight_dtype: call before kk_csm_finalize");
  if (dtype != KK_DTYPE_F32 && dtype != KK_DTYPE_BF16) return kk_fail("kk_csm_set_weight_dtype: F32 or BF16");
  m->wdt = dtype == KK_DTYPE_BF16 ? KK_BF16 : KK_F32;
  return 0;
}

extern "C" int kk_csm_load_tensor(kk_csm* m, const char* name, const int64_t* shape, int ndim, const float* data) {
  KK_TRY(kk_host_load_tensor("kk_csm_load_tensor", m ? &m->arena.host : nullptr, m && m->finalized, name, shape, ndim, data));
  m->qhost.erase(name);
  return 0;
}

extern "C" int kk_csm_finalize(kk_csm* m, void* stream) {
  if (!m) return kk_fail("kk_csm_finalize: null model");
  if (m->finalized) return kk_fail("kk_csm_finalize: already finalized");
  const kk_csm_config& c = m->cfg;
  Packer P{m, m->arena};
  const int D = c.backbone.hidden, Dd = c.decoder.hidden, V = c.audio_vocab_size, ncb = c.audio_num_codebooks;
  if (!m->qhost.empty()) {
    // A quantised checkpoint.  Packed storage if the whole fast path can run from quantised packs (csm_can_pack), else today's arithmetic on the
    // dequantised weights: bf16 weight mode either way.  Whatever is not a packed Linear (the embedding tables; everything on the fallback) is
    // dequantised here, by the checkpoint's own rule, and then treated as a float tensor of that name.
    m->q_reason = csm_can_pack(m);
    m->packed = m->q_reason.empty();
    m->q_fallback = !m->packed;
    m->wdt = KK_BF16;
    std::set<std::string> keep;
    if (m->packed) {
      std::vector<LinSpec> v;
      stack_specs("backbone", c.backbone, v);
      stack_specs("decoder", c.decoder, v);
      for (const LinSpec& sp : v) keep.insert(sp.names.begin(), sp.names.end());
      keep.insert("projection.weight");
      keep.insert("codebook0_head.weight");
    }
    for (auto it = m->qhost.begin(); it != m->qhost.end();) {
      if (keep.count(it->first)) { ++it; continue; }
      HostTensor& t = m->arena.host[it->first];
      dequantize_host(it->second, t.d);
      t.shape = {it->second.O, it->second.I};
      it = m->qhost.erase(it);
    }
  }
  pack_stack(P, "backbone", m->bb, c.max_seq_len);
  pack_stack(P, "decoder", m->dec, ncb + 1);
  m->text_emb = P.vec("text_embeddings.weight", (size_t)c.text_vocab_size * D);
  m->audio_emb = P.vec("audio_embeddings.weight", (size_t)V * ncb * D);
  m->proj = P.any_linear({"projection.weight"}, {Dd}, D);
  m->c0_head = P.any_linear({"codebook0_head.weight"}, {V}, D);
  m->audio_head.resize(ncb > 1 ? ncb - 1 : 0);
  if (ncb > 1) {
    const HostTensor* ah = P.a.get("audio_head", (size_t)(ncb - 1) * Dd * V);
    if (ah)
      for (int i = 0; i < ncb - 1; ++i) m->audio_head[i] = P.linear({}, {V}, Dd, ah->d.data() + (size_t)i * Dd * V, false, !m->packed);  // [Dd][V] used as x @ W
  }
  if (!P.a.err.empty()) return kk_failf("kk_csm_finalize: %s", P.a.err.c_str());
  m->qhost.clear();
  m->total_bytes = m->arena.pack.size() * 4 + m->packb.size() * 2 + m->packq.size();
  KK_TRY(m->arena.upload((hipStream_t)stream, "kk_csm_finalize"));
  if (!m->packb.empty()) KK_TRY(kk_upload(m->packb, &m->devb, (hipStream_t)stream, "kk_csm_finalize"));
  if (!m->packq.empty()) KK_TRY(kk_upload(m->packq, &m->devq, (hipStream_t)stream, "kk_csm_finalize"));
  resolve(m, m->bb); resolve(m, m->audio_emb); resolve(m, m->proj);
  if (m->proj.wm && ncb > 1) {
    // projection(audio_embeddings): every input the depth decoder's later steps can see (sesame.py:373-392: curr_h = projection(embed(c_{i-1})))
    const size_t rows = (size_t)V * ncb;
    if (hipMalloc((void**)&m->proj_table, rows * Dd * sizeof(float)) != hipSuccess) return kk_fail("kk_csm_finalize: hipMalloc failed");
    GPArgs g;
    memset(&g, 0, sizeof g);
    g.x = m->audio_emb.p; g.xrs = D; g.K = D; g.N = Dd; g.M = (int)rows; g.out = m->proj_table; g.ors = Dd;
    gemmp_weights(g, m->proj);
    m->table_bytes = rows * Dd * sizeof(float);
    m->total_bytes += m->table_bytes;
    if (launch_gemmp(g, (hipStream_t)stream) != 0 || hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return kk_fail("kk_csm_finalize: projection table failed");
  }
  resolve(m, m->bb); resolve(m, m->dec); resolve(m, m->text_emb); resolve(m, m->audio_emb); resolve(m, m->proj); resolve(m, m->c0_head);
  for (auto& l : m->audio_head) resolve(m, l);
  if (m->packed) {  // the decision above promised the fast path: never a frame that could reach a matrix without its fp32 copy
    bool ok = stack_can_step(m->bb) && stack_can_step(m->dec) && m->proj.wm && m->c0_head.wm;
    for (const auto& l : m->audio_head) ok = ok && l.wm;
    if (!ok) return kk_fail("kk_csm_finalize: internal: packed storage without a complete fast path");
  }
  static std::atomic<unsigned long long> next_weights_id{1};
  m->weights_id = next_weights_id++;
  m->finalized = true;
  return 0;
}

extern "C" int kk_csm_load_quantized(kk_csm* m, const char* name, const int64_t* shape, const uint32_t* words, const float* scales, const float* biases,
                                     int group_size, int bits) {
  KK_TRY(kk_host_load_quantized("kk_csm_load_quantized", m ? &m->qhost : nullptr, m && m->finalized, name, shape, words, scales, biases, group_size, bits));
  m->arena.host.erase(name);
  return 0;
}

extern "C" int kk_csm_weight_format(const kk_csm* m) {
  if (!m || !m->finalized) { kk_fail("kk_csm_weight_format: needs a finalized generator"); return -1; }
  if (m->packed) return (m->n_q8 ? KK_CSM_WEIGHTS_Q8 : KK_CSM_WEIGHTS_Q4) | (m->n_q8 && m->n_q4 ? KK_CSM_WEIGHTS_MIXED : 0);
  return (m->wdt == KK_BF16 ? KK_CSM_WEIGHTS_BF16 : KK_CSM_WEIGHTS_F32) | (m->q_fallback ? KK_CSM_WEIGHTS_DEQUANTIZED : 0);
}

extern "C" const char* kk_csm_weight_fallback_reason(const kk_csm* m) { return m ? m->q_reason.c_str() : ""; }

extern "C" int kk_csm_weight_bytes(const kk_csm* m, size_t* linear_bytes, size_t* total_bytes) {
  if (!m || !m->finalized) return kk_fail("kk_csm_weight_bytes: needs a finalized generator");
  if (linear_bytes) *linear_bytes = m->linear_bytes;
  if (total_bytes) *total_bytes = m->total_bytes;
  return 0;
}

// SesameModel.setup_caches / reset_caches (sesame.py:320-345): device KV caches for `max_batch` items; positions restart at 0
extern "C" int kk_csm_setup_caches(kk_csm* m, int max_batch) {
  if (!m || !m->finalized || max_batch < 1) return kk_fail("kk_csm_setup_caches: bad argument");
  // captured frame steps have the OLD cache / logits pointers baked in: drop every graph before the buffers they point at are freed
  // (a replay after a second setup_caches would read and write freed memory)
  m->graphs.clear();
  (void)hipDeviceSynchronize();  // nothing in flight may still use the caches about to be freed
  for (Stack* s : {&m->bb, &m->dec}) {
    if (s->kc) (void)hipFree(s->kc);
    if (s->vc) (void)hipFree(s->vc);
    s->kc = s->vc = nullptr;
    const size_t n = (size_t)s->a.num_layers * max_batch * s->max_pos * s->a.num_kv_heads * s->a.head_dim * 4;
    if (hipMalloc((void**)&s->kc, n) != hipSuccess || hipMalloc((void**)&s->vc, n) != hipSuccess) return kk_fail("kk_csm_setup_caches: hipMalloc failed");
    s->offset = 0;
  }
  if (m->dbg_logits) (void)hipFree(m->dbg_logits);
  m->dbg_logits = nullptr;
  if (hipMalloc((void**)&m->dbg_logits, (size_t)m->cfg.audio_num_codebooks * max_batch * m->cfg.audio_vocab_size * 4) != hipSuccess)
    return kk_fail("kk_csm_setup_caches: hipMalloc failed");
  if (!m->bb.pos_dev && hipMalloc((void**)&m->bb.pos_dev, 4) != hipSuccess) return kk_fail("kk_csm_setup_caches: hipMalloc failed");
  if (hipMemset(m->bb.pos_dev, 0, 4) != hipSuccess) return kk_fail("kk_csm_setup_caches: memset failed");
  if (!m->seed_dev && hipMalloc((void**)&m->seed_dev, 8) != hipSuccess) return kk_fail("kk_csm_setup_caches: hipMalloc failed");
  if (!m->admit_sid_dev && hipMalloc((void**)&m->admit_sid_dev, 4) != hipSuccess) return kk_fail("kk_csm_setup_caches: hipMalloc failed");
  if (m->bb.pad_dev) (void)hipFree(m->bb.pad_dev);
  m->bb.pad_dev = nullptr;
  if (hipMalloc((void**)&m->bb.pad_dev, (size_t)max_batch * 4) != hipSuccess || hipMemset(m->bb.pad_dev, 0, (size_t)max_batch * 4) != hipSuccess)
    return kk_fail("kk_csm_setup_caches: hipMalloc failed");
  if (m->row_samplers) (void)hipFree(m->row_samplers);
  m->row_samplers = nullptr;
  if (hipMalloc(&m->row_samplers, (size_t)max_batch * sizeof(RowSampler)) != hipSuccess ||
      hipMemset(m->row_samplers, 0, (size_t)max_batch * sizeof(RowSampler)) != hipSuccess)
    return kk_fail("kk_csm_setup_caches: hipMalloc failed");
  m->max_batch = max_batch;
  m->pad_host.assign((size_t)max_batch, 0);
  m->reset_pending = m->pad_pending = m->row_samplers_zero_pending = false;  // freshly zeroed above
  return 0;
}
// Ragged prompts: the streams of a batch are LEFT-padded to the longest prompt (padding frames carry an all-zero mask); pad[b] = number of
// padding frames of item b.  Item b's token in cache slot p then has position p - pad[b] (RoPE) and sees the slots >= pad[b] only, so its
// results are bit-identical to running it alone.  Call on an empty cache (after setup / reset), before the prompt block; reset clears it.
extern "C" int kk_csm_set_padding(kk_csm* m, int B, const int32_t* pad_host) {
  if (!m || !m->bb.pad_dev || B < 1 || B > m->max_batch || !pad_host) return kk_fail("kk_csm_set_padding: bad argument (call kk_csm_setup_caches first)");
  if (m->bb.offset != 0) return kk_fail("kk_csm_set_padding: the cache is not empty");
  for (int b = 0; b < B; ++b)
    if (pad_host[b] < 0 || pad_host[b] >= m->bb.max_pos) return kk_fail("kk_csm_set_padding: padding out of range");
  m->pad_host.assign((size_t)m->max_batch, 0);
  for (int b = 0; b < B; ++b) m->pad_host[b] = pad_host[b];
  m->pad_pending = true;  // uploaded on the next frame's stream
  return 0;
}
extern "C" int kk_csm_reset_caches(kk_csm* m) {
  if (!m) return kk_fail("kk_csm_reset_caches: null model");
  m->bb.offset = 0;
  m->dec.offset = 0;
  m->reset_pending = true;  // position counter and padding are cleared on the next frame's stream
  m->pad_pending = false;
  m->pad_host.assign((size_t)m->max_batch, 0);
  return 0;
}
extern "C" int kk_csm_position(const kk_csm* m) { return m ? m->bb.offset : -1; }

extern "C" size_t kk_csm_workspace_bytes(kk_csm* m, int B, int S) {
  if (!m || !m->finalized || B <= 0 || S <= 0) return 0;
  Run r(m, nullptr, B, nullptr, 0);
  if (run_frame(r, S, nullptr, nullptr, SampleCfg(), nullptr, nullptr, nullptr, nullptr) != 0) return 0;
  return r.used + 256;
}

// what kk_csm_reset_caches / kk_csm_set_padding / kk_csm_park_row deferred, in stream order before the next frame, admission or shift (never
// inside a capture)
static int flush_pending(kk_csm* m, hipStream_t st) {
  if (m->reset_pending) {  // deferred kk_csm_reset_caches
    if (hipMemsetAsync(m->bb.pos_dev, 0, 4, st) != hipSuccess || hipMemsetAsync(m->bb.pad_dev, 0, (size_t)m->max_batch * 4, st) != hipSuccess)
      return kk_fail("kk_csm_generate_frame: cache reset failed");
    m->reset_pending = false;
  }
  if (m->pad_pending) {  // deferred kk_csm_set_padding / kk_csm_park_row
    if (hipMemcpyAsync(m->bb.pad_dev, m->pad_host.data(), (size_t)m->max_batch * 4, hipMemcpyHostToDevice, st) != hipSuccess)
      return kk_fail("kk_csm_generate_frame: padding upload failed");
    m->pad_pending = false;
  }
  if (m->row_samplers_zero_pending) {  // deferred kk_csm_reset_caches_parked: every row's sampler entry back to zero (arg-max)
    if (hipMemsetAsync(m->row_samplers, 0, (size_t)m->max_batch * sizeof(RowSampler), st) != hipSuccess)
      return kk_fail("kk_csm_generate_frame: sampler table reset failed");
    m->row_samplers_zero_pending = false;
  }
  return 0;
}
// the Philox seed lives in device memory: a new one does not re-capture the graph
static int upload_seed(kk_csm* m, unsigned long long seed, hipStream_t st) {
  if (m->seed_valid && m->seed_host == seed) return 0;
  m->seed_host = seed;
  if (hipMemcpyAsync(m->seed_dev, &m->seed_host, 8, hipMemcpyHostToDevice, st) != hipSuccess) return kk_fail("kk_csm_generate_frame: seed upload failed");
  m->seed_valid = true;
  return 0;
}

extern "C" int kk_csm_generate_frame(kk_csm* m, void* stream, int B, int S, const int32_t* tokens, const float* tokens_mask, float temperature,
                                     int top_k, const float* uniforms, void* workspace, size_t workspace_bytes, int32_t* codes_out) {
  kk_csm_sampler sp;
  memset(&sp, 0, sizeof sp);
  sp.temperature = temperature; sp.top_k = top_k; sp.min_tokens_to_keep = 1;
  return kk_csm_generate_frame_ex(m, stream, B, S, tokens, tokens_mask, &sp, uniforms, nullptr, workspace, workspace_bytes, codes_out);
}

extern "C" int kk_csm_generate_frame_ex(kk_csm* m, void* stream, int B, int S, const int32_t* tokens, const float* tokens_mask, const kk_csm_sampler* sampler,
                                        const float* uniforms, const int32_t* stream_ids, void* workspace, size_t workspace_bytes, int32_t* codes_out) {
  if (!m || !m->finalized) return kk_fail("kk_csm_generate_frame: model not finalized");
  if (m->max_batch < 1) return kk_fail("kk_csm_generate_frame: call kk_csm_setup_caches first");
  if (B <= 0 || B > m->max_batch || S <= 0 || !tokens || !tokens_mask || !workspace || !codes_out) return kk_fail("kk_csm_generate_frame: bad argument");
  if (m->bb.offset + S > m->bb.max_pos) return kk_fail("kk_csm_generate_frame: sequence exceeds max_seq_len");
  if (S > 1 && m->bb.offset != 0) return kk_fail("kk_csm_generate_frame: a multi-token block must start an empty cache (sesame.py:41-48)");
  if (workspace_bytes < kk_csm_workspace_bytes(m, B, S)) return kk_fail("kk_csm_generate_frame: workspace too small");
  KK_TRY(flush_pending(m, (hipStream_t)stream));
  SampleCfg sc;
  KK_TRY(sampler_cfg(sampler, &sc, "kk_csm_generate_frame"));
  const bool dev_rng = !uniforms && sampler->use_device_rng && sc.temp > 0.f;
  if (dev_rng) KK_TRY(upload_seed(m, sampler->seed, (hipStream_t)stream));
  auto eager = [&](void* on_stream) -> int {
    Run r(m, (hipStream_t)on_stream, B, workspace, workspace_bytes);
    return run_frame(r, S, tokens, tokens_mask, sc, uniforms, dev_rng ? m->seed_dev : nullptr, dev_rng ? stream_ids : nullptr, codes_out);
  };
  int rc;
  if (!m->graph_mode || S != 1) {
    rc = eager(stream);
  } else {
    // the single-token step (~1400 launches) as one hipGraphLaunch: every position-dependent kernel reads the device counter
    unsigned tbits, pbits, mbits;
    memcpy(&tbits, &sc.temp, 4);
    memcpy(&pbits, &sc.top_p, 4);
    memcpy(&mbits, &sc.min_p, 4);
    const std::vector<unsigned long long> key = {(unsigned long long)B, (unsigned long long)(uintptr_t)tokens, (unsigned long long)(uintptr_t)tokens_mask,
        (unsigned long long)tbits, (unsigned long long)(long long)sc.top_k, (unsigned long long)(uintptr_t)uniforms, (unsigned long long)(uintptr_t)workspace,
        (unsigned long long)workspace_bytes, (unsigned long long)(uintptr_t)codes_out, (unsigned long long)(uintptr_t)g_ts,
        (unsigned long long)pbits, (unsigned long long)mbits, (unsigned long long)sc.min_keep, (unsigned long long)dev_rng,
        (unsigned long long)(uintptr_t)(dev_rng ? stream_ids : nullptr)};
    hipGraphExec_t ex = nullptr;
    rc = m->graphs.run(key, (hipStream_t)stream, [&](hipStream_t on_stream, bool) { return eager((void*)on_stream); }, &ex, "kk_csm");
    if (rc != 0) return rc;
    if (ex && hipGraphLaunch(ex, (hipStream_t)stream) != hipSuccess) return kk_fail("kk_csm: hipGraphLaunch failed");
  }
  if (rc == 0) m->bb.offset += S;
  return rc;
}

// ---- per-row sampler settings ---------------------------------------------------------------------------------------------------
extern "C" int kk_csm_set_row_sampler(kk_csm* m, void* stream, int row, const kk_csm_sampler* sampler) {
  if (!m || m->max_batch < 1 || !m->row_samplers) return kk_fail("kk_csm_set_row_sampler: call kk_csm_setup_caches first");
  if (row < 0 || row >= m->max_batch) return kk_fail("kk_csm_set_row_sampler: row out of range");
  SampleCfg sc;
  KK_TRY(sampler_cfg(sampler, &sc, "kk_csm_set_row_sampler"));
  hipStream_t st = (hipStream_t)stream;
  KK_TRY(flush_pending(m, st));  // a deferred zeroing of the table must not land behind this entry
  RowSampler e;
  e.temp = sc.temp; e.top_k = sc.top_k; e.top_p = sc.top_p; e.min_p = sc.min_p; e.min_keep = sc.min_keep; e.pad_ = 0; e.seed = sampler->seed;
  hipLaunchKernelGGL(set_row_sampler_kernel, dim3(1), dim3(1), 0, st, (RowSampler*)m->row_samplers, row, e);
  KK_CHECK_LAUNCH();
  return 0;
}

extern "C" int kk_csm_generate_frame_rows(kk_csm* m, void* stream, int B, int S, const int32_t* tokens, const float* tokens_mask, int use_device_rng,
                                          const float* uniforms, const int32_t* stream_ids, void* workspace, size_t workspace_bytes, int32_t* codes_out) {
  if (!m || !m->finalized) return kk_fail("kk_csm_generate_frame_rows: model not finalized");
  if (m->max_batch < 1 || !m->row_samplers) return kk_fail("kk_csm_generate_frame_rows: call kk_csm_setup_caches first");
  if (B <= 0 || B > m->max_batch || S <= 0 || !tokens || !tokens_mask || !workspace || !codes_out) return kk_fail("kk_csm_generate_frame_rows: bad argument");
  if (m->bb.offset + S > m->bb.max_pos) return kk_fail("kk_csm_generate_frame_rows: sequence exceeds max_seq_len");
  if (S > 1 && m->bb.offset != 0) return kk_fail("kk_csm_generate_frame_rows: a multi-token block must start an empty cache (sesame.py:41-48)");
  if (workspace_bytes < kk_csm_workspace_bytes(m, B, S)) return kk_fail("kk_csm_generate_frame_rows: workspace too small");
  KK_TRY(flush_pending(m, (hipStream_t)stream));
  const bool dev_rng = !uniforms && use_device_rng != 0;
  const RowSampler* table = (const RowSampler*)m->row_samplers;
  auto eager = [&](void* on_stream) -> int {
    Run r(m, (hipStream_t)on_stream, B, workspace, workspace_bytes);
    // (`seed` non-null only tells run_frame that the launches draw on the device: in table mode the word itself is the row's entry)
    return run_frame(r, S, tokens, tokens_mask, SampleCfg(), uniforms, dev_rng ? &table->seed : nullptr, dev_rng ? stream_ids : nullptr, codes_out, -1, false, table);
  };
  int rc;
  if (!m->graph_mode || S != 1) {
    rc = eager(stream);
  } else {
    // keyed by the MODE (the leading tag; the key of kk_csm_generate_frame_ex has another length), B, the pointers and the uniform source -- never by
    // what the table holds: kk_csm_set_row_sampler between two replays changes the next replay's picks without a new capture
    const std::vector<unsigned long long> key = {~0ull, (unsigned long long)B, (unsigned long long)(uintptr_t)tokens, (unsigned long long)(uintptr_t)tokens_mask,
        (unsigned long long)(uintptr_t)uniforms, (unsigned long long)(uintptr_t)workspace, (unsigned long long)workspace_bytes,
        (unsigned long long)(uintptr_t)codes_out, (unsigned long long)(uintptr_t)g_ts, (unsigned long long)dev_rng,
        (unsigned long long)(uintptr_t)(dev_rng ? stream_ids : nullptr), (unsigned long long)(uintptr_t)table};
    hipGraphExec_t ex = nullptr;
    rc = m->graphs.run(key, (hipStream_t)stream, [&](hipStream_t on_stream, bool) { return eager((void*)on_stream); }, &ex, "kk_csm");
    if (rc != 0) return rc;
    if (ex && hipGraphLaunch(ex, (hipStream_t)stream) != hipSuccess) return kk_fail("kk_csm: hipGraphLaunch failed");
  }
  if (rc == 0) m->bb.offset += S;
  return rc;
}

// ---- continuous batching: streams enter and leave a running batch -------------------------------------------------------------
// All rows share the slot counter P (bb.offset / *bb.pos_dev); row b's tokens live in slots [pad[b], P) at position slot - pad[b].  A PARKED row
// has pad[b] = max_pos: every attention form sees nk <= 0 for it (zero output, nothing appended), so it rides through the frame step's GEMVs
// with finite values and cannot reach another row.

// kk_csm_reset_caches with every row parked: P = 0, pad[b] = max_pos (the start of a serving session; the classic reset leaves all rows live)
extern "C" int kk_csm_reset_caches_parked(kk_csm* m) {
  if (!m || m->max_batch < 1) return kk_fail("kk_csm_reset_caches_parked: call kk_csm_setup_caches first");
  KK_TRY(kk_csm_reset_caches(m));
  m->pad_host.assign((size_t)m->max_batch, m->bb.max_pos);
  m->pad_pending = true;  // uploaded behind the deferred reset
  m->row_samplers_zero_pending = true;
  return 0;
}

extern "C" int kk_csm_park_row(kk_csm* m, int row) {
  if (!m || m->max_batch < 1) return kk_fail("kk_csm_park_row: call kk_csm_setup_caches first");
  if (row < 0 || row >= m->max_batch) return kk_fail("kk_csm_park_row: row out of range");
  m->pad_host[row] = m->bb.max_pos;
  m->pad_pending = true;  // uploaded on the next frame's stream
  return 0;
}

extern "C" int kk_csm_row_state(const kk_csm* m, int32_t* pad_out, int32_t* position) {
  if (!m || m->max_batch < 1) return kk_fail("kk_csm_row_state: call kk_csm_setup_caches first");
  if (pad_out) memcpy(pad_out, m->pad_host.data(), (size_t)m->max_batch * 4);
  if (position) *position = m->bb.offset;
  return 0;
}

extern "C" int kk_csm_shift_caches(kk_csm* m, void* stream, int delta, void* workspace, size_t workspace_bytes) {
  (void)workspace; (void)workspace_bytes;  // the walk is ordered per thread (shift_cache_kernel): no bounce buffer
  if (!m || m->max_batch < 1) return kk_fail("kk_csm_shift_caches: call kk_csm_setup_caches first");
  const int P = m->bb.offset, mp = m->bb.max_pos;
  if (P + delta < 0 || P + delta > mp) return kk_fail("kk_csm_shift_caches: the position would leave the cache");
  for (int b = 0; b < m->max_batch; ++b)
    if (m->pad_host[b] < mp && m->pad_host[b] + delta < 0) return kk_fail("kk_csm_shift_caches: a live row's window would leave the cache");
  if (delta == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  KK_TRY(flush_pending(m, st));
  const kk_llama_args& a = m->bb.a;
  const int rowf4 = a.num_kv_heads * a.head_dim / 4;
  hipLaunchKernelGGL(shift_cache_kernel, dim3((rowf4 + 63) / 64, m->max_batch, 2 * a.num_layers), dim3(64), 0, st, m->bb.kc, m->bb.vc, m->max_batch, mp, rowf4,
                     m->bb.pos_dev, m->bb.pad_dev, delta);
  KK_CHECK_LAUNCH();
  hipLaunchKernelGGL(advance_pos_kernel, dim3(1), dim3(1), 0, st, m->bb.pos_dev, delta);
  KK_CHECK_LAUNCH();
  for (int b = 0; b < m->max_batch; ++b)
    if (m->pad_host[b] < mp) m->pad_host[b] += delta;
  m->bb.offset = P + delta;
  if (hipMemcpyAsync(m->bb.pad_dev, m->pad_host.data(), (size_t)m->max_batch * 4, hipMemcpyHostToDevice, st) != hipSuccess)
    return kk_fail("kk_csm_shift_caches: padding upload failed");
  return 0;
}

namespace {
// The backbone as kk_csm_admit sees it: ONE row of the caches (layer pitch unchanged: max_batch rows), that row's padding entry, and the
// slot offset as a launch constant instead of the device counter.  Restored on every way out.
struct RowView {
  Stack& s;
  float *kc, *vc;
  int *pos, *pad;
  int off;
  RowView(Stack& st, int row, int slot0) : s(st), kc(st.kc), vc(st.vc), pos(st.pos_dev), pad(st.pad_dev), off(st.offset) {
    const size_t rs = (size_t)st.max_pos * st.a.num_kv_heads * st.a.head_dim;
    s.kc = kc + row * rs; s.vc = vc + row * rs; s.pos_dev = nullptr; s.pad_dev = pad + row; s.offset = slot0;
  }
  ~RowView() { s.kc = kc; s.vc = vc; s.pos_dev = pos; s.pad_dev = pad; s.offset = off; }
};
}  // namespace

extern "C" int kk_csm_admit(kk_csm* m, void* stream, int row, int S, const int32_t* tokens, const float* tokens_mask, const kk_csm_sampler* sampler,
                            const float* uniforms, int32_t stream_id, void* workspace, size_t workspace_bytes, int32_t* codes_out) {
  if (!m || !m->finalized) return kk_fail("kk_csm_admit: model not finalized");
  if (m->max_batch < 1) return kk_fail("kk_csm_admit: call kk_csm_setup_caches first");
  if (row < 0 || row >= m->max_batch) return kk_fail("kk_csm_admit: row out of range");
  if (S <= 0 || !tokens || !tokens_mask || !sampler || !workspace || !codes_out) return kk_fail("kk_csm_admit: bad argument");
  const int P = m->bb.offset, mp = m->bb.max_pos;
  if (m->pad_host[row] < mp) return kk_fail("kk_csm_admit: the row is live (kk_csm_park_row first)");
  if (S > P) return kk_fail("kk_csm_admit: the prompt is longer than the cache position (kk_csm_shift_caches by S - P first)");
  if (workspace_bytes < kk_csm_workspace_bytes(m, 1, S)) return kk_fail("kk_csm_admit: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  SampleCfg sc;
  KK_TRY(sampler_cfg(sampler, &sc, "kk_csm_admit"));
  const bool dev_rng = !uniforms && sampler->use_device_rng && sc.temp > 0.f;
  m->pad_host[row] = P - S;
  m->pad_pending = true;
  KK_TRY(flush_pending(m, st));
  if (dev_rng) {
    KK_TRY(upload_seed(m, sampler->seed, st));
    m->admit_sid_host = stream_id;
    if (hipMemcpyAsync(m->admit_sid_dev, &m->admit_sid_host, 4, hipMemcpyHostToDevice, st) != hipSuccess) return kk_fail("kk_csm_admit: stream id upload failed");
  }
  RowView view(m->bb, row, P - S);
  Run r(m, st, 1, workspace, workspace_bytes);
  return run_frame(r, S, tokens, tokens_mask, sc, uniforms, dev_rng ? m->seed_dev : nullptr, dev_rng ? m->admit_sid_dev : nullptr, codes_out, S);
}

// ---- shared voice prefixes -----------------------------------------------------------------------------------------------------
struct kk_csm_prefix {
  float* buf = nullptr;  // [layers][K|V][n][KV hd]
  int n = 0, layers = 0, kvw = 0;
  unsigned long long weights_id = 0;
};
static size_t kk_csm_prefix_bytes_of(const kk_csm_prefix* p) { return (size_t)2 * p->layers * p->n * p->kvw * 4; }

namespace {
// the live prefixes: a destroyed (or never created) handle is refused by address, without reading through it
std::mutex g_prefix_mu;
std::set<const kk_csm_prefix*> g_prefixes;
bool prefix_live(const kk_csm_prefix* p) {
  std::lock_guard<std::mutex> lk(g_prefix_mu);
  return p && g_prefixes.count(p) != 0;
}
// The backbone as kk_csm_prefix_create sees it: the prefix buffer as a one-row cache of its own (layer pitch 2 n KV hd, K in front of V), positions
// from 0 as launch constants, no padding.  No cache row, counter or padding entry of the generator is read or written.  Restored on every way out.
struct PrefixView {
  Stack& s;
  float *kc, *vc;
  int *pos, *pad;
  int off;
  size_t lp;
  PrefixView(Stack& st, float* buf, int n) : s(st), kc(st.kc), vc(st.vc), pos(st.pos_dev), pad(st.pad_dev), off(st.offset), lp(st.layer_pitch) {
    const size_t seg = (size_t)n * st.a.num_kv_heads * st.a.head_dim;
    s.kc = buf; s.vc = buf + seg; s.pos_dev = nullptr; s.pad_dev = nullptr; s.offset = 0; s.layer_pitch = 2 * seg;
  }
  ~PrefixView() { s.kc = kc; s.vc = vc; s.pos_dev = pos; s.pad_dev = pad; s.offset = off; s.layer_pitch = lp; }
};
// the workspace of a block run by the two entries below: a one-row block takes the prompt path, whose scratch the S = 2 plan covers
size_t split_workspace_bytes(kk_csm* m, int S) { return kk_csm_workspace_bytes(m, 1, S < 2 ? 2 : S); }
}  // namespace

extern "C" int kk_csm_prefix_create(kk_csm* m, void* stream, int S, const int32_t* tokens, const float* tokens_mask, void* workspace,
                                    size_t workspace_bytes, kk_csm_prefix** out) {
  if (!m || !m->finalized) return kk_fail("kk_csm_prefix_create: model not finalized");
  if (S <= 0 || !tokens || !tokens_mask || !workspace || !out) return kk_fail("kk_csm_prefix_create: bad argument");
  const kk_llama_args& a = m->bb.a;
  const int kvw = a.num_kv_heads * a.head_dim;
  if (kvw % 4 != 0) return kk_fail("kk_csm_prefix_create: kv_heads * head_dim must be a multiple of 4");
  if (S >= m->bb.max_pos) return kk_fail("kk_csm_prefix_create: the prefix must leave room for a suffix below max_seq_len");
  if (m->cfg.audio_num_codebooks > 71) return kk_fail("kk_csm: more than 71 code books");
  if (workspace_bytes < split_workspace_bytes(m, S)) return kk_fail("kk_csm_prefix_create: workspace too small");
  kk_csm_prefix* p = new (std::nothrow) kk_csm_prefix();
  if (!p) return kk_fail("kk_csm_prefix_create: out of memory");
  p->n = S; p->layers = a.num_layers; p->kvw = kvw; p->weights_id = m->weights_id;
  if (hipMalloc((void**)&p->buf, kk_csm_prefix_bytes_of(p)) != hipSuccess) {
    delete p;
    return kk_fail("kk_csm_prefix_create: hipMalloc failed");
  }
  int rc;
  {
    hipStream_t st = (hipStream_t)stream;
    const kk_csm_config& c = m->cfg;
    const int D = c.backbone.hidden;
    PrefixView view(m->bb, p->buf, S);
    Run r(m, st, 1, workspace, workspace_bytes);
    float* h = r.f32((size_t)S * D);
    float* hn = r.f32((size_t)S * D);
    if (r.oom) rc = kk_fail("kk_csm_prefix_create: workspace too small");
    else {
      hipLaunchKernelGGL(embed_sum_kernel, dim3(S, (D + 255) / 256), dim3(256), 0, st, tokens, tokens_mask, m->audio_emb.p, m->text_emb.p,
                         c.audio_num_codebooks, c.audio_vocab_size, c.text_vocab_size, D, h);
      rc = hipGetLastError() == hipSuccess ? 0 : kk_fail("kk_csm_prefix_create: launch failed");
      r.lin_mode = Run::LIN_PROMPT;
      if (rc == 0) rc = stack_forward(r, m->bb, h, S, 0, hn);
    }
  }
  if (rc != 0) {
    (void)hipStreamSynchronize((hipStream_t)stream);  // nothing in flight may still write the buffer
    (void)hipFree(p->buf);
    delete p;
    return rc;
  }
  {
    std::lock_guard<std::mutex> lk(g_prefix_mu);
    g_prefixes.insert(p);
  }
  *out = p;
  return 0;
}

extern "C" int kk_csm_prefix_length(const kk_csm_prefix* p) { return prefix_live(p) ? p->n : -1; }
extern "C" size_t kk_csm_prefix_bytes(const kk_csm_prefix* p) { return prefix_live(p) ? kk_csm_prefix_bytes_of(p) : 0; }

extern "C" int kk_csm_prefix_read(const kk_csm_prefix* p, void* stream, float* dst, size_t dst_bytes) {
  if (!prefix_live(p)) return kk_fail("kk_csm_prefix_read: null or destroyed prefix");
  if (!dst || dst_bytes < kk_csm_prefix_bytes_of(p)) return kk_fail("kk_csm_prefix_read: destination too small");
  if (hipMemcpyAsync(dst, p->buf, kk_csm_prefix_bytes_of(p), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
    return kk_fail("kk_csm_prefix_read: copy failed");
  return 0;
}

extern "C" void kk_csm_prefix_destroy(kk_csm_prefix* p) {
  {
    std::lock_guard<std::mutex> lk(g_prefix_mu);
    if (!p || g_prefixes.erase(p) == 0) return;
  }
  (void)hipDeviceSynchronize();  // an admission in flight may still read it
  (void)hipFree(p->buf);
  delete p;
}

extern "C" int kk_csm_admit_prefixed(kk_csm* m, void* stream, int row, const kk_csm_prefix* prefix, int S, const int32_t* tokens,
                                     const float* tokens_mask, const kk_csm_sampler* sampler, const float* uniforms, int32_t stream_id,
                                     void* workspace, size_t workspace_bytes, int32_t* codes_out) {
  if (!m || !m->finalized) return kk_fail("kk_csm_admit_prefixed: model not finalized");
  if (m->max_batch < 1) return kk_fail("kk_csm_admit_prefixed: call kk_csm_setup_caches first");
  if (row < 0 || row >= m->max_batch) return kk_fail("kk_csm_admit_prefixed: row out of range");
  if (!prefix_live(prefix)) return kk_fail("kk_csm_admit_prefixed: null or destroyed prefix");
  if (S <= 0 || !tokens || !tokens_mask || !sampler || !workspace || !codes_out) return kk_fail("kk_csm_admit_prefixed: bad argument");
  const kk_llama_args& a = m->bb.a;
  const int P = m->bb.offset, mp = m->bb.max_pos, n = prefix->n, kvw = a.num_kv_heads * a.head_dim;
  if (prefix->weights_id != m->weights_id || prefix->layers != a.num_layers || prefix->kvw != kvw)
    return kk_fail("kk_csm_admit_prefixed: the prefix was computed with another weight set");
  if (m->pad_host[row] < mp) return kk_fail("kk_csm_admit_prefixed: the row is live (kk_csm_park_row first)");
  if (n + S > P) return kk_fail("kk_csm_admit_prefixed: prefix + suffix are longer than the cache position (kk_csm_shift_caches by n + S - P first)");
  if (workspace_bytes < split_workspace_bytes(m, S)) return kk_fail("kk_csm_admit_prefixed: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  SampleCfg sc;
  KK_TRY(sampler_cfg(sampler, &sc, "kk_csm_admit_prefixed"));
  const bool dev_rng = !uniforms && sampler->use_device_rng && sc.temp > 0.f;
  m->pad_host[row] = P - n - S;
  m->pad_pending = true;
  KK_TRY(flush_pending(m, st));
  if (dev_rng) {
    KK_TRY(upload_seed(m, sampler->seed, st));
    m->admit_sid_host = stream_id;
    if (hipMemcpyAsync(m->admit_sid_dev, &m->admit_sid_host, 4, hipMemcpyHostToDevice, st) != hipSuccess)
      return kk_fail("kk_csm_admit_prefixed: stream id upload failed");
  }
  {  // the prefix under the suffix: slots [P - n - S, P - S) of the row, every layer's K and V in one launch (0 <= P - n - S and P - S < max_pos: inside the row)
    const size_t at = ((size_t)row * mp + (size_t)(P - n - S)) * kvw;
    const long long seg4 = (long long)n * kvw / 4, pitch4 = (long long)m->max_batch * mp * kvw / 4;
    hipLaunchKernelGGL(prefix_restore_kernel, dim3((unsigned)((seg4 + 1023) / 1024), 2 * a.num_layers), dim3(256), 0, st, (const float4*)prefix->buf,
                       m->bb.kc + at, m->bb.vc + at, pitch4, seg4);
    KK_CHECK_LAUNCH();
  }
  RowView view(m->bb, row, P - S);
  Run r(m, st, 1, workspace, workspace_bytes);
  return run_frame(r, S, tokens, tokens_mask, sc, uniforms, dev_rng ? m->seed_dev : nullptr, dev_rng ? m->admit_sid_dev : nullptr, codes_out, n + S, true);
}

// The first n positions of live row `row` as a new prefix: slots [pad[row], pad[row] + n) of every layer's K and V, one launch.  The row's window is
// [pad[row], P), so n <= P - pad[row] keeps the read inside it; the write goes to the new buffer alone.  P, pad, the frame-step graph and its key are
// untouched: legal between two frames of a running batch.
extern "C" int kk_csm_prefix_capture(kk_csm* m, void* stream, int row, int n, kk_csm_prefix** out) {
  if (!m || !m->finalized) return kk_fail("kk_csm_prefix_capture: model not finalized");
  if (!out) return kk_fail("kk_csm_prefix_capture: bad argument");
  if (m->max_batch < 1 || !m->bb.kc || !m->bb.vc) return kk_fail("kk_csm_prefix_capture: call kk_csm_setup_caches first");
  if (row < 0 || row >= m->max_batch) return kk_fail("kk_csm_prefix_capture: row out of range");
  const kk_llama_args& a = m->bb.a;
  const int P = m->bb.offset, mp = m->bb.max_pos, kvw = a.num_kv_heads * a.head_dim, pad = m->pad_host[row];
  if (pad >= mp) return kk_fail("kk_csm_prefix_capture: the row is parked");
  if (n < 1) return kk_fail("kk_csm_prefix_capture: n must be at least 1");
  if (pad < 0 || n > P - pad) return kk_fail("kk_csm_prefix_capture: the row holds fewer than n positions");
  if (kvw % 4 != 0) return kk_fail("kk_csm_prefix_capture: kv_heads * head_dim must be a multiple of 4");
  kk_csm_prefix* p = new (std::nothrow) kk_csm_prefix();
  if (!p) return kk_fail("kk_csm_prefix_capture: out of memory");
  p->n = n; p->layers = a.num_layers; p->kvw = kvw; p->weights_id = m->weights_id;
  if (hipMalloc((void**)&p->buf, kk_csm_prefix_bytes_of(p)) != hipSuccess) {
    delete p;
    return kk_fail("kk_csm_prefix_capture: hipMalloc failed");
  }
  hipStream_t st = (hipStream_t)stream;
  int rc = flush_pending(m, st);
  if (rc == 0) {
    const size_t at = ((size_t)row * mp + (size_t)pad) * kvw;
    const long long seg4 = (long long)n * kvw / 4, pitch4 = (long long)m->max_batch * mp * kvw / 4;
    hipLaunchKernelGGL(prefix_capture_kernel, dim3((unsigned)((seg4 + 1023) / 1024), 2 * a.num_layers), dim3(256), 0, st, m->bb.kc + at, m->bb.vc + at,
                       (float4*)p->buf, pitch4, seg4);
    rc = hipGetLastError() == hipSuccess ? 0 : kk_fail("kk_csm_prefix_capture: launch failed");
  }
  if (rc != 0) {
    (void)hipStreamSynchronize(st);  // nothing in flight may still write the buffer
    (void)hipFree(p->buf);
    delete p;
    return rc;
  }
  {
    std::lock_guard<std::mutex> lk(g_prefix_mu);
    g_prefixes.insert(p);
  }
  *out = p;
  return 0;
}

// A finished admission moves from another generator's cache row into a parked row of this one: the window [pad_s, P_s) of live row
// `src_row` of `src` -- L positions -- goes to slots [P - L, P) of `row`, pad[row] = P - L, every layer's K and V in one launch.  No prompt
// block, no depth decoder, no sampler; P, the other rows, the frame-step graph and its key are untouched: legal between two replays.  The
// ordering is made here: `stream` waits for what `src_stream` holds now (the admission), and `src_stream` waits for the copy, so the source's
// next reset or admission cannot overwrite the window early.  Everything is refused on the host before anything is enqueued.
extern "C" int kk_csm_admit_transfer(kk_csm* m, void* stream, int row, kk_csm* src, void* src_stream, int src_row) {
  if (!m || !src || !m->finalized || !src->finalized) return kk_fail("kk_csm_admit_transfer: needs two finalized generators");
  if (m == src) return kk_fail("kk_csm_admit_transfer: source and destination are the same generator");
  if (m->max_batch < 1 || !m->bb.kc || !m->bb.vc || src->max_batch < 1 || !src->bb.kc || !src->bb.vc)
    return kk_fail("kk_csm_admit_transfer: call kk_csm_setup_caches on both generators first");
  if (row < 0 || row >= m->max_batch) return kk_fail("kk_csm_admit_transfer: row out of range");
  if (src_row < 0 || src_row >= src->max_batch) return kk_fail("kk_csm_admit_transfer: source row out of range");
  const kk_llama_args &a = m->bb.a, &sa = src->bb.a;
  const int P = m->bb.offset, mp = m->bb.max_pos, smp = src->bb.max_pos, kvw = a.num_kv_heads * a.head_dim, spad = src->pad_host[src_row];
  if (m->pad_host[row] < mp) return kk_fail("kk_csm_admit_transfer: the row is live (kk_csm_park_row first)");
  if (spad >= smp) return kk_fail("kk_csm_admit_transfer: the source row is parked");
  const int L = src->bb.offset - spad;
  if (spad < 0 || L < 1) return kk_fail("kk_csm_admit_transfer: the source row holds no position");
  if (L > P) {
    char msg[160];
    snprintf(msg, sizeof msg, "kk_csm_admit_transfer: the admission is longer than the cache position (kk_csm_shift_caches by %d first)", L - P);
    return kk_fail(msg);
  }
  if (src->weights_id != m->weights_id || sa.num_layers != a.num_layers || sa.num_kv_heads * sa.head_dim != kvw)
    return kk_fail("kk_csm_admit_transfer: the two generators run on different weight sets");
  if (kvw % 4 != 0) return kk_fail("kk_csm_admit_transfer: kv_heads * head_dim must be a multiple of 4");
  if (!m->xfer_ready && hipEventCreateWithFlags(&m->xfer_ready, hipEventDisableTiming) != hipSuccess) {
    m->xfer_ready = nullptr;
    return kk_fail("kk_csm_admit_transfer: event creation failed");
  }
  if (!m->xfer_done && hipEventCreateWithFlags(&m->xfer_done, hipEventDisableTiming) != hipSuccess) {
    m->xfer_done = nullptr;
    return kk_fail("kk_csm_admit_transfer: event creation failed");
  }
  hipStream_t st = (hipStream_t)stream, sst = (hipStream_t)src_stream;
  if (hipEventRecord(m->xfer_ready, sst) != hipSuccess || hipStreamWaitEvent(st, m->xfer_ready, 0) != hipSuccess)
    return kk_fail("kk_csm_admit_transfer: could not order the copy behind the source stream");
  m->pad_host[row] = P - L;
  m->pad_pending = true;
  KK_TRY(flush_pending(m, st));
  {  // source [spad, spad + L) of src_row (spad + L = P_s <= its max_pos), destination [P - L, P) of row (0 <= P - L, P <= max_pos): both inside their rows
    const size_t sat = ((size_t)src_row * smp + (size_t)spad) * kvw, at = ((size_t)row * mp + (size_t)(P - L)) * kvw;
    const long long seg4 = (long long)L * kvw / 4, spitch4 = (long long)src->max_batch * smp * kvw / 4, pitch4 = (long long)m->max_batch * mp * kvw / 4;
    hipLaunchKernelGGL(row_transfer_kernel, dim3((unsigned)((seg4 + 1023) / 1024), 2 * a.num_layers), dim3(256), 0, st, src->bb.kc + sat, src->bb.vc + sat,
                       spitch4, m->bb.kc + at, m->bb.vc + at, pitch4, seg4);
    KK_CHECK_LAUNCH();
  }
  if (hipEventRecord(m->xfer_done, st) != hipSuccess || hipStreamWaitEvent(sst, m->xfer_done, 0) != hipSuccess)
    return kk_fail("kk_csm_admit_transfer: could not order the source stream behind the copy");
  return 0;
}

extern "C" int kk_csm_debug_timestamps(unsigned long long* buf, int capacity) {
  g_ts = buf;
  g_ts_cap = buf ? capacity : 0;
  g_ts_next = 0;
  return 0;
}

extern "C" int kk_csm_set_graph_mode(kk_csm* m, int on) {
  if (!m) return kk_fail("kk_csm_set_graph_mode: null model");
  m->graph_mode = on != 0;
  return 0;
}

// logits of the last frame (tests): [n_cb][B][V] float32, device to device
extern "C" int kk_csm_debug_logits(kk_csm* m, void* stream, int B, float* dst) {
  if (!m || !m->dbg_logits || !dst || B < 1 || B > m->max_batch) return kk_fail("kk_csm_debug_logits: bad argument");
  const int V = m->cfg.audio_vocab_size;
  for (int i = 0; i < m->cfg.audio_num_codebooks; ++i)
    if (hipMemcpyAsync(dst + (size_t)i * B * V, m->dbg_logits + (size_t)i * m->max_batch * V, (size_t)B * V * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) !=
        hipSuccess)
      return kk_fail("kk_csm_debug_logits: copy failed");
  return 0;
}
