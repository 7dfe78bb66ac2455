// KV-cache attention family, fp32: interleaved-pair RoPE + cache append, and softmax attention of new positions over a cache
// [item][max_pos][KV hd].  Users: the CSM Llama stacks (kk_csm.hip: attn_single / attn_prompt, positions and left padding in device
// memory so that a captured frame step replays) and Mimi's streaming transformer (kk_mimi.hip: the kk_launch_* block forms, launch-wide
// or with a position per row).  The block forms come in pairs -- launch-wide and per-row -- that share ONE __device__ body each
// (rope_append_body, attn_cache_body); the __global__ wrappers only resolve the position and the guards, so a row's bits cannot
// depend on which of the two ran it.
#include <math.h>

#include "../../include/kokoro_hip.h"
#include "kk_common.h"
#include "kk_host.h"
#include "kk_kernels.h"

namespace {

#include "kk_ts.h"

// RoPE on q (in place) and k, then k / v of the new rows go into the cache at [offset + s]
// `pad` (nullable, [B]): ragged prompts are LEFT-padded to a common length; item b's first pad[b] cache slots hold nothing, its token in
// slot p sits at position p - pad[b] (RoPE) and attends to slots >= pad[b] only.  Padding rows are rotated with position 0 (never read).
// The body, for (new row s = blockIdx.x, item b = blockIdx.y): the item's block sits at slot `offset`, its left padding is `pd`.  Both come
// resolved from the __global__ wrappers below (launch-wide: rope_append_kernel; a position per row: rope_append_rows_kernel).
__device__ __forceinline__ void rope_append_body(float* qkv, int S, int H, int KV, int hd, const float* rope, int offset, int pd, float* kc, float* vc,
                                                 int max_pos) {
  const int s = blockIdx.x, b = blockIdx.y;
  const int W = (H + 2 * KV) * hd, half = hd / 2;
  float* row = qkv + ((long long)b * S + s) * W;
  const int rpos = offset + s - pd > 0 ? offset + s - pd : 0;
  const float* cs = rope + (long long)rpos * half * 2;
  float* kdst = kc + ((long long)b * max_pos + offset + s) * KV * hd;
  float* vdst = vc + ((long long)b * max_pos + offset + s) * KV * hd;
  for (int e = threadIdx.x; e < (H + KV) * half; e += 256) {
    const int hh = e / half, i = e - hh * half;
    float* p = row + hh * hd + 2 * i;  // q heads first, k heads right behind them
    const float c = cs[2 * i], sn = cs[2 * i + 1];
    const float x0 = p[0], x1 = p[1];
    const float y0 = x0 * c - x1 * sn, y1 = x1 * c + x0 * sn;
    if (hh < H) {
      p[0] = y0; p[1] = y1;
    } else {
      kdst[(hh - H) * hd + 2 * i] = y0;
      kdst[(hh - H) * hd + 2 * i + 1] = y1;
    }
  }
  const float* vsrc = row + (H + KV) * hd;
  for (int e = threadIdx.x; e < KV * hd; e += 256) vdst[e] = vsrc[e];
}
__global__ __launch_bounds__(256) void rope_append_kernel(float* qkv, int S, int H, int KV, int hd, const float* rope, const int* pos_dev, int offset,
                                                          float* kc, float* vc, int max_pos, const int* pad) {
  if (pos_dev) offset += *pos_dev;  // the backbone's position lives in device memory so that a captured frame step can be replayed
  const int pd = pad ? pad[blockIdx.y] : 0;
  if (pd >= max_pos) return;  // a parked row (kk_csm_park_row): no key of its own, nothing appended -- as the single-token attention forms treat nk <= 0
  rope_append_body(qkv, S, H, KV, hd, rope, offset, pd, kc, vc, max_pos);
}

// one workgroup per (query s, head h, item b): scores over the cached keys 0 .. offset+s, softmax, weighted sum of V.
// Single-token steps are latency-bound, so the dependent chains are kept short: a thread takes a whole key row as independent 16-byte
// loads (q sits in LDS), and the P.V product splits the keys over G = 512 / hd groups of threads (each thread one float4 of the head
// dimension), whose partial sums are added in group order through LDS.
// `causal`: 1 = query s sees keys 0 .. offset+s (index_causal_mask, sesame.py:41-48); 0 = every query of the block sees all offset+S
// keys (Mimi's streaming transformer passes no mask, transformer.py:79-104).  `ctx` >= 0: only the last ctx CACHED keys (+ the block).
// FUSE (single-token steps: S = 1, causal, no context limit): the RoPE of q and of the new key and the append of the new key / value row
// happen HERE instead of in rope_append_kernel (one launch less per layer and step): q and the new k are rotated while they are staged in
// LDS -- the same expressions, so the same bits as the two-kernel path --, the new row is the last key / value of the walk, and the first
// query head of each kv group writes it to the cache for the steps to come (the other heads of the group never read that row here).
// The body is shared by the launch-wide kernel (attn_cache_kernel) and the per-row one (attn_cache_rows_kernel): the wrappers resolve the
// block's slot `offset` and the left padding `pd` (the keys start at slot pd, key j of the walk is slot klo + j) and own the LDS -- sc:
// [sc_len rounded up to 4] scores, [hd] q, [G][hd] partial outputs, (FUSE) [hd] new k, [hd] new v; red: 2 floats.  sc_len bounds the key count.
__device__ __forceinline__ int attn_first_key(int offset, int ctx, int pd) { return ctx >= 0 && offset > ctx ? offset - ctx : pd; }
__device__ __forceinline__ void attn_zero_output(float* out, int S, int H, int hd) {  // no key: the output is defined as zero
  for (int e = threadIdx.x; e < hd; e += 128) out[((long long)blockIdx.z * S + blockIdx.x) * H * hd + blockIdx.y * hd + e] = 0.f;
}
template <bool FUSE>
__device__ __forceinline__ void attn_cache_body(const float* qkv, int S, int H, int KV, int hd, int offset, int pd, float* kc, float* vc, int max_pos,
                                                float scale, float* out, int causal, int ctx, const float* rope, int sc_len, float* sc, float* red) {
  const int s = blockIdx.x, h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int klo = attn_first_key(offset, ctx, pd);
  const int W = (H + 2 * KV) * hd, kvh = h / (H / KV), nk = (causal ? offset + s + 1 : offset + S) - klo;
  if (nk <= 0) {  // a padding row (nothing reads its output)
    attn_zero_output(out, S, H, hd);
    return;
  }
  const int mp4 = (sc_len + 3) & ~3;
  float* qs = sc + mp4;        // [hd]
  float* po = qs + hd;         // [G][hd]
  float* kn = po + (512 / hd) * hd;  // [hd] (FUSE)
  float* vn = kn + hd;               // [hd] (FUSE)
  const float* q = qkv + ((long long)b * S + s) * W + h * hd;
  const float* kb = kc + ((long long)b * max_pos + klo) * KV * hd + kvh * hd;
  const float* vb = vc + ((long long)b * max_pos + klo) * KV * hd + kvh * hd;
  const int jn = FUSE ? nk - 1 : -1;  // the key that is not in the cache yet
  if (FUSE) {
    const float* cs = rope + (long long)(offset + s - pd) * (hd / 2) * 2;
    const float* kq = qkv + ((long long)b * S + s) * W + (H + kvh) * hd;
    const float* vq = qkv + ((long long)b * S + s) * W + (H + KV + kvh) * hd;
    for (int i = tid; i < hd / 2; i += 128) {
      const float c = cs[2 * i], sn = cs[2 * i + 1];
      const float x0 = q[2 * i], x1 = q[2 * i + 1];
      qs[2 * i] = x0 * c - x1 * sn;
      qs[2 * i + 1] = x1 * c + x0 * sn;
      const float k0 = kq[2 * i], k1 = kq[2 * i + 1];
      kn[2 * i] = k0 * c - k1 * sn;
      kn[2 * i + 1] = k1 * c + k0 * sn;
    }
    for (int e = tid; e < hd; e += 128) vn[e] = vq[e];
  } else {
    for (int e = tid; e < hd; e += 128) qs[e] = q[e];
  }
  __syncthreads();
  if (FUSE && h % (H / KV) == 0) {
    float* kdst = kc + ((long long)b * max_pos + offset + s) * KV * hd + kvh * hd;
    float* vdst = vc + ((long long)b * max_pos + offset + s) * KV * hd + kvh * hd;
    for (int e = tid; e < hd; e += 128) { kdst[e] = kn[e]; vdst[e] = vn[e]; }
  }
  const int hd4 = hd >> 2;
  float mx = -INFINITY;
  for (int j = tid; j < nk; j += 128) {
    const float4* kr = j == jn ? (const float4*)kn : (const float4*)(kb + (long long)j * KV * hd);
    float d = 0.f;
    for (int e0 = 0; e0 < hd4; e0 += 16) {  // hd = 64 or 128: 16 independent loads per trip
      float4 kv[16];
#pragma unroll
      for (int t = 0; t < 16; ++t) kv[t] = kr[e0 + t];
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const float4 qv = *(const float4*)(qs + 4 * (e0 + t));
        d = __builtin_fmaf(qv.x, kv[t].x, d);
        d = __builtin_fmaf(qv.y, kv[t].y, d);
        d = __builtin_fmaf(qv.z, kv[t].z, d);
        d = __builtin_fmaf(qv.w, kv[t].w, d);
      }
    }
    d *= scale;
    sc[j] = d;
    mx = fmaxf(mx, d);
  }
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(red[0], red[1]);
  __syncthreads();
  float sum = 0.f;
  for (int j = tid; j < nk; j += 128) {
    const float p = expf(sc[j] - mx);
    sc[j] = p;
    sum += p;
  }
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if ((tid & 63) == 0) red[tid >> 6] = sum;
  __syncthreads();
  const float inv = 1.0f / (red[0] + red[1]);
  const int G = 128 / hd4, e4 = tid % hd4, g = tid / hd4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int j = g; j < nk; j += G) {
    const float p = sc[j];
    const float4 v = j == jn ? *(const float4*)(vn + 4 * e4) : *(const float4*)(vb + (long long)j * KV * hd + 4 * e4);
    acc.x = __builtin_fmaf(p, v.x, acc.x);
    acc.y = __builtin_fmaf(p, v.y, acc.y);
    acc.z = __builtin_fmaf(p, v.z, acc.z);
    acc.w = __builtin_fmaf(p, v.w, acc.w);
  }
  *(float4*)(po + g * hd + 4 * e4) = acc;
  __syncthreads();
  for (int e = tid; e < hd; e += 128) {
    float a = 0.f;
    for (int gg = 0; gg < G; ++gg) a += po[gg * hd + e];  // group order
    out[((long long)b * S + s) * H * hd + h * hd + e] = a * inv;
  }
}

template <bool FUSE>
__global__ __launch_bounds__(128) void attn_cache_kernel(const float* qkv, int S, int H, int KV, int hd, const int* pos_dev, int offset, float* kc,
                                                         float* vc, int max_pos, float scale, float* out, int causal, int ctx, const float* rope,
                                                         const int* pad) {
  extern __shared__ __attribute__((aligned(16))) float sc[];  // attn_lds_bytes: the score buffer holds max_pos keys
  __shared__ float red[2];
  if (pos_dev) offset += *pos_dev;
  const int pd = pad ? pad[blockIdx.z] : 0;  // left padding of a ragged prompt
  attn_cache_body<FUSE>(qkv, S, H, KV, hd, offset, pd, kc, vc, max_pos, scale, out, causal, ctx, rope, max_pos, sc, red);
}

// ---- per-row-offset forms (the row-mode streaming codec, kk_mimi_decode_step_rows): item b's block of S rows sits at ITS OWN position
// row_pos[b] (device memory) instead of one launch-wide offset, and only rows with active[b] != 0 take part.  A row runs the bodies above
// with offset = row_pos[b], no padding and no causal mask, so its bits are those of a kk_launch_rope_append / kk_launch_attn_cache call at the
// same position.  An inactive row appends nothing (its K / V and position stay as they are) and gets a zero attention output (finite,
// never used).  The host has checked row_pos[b] + S <= max_pos for every active row; the same test here turns a violation into an inactive row.
__global__ __launch_bounds__(256) void rope_append_rows_kernel(float* qkv, int S, int H, int KV, int hd, const float* rope, const int* row_pos,
                                                               const int* active, float* kc, float* vc, int max_pos) {
  const int b = blockIdx.y, offset = row_pos[b];
  if (!active[b] || offset < 0 || offset + S > max_pos) return;
  rope_append_body(qkv, S, H, KV, hd, rope, offset, 0, kc, vc, max_pos);
}
// every query of row b's block sees the keys [max(0, row_pos[b] - ctx), row_pos[b] + S): at most sc_cap = min(max_pos, ctx + S) of them,
// which is what the score buffer holds (dynamic LDS: attn_rows_lds_bytes, without the fused form's new k / v rows)
__global__ __launch_bounds__(128) void attn_cache_rows_kernel(const float* qkv, int S, int H, int KV, int hd, const int* row_pos, const int* active,
                                                              const float* kc, const float* vc, int max_pos, float scale, float* out, int ctx,
                                                              int sc_cap) {
  extern __shared__ __attribute__((aligned(16))) float sc[];
  __shared__ float red[2];
  const int b = blockIdx.z, offset = row_pos[b];
  if (!active[b] || offset < 0 || offset + S > max_pos || offset + S - attn_first_key(offset, ctx, 0) > sc_cap) {
    attn_zero_output(out, S, H, hd);
    return;
  }
  attn_cache_body<false>(qkv, S, H, KV, hd, offset, 0, const_cast<float*>(kc), const_cast<float*>(vc), max_pos, scale, out, 0, ctx, nullptr, sc_cap, sc, red);
}

// attn_step_kernel (round 3): the single-token attention over a SHORT cache (max_pos <= 64: the depth decoder's 33 positions, small test
// stacks) as ONE memory round trip.  attn_cache_kernel walks the keys in dependent steps (a thread per key with 2 x 16 loads, then the
// values 4 keys at a time): 7.6 us per launch in the frame (frame time with it not launched), 124 launches.  Here a workgroup owns one (item, kv
// head) and its G = H / KV query heads: every cached K and V row, the new q / k / v and the RoPE row are requested at once, land in LDS
// (K rows padded to hd + 4 floats: a lane per key reads 16-byte pieces without bank conflicts), and scores, softmax (a lane per key, one
// wave per head) and the weighted sum run out of LDS.  RoPE of q / k and the cache append are fused as in attn_cache_kernel<true>.
template <int HD>
__global__ __launch_bounds__(256) void attn_step_kernel(const float* qkv, int H, int KV, const int* pos_dev, int offset, float* kc, float* vc, int max_pos,
                                                         float scale, float* out, const float* rope, const int* pad, unsigned long long* ts) {
  constexpr int HD4 = HD / 4, KP = HD + 4;
  extern __shared__ __attribute__((aligned(16))) float sma[];
  ts_begin(ts, 1);
  const int G = H / KV, kvh = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* ks = sma;                   // [max_pos][KP]
  float* vs = ks + max_pos * KP;     // [max_pos rounded up to 4][HD]
  float* qs = vs + ((max_pos + 3) & ~3) * HD;  // [G][HD]
  float* sc = qs + G * HD;           // [G][64]
  float* inv = sc + G * 64;          // [G]
  if (pos_dev) offset += *pos_dev;
  const int pd = pad ? pad[b] : 0, nk = offset + 1 - pd;
  const int W = (H + 2 * KV) * HD;
  if (nk <= 0) {  // a padding row: no key, the output is defined as zero (nothing reads it)
    for (int o = tid; o < G * HD; o += 256) out[(long long)b * H * HD + (long long)kvh * G * HD + o] = 0.f;
    return;
  }
  const float* kb = kc + ((long long)b * max_pos + pd) * KV * HD + kvh * HD;
  const float* vb = vc + ((long long)b * max_pos + pd) * KV * HD + kvh * HD;
  const int nold = (nk - 1) * HD4;  // float4 of the cached rows (<= 63 * 32)
  float4 kr[8], vr[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int idx = tid + 256 * i;
    if (idx < nold) {  // (kept under the branch: at the depth decoder's 2-32 keys most of the 8 rounds are skipped by whole waves; clamped unconditional loads measured 3 % slower per frame)
      const int j = idx / HD4, e = idx - j * HD4;
      kr[i] = *(const float4*)(kb + (long long)j * KV * HD + 4 * e);
      vr[i] = *(const float4*)(vb + (long long)j * KV * HD + 4 * e);
    }
  }
  {  // the new position: RoPE on q (G heads) and k, v as is; k / v also go to the cache
    const float* cs = rope + (long long)(offset - pd) * (HD / 2) * 2;
    const float* q = qkv + (long long)b * W + (long long)kvh * G * HD;
    const float* kq = qkv + (long long)b * W + (H + kvh) * HD;
    const float* vq = qkv + (long long)b * W + (H + KV + kvh) * HD;
    float* kdst = kc + ((long long)b * max_pos + offset) * KV * HD + kvh * HD;
    float* vdst = vc + ((long long)b * max_pos + offset) * KV * HD + kvh * HD;
    for (int i = tid; i < G * (HD / 2); i += 256) {
      const int ii = i % (HD / 2);
      const float2 c = *(const float2*)(cs + 2 * ii), x = *(const float2*)(q + 2 * i);
      *(float2*)(qs + 2 * i) = make_float2(x.x * c.x - x.y * c.y, x.y * c.x + x.x * c.y);
    }
    if (tid < HD / 2) {
      const float2 c = *(const float2*)(cs + 2 * tid), x = *(const float2*)(kq + 2 * tid);
      const float2 kn = make_float2(x.x * c.x - x.y * c.y, x.y * c.x + x.x * c.y);
      *(float2*)(ks + (nk - 1) * KP + 2 * tid) = kn;
      *(float2*)(kdst + 2 * tid) = kn;
    } else if (tid >= 128 && tid < 128 + HD / 2) {
      const int t = tid - 128;
      const float2 v = *(const float2*)(vq + 2 * t);
      *(float2*)(vs + (nk - 1) * HD + 2 * t) = v;
      *(float2*)(vdst + 2 * t) = v;
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int idx = tid + 256 * i;
    if (idx < nold) {
      const int j = idx / HD4, e = idx - j * HD4;
      *(float4*)(ks + j * KP + 4 * e) = kr[i];
      *(float4*)(vs + j * HD + 4 * e) = vr[i];
    }
  }
  for (int i = tid; i < (((nk + 3) & ~3) - nk) * HD; i += 256) vs[nk * HD + i] = 0.f;  // V rows of the padded key count (weight exactly 0)
  __syncthreads();
  ts_mid(ts);
  for (int p = tid >> 2; p < G * nk; p += 64) {  // (head, key) per 4 lanes: each lane a quarter of the head dimension, then two butterfly adds
    const int g = p / nk, j = p - g * nk, qd = tid & 3;
    const float4* kr4 = (const float4*)(ks + j * KP) + qd * (HD4 / 4);
    const float4* q4 = (const float4*)(qs + g * HD) + qd * (HD4 / 4);
    float d0 = 0.f, d1 = 0.f;
#pragma unroll
    for (int e = 0; e < HD4 / 4; e += 2) {
      const float4 ka = kr4[e], qa = q4[e], kb2 = kr4[e + 1], qb = q4[e + 1];
      d0 = __builtin_fmaf(qa.x, ka.x, d0); d0 = __builtin_fmaf(qa.y, ka.y, d0); d0 = __builtin_fmaf(qa.z, ka.z, d0); d0 = __builtin_fmaf(qa.w, ka.w, d0);
      d1 = __builtin_fmaf(qb.x, kb2.x, d1); d1 = __builtin_fmaf(qb.y, kb2.y, d1); d1 = __builtin_fmaf(qb.z, kb2.z, d1); d1 = __builtin_fmaf(qb.w, kb2.w, d1);
    }
    float d = d0 + d1;
    d += __shfl_xor(d, 1);
    d += __shfl_xor(d, 2);
    if (qd == 0) sc[g * 64 + j] = d * scale;
  }
  __syncthreads();
  for (int g = wave; g < G; g += 4) {  // softmax of one head: a lane per key (nk <= 64)
    const float v = lane < nk ? sc[g * 64 + lane] : -INFINITY;
    float mx = v;
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    const float pr = lane < nk ? expf(v - mx) : 0.f;
    float sum = pr;
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    sc[g * 64 + lane] = pr;  // (lanes >= nk: exact zeros, so the weighted sum below may run over a padded key count)
    if (lane == 0) inv[g] = 1.0f / sum;
  }
  __syncthreads();
  const int nk4 = (nk + 3) & ~3;  // <= 64; the V rows behind nk are finite (stale or zero-filled below) and meet weight 0
  for (int o = tid; o < G * HD; o += 256) {
    const int g = o / HD, e = o - g * HD;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int j = 0; j < nk4; j += 4) {  // (four chains; key order inside each)
      const float4 pw = *(const float4*)(sc + g * 64 + j);
      a0 = __builtin_fmaf(pw.x, vs[j * HD + e], a0);
      a1 = __builtin_fmaf(pw.y, vs[(j + 1) * HD + e], a1);
      a2 = __builtin_fmaf(pw.z, vs[(j + 2) * HD + e], a2);
      a3 = __builtin_fmaf(pw.w, vs[(j + 3) * HD + e], a3);
    }
    out[(long long)b * H * HD + (long long)kvh * G * HD + o] = ((a0 + a1) + (a2 + a3)) * inv[g];
  }
  ts_end(ts);
}
static size_t attn_step_lds_bytes(int max_pos, int hd, int G) {
  return ((size_t)max_pos * (hd + 4) + (size_t)((max_pos + 3) & ~3) * hd + (size_t)G * hd + (size_t)G * 64 + 16) * 4;
}

// attn_decode_kernel (round 3): the single-token attention over a LONG cache (the backbone: up to 2048 positions) in chunks of 8192 / hd keys
// with an online softmax.  attn_cache_kernel<true> walks the keys in dependent steps (a thread per key, then the values 8 keys at a
// time, one L2 round trip per step): ~9 us at 70 keys, ~20 us at 315 (config 4's prompts), x 16 layers per frame.  Here, as in
// attn_step_kernel, a workgroup owns one (item, kv head) and its G query heads; a chunk's K and V rows are requested at once (8 + 8
// 16-byte loads per thread) one chunk AHEAD of the arithmetic, land in LDS, and scores (4 lanes per (head, key)), the running maximum /
// sum (a wave per head) and the weighted sum (a thread per output, rescaled per chunk) run out of LDS.  RoPE + cache append fused.
template <int HD>
__global__ __launch_bounds__(256) void attn_decode_kernel(const float* qkv, int H, int KV, const int* pos_dev, int offset, float* kc, float* vc, int max_pos,
                                                           float scale, float* out, const float* rope, const int* pad, int nsplit, float* part) {
  constexpr int HD4 = HD / 4, KP = HD + 4, CH = 8192 / HD;
  extern __shared__ __attribute__((aligned(16))) float smd[];
  const int G = H / KV, kvh = blockIdx.x, b = blockIdx.y, z = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* ks = smd;                 // [CH][KP]
  float* vs = ks + CH * KP;        // [CH][HD]
  float* qs = vs + CH * HD;        // [G][HD]
  float* sc = qs + G * HD;         // [G][CH]
  float* kn = sc + G * CH;         // [HD] the new key (RoPE applied)
  float* vn = kn + HD;             // [HD]
  float* mrun = vn + HD;           // [G] running maximum
  float* lrun = mrun + 8;          // [G] running sum
  float* alpha = lrun + 8;         // [G] rescale factor of the current chunk
  if (pos_dev) offset += *pos_dev;
  const int pd = pad ? pad[b] : 0, nk = offset + 1 - pd;
  const int W = (H + 2 * KV) * HD;
  // key split (flash decoding): workgroup z of nsplit takes the chunks z, z + nsplit, ...; with nsplit > 1 it leaves an UNNORMALISED partial result
  // (sum, running maximum, running sum per head) in `part` and attn_merge_kernel combines the splits
  float* pz = part + (((long long)b * KV + kvh) * nsplit + z) * (long long)G * (HD + 2);
  if (nk <= 0 || z * CH >= nk) {  // a padding row (no key: the output is defined as zero) or a split without keys
    if (nsplit == 1) {
      for (int o = tid; o < G * HD; o += 256) out[(long long)b * H * HD + (long long)kvh * G * HD + o] = 0.f;
    } else {
      for (int o = tid; o < G * (HD + 2); o += 256) pz[o] = (o % (HD + 2)) == HD ? -INFINITY : 0.f;
    }
    return;
  }
  const float* kb = kc + ((long long)b * max_pos + pd) * KV * HD + kvh * HD;
  const float* vb = vc + ((long long)b * max_pos + pd) * KV * HD + kvh * HD;
  const int nold = nk - 1;  // cached keys; key nk - 1 is the new one (kn / vn)
  float4 kr[8], vr[8];
  // rows j0 .. j0 + CH - 1 of the cache (clamped: rows past nold are read and never used; every load unconditional)
#define KK_LOAD_CHUNK(J0)                                                                                             \
  _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                                                     \
    const int idx = tid + 256 * i, j = (J0) + idx / HD4, e = idx % HD4, jc = j < nold ? j : (nold > 0 ? nold - 1 : 0); \
    kr[i] = *(const float4*)(kb + (long long)jc * KV * HD + 4 * e);                                                   \
    vr[i] = *(const float4*)(vb + (long long)jc * KV * HD + 4 * e);                                                   \
  }
  KK_LOAD_CHUNK(z * CH)
  {  // the new position: RoPE on q (G heads) and k, v as is; k / v also go to the cache
    const float* cs = rope + (long long)(offset - pd) * (HD / 2) * 2;
    const float* q = qkv + (long long)b * W + (long long)kvh * G * HD;
    const float* kq = qkv + (long long)b * W + (H + kvh) * HD;
    const float* vq = qkv + (long long)b * W + (H + KV + kvh) * HD;
    float* kdst = kc + ((long long)b * max_pos + offset) * KV * HD + kvh * HD;
    float* vdst = vc + ((long long)b * max_pos + offset) * KV * HD + kvh * HD;
    const bool appender = (nold / CH) % nsplit == z;  // the split that owns the new key's chunk also appends it to the cache
    for (int i = tid; i < G * (HD / 2); i += 256) {
      const int ii = i % (HD / 2);
      const float2 c = *(const float2*)(cs + 2 * ii), x = *(const float2*)(q + 2 * i);
      *(float2*)(qs + 2 * i) = make_float2(x.x * c.x - x.y * c.y, x.y * c.x + x.x * c.y);
    }
    if (tid < HD / 2) {
      const float2 c = *(const float2*)(cs + 2 * tid), x = *(const float2*)(kq + 2 * tid);
      const float2 k2 = make_float2(x.x * c.x - x.y * c.y, x.y * c.x + x.x * c.y);
      *(float2*)(kn + 2 * tid) = k2;
      if (appender) *(float2*)(kdst + 2 * tid) = k2;
    } else if (tid >= 128 && tid < 128 + HD / 2) {
      const int t = tid - 128;
      const float2 v = *(const float2*)(vq + 2 * t);
      *(float2*)(vn + 2 * t) = v;
      if (appender) *(float2*)(vdst + 2 * t) = v;
    }
    if (tid < 8) { mrun[tid] = -INFINITY; lrun[tid] = 0.f; }
  }
  float acc[4] = {0.f, 0.f, 0.f, 0.f};  // outputs o = tid + 256 i of the G x HD (<= 1024)
  for (int j0 = z * CH; j0 < nk; j0 += nsplit * CH) {
    const int cn = nk - j0 < CH ? nk - j0 : CH, cn4 = (cn + 3) & ~3;
    // this chunk's rows into LDS (the loads went out a chunk ago); the new key / value take their slot if it falls into the chunk
    // (rows past the cached keys get zeros: the new key's slot is filled below -- kn / vn are visible only behind the barrier -- and the rows that pad
    // the key count to a multiple of 4 meet weight exactly 0; unconditional stores, so the loop unrolls and the rows stay in registers)
#pragma clang loop unroll(full)
    for (int i = 0; i < 8; ++i) {
      const int idx = tid + 256 * i, j = idx / HD4, e = idx % HD4;
      const bool live = j0 + j < nold;
      *(float4*)(ks + j * KP + 4 * e) = live ? kr[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      *(float4*)(vs + j * HD + 4 * e) = live ? vr[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    if (nold >= j0 && nold < j0 + CH) {  // (uniform) the new position lies in this chunk: row nold - j0
      const int jn = nold - j0;
      for (int e = tid; e < HD; e += 256) { ks[jn * KP + e] = kn[e]; vs[jn * HD + e] = vn[e]; }
    }
    KK_LOAD_CHUNK(j0 + nsplit * CH)  // this split's next chunk: its loads go out behind the LDS stores that freed the registers
    __syncthreads();
    for (int p = tid >> 2; p < G * cn; p += 64) {  // (head, key) per 4 lanes
      const int g = p / cn, j = p - g * cn, qd = tid & 3;
      const float4* kr4 = (const float4*)(ks + j * KP) + qd * (HD4 / 4);
      const float4* q4 = (const float4*)(qs + g * HD) + qd * (HD4 / 4);
      float d0 = 0.f, d1 = 0.f;
#pragma unroll
      for (int e = 0; e < HD4 / 4; e += 2) {
        const float4 ka = kr4[e], qa = q4[e], kb2 = kr4[e + 1], qb = q4[e + 1];
        d0 = __builtin_fmaf(qa.x, ka.x, d0); d0 = __builtin_fmaf(qa.y, ka.y, d0); d0 = __builtin_fmaf(qa.z, ka.z, d0); d0 = __builtin_fmaf(qa.w, ka.w, d0);
        d1 = __builtin_fmaf(qb.x, kb2.x, d1); d1 = __builtin_fmaf(qb.y, kb2.y, d1); d1 = __builtin_fmaf(qb.z, kb2.z, d1); d1 = __builtin_fmaf(qb.w, kb2.w, d1);
      }
      float d = d0 + d1;
      d += __shfl_xor(d, 1);
      d += __shfl_xor(d, 2);
      if (qd == 0) sc[g * CH + j] = d * scale;
    }
    __syncthreads();
    for (int g = wave; g < G; g += 4) {  // running softmax of one head over this chunk (<= 128 keys: two per lane)
      const float v0 = lane < cn ? sc[g * CH + lane] : -INFINITY, v1 = (CH > 64 && lane + 64 < cn) ? sc[g * CH + lane + 64] : -INFINITY;
      float mx = fmaxf(v0, v1);
      for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
      const float mo = mrun[g], mn = fmaxf(mo, mx);
      const float p0 = lane < cn ? expf(v0 - mn) : 0.f, p1 = (CH > 64 && lane + 64 < cn) ? expf(v1 - mn) : 0.f;
      float sum = p0 + p1;
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
      sc[g * CH + lane] = p0;  // (slots >= cn: exact zeros, the weighted sum runs over the padded count)
      if (CH > 64) sc[g * CH + lane + 64] = p1;
      if (lane == 0) {
        const float al = expf(mo - mn);  // exp(-inf) = 0 on the first chunk
        alpha[g] = al;
        mrun[g] = mn;
        lrun[g] = lrun[g] * al + sum;
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int o = tid + 256 * i;
      if (o < G * HD) {
        const int g = o / HD, e = o - g * HD;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (int j = 0; j < cn4; j += 4) {
          const float4 pw = *(const float4*)(sc + g * CH + j);
          a0 = __builtin_fmaf(pw.x, vs[j * HD + e], a0);
          a1 = __builtin_fmaf(pw.y, vs[(j + 1) * HD + e], a1);
          a2 = __builtin_fmaf(pw.z, vs[(j + 2) * HD + e], a2);
          a3 = __builtin_fmaf(pw.w, vs[(j + 3) * HD + e], a3);
        }
        acc[i] = acc[i] * alpha[g] + ((a0 + a1) + (a2 + a3));
      }
    }
    __syncthreads();  // ks / vs / sc are rewritten by the next chunk
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int o = tid + 256 * i;
    if (o < G * HD) {
      if (nsplit == 1) out[(long long)b * H * HD + (long long)kvh * G * HD + o] = acc[i] / lrun[o / HD];
      else pz[(o / HD) * (HD + 2) + o % HD] = acc[i];
    }
  }
  if (nsplit > 1 && tid < G) { pz[tid * (HD + 2) + HD] = mrun[tid]; pz[tid * (HD + 2) + HD + 1] = lrun[tid]; }
}
// out[b][head][:] = sum_z exp(m_z - m) O_z / sum_z exp(m_z - m) l_z over the key splits of attn_decode_kernel (split order; <= 8 splits, all loads at once).
// part is [b][kv head][split][G][HD + 2]: head = kv head * G + g, the splits of one head sit G (HD + 2) floats apart.
template <int HD>
__global__ __launch_bounds__(HD) void attn_merge_kernel(const float* part, int H, int G, int nsplit, float* out) {
  const int h = blockIdx.x, b = blockIdx.y, e = threadIdx.x;
  const int kvh = h / G, g = h - kvh * G;
  const long long zs = (long long)G * (HD + 2);
  const float* base = part + (((long long)b * (H / G) + kvh) * nsplit) * zs + (long long)g * (HD + 2);
  float mz[8], lz[8], oz[8];
#pragma unroll
  for (int zz = 0; zz < 8; ++zz) {
    const float* q = base + (long long)(zz < nsplit ? zz : 0) * zs;
    mz[zz] = zz < nsplit ? q[HD] : -INFINITY;
    lz[zz] = q[HD + 1];
    oz[zz] = q[e];
  }
  float m = mz[0];
#pragma unroll
  for (int zz = 1; zz < 8; ++zz) m = fmaxf(m, mz[zz]);
  float num = 0.f, den = 0.f;
#pragma unroll
  for (int zz = 0; zz < 8; ++zz) {
    const float w = mz[zz] == -INFINITY ? 0.f : expf(mz[zz] - m);  // an empty or absent split weighs nothing
    num = __builtin_fmaf(w, oz[zz], num);
    den = __builtin_fmaf(w, lz[zz], den);
  }
  out[((long long)b * H + h) * HD + e] = den > 0.f ? num / den : 0.f;  // (no key at all: zero, as in the unsplit form)
}
#undef KK_LOAD_CHUNK
// key splits of attn_decode_kernel: one per 2 chunks of the longest cache, at most 8 (the backbone's 2048 positions: 8 splits of 2 chunks;
// short test stacks: 1-2)
static int attn_nsplit(int max_pos, int hd) {
  const int CHk = 8192 / hd, nchunks = (max_pos + CHk - 1) / CHk;
  const int nsplit = (nchunks + 1) / 2;
  return nsplit < 1 ? 1 : (nsplit > 8 ? 8 : nsplit);
}
static size_t attn_decode_lds_bytes(int hd, int G) {
  const size_t CH = 8192 / hd;
  return (CH * (hd + 4) + CH * hd + (size_t)G * hd + (size_t)G * CH + 2 * hd + 24) * 4;
}

// dynamic LDS of attn_cache_kernel: scores (padded to 4) + q + G partial outputs of hd floats (G = 512 / hd) + the new k and v rows
static size_t attn_lds_bytes(int max_pos, int hd) { return ((size_t)((max_pos + 3) & ~3) + hd + (size_t)(512 / hd) * hd + 2 * hd) * 4; }
// of attn_cache_rows_kernel: the score buffer holds the key window only (at most ctx cached keys + the block's S), and no new k / v rows
static int attn_rows_window(int max_pos, int S, int ctx) { return ctx >= 0 && ctx + S < max_pos ? ctx + S : max_pos; }
static size_t attn_rows_lds_bytes(int cap, int hd) { return ((size_t)((cap + 3) & ~3) + hd + (size_t)(512 / hd) * hd) * 4; }

}  // namespace

// The attention of one new position per item (qkv [B][(H + 2 KV) hd]) over a cache of max_pos slots, RoPE of q / the new key and the cache
// append at slot offset (+ *pos_dev) inside.  `form`: ATTN_AUTO = the single-token step's choice -- attn_step_kernel for a short cache,
// attn_decode_kernel (+ attn_merge_kernel over its key splits) for a long one, attn_cache_kernel<true> past G = 8 --, or a forced one.
// attp: the key-split partials, 8 B H (hd + 2) floats.  ts: the debug timestamp slot of attn_step_kernel (the one instrumented kernel of the
// family; the slots belong to kk_csm.hip), null in production and for every other form.
int attn_single(int form, const float* qkv, int B, int H, int KV, int hd, const int* pos_dev, int offset, float* kc, float* vc, int max_pos,
                const float* rope, const int* pad, float* att, float* attp, unsigned long long* ts, hipStream_t st) {
  const int G = H / KV;
  if (form == ATTN_AUTO) form = attn_auto_form(G, max_pos);
  if (form == ATTN_STEP) {
    const size_t lds = attn_step_lds_bytes(max_pos, hd, G);
    static KKDevOnce attr;
    if (attr.first()) {
      (void)hipFuncSetAttribute((const void*)attn_step_kernel<128>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)attn_step_lds_bytes(64, 128, 8));
      (void)hipFuncSetAttribute((const void*)attn_step_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)attn_step_lds_bytes(64, 64, 8));
      attr.done();
    }
    if (hd == 128)
      hipLaunchKernelGGL(attn_step_kernel<128>, dim3(KV, B), dim3(256), lds, st, qkv, H, KV, pos_dev, offset, kc, vc, max_pos, 1.0f / sqrtf((float)hd), att, rope,
                         pad, ts);
    else
      hipLaunchKernelGGL(attn_step_kernel<64>, dim3(KV, B), dim3(256), lds, st, qkv, H, KV, pos_dev, offset, kc, vc, max_pos, 1.0f / sqrtf((float)hd), att, rope,
                         pad, ts);
    KK_CHECK_LAUNCH();
  } else if (form == ATTN_DECODE) {
    const size_t lds = attn_decode_lds_bytes(hd, G);
    static KKDevOnce attr;
    if (attr.first()) {
      (void)hipFuncSetAttribute((const void*)attn_decode_kernel<128>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)attn_decode_lds_bytes(128, 8));
      (void)hipFuncSetAttribute((const void*)attn_decode_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)attn_decode_lds_bytes(64, 8));
      attr.done();
    }
    const int nsplit = attn_nsplit(max_pos, hd);
    if (nsplit > 1 && !attp) return kk_fail("kk_csm: internal: attention partials");
    if (hd == 128)
      hipLaunchKernelGGL(attn_decode_kernel<128>, dim3(KV, B, nsplit), dim3(256), lds, st, qkv, H, KV, pos_dev, offset, kc, vc, max_pos, 1.0f / sqrtf((float)hd),
                         att, rope, pad, nsplit, attp);
    else
      hipLaunchKernelGGL(attn_decode_kernel<64>, dim3(KV, B, nsplit), dim3(256), lds, st, qkv, H, KV, pos_dev, offset, kc, vc, max_pos, 1.0f / sqrtf((float)hd),
                         att, rope, pad, nsplit, attp);
    KK_CHECK_LAUNCH();
    if (nsplit > 1) {
      if (hd == 128) hipLaunchKernelGGL(attn_merge_kernel<128>, dim3(H, B), dim3(128), 0, st, attp, H, G, nsplit, att);
      else hipLaunchKernelGGL(attn_merge_kernel<64>, dim3(H, B), dim3(64), 0, st, attp, H, G, nsplit, att);
    }
    KK_CHECK_LAUNCH();
  } else {
    hipLaunchKernelGGL(attn_cache_kernel<true>, dim3(1, H, B), dim3(128), attn_lds_bytes(max_pos, hd), st, qkv, 1, H, KV, hd, pos_dev, offset, kc, vc, max_pos,
                       1.0f / sqrtf((float)hd), att, 1, -1, rope, pad);
    KK_CHECK_LAUNCH();
  }
  return 0;
}

// A block of S > 1 new positions per item: RoPE (q in place in qkv) + cache append, then causal attention of the block over the cache
int attn_prompt(float* qkv, int B, int S, int H, int KV, int hd, const int* pos_dev, int offset, float* kc, float* vc, int max_pos, const float* rope,
                const int* pad, float* att, hipStream_t st) {
  hipLaunchKernelGGL(rope_append_kernel, dim3(S, B), dim3(256), 0, st, qkv, S, H, KV, hd, rope, pos_dev, offset, kc, vc, max_pos, pad);
  KK_CHECK_LAUNCH();
  hipLaunchKernelGGL(attn_cache_kernel<false>, dim3(S, H, B), dim3(128), attn_lds_bytes(max_pos, hd), st, qkv, S, H, KV, hd, pos_dev, offset, kc, vc, max_pos,
                     1.0f / sqrtf((float)hd), att, 1, -1, (const float*)nullptr, pad);
  KK_CHECK_LAUNCH();
  return 0;
}

// the cache kernels on their own (Mimi's streaming transformer, kk_mimi.hip): interleaved-pair RoPE from a [max_pos][hd/2][2] cos|sin
// table on q (in place) and k, k / v appended to the caches at `offset`; attention of the S new queries over the cache
int kk_launch_rope_append(float* qkv, int S, int H, int KV, int hd, const float* rope, int offset, float* kc, float* vc, int max_pos, int B, hipStream_t st) {
  if (hd != 64 && hd != 128) return kk_fail("rope_append: head_dim must be 64 or 128");
  hipLaunchKernelGGL(rope_append_kernel, dim3(S, B), dim3(256), 0, st, qkv, S, H, KV, hd, rope, (const int*)nullptr, offset, kc, vc, max_pos, (const int*)nullptr);
  KK_CHECK_LAUNCH();
  return 0;
}
int kk_launch_attn_cache(const float* qkv, int S, int H, int KV, int hd, int offset, const float* kc, const float* vc, int max_pos, float scale, float* out,
                         int causal, int ctx, int B, hipStream_t st) {
  if (hd != 64 && hd != 128) return kk_fail("attn_cache: head_dim must be 64 or 128");
  hipLaunchKernelGGL(attn_cache_kernel<false>, dim3(S, H, B), dim3(128), attn_lds_bytes(max_pos, hd), st, qkv, S, H, KV, hd, (const int*)nullptr, offset,
                     const_cast<float*>(kc), const_cast<float*>(vc), max_pos, scale, out, causal, ctx, (const float*)nullptr, (const int*)nullptr);
  KK_CHECK_LAUNCH();
  return 0;
}
// the per-row-offset forms: row b's S rows sit at position row_pos[b] (device, [B]); rows with active[b] == 0 (device, [B]) are left alone.
// No causal mask (Mimi's streaming transformer); ctx >= 0 limits the look-back to the last ctx cached keys of the row.
int kk_launch_rope_append_rows(float* qkv, int S, int H, int KV, int hd, const float* rope, const int* row_pos, const int* active, float* kc, float* vc,
                               int max_pos, int B, hipStream_t st) {
  if (hd != 64 && hd != 128) return kk_fail("rope_append_rows: head_dim must be 64 or 128");
  hipLaunchKernelGGL(rope_append_rows_kernel, dim3(S, B), dim3(256), 0, st, qkv, S, H, KV, hd, rope, row_pos, active, kc, vc, max_pos);
  KK_CHECK_LAUNCH();
  return 0;
}
int kk_launch_attn_cache_rows(const float* qkv, int S, int H, int KV, int hd, const int* row_pos, const int* active, const float* kc, const float* vc,
                              int max_pos, float scale, float* out, int ctx, int B, hipStream_t st) {
  if (hd != 64 && hd != 128) return kk_fail("attn_cache_rows: head_dim must be 64 or 128");
  const int cap = attn_rows_window(max_pos, S, ctx);
  const size_t lds = attn_rows_lds_bytes(cap, hd);
  if (lds > 64 * 1024) return kk_fail("attn_cache_rows: the key window does not fit the score buffer");
  hipLaunchKernelGGL(attn_cache_rows_kernel, dim3(S, H, B), dim3(128), lds, st, qkv, S, H, KV, hd, row_pos, active, kc, vc, max_pos, scale, out, ctx, cap);
  KK_CHECK_LAUNCH();
  return 0;
}

extern "C" int kk_op_csm_attn_single(void* stream, int form, int B, int H, int KV, int hd, const float* qkv, float* kc, float* vc, int max_pos, int offset,
                                     const float* rope, const int32_t* pad, float* out, float* part) {
  if (!qkv || !kc || !vc || !rope || !out || B < 1 || H < 1 || KV < 1 || H % KV != 0 || offset < 0 || offset >= max_pos || form < 0 || form > 3)
    return kk_fail("kk_op_csm_attn_single: bad argument");
  if (hd != 64 && hd != 128) return kk_fail("kk_op_csm_attn_single: head_dim must be 64 or 128");
  const int G = H / KV;
  if (form == ATTN_AUTO) form = attn_auto_form(G, max_pos);
  if (form == ATTN_STEP && (max_pos > 64 || G > 8)) return kk_fail("kk_op_csm_attn_single: the short-cache kernel needs max_pos <= 64 and G <= 8");
  if (form == ATTN_DECODE && (G > 8 || (attn_nsplit(max_pos, hd) > 1 && !part))) return kk_fail("kk_op_csm_attn_single: the long-cache kernel needs G <= 8 and partials");
  if (form == ATTN_CACHE && attn_lds_bytes(max_pos, hd) > 64 * 1024) return kk_fail("kk_op_csm_attn_single: cache too long");
  return attn_single(form, qkv, B, H, KV, hd, nullptr, offset, kc, vc, max_pos, rope, pad, out, part, nullptr, (hipStream_t)stream);
}

extern "C" int kk_op_csm_attn_prompt(void* stream, int B, int S, int H, int KV, int hd, float* qkv, float* kc, float* vc, int max_pos, int offset, const float* rope,
                                     const int32_t* pad, float* out) {
  if (!qkv || !kc || !vc || !rope || !out || B < 1 || S < 1 || H < 1 || KV < 1 || H % KV != 0 || offset < 0 || offset + S > max_pos)
    return kk_fail("kk_op_csm_attn_prompt: bad argument");
  if (hd != 64 && hd != 128) return kk_fail("kk_op_csm_attn_prompt: head_dim must be 64 or 128");
  if (attn_lds_bytes(max_pos, hd) > 64 * 1024) return kk_fail("kk_op_csm_attn_prompt: cache too long");
  return attn_prompt(qkv, B, S, H, KV, hd, nullptr, offset, kc, vc, max_pos, rope, pad, out, (hipStream_t)stream);
}

extern "C" int kk_op_attn_cache_block(void* stream, int B, int S, int H, int KV, int hd, float* qkv, float* kc, float* vc, int max_pos, int offset,
                                      const int32_t* row_pos, const int32_t* active, const float* rope, int ctx, float* out) {
  if (!qkv || !kc || !vc || !rope || !out || B < 1 || S < 1 || H < 1 || KV < 1 || H % KV != 0 || max_pos < 1 || S > max_pos)
    return kk_fail("kk_op_attn_cache_block: bad argument");
  if (row_pos ? !active : (offset < 0 || offset + S > max_pos)) return kk_fail("kk_op_attn_cache_block: bad argument");
  if (hd != 64 && hd != 128) return kk_fail("kk_op_attn_cache_block: head_dim must be 64 or 128");
  const float scale = 1.0f / sqrtf((float)hd);
  if (!row_pos) {
    if (attn_lds_bytes(max_pos, hd) > 64 * 1024) return kk_fail("kk_op_attn_cache_block: cache too long");
    KK_TRY(kk_launch_rope_append(qkv, S, H, KV, hd, rope, offset, kc, vc, max_pos, B, (hipStream_t)stream));
    return kk_launch_attn_cache(qkv, S, H, KV, hd, offset, kc, vc, max_pos, scale, out, 0, ctx, B, (hipStream_t)stream);
  }
  if (attn_rows_lds_bytes(attn_rows_window(max_pos, S, ctx), hd) > 64 * 1024) return kk_fail("kk_op_attn_cache_block: the key window does not fit the score buffer");
  KK_TRY(kk_launch_rope_append_rows(qkv, S, H, KV, hd, rope, row_pos, active, kc, vc, max_pos, B, (hipStream_t)stream));
  return kk_launch_attn_cache_rows(qkv, S, H, KV, hd, row_pos, active, kc, vc, max_pos, scale, out, ctx, B, (hipStream_t)stream);
}
