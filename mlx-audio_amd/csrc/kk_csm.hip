// CSM-1B frame generator: SesameModel.generate_frame, mlx_audio/tts/models/sesame/sesame.py:349-395
//   tokens [B][S][n_cb+1] -> masked sum of 33 embeddings -> Llama backbone (KV cache) -> codebook0 head -> sample ->
//   31 x { projection -> Llama depth decoder (fresh cache per frame) -> audio_head[i-1] -> sample -> embed } -> codes [B][n_cb]
// Llama layer (mlx_lm LlamaModel with the reference's Attention, sesame.py:296-299; attention.py:113-195):
//   h += Wo . attn(rope(Wq x), rope(Wk x), Wv x), x = rms(h);   h += Wdown (silu(Wgate x) * Wup x), x = rms(h);   final rms
//   RoPE: interleaved pairs, llama3-scaled frequencies (attention.py:33-110); GQA: query head h reads kv head h / (H / KV);
//   mask: causal inside the new block, every cached key visible (sesame.py:37-48).
// This file is the HANDLE: the weight packers (Packer, pack_stack, kk_csm_finalize), the caches, the workspace plan (Run), the two forms of a
// Llama stack (stack_forward: any block; stack_step: the fused single-token layers of bf16 / quantised weights), run_frame, and the host state machine
// of the kk_csm_* entries -- frames, graph replay, continuous batching, prefixes, transfer.  It holds no device code: what it launches is declared in
// the "CSM generator" block of kk_kernels.h and lives in kk_csm_kernels.hip (glue, Linears, packs), kk_csm_sample.hip (the sampler family) and
// kk_attn_cache.hip (attention).  The KV caches are library-owned device memory (kk_csm_setup_caches), like the module-owned caches of the reference
// (sesame.py:320-333).
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
#include "kk_kernels.h"

namespace {

struct Lin : KKCsmWeight {  // + where the matrix lives in the arenas
  size_t off = 0;              // fp32 generic-kernel pack [1][Cin][ldw] in kk_csm::arena (`w`)
  bool has_f32 = true;
  size_t moff = 0;             // bf16 weight mode (kk_csm_set_weight_dtype): the same matrix as a bf16 fragment pack in kk_csm::packb (`wm`)
  // packed storage of a quantised checkpoint (kk_csm_load_quantized): `wm` points at the quantised fragment pack instead, `wp` at its (scale, bias)
  // pairs; such a matrix has NO fp32 copy (w == nullptr) and no bf16 one
  size_t qoff = 0, poff = 0;   // byte offsets into kk_csm::packq
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
  // per-row sampler table (kk_csm_set_row_sampler / kk_csm_generate_frame_rows): [max_batch] entries of KK_CSM_ROW_SAMPLER_BYTES, zero = arg-max
  void* row_samplers = nullptr;
  bool row_samplers_zero_pending = false;  // kk_csm_reset_caches_parked takes no stream: zeroed on the next stream that flushes
  unsigned long long weights_id = 0;   // the weight set (kk_csm_finalize; kk_csm_share copies it): what a kk_csm_prefix is tied to
  const kk_csm* weights_of = nullptr;  // kk_csm_share: `dev` / `devb` / `devq` belong to that generator (immutable after finalize), not to this one
  // kk_csm_admit_transfer into THIS generator: the source's stream has finished the admission / this stream has finished the copy.  Created at the
  // first transfer, destroyed with the generator (a kk_csm_share copy starts without them).
  hipEvent_t xfer_ready = nullptr, xfer_done = nullptr;
};

namespace {

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
        u = kk_csm_bf16_round(u) << 16;
        memcpy(&dst[e], &u, 4);
      }
      int ks = 1, nsub = 0;
      kk_csm_frag_plan(I, O, split_ok, &ks, &nsub);
      if (nsub) {
        l.ks = ks; l.nsub = nsub;
        l.moff = m->packb.size();
        m->packb.resize(l.moff + kk_csm_frag_elems(I, O, nsub));
        kk_csm_frag_pack_rows(dst, I, O, l.ldw, nsub, &m->packb[l.moff]);
        m->linear_bytes += kk_csm_frag_elems(I, O, nsub) * 2;
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
    kk_csm_frag_plan(I, O, split_ok, &l.ks, &l.nsub);
    const size_t qb = kk_csm_qfrag_q_bytes(I, O, l.nsub, first.bits), pb = kk_csm_qfrag_pair_bytes(I, O, l.nsub, l.group);
    l.qoff = (m->packq.size() + 255) & ~(size_t)255;
    l.poff = (l.qoff + qb + 255) & ~(size_t)255;
    m->packq.resize(l.poff + pb, 0);
    int base = 0;
    for (size_t k = 0; k < outs.size(); ++k) {
      const QuantHost& t = m->qhost.at(names[k]);
      kk_csm_qfrag_pack_part(t.words.data(), t.scales.data(), t.biases.data(), outs[k], base, I, l.nsub, l.group, t.bits, &m->packq[l.qoff],
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
    if (!kk_csm_group_ok(s.I, group)) return s.names[0] + ": group size " + std::to_string(group) + " (a multiple of 32 that divides K)";
    int ks = 1, nsub = 0;
    kk_csm_frag_plan(s.I, O, s.split_ok, &ks, &nsub);
    if (!nsub) return s.names[0] + ": no fragment pack for K = " + std::to_string(s.I);
  }
  if (c.audio_num_codebooks > 1) {
    int ks = 1, nsub = 0;
    kk_csm_frag_plan(c.decoder.hidden, c.audio_vocab_size, false, &ks, &nsub);
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
      if (kk_csm_skinny_floats(w.Cin, w.Cout) <= skinny_floats) {
        KK_TRY(kk_launch_csm_skinny(st, w, x, Mtot, res, out, skinny_scratch));
        // (one workgroup per row summing the slices AND normalising was tried: 17-38 us against 5 + 5 for the two launches)
        return xn ? kk_launch_csm_rmsnorm(st, out, nw, w.Cout, eps, xn, Mtot) : 0;
      }
    }
    if (xbs == (long long)rows * w.Cin && obs == (long long)rows * w.Cout && w.wm && w.nsub && (rows > 2 || !w.w || lin_mode == LIN_PROMPT) &&
        lin_mode != LIN_GENERIC) {
      // the prompt block in bf16 weight mode: matrix cores (gemmp_kernel); without a fragment pack, the generic fp32 kernel below.
      // The choice depends on the rows PER ITEM only, never on B: a stream's bits do not depend on its batch.  (A packed quantised matrix has
      // no fp32 copy for the skinny GEMM: its one- and two-row blocks come here too.)
      KK_TRY(kk_launch_csm_gemm_prompt(st, w, x, w.Cin, B * rows, res, w.Cout, out, w.Cout));
      return xn ? kk_launch_csm_rmsnorm(st, out, nw, w.Cout, eps, xn, B * rows) : 0;
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
    return kk_launch_csm_rmsnorm(st, out, nw, w.Cout, eps, xn, B * rows);
  }
};

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
  if (!r.dry) KK_TRY(kk_launch_csm_rmsnorm(r.st, h, st.layers[0].n1.p, D, a.rms_eps, x, B * S));
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
    if (!r.dry) KK_TRY(kk_launch_csm_swiglu(r.st, gu, I, (long long)B * S * I, act));
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
// `gather` (optional): layer 0 reads its input rows from a table by code instead of from h, and writes them to h (KKCsmGemv codes / cstride / cb / V / emb)
int stack_step(Run& r, Stack& st, float* h, int rows, int offset, const KKCsmGemv* gather = nullptr) {
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
    KKCsmGemv g;
    g.x = h; g.xrs = D; g.nw = L.n1.p; g.eps = a.rms_eps; g.out = qkv; g.ors = W;
    if (l == 0 && gather) { g.codes = gather->codes; g.cstride = gather->cstride; g.cb = gather->cb; g.V = gather->V; g.emb = gather->emb; g.gather_out = h; }
    KK_TRY(kk_launch_csm_gemv(r.st, L.qkv, 1, 0, g, M));
    if (rows == 1) {
      const int form = attn_auto_form(H / KV, st.max_pos);  // (the short-cache kernel is the instrumented one)
      KK_TRY(attn_single(form, qkv, B, H, KV, hd, st.pos_dev, st.pos_dev ? 0 : offset, kc, vc, st.max_pos, st.rope.p, st.pad_dev, att, attp,
                         form == ATTN_STEP ? kk_csm_ts_slot() : nullptr, r.st));
    } else KK_TRY(attn_prompt(qkv, B, rows, H, KV, hd, st.pos_dev, st.pos_dev ? 0 : offset, kc, vc, st.max_pos, st.rope.p, st.pad_dev, att, r.st));
    g = KKCsmGemv();
    g.x = att; g.xrs = (long long)H * hd; g.res = h; g.rrs = D; g.out = h; g.ors = D;
    KK_TRY(kk_launch_csm_gemv(r.st, L.o, 0, 1, g, M));
    g = KKCsmGemv();
    g.x = h; g.xrs = D; g.nw = L.n2.p; g.eps = a.rms_eps; g.out = gu; g.ors = 2 * I;
    KK_TRY(kk_launch_csm_gemv(r.st, L.gu, 1, 0, g, M));
    g = KKCsmGemv();
    g.x = gu; g.xrs = 2 * I;
    KK_TRY(kk_launch_csm_gemv_accumulate(r.st, L.down, 2, g, M, h, part));
  }
  return 0;
}

// `seed`: the device seed of the Philox uniforms, or null (injected uniforms / argmax)
// `own_pos` >= 0 (kk_csm_admit): the frame is the prompt block of ONE stream in a row view of the backbone cache -- its Philox position is that
// constant (the stream's own position, not slot - padding) and the shared slot counter is NOT advanced
// `split` (kk_csm_admit_prefixed): the block is the tail of a longer prompt -- its backbone rows and the first head take the kernels the rows of the
// unsplit block take, whatever S (Run::lin_mode); the depth decoder sees the same shapes either way
int run_frame(Run& r, int S, const int* tokens, const float* mask, const KKCsmSampleCfg& sc, const float* uniforms, const unsigned long long* seed,
              const int* stream_ids, int* codes, int own_pos = -1, bool split = false, const void* table = nullptr) {
  kk_csm* m = r.m;
  // the uniform of (item, code book i): uniforms[b][i], or Philox at the position of the frame being generated (slot *pos_dev + S, minus the padding)
  auto src_of = [&](int i) {
    KKCsmSampleSrc s;
    s.u = uniforms ? uniforms + i : nullptr; s.ustride = m->cfg.audio_num_codebooks;
    s.seed = uniforms ? nullptr : seed; s.sid = stream_ids; s.pos = m->bb.pos_dev; s.pos_stride = 0; s.pos_add = S; s.pad = m->bb.pad_dev; s.cb = i;
    if (own_pos >= 0) { s.pos = nullptr; s.pad = nullptr; s.pos_add = own_pos; }
    return s;
  };
  // the sampling launch of code book i: the settings as launch arguments, or (table mode: `seed` only says that the launch draws) row b's from table[b]
  auto sample = [&](const float* lg, int i, int* out) {
    return table ? kk_launch_csm_sample_rows(r.st, lg, m->cfg.audio_vocab_size, table, src_of(i), out, m->cfg.audio_num_codebooks, r.B)
                 : kk_launch_csm_sample(r.st, lg, m->cfg.audio_vocab_size, sc, src_of(i), out, m->cfg.audio_num_codebooks, r.B);
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
    r.skinny_floats = (size_t)2 * 1024 * 256 * KK_CSM_SKINNY_MAXM;
    r.skinny_scratch = r.f32(r.skinny_floats);
  }
  if (r.oom) return kk_fail("kk_csm_generate_frame: workspace too small");
  if (!r.dry) KK_TRY(kk_launch_csm_embed_sum(r.st, tokens, mask, m->audio_emb.p, m->text_emb.p, ncb, V, c.text_vocab_size, D, B * S, h));
  const size_t inner = r.used;
  // bf16 weight mode: single-token frames (and every depth-decoder step) run on the fused five-launch layers
  const bool fast = m->wdt == KK_BF16 && stack_can_step(m->bb) && stack_can_step(m->dec) && m->proj.wm && m->c0_head.wm;
  bool heads_fast = fast;
  for (const auto& l : m->audio_head) heads_fast = heads_fast && l.wm;
  const float* last_h;   // the backbone's final-normed last position of every item
  long long last_rs;     // its item pitch
  if (fast && heads_fast && S == 1 && !split) {
    KK_TRY(stack_step(r, m->bb, h, 1, m->bb.offset));
    if (!r.dry) KK_TRY(kk_launch_csm_rmsnorm(r.st, h, m->bb.norm.p, D, c.backbone.rms_eps, hn, B));
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
      KKCsmGemv g;
      g.x = last_h; g.xrs = last_rs; g.out = logits; g.ors = V;
      KK_TRY(kk_launch_csm_gemv(r.st, m->c0_head, 0, 0, g, B));
      KK_TRY(sample(logits, 0, codes));
    }
    int rows = 2, dpos = 0;
    for (int i = 1; i < ncb; ++i) {
      r.used = inner;
      // curr = [last_h, embed(0, c0)] for the first step, [embed(i-1, c_{i-1})] afterwards (sesame.py:373-392): gathered by the projection's prologue
      // later steps (one row per item): the projection of an embedding row is a row of the table built at finalize -- no launch; the decoder's first
      // kernel gathers it and materialises the residual stream
      const bool tabled = rows == 1 && m->proj_table && m->dec.layers[0].qkv.wm;
      KKCsmGemv gat;
      gat.codes = codes + (i - 1); gat.cstride = ncb; gat.cb = i - 1; gat.V = V; gat.emb = m->proj_table;
      if (!r.dry && !tabled) {
        KKCsmGemv g;
        g.x = last_h; g.xrs = last_rs; g.codes = codes + (i - 1); g.cstride = ncb; g.cb = i - 1; g.V = V; g.rows = rows; g.emb = m->audio_emb.p;
        g.out = pin; g.ors = Dd;
        KK_TRY(kk_launch_csm_gemv(r.st, m->proj, 3, 0, g, B * rows));
      }
      KK_TRY(stack_step(r, m->dec, pin, rows, dpos, tabled ? &gat : nullptr));
      if (r.used > peak) peak = r.used;
      dpos += rows;
      if (!r.dry) {
        if (dbg) logits = m->dbg_logits + (size_t)i * m->max_batch * V;
        KKCsmGemv g;
        g.x = pin + (size_t)(rows - 1) * Dd; g.xrs = (long long)rows * Dd; g.nw = m->dec.norm.p; g.eps = c.decoder.rms_eps; g.out = logits; g.ors = V;
        KK_TRY(kk_launch_csm_gemv(r.st, m->audio_head[i - 1], 1, 0, g, B));
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
    KK_TRY(kk_launch_csm_copy_rows(r.st, last_h, last_rs, curr, (long long)2 * D, D, B));
    KK_TRY(kk_launch_csm_embed_audio(r.st, codes, ncb, m->audio_emb.p, 0, V, D, curr, 2, 1, B));
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
      KK_TRY(kk_launch_csm_embed_audio(r.st, codes + i, ncb, m->audio_emb.p, i, V, D, curr, 1, 0, B));
    }
    rows = 1;
  }
  }
  if (!r.dry && own_pos < 0) KK_TRY(kk_launch_csm_advance_pos(r.st, m->bb.pos_dev, S));
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
    m->table_bytes = rows * Dd * sizeof(float);
    m->total_bytes += m->table_bytes;
    if (kk_launch_csm_gemm_prompt((hipStream_t)stream, m->proj, m->audio_emb.p, D, (int)rows, nullptr, 0, m->proj_table, Dd) != 0 ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
      return kk_fail("kk_csm_finalize: projection table failed");
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
  if (hipMalloc(&m->row_samplers, (size_t)max_batch * KK_CSM_ROW_SAMPLER_BYTES) != hipSuccess ||
      hipMemset(m->row_samplers, 0, (size_t)max_batch * KK_CSM_ROW_SAMPLER_BYTES) != hipSuccess)
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
  if (run_frame(r, S, nullptr, nullptr, KKCsmSampleCfg(), nullptr, nullptr, nullptr, nullptr) != 0) return 0;
  return r.used + 256;
}

// ---- host steps the entries share.  Each takes the entry's name (`who`): the refusals, and the order an entry tests its arguments in, are the entry's own
namespace {
// The preconditions most entries start with, in this order: a finalized model, caches set up, a row inside them.
enum { NEED_FINAL = 1, NEED_CACHES = 2, NEED_ROW = 4 };
int need(const char* who, const kk_csm* m, int what, int row = 0) {
  if ((what & NEED_FINAL) && (!m || !m->finalized)) return kk_failf("%s: model not finalized", who);
  if ((what & NEED_CACHES) && (!m || m->max_batch < 1)) return kk_failf("%s: call kk_csm_setup_caches first", who);
  if ((what & NEED_ROW) && (row < 0 || row >= m->max_batch)) return kk_failf("%s: row out of range", who);
  return 0;
}

// what kk_csm_reset_caches / kk_csm_set_padding / kk_csm_park_row deferred, in stream order before the next frame, admission or shift (never
// inside a capture)
int flush_pending(kk_csm* m, hipStream_t st) {
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
    if (hipMemsetAsync(m->row_samplers, 0, (size_t)m->max_batch * KK_CSM_ROW_SAMPLER_BYTES, st) != hipSuccess)
      return kk_fail("kk_csm_generate_frame: sampler table reset failed");
    m->row_samplers_zero_pending = false;
  }
  return 0;
}
// the Philox seed lives in device memory: a new one does not re-capture the graph
int upload_seed(kk_csm* m, unsigned long long seed, hipStream_t st) {
  if (m->seed_valid && m->seed_host == seed) return 0;
  m->seed_host = seed;
  if (hipMemcpyAsync(m->seed_dev, &m->seed_host, 8, hipMemcpyHostToDevice, st) != hipSuccess) return kk_fail("kk_csm_generate_frame: seed upload failed");
  m->seed_valid = true;
  return 0;
}

// One frame of the whole batch: the body of kk_csm_generate_frame_ex (`sampler`: the settings of the launch) and of kk_csm_generate_frame_rows (`rows`:
// every row's settings from the table, `sampler` null, `use_device_rng` the entry's flag).  The single-token step in graph mode (~1400 launches) is one
// hipGraphLaunch: every position-dependent kernel reads the device counter.  The two key layouts are the entries' own and must not change (a changed
// key silently re-captures): table mode is keyed by the MODE (the leading tag; the other key has another length), B, the pointers and the uniform
// source -- never by what the table holds: kk_csm_set_row_sampler between two replays changes the next replay's picks without a new capture.
int frame_body(const char* who, kk_csm* m, void* stream, int B, int S, const int32_t* tokens, const float* tokens_mask, bool rows, const kk_csm_sampler* sampler,
               int use_device_rng, const float* uniforms, const int32_t* stream_ids, void* workspace, size_t workspace_bytes, int32_t* codes_out) {
  KK_TRY(need(who, m, NEED_FINAL | NEED_CACHES));
  if (rows && !m->row_samplers) return kk_failf("%s: call kk_csm_setup_caches first", who);
  if (B <= 0 || B > m->max_batch || S <= 0 || !tokens || !tokens_mask || !workspace || !codes_out) return kk_failf("%s: bad argument", who);
  if (m->bb.offset + S > m->bb.max_pos) return kk_failf("%s: sequence exceeds max_seq_len", who);
  if (S > 1 && m->bb.offset != 0) return kk_failf("%s: a multi-token block must start an empty cache (sesame.py:41-48)", who);
  if (workspace_bytes < kk_csm_workspace_bytes(m, B, S)) return kk_failf("%s: workspace too small", who);
  KK_TRY(flush_pending(m, (hipStream_t)stream));
  KKCsmSampleCfg sc;
  bool dev_rng = !uniforms && use_device_rng != 0;
  if (!rows) {
    KK_TRY(kk_csm_sampler_cfg(sampler, &sc, who));
    dev_rng = !uniforms && sampler->use_device_rng && sc.temp > 0.f;
    if (dev_rng) KK_TRY(upload_seed(m, sampler->seed, (hipStream_t)stream));
  }
  const void* table = rows ? m->row_samplers : nullptr;
  // (table mode: a non-null `seed` only tells run_frame that the launches draw on the device; the word itself is the row's entry)
  const unsigned long long* seed = !dev_rng ? nullptr : (rows ? (const unsigned long long*)table : m->seed_dev);
  auto eager = [&](hipStream_t on_stream) -> int {
    Run r(m, on_stream, B, workspace, workspace_bytes);
    return run_frame(r, S, tokens, tokens_mask, sc, uniforms, seed, dev_rng ? stream_ids : nullptr, codes_out, -1, false, table);
  };
  if (!m->graph_mode || S != 1) {
    KK_TRY(eager((hipStream_t)stream));
  } else {
    typedef unsigned long long u64;
    const u64 ts = (u64)(uintptr_t)kk_csm_ts_buffer(), sid = (u64)(uintptr_t)(dev_rng ? stream_ids : nullptr);
    std::vector<u64> key;
    if (rows) {
      key = {~0ull, (u64)B, (u64)(uintptr_t)tokens, (u64)(uintptr_t)tokens_mask, (u64)(uintptr_t)uniforms, (u64)(uintptr_t)workspace, (u64)workspace_bytes,
             (u64)(uintptr_t)codes_out, ts, (u64)dev_rng, sid, (u64)(uintptr_t)table};
    } else {
      unsigned tbits, pbits, mbits;
      memcpy(&tbits, &sc.temp, 4);
      memcpy(&pbits, &sc.top_p, 4);
      memcpy(&mbits, &sc.min_p, 4);
      key = {(u64)B, (u64)(uintptr_t)tokens, (u64)(uintptr_t)tokens_mask, (u64)tbits, (u64)(long long)sc.top_k, (u64)(uintptr_t)uniforms,
             (u64)(uintptr_t)workspace, (u64)workspace_bytes, (u64)(uintptr_t)codes_out, ts, (u64)pbits, (u64)mbits, (u64)sc.min_keep, (u64)dev_rng, sid};
    }
    hipGraphExec_t ex = nullptr;
    KK_TRY(m->graphs.run(key, (hipStream_t)stream, [&](hipStream_t on_stream, bool) { return eager(on_stream); }, &ex, "kk_csm"));
    if (ex && hipGraphLaunch(ex, (hipStream_t)stream) != hipSuccess) return kk_fail("kk_csm: hipGraphLaunch failed");
  }
  m->bb.offset += S;
  return 0;
}
}  // namespace

extern "C" int kk_csm_generate_frame(kk_csm* m, void* stream, int B, int S, const int32_t* tokens, const float* tokens_mask, float temperature,
                                     int top_k, const float* uniforms, void* workspace, size_t workspace_bytes, int32_t* codes_out) {
  kk_csm_sampler sp;
  memset(&sp, 0, sizeof sp);
  sp.temperature = temperature; sp.top_k = top_k; sp.min_tokens_to_keep = 1;
  return kk_csm_generate_frame_ex(m, stream, B, S, tokens, tokens_mask, &sp, uniforms, nullptr, workspace, workspace_bytes, codes_out);
}

extern "C" int kk_csm_generate_frame_ex(kk_csm* m, void* stream, int B, int S, const int32_t* tokens, const float* tokens_mask, const kk_csm_sampler* sampler,
                                        const float* uniforms, const int32_t* stream_ids, void* workspace, size_t workspace_bytes, int32_t* codes_out) {
  return frame_body("kk_csm_generate_frame", m, stream, B, S, tokens, tokens_mask, false, sampler, 0, uniforms, stream_ids, workspace, workspace_bytes, codes_out);
}

// ---- per-row sampler settings ---------------------------------------------------------------------------------------------------
extern "C" int kk_csm_set_row_sampler(kk_csm* m, void* stream, int row, const kk_csm_sampler* sampler) {
  if (!m || m->max_batch < 1 || !m->row_samplers) return kk_fail("kk_csm_set_row_sampler: call kk_csm_setup_caches first");
  KK_TRY(need("kk_csm_set_row_sampler", m, NEED_ROW, row));
  KKCsmSampleCfg sc;
  KK_TRY(kk_csm_sampler_cfg(sampler, &sc, "kk_csm_set_row_sampler"));
  KK_TRY(flush_pending(m, (hipStream_t)stream));  // a deferred zeroing of the table must not land behind this entry
  return kk_launch_csm_set_row_sampler((hipStream_t)stream, m->row_samplers, row, sc, sampler->seed);
}

extern "C" int kk_csm_generate_frame_rows(kk_csm* m, void* stream, int B, int S, const int32_t* tokens, const float* tokens_mask, int use_device_rng,
                                          const float* uniforms, const int32_t* stream_ids, void* workspace, size_t workspace_bytes, int32_t* codes_out) {
  return frame_body("kk_csm_generate_frame_rows", m, stream, B, S, tokens, tokens_mask, true, nullptr, use_device_rng, uniforms, stream_ids, workspace,
                    workspace_bytes, codes_out);
}

// ---- continuous batching: streams enter and leave a running batch -------------------------------------------------------------
// All rows share the slot counter P (bb.offset / *bb.pos_dev); row b's tokens live in slots [pad[b], P) at position slot - pad[b].  A PARKED row
// has pad[b] = max_pos: every attention form sees nk <= 0 for it (zero output, nothing appended), so it rides through the frame step's GEMVs
// with finite values and cannot reach another row.

// kk_csm_reset_caches with every row parked: P = 0, pad[b] = max_pos (the start of a serving session; the classic reset leaves all rows live)
extern "C" int kk_csm_reset_caches_parked(kk_csm* m) {
  KK_TRY(need("kk_csm_reset_caches_parked", m, NEED_CACHES));
  KK_TRY(kk_csm_reset_caches(m));
  m->pad_host.assign((size_t)m->max_batch, m->bb.max_pos);
  m->pad_pending = true;  // uploaded behind the deferred reset
  m->row_samplers_zero_pending = true;
  return 0;
}

extern "C" int kk_csm_park_row(kk_csm* m, int row) {
  KK_TRY(need("kk_csm_park_row", m, NEED_CACHES | NEED_ROW, row));
  m->pad_host[row] = m->bb.max_pos;
  m->pad_pending = true;  // uploaded on the next frame's stream
  return 0;
}

extern "C" int kk_csm_row_state(const kk_csm* m, int32_t* pad_out, int32_t* position) {
  KK_TRY(need("kk_csm_row_state", m, NEED_CACHES));
  if (pad_out) memcpy(pad_out, m->pad_host.data(), (size_t)m->max_batch * 4);
  if (position) *position = m->bb.offset;
  return 0;
}

extern "C" int kk_csm_shift_caches(kk_csm* m, void* stream, int delta, void* workspace, size_t workspace_bytes) {
  (void)workspace; (void)workspace_bytes;  // the walk is ordered per thread (shift_cache_kernel): no bounce buffer
  KK_TRY(need("kk_csm_shift_caches", m, NEED_CACHES));
  const int P = m->bb.offset, mp = m->bb.max_pos;
  if (P + delta < 0 || P + delta > mp) return kk_fail("kk_csm_shift_caches: the position would leave the cache");
  for (int b = 0; b < m->max_batch; ++b)
    if (m->pad_host[b] < mp && m->pad_host[b] + delta < 0) return kk_fail("kk_csm_shift_caches: a live row's window would leave the cache");
  if (delta == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  KK_TRY(flush_pending(m, st));
  const kk_llama_args& a = m->bb.a;
  KK_TRY(kk_launch_csm_shift_cache(st, m->bb.kc, m->bb.vc, m->max_batch, mp, a.num_kv_heads * a.head_dim / 4, a.num_layers, m->bb.pos_dev, m->bb.pad_dev, delta));
  KK_TRY(kk_launch_csm_advance_pos(st, m->bb.pos_dev, delta));
  for (int b = 0; b < m->max_batch; ++b)
    if (m->pad_host[b] < mp) m->pad_host[b] += delta;
  m->bb.offset = P + delta;
  if (hipMemcpyAsync(m->bb.pad_dev, m->pad_host.data(), (size_t)m->max_batch * 4, hipMemcpyHostToDevice, st) != hipSuccess)
    return kk_fail("kk_csm_shift_caches: padding upload failed");
  return 0;
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
// The life of a prefix in the two entries that make one (kk_csm_prefix_create computes it, kk_csm_prefix_capture copies it out of a row): a new object of
// n positions on m's weight set with its buffer; then either published -- from here on the other entries accept the handle -- or discarded.
int prefix_new(const char* who, const kk_csm* m, int n, kk_csm_prefix** out) {
  kk_csm_prefix* p = new (std::nothrow) kk_csm_prefix();
  if (!p) return kk_failf("%s: out of memory", who);
  p->n = n; p->layers = m->bb.a.num_layers; p->kvw = m->bb.a.num_kv_heads * m->bb.a.head_dim; p->weights_id = m->weights_id;
  if (hipMalloc((void**)&p->buf, kk_csm_prefix_bytes_of(p)) != hipSuccess) {
    delete p;
    return kk_failf("%s: hipMalloc failed", who);
  }
  *out = p;
  return 0;
}
void prefix_publish(kk_csm_prefix* p) {
  std::lock_guard<std::mutex> lk(g_prefix_mu);
  g_prefixes.insert(p);
}
void prefix_discard(kk_csm_prefix* p, hipStream_t st) {
  (void)hipStreamSynchronize(st);  // nothing in flight may still write the buffer
  (void)hipFree(p->buf);
  delete p;
}

// The backbone seen through ONE run of slots per layer instead of its caches, with the slot offset as a launch constant instead of the device counter;
// restored on every way out.  Two users:
//   an admission   ONE row of the caches (layer pitch unchanged: max_batch rows) and that row's padding entry;
//   prefix_create  the prefix buffer as a one-row cache of its own (layer pitch 2 n KV hd, K in front of V), positions from 0, no padding: no cache
//                  row, counter or padding entry of the generator is read or written.
struct StackView {
  Stack& s;
  float *kc, *vc;
  int *pos, *pad;
  int off;
  size_t lp;
  StackView(Stack& st, float* k, float* v, int* pad_, int off_, size_t lp_)
      : s(st), kc(st.kc), vc(st.vc), pos(st.pos_dev), pad(st.pad_dev), off(st.offset), lp(st.layer_pitch) {
    s.kc = k; s.vc = v; s.pos_dev = nullptr; s.pad_dev = pad_; s.offset = off_; s.layer_pitch = lp_;
  }
  ~StackView() { s.kc = kc; s.vc = vc; s.pos_dev = pos; s.pad_dev = pad; s.offset = off; s.layer_pitch = lp; }
};
// the workspace of a block run by kk_csm_prefix_create / kk_csm_admit_prefixed: a one-row block takes the prompt path, whose scratch the S = 2 plan covers
size_t split_workspace_bytes(kk_csm* m, int S) { return kk_csm_workspace_bytes(m, 1, S < 2 ? 2 : S); }

// The prompt block of ONE new stream into the parked row `row`: the body of kk_csm_admit (`prefixed` false, `prefix` not read) and of
// kk_csm_admit_prefixed (the n positions of `prefix` are copied under the S new ones).  What the two entries do differently beside the copy must stay:
//   plain     workspace kk_csm_workspace_bytes(m, 1, S); run_frame(own_pos = S, split = false);
//   prefixed  workspace split_workspace_bytes(m, S);     run_frame(own_pos = n + S, split = true).
int admit_body(const char* who, kk_csm* m, void* stream, int row, bool prefixed, const kk_csm_prefix* prefix, int S, const int32_t* tokens,
               const float* tokens_mask, const kk_csm_sampler* sampler, const float* uniforms, int32_t stream_id, void* workspace, size_t workspace_bytes,
               int32_t* codes_out) {
  KK_TRY(need(who, m, NEED_FINAL | NEED_CACHES | NEED_ROW, row));
  if (prefixed && !prefix_live(prefix)) return kk_failf("%s: null or destroyed prefix", who);
  if (S <= 0 || !tokens || !tokens_mask || !sampler || !workspace || !codes_out) return kk_failf("%s: bad argument", who);
  const kk_llama_args& a = m->bb.a;
  const int P = m->bb.offset, mp = m->bb.max_pos, n = prefixed ? prefix->n : 0, kvw = a.num_kv_heads * a.head_dim;
  if (prefixed && (prefix->weights_id != m->weights_id || prefix->layers != a.num_layers || prefix->kvw != kvw))
    return kk_failf("%s: the prefix was computed with another weight set", who);
  if (m->pad_host[row] < mp) return kk_failf("%s: the row is live (kk_csm_park_row first)", who);
  if (n + S > P)
    return prefixed ? kk_failf("%s: prefix + suffix are longer than the cache position (kk_csm_shift_caches by n + S - P first)", who)
                    : kk_failf("%s: the prompt is longer than the cache position (kk_csm_shift_caches by S - P first)", who);
  if (workspace_bytes < (prefixed ? split_workspace_bytes(m, S) : kk_csm_workspace_bytes(m, 1, S))) return kk_failf("%s: workspace too small", who);
  hipStream_t st = (hipStream_t)stream;
  KKCsmSampleCfg sc;
  KK_TRY(kk_csm_sampler_cfg(sampler, &sc, who));
  const bool dev_rng = !uniforms && sampler->use_device_rng && sc.temp > 0.f;
  m->pad_host[row] = P - n - S;
  m->pad_pending = true;
  KK_TRY(flush_pending(m, st));
  if (dev_rng) {
    KK_TRY(upload_seed(m, sampler->seed, st));
    m->admit_sid_host = stream_id;
    if (hipMemcpyAsync(m->admit_sid_dev, &m->admit_sid_host, 4, hipMemcpyHostToDevice, st) != hipSuccess) return kk_failf("%s: stream id upload failed", who);
  }
  const size_t rs = (size_t)mp * kvw;  // floats of one cache row
  if (prefixed) {  // the prefix under the suffix: slots [P - n - S, P - S) of the row (0 <= P - n - S and P - S < max_pos: inside the row)
    const size_t at = row * rs + (size_t)(P - n - S) * kvw, seg = (size_t)n * kvw;
    KK_TRY(kk_launch_csm_kv_runs(prefix->buf, prefix->buf + seg, (long long)(2 * seg / 4), m->bb.kc + at, m->bb.vc + at, (long long)m->max_batch * mp * kvw / 4,
                                 (long long)(seg / 4), a.num_layers, st));
  }
  StackView view(m->bb, m->bb.kc + row * rs, m->bb.vc + row * rs, m->bb.pad_dev + row, P - S, m->bb.layer_pitch);
  Run r(m, st, 1, workspace, workspace_bytes);
  return run_frame(r, S, tokens, tokens_mask, sc, uniforms, dev_rng ? m->seed_dev : nullptr, dev_rng ? m->admit_sid_dev : nullptr, codes_out, n + S, prefixed);
}
}  // namespace

extern "C" int kk_csm_admit(kk_csm* m, void* stream, int row, int S, const int32_t* tokens, const float* tokens_mask, const kk_csm_sampler* sampler,
                            const float* uniforms, int32_t stream_id, void* workspace, size_t workspace_bytes, int32_t* codes_out) {
  return admit_body("kk_csm_admit", m, stream, row, false, nullptr, S, tokens, tokens_mask, sampler, uniforms, stream_id, workspace, workspace_bytes, codes_out);
}

extern "C" int kk_csm_admit_prefixed(kk_csm* m, void* stream, int row, const kk_csm_prefix* prefix, int S, const int32_t* tokens,
                                     const float* tokens_mask, const kk_csm_sampler* sampler, const float* uniforms, int32_t stream_id,
                                     void* workspace, size_t workspace_bytes, int32_t* codes_out) {
  return admit_body("kk_csm_admit_prefixed", m, stream, row, true, prefix, S, tokens, tokens_mask, sampler, uniforms, stream_id, workspace, workspace_bytes,
                    codes_out);
}

extern "C" int kk_csm_prefix_create(kk_csm* m, void* stream, int S, const int32_t* tokens, const float* tokens_mask, void* workspace,
                                    size_t workspace_bytes, kk_csm_prefix** out) {
  KK_TRY(need("kk_csm_prefix_create", m, NEED_FINAL));
  if (S <= 0 || !tokens || !tokens_mask || !workspace || !out) return kk_fail("kk_csm_prefix_create: bad argument");
  const kk_csm_config& c = m->cfg;
  const int kvw = m->bb.a.num_kv_heads * m->bb.a.head_dim, D = c.backbone.hidden;
  if (kvw % 4 != 0) return kk_fail("kk_csm_prefix_create: kv_heads * head_dim must be a multiple of 4");
  if (S >= m->bb.max_pos) return kk_fail("kk_csm_prefix_create: the prefix must leave room for a suffix below max_seq_len");
  if (c.audio_num_codebooks > 71) return kk_fail("kk_csm: more than 71 code books");
  if (workspace_bytes < split_workspace_bytes(m, S)) return kk_fail("kk_csm_prefix_create: workspace too small");
  kk_csm_prefix* p = nullptr;
  KK_TRY(prefix_new("kk_csm_prefix_create", m, S, &p));
  hipStream_t st = (hipStream_t)stream;
  int rc;
  {
    const size_t seg = (size_t)S * kvw;
    StackView view(m->bb, p->buf, p->buf + seg, nullptr, 0, 2 * seg);
    Run r(m, st, 1, workspace, workspace_bytes);
    float* h = r.f32((size_t)S * D);
    float* hn = r.f32((size_t)S * D);
    if (r.oom) rc = kk_fail("kk_csm_prefix_create: workspace too small");
    else {
      rc = kk_launch_csm_embed_sum(st, tokens, tokens_mask, m->audio_emb.p, m->text_emb.p, c.audio_num_codebooks, c.audio_vocab_size, c.text_vocab_size, D, S, h);
      if (rc != 0) rc = kk_fail("kk_csm_prefix_create: launch failed");
      r.lin_mode = Run::LIN_PROMPT;
      if (rc == 0) rc = stack_forward(r, m->bb, h, S, 0, hn);
    }
  }
  if (rc != 0) {
    prefix_discard(p, st);
    return rc;
  }
  prefix_publish(p);
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

// The first n positions of live row `row` as a new prefix: slots [pad[row], pad[row] + n) of every layer's K and V, one launch.  The row's window is
// [pad[row], P), so n <= P - pad[row] keeps the read inside it; the write goes to the new buffer alone.  P, pad, the frame-step graph and its key are
// untouched: legal between two frames of a running batch.
extern "C" int kk_csm_prefix_capture(kk_csm* m, void* stream, int row, int n, kk_csm_prefix** out) {
  KK_TRY(need("kk_csm_prefix_capture", m, NEED_FINAL));
  if (!out) return kk_fail("kk_csm_prefix_capture: bad argument");
  if (m->max_batch < 1 || !m->bb.kc || !m->bb.vc) return kk_fail("kk_csm_prefix_capture: call kk_csm_setup_caches first");
  KK_TRY(need("kk_csm_prefix_capture", m, NEED_ROW, row));
  const kk_llama_args& a = m->bb.a;
  const int P = m->bb.offset, mp = m->bb.max_pos, kvw = a.num_kv_heads * a.head_dim, pad = m->pad_host[row];
  if (pad >= mp) return kk_fail("kk_csm_prefix_capture: the row is parked");
  if (n < 1) return kk_fail("kk_csm_prefix_capture: n must be at least 1");
  if (pad < 0 || n > P - pad) return kk_fail("kk_csm_prefix_capture: the row holds fewer than n positions");
  if (kvw % 4 != 0) return kk_fail("kk_csm_prefix_capture: kv_heads * head_dim must be a multiple of 4");
  kk_csm_prefix* p = nullptr;
  KK_TRY(prefix_new("kk_csm_prefix_capture", m, n, &p));
  hipStream_t st = (hipStream_t)stream;
  int rc = flush_pending(m, st);
  if (rc == 0) {
    const size_t at = ((size_t)row * mp + (size_t)pad) * kvw, seg = (size_t)n * kvw;
    rc = kk_launch_csm_kv_runs(m->bb.kc + at, m->bb.vc + at, (long long)m->max_batch * mp * kvw / 4, p->buf, p->buf + seg, (long long)(2 * seg / 4),
                               (long long)(seg / 4), a.num_layers, st);
    if (rc != 0) rc = kk_fail("kk_csm_prefix_capture: launch failed");
  }
  if (rc != 0) {
    prefix_discard(p, st);
    return rc;
  }
  prefix_publish(p);
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
  KK_TRY(need("kk_csm_admit_transfer", m, NEED_ROW, row));
  if (src_row < 0 || src_row >= src->max_batch) return kk_fail("kk_csm_admit_transfer: source row out of range");
  const kk_llama_args &a = m->bb.a, &sa = src->bb.a;
  const int P = m->bb.offset, mp = m->bb.max_pos, smp = src->bb.max_pos, kvw = a.num_kv_heads * a.head_dim, spad = src->pad_host[src_row];
  if (m->pad_host[row] < mp) return kk_fail("kk_csm_admit_transfer: the row is live (kk_csm_park_row first)");
  if (spad >= smp) return kk_fail("kk_csm_admit_transfer: the source row is parked");
  const int L = src->bb.offset - spad;
  if (spad < 0 || L < 1) return kk_fail("kk_csm_admit_transfer: the source row holds no position");
  if (L > P) return kk_failf("kk_csm_admit_transfer: the admission is longer than the cache position (kk_csm_shift_caches by %d first)", L - P);
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
    KK_TRY(kk_launch_csm_kv_runs(src->bb.kc + sat, src->bb.vc + sat, (long long)src->max_batch * smp * kvw / 4, m->bb.kc + at, m->bb.vc + at,
                                 (long long)m->max_batch * mp * kvw / 4, (long long)L * kvw / 4, a.num_layers, st));
  }
  if (hipEventRecord(m->xfer_done, st) != hipSuccess || hipStreamWaitEvent(sst, m->xfer_done, 0) != hipSuccess)
    return kk_fail("kk_csm_admit_transfer: could not order the source stream behind the copy");
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
