// Whisper, text side (gfx950): the text decoder behind a handle -- weights, the caller-owned state layouts (window, beam, rows) and the kk_whisper_text_*
// entry points.  Its kernels and their launchers are kk_whisper_text_kernels.hip (declared in kk_kernels.h); nothing here is device code.  Restates
// TextDecoder (mlx_audio/stt/models/whisper/whisper.py:202-248, blocks :140-168, attention :90-137); DESIGN 8g.
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
//   A row picks greedily unless rows_set_draw gave it a draw after its admission; the round's one pick launch serves both kinds.
//   Groups (rows_groups_bind, rows_admit_group): G >= 1 rows on their leader's cross K/V that are admitted, stepped, picked and released together --
//   a beam group (top-k in the same pick launch, one select workgroup per group, the step's self keys through the group's owner table) or a plain one.
//   A single row is the plain group of one: the same items, launches and values.  There is ONE admission (rows_admit_check, rows_admit_body) behind two
//   entries: rows_admit_group, and rows_admit -- one row in no group, on a handle with or without the groups buffer, admitted over without a release.  The
//   serving code binds the buffer when it opens row mode and admits every request as a group; rows of no group come from rows_admit alone.
#include "kk_host.h"
#include "kk_philox.h"
#include "../../include/kokoro_hip.h"

#include <math.h>

// ================================================================================================================================ the handle
enum { TW_BF16 = 0, TW_Q8 = 8, TW_Q4 = 4 };  // a matrix's storage; the packed ones by their bits
struct TLin {  // a Linear: bf16 [N][K] dense at `w` of wdev, or (fmt != TW_BF16) the checkpoint's words at `qw` of qdev with its (scale, bias)
               // pairs at `qp` of pdev, quantised in groups of `group`; fp32 bias [N] at `b` of fdev
  size_t w = 0, b = 0, qw = 0, qp = 0;
  int N = 0, K = 0, fmt = TW_BF16, group = 0;
  bool bias = false;
};
struct TLayer {
  TLin q, k, v, out, cq, ckv, cout, mlp1, mlp2;
  size_t attn_ln_w = 0, attn_ln_b = 0, cross_ln_w = 0, cross_ln_b = 0, mlp_ln_w = 0, mlp_ln_b = 0;
};

struct kk_whisper_text {
  kk_whisper_text_config cfg;
  std::map<std::string, HostTensor> host;
  std::map<std::string, QuantHost> qhost;
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
    int group = -1, slot = 0;  // the group it belongs to (by its leader row) and its slot there; -1: a single row
    int at = 0;          // positions it holds: pos + count of its last round
  };
  char* rows_state = nullptr;
  std::vector<Row> rows;
  const float* rows_logits = nullptr;  // the last rows_forward's logits_out
  // groups of row mode (rows_groups_bind): G rows admitted and retired together on the leader's cross K/V; a group is known by its leader row
  struct Group {
    bool live = false;
    int kind = 0, G = 0, rows[KK_WHISPER_MAX_GROUP] = {0};
    int max_candidates = 0, flip = 0, picks = 0, begin = 0;  // beam: finished sequences kept, the current owner table, selects so far, the first sampled position
  };
  char* groups_state = nullptr;
  std::vector<Group> groups;  // [max_rows], by leader row
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
  p.scratch = (float*)ws.raw(kk_whisper_attn_scratch_floats((int)R, c.n_text_head, Tmax) * 4);
  p.item = (int*)ws.raw(R * 4);
  p.posr = (int*)ws.raw(R * 4);
  p.len_self = (int*)ws.raw(R * 4);
  p.len_cross = (int*)ws.raw(R * 4);
  p.cache_row = (int*)ws.raw(R * 4);
  p.feat = (bf16_t*)ws.raw((size_t)B * c.n_audio_ctx * D * 2);  // set_audio only
  p.item_cross = (int*)ws.raw(R * 4);
}
void bind(Workspace& ws, void* mem, size_t bytes) {
  ws.base = (char*)(((uintptr_t)mem + 255) & ~(uintptr_t)255);
  const size_t skip = (size_t)(ws.base - (char*)mem);
  ws.cap = bytes > skip ? bytes - skip : 0;
}
// the window's state buffer as set_audio laid it out.  A handle without one -- or, for the entries that need more than the state, with !ok -- is refused
// in the entry's own words
int window_bound(const char* who, const kk_whisper_text* m, TextState& s, const char* first = "set_audio first", bool ok = true) {
  if (!m->state || !ok) return kk_failf("%s: %s", who, first);
  Workspace ss;
  bind(ss, m->state, (size_t)-1 / 2);
  plan_state(m->cfg, m->n_audio, m->B, ss, s);
  return 0;
}
// the beam state of a handle whose `beam` is set (beam_setup sized and checked it)
void beam_bufs(const kk_whisper_text* m, kk_whisper_beam_bufs& bb) {
  Workspace bs;
  bind(bs, m->beam_state, (size_t)-1 / 2);
  plan_beam(m->cfg, m->n_audio, m->n_group, m->beam_cands, bs, bb);
}
int beam_bound(const char* who, const kk_whisper_text* m, kk_whisper_beam_bufs& bb) {
  if (!m) return kk_failf("%s: null model", who);
  if (!m->state || !m->beam) return kk_failf("%s: no beam: kk_whisper_text_beam_setup first", who);
  beam_bufs(m, bb);
  return 0;
}
// whisper.py:114-116, once per window: `n` windows of fp32 features are rounded to bf16 once (into feat), then key | value of every layer on the bf16 MFMA
// kernel, into windows slot0 .. slot0 + n - 1 of the layer's `slots` in the cross store
int project_cross(const kk_whisper_text* m, hipStream_t st, const float* features, int n, bf16_t* feat, bf16_t* cross, int slots, int slot0) {
  const kk_whisper_text_config& c = m->cfg;
  const int D = c.n_text_state, ctx = c.n_audio_ctx;
  KK_TRY(kk_launch_convert(features, KK_F32, (long long)ctx * D, D, feat, KK_BF16, (long long)ctx * D, D, D, ctx, n, st));
  for (int li = 0; li < c.n_text_layer; ++li) {
    const TLin& l = m->layers[li].ckv;
    KKMfmaArgs g;
    memset(&g, 0, sizeof g);
    g.x = feat; g.xbs = (long long)ctx * D; g.ldx = D; g.w = m->wdev + l.w; g.CinP = D; g.CoutP = 2 * D; g.Cin = D;
    g.bias = m->fdev + l.b; g.out = cross + ((size_t)li * slots + slot0) * ctx * 2 * D; g.obs = (long long)ctx * 2 * D; g.ldo = 2 * D;
    g.Cout = 2 * D; g.Kw = 1; g.mode = KK_CONV; g.stride = 1; g.pad = 0; g.dil = 1; g.Q = ctx; g.Lo_rows = ctx;
    g.lin = KKLen{nullptr, 0, ctx}; g.lout = KKLen{nullptr, 0, ctx};
    g.in_slope = 1.0f; g.scale = 1.0f; g.act = KK_ACT_NONE;
    KK_TRY(kk_launch_conv_mfma(g, n, KK_BF16, st));
  }
  return 0;
}
inline size_t mask_words(const kk_whisper_text_config& c) { return ((size_t)c.n_vocab + 31) / 32; }
// a pick's parameters against the model, and their upload with the suppress bitmask (null: nothing suppressed); NOT synchronised: the caller
// synchronises the stream before it returns, the host arrays may go away then
int check_pick_params(const char* who, const kk_whisper_text_config& c, const kk_whisper_pick_params* params) {
  if (params->n_vocab != c.n_vocab) return kk_failf("%s: params.n_vocab differs from the model's", who);
  if (params->eot < 0 || params->eot >= c.n_vocab || params->timestamp_begin < 0 || params->timestamp_begin > c.n_vocab)
    return kk_failf("%s: token ids outside the vocabulary", who);
  return 0;
}
int upload_pick_params(const char* who, hipStream_t st, const kk_whisper_text_config& c, const kk_whisper_pick_params* params, const uint32_t* suppress,
                       kk_whisper_pick_params* dparams, uint32_t* dmask) {
  const size_t bytes = mask_words(c) * 4;
  if (hipMemcpyAsync(dparams, params, sizeof *params, hipMemcpyHostToDevice, st) != hipSuccess ||
      (suppress ? hipMemcpyAsync(dmask, suppress, bytes, hipMemcpyHostToDevice, st) : hipMemsetAsync(dmask, 0, bytes, st)) != hipSuccess)
    return kk_failf("%s: upload failed", who);
  return 0;
}
// The live prefixes of B rows that were read back (pick states, token stores [B][T]) into the caller's live_tokens [B][cap], live_sum and live_length.
// own: the rows' owner rows [B][T], or null.  A live beam's tokens lie where its ancestors wrote them: token i in the row that owns position begin + i;
// slot_of maps that owner row to its place among the B (-1: not one of them, the row keeps its own token, as it does without a table).
template <class SlotOf>
void live_prefixes(int B, int T, int n, int cap, int begin, const kk_whisper_pick_state* rows, const int32_t* tok, const int32_t* own, SlotOf slot_of,
                   int32_t* live_tokens, float* live_sum, int32_t* live_length) {
  for (int b = 0; b < B; ++b) {
    const int len = rows[b].count < 0 ? 0 : (rows[b].count < n ? rows[b].count : n);
    live_sum[b] = rows[b].sum_logprob;
    live_length[b] = len;
    for (int i = 0; i < len; ++i) {
      const int o = own && begin + i < T ? slot_of(own[(size_t)b * T + begin + i]) : b;
      live_tokens[(size_t)b * cap + i] = tok[(size_t)(o < 0 ? b : o) * T + i];
    }
  }
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
  KK_TRY(kk_host_load_tensor("kk_whisper_text_load_tensor", m ? &m->host : nullptr, m && m->finalized, name, shape, ndim, data));
  m->qhost.erase(name);
  return 0;
}

extern "C" int kk_whisper_text_load_quantized(kk_whisper_text* m, const char* name, const int64_t* shape, const uint32_t* words, const float* scales,
                                              const float* biases, int group_size, int bits) {
  KK_TRY(kk_host_load_quantized("kk_whisper_text_load_quantized", m ? &m->qhost : nullptr, m && m->finalized, name, shape, words, scales, biases, group_size, bits));
  m->host.erase(name);
  return 0;
}

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
      const QuantHost& t = it->second;
      if (const char* why = kk_whisper_q_refusal(K, t.group, t.bits)) {
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
  std::vector<float> fpack(fn, 0.f);
  auto vecp = [&](size_t off, const std::string& name, int n) {
    if (const HostTensor* t = kk_host_want(m->host, name, {n}, err)) memcpy(&fpack[off], t->d.data(), (size_t)n * 4);
  };
  struct Job { const TLin* l; std::string name; int row0, N; };
  std::vector<Job> jobs;
  auto needw = [&](const std::string& name, int N, int K) {  // a matrix: as floats, or quantised
    const auto it = m->qhost.find(name);
    if (it == m->qhost.end()) kk_host_want(m->host, name, {N, K}, err);
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
  if (const HostTensor* t = kk_host_want(m->host, "decoder.positional_embedding", {c.n_text_ctx, D}, err)) memcpy(&fpack[m->pos], t->d.data(), t->d.size() * 4);
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
      const QuantHost& t = qi->second;
      const size_t np = t.scales.size();
      pairs.resize(2 * np);
      for (size_t i = 0; i < np; ++i) { pairs[2 * i] = t.scales[i]; pairs[2 * i + 1] = t.biases[i]; }
      ok = hipMemcpyAsync(m->qdev + j.l->qw, t.words.data(), t.words.size() * 4, hipMemcpyHostToDevice, st) == hipSuccess &&
           hipMemcpyAsync(m->pdev + j.l->qp, pairs.data(), np * sizeof(float2), hipMemcpyHostToDevice, st) == hipSuccess;
    } else {
      if (qi != m->qhost.end()) dequantize_host(qi->second, deq);
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
  const int B = n_audio * n_group;
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
  KK_TRY(project_cross(m, st, audio_features, n_audio, p.feat, s.cross, n_audio, 0));
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
      KKLinRows a{x + (long long)r0 * ldx, ldx, m->wdev + l.w + (size_t)n0 * l.K, l.bias ? m->fdev + l.b + n0 : nullptr, res ? res + (long long)r0 * ldo : nullptr, ldo,
                out ? out + (long long)r0 * ldo : nullptr, ldo, ob, 2 * D, dst ? dst + r0 : nullptr, items * m->cfg.n_text_ctx, rows - r0 < 16 ? rows - r0 : 16, N, l.K,
                act};
      if (l.fmt == TW_BF16) {
        KK_TRY(kk_launch_whisper_linear_rows(st, a));
      } else {  // the matrix stayed packed: the same product, the B fragments decoded in registers
        a.w = nullptr;
        KK_TRY(kk_launch_whisper_linear_rows_q(st, a, m->qdev + l.qw + (size_t)n0 * (l.K / 32 * l.fmt), m->pdev + l.qp + (size_t)n0 * (l.K / l.group), l.group, l.fmt));
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
      // causal: row (b, s) sees pos + s + 1 keys
      KK_TRY(kk_launch_whisper_attn_rows(st, owner != nullptr, R, H, p.q, selfc, 0, D, items, c.n_text_ctx, 2 * D, owner ? owner : p.item, p.len_self, p.att, p.scratch));
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
      KK_TRY(kk_launch_whisper_attn_rows(st, false, R, H, p.q, crossc, 0, D, items_cross, c.n_audio_ctx, 2 * D, item_cross, p.len_cross, p.att, p.scratch));
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
      return kk_launch_whisper_embed_q(st, R, c.n_text_state, tok, posr, m->qdev + e.qw, m->pdev + e.qp, e.group, e.fmt, c.n_vocab, m->fdev + m->pos, c.n_text_ctx, p.x);
    return kk_launch_whisper_embed(st, R, c.n_text_state, tok, posr, m->wdev + e.w, c.n_vocab, m->fdev + m->pos, c.n_text_ctx, p.x);
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
  TextState s;
  KK_TRY(window_bound(who, m, s, "set_audio first, with the same B", B == m->B));
  const kk_whisper_text_config& c = m->cfg;
  if (m->at + S > c.n_text_ctx) return kk_failf("%s: position %d + %d tokens exceeds n_text_ctx = %d", who, m->at, S, c.n_text_ctx);
  const int D = c.n_text_state, V = c.n_vocab, R = B * S;
  hipStream_t st = (hipStream_t)stream;
  Workspace ws;
  bind(ws, workspace, workspace_bytes);
  TextWork p;
  plan_work(c, B, S, ws, p);
  if (ws.oom) return kk_failf("%s: workspace too small", who);
  if (cap && m->n_group != 1) return kk_failf("%s: the window was set with n_group = %d; the capturing forward runs on a plain set_audio state", who, m->n_group);
  int* item_cross = m->n_group > 1 ? p.item_cross : nullptr;  // n_group 1: the row's own slot, one table as before
  const int* owner = nullptr;
  if (m->beam && m->beam_picks > 0) {  // before the first select every row holds its own keys
    if (S != 1) return kk_failf("%s: a beam that has stepped takes one position at a time", who);
    kk_whisper_beam_bufs bb;
    beam_bufs(m, bb);
    owner = bb.owner[m->beam_flip];
  }
  if (!tokens) {  // the step after a pick: the tokens it chose
    if (S != 1) return kk_failf("%s: tokens may be null only for S = 1 (the tokens of the last pick)", who);
    tokens = s.next;
  }
  KK_TRY(kk_launch_whisper_text_rows(st, B, S, m->at, c.n_text_ctx, c.n_audio_ctx, m->n_group, p.item, item_cross, p.posr, p.len_self, p.len_cross, p.cache_row));
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
  const char* who = "kk_whisper_text_pick_setup";
  TextState s;
  KK_TRY(window_bound(who, m, s));
  KK_TRY(check_pick_params(who, m->cfg, params));
  KK_TRY(upload_pick_params(who, (hipStream_t)stream, m->cfg, params, suppress, s.params, s.suppress));
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return kk_failf("%s: stream sync failed", who);
  m->sampling = m->beam = false;
  m->picking = true;
  return kk_op_whisper_pick_reset(stream, m->B, s.rows, s.not_ended);
}

extern "C" int kk_whisper_text_sample_setup(kk_whisper_text* m, void* stream, float temperature, uint64_t seed, const uint32_t* streams) {
  const char* who = "kk_whisper_text_sample_setup";
  if (!m || !streams) return kk_failf("%s: null argument", who);
  TextState s;
  KK_TRY(window_bound(who, m, s));
  if (!(temperature > 0.f) || !std::isfinite(temperature) || !std::isfinite(1.0f / temperature))
    return kk_failf("%s: temperature must be finite and > 0 (temperature 0 is the greedy pick: leave this call out)", who);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(s.streams, streams, (size_t)m->B * 4, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return kk_failf("%s: upload failed", who);  // synchronised: the host array may go away
  m->sampling = true;
  m->temperature = temperature;
  m->seed = seed;
  return 0;
}

extern "C" int kk_whisper_text_pick(kk_whisper_text* m, void* stream) {
  if (!m) return kk_fail("kk_whisper_text_pick: null model");
  TextState s;
  KK_TRY(window_bound("kk_whisper_text_pick", m, s, "no logits: run forward first", m->last_logits != nullptr));
  if (m->beam) {
    kk_whisper_beam_bufs bb;
    beam_bufs(m, bb);
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
  TextState s;
  KK_TRY(window_bound("kk_whisper_text_not_ended", m, s));
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(out, s.not_ended, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return kk_fail("kk_whisper_text_not_ended: read failed");
  return 0;
}

extern "C" int kk_whisper_text_read(kk_whisper_text* m, void* stream, int32_t* tokens, int cap, kk_whisper_pick_state* rows) {
  if (!m || !tokens || !rows || cap < 1) return kk_fail("kk_whisper_text_read: bad argument");
  TextState s;
  KK_TRY(window_bound("kk_whisper_text_read", m, s));
  hipStream_t st = (hipStream_t)stream;
  const int n = cap < m->cfg.n_text_ctx ? cap : m->cfg.n_text_ctx;
  if (hipMemcpy2DAsync(tokens, (size_t)cap * 4, s.tokens, (size_t)m->cfg.n_text_ctx * 4, (size_t)n * 4, m->B, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(rows, s.rows, (size_t)m->B * sizeof *rows, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return kk_fail("kk_whisper_text_read: read failed");
  return 0;
}

// ---- beam search on a grouped window state ---------------------------------------------------------------------------------------------
extern "C" size_t kk_whisper_text_beam_state_bytes(const kk_whisper_text* m, int n_audio, int beam_size, int max_candidates) {
  if (!m || n_audio < 1 || beam_size < 1 || beam_size > KK_WHISPER_MAX_GROUP || max_candidates < 1 || max_candidates > KK_WHISPER_BEAM_FIN) return 0;
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
  if (max_candidates < 1 || max_candidates > KK_WHISPER_BEAM_FIN) return kk_failf("%s: max_candidates = %d is outside [1, %d]", who, max_candidates, KK_WHISPER_BEAM_FIN);
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
  TextState s;
  KK_TRY(window_bound(who, m, s));
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
  live_prefixes(B, T, n, cap, m->beam_begin, rows.data(), tok.data(), own.data(), [B](int o) { return o >= 0 && o < B ? o : -1; }, live_tokens, live_sum,
                live_length);  // the window's table names batch rows
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
  PickDraw* draws;                 // [max_rows]; inv_t 0: the row picks greedily (rows_admit), > 0: it samples (rows_set_draw).  Behind everything older
};
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
  s.draws = (PickDraw*)ws.raw((size_t)N * sizeof(PickDraw));
}
struct RowsWork {
  TextWork t;    // t.feat: ONE window (rows_admit)
  int32_t* tok;  // [R]
  int* own;      // [R][n_text_ctx]: the round's owner table (groups bound only)
};
void plan_rows_work(const kk_whisper_text_config& c, int R, bool groups, Workspace& ws, RowsWork& p) {
  plan_work(c, 1, R, ws, p.t);  // B = 1, S = R: R flat rows and one window of features
  p.tok = (int32_t*)ws.raw((size_t)R * 4);
  p.own = groups ? (int*)ws.raw((size_t)R * c.n_text_ctx * 4) : nullptr;
}
// the caller's second row-mode buffer: what groups keep beside the row state (kk_kernels.h: KKGroupBufs)
void plan_groups_state(const kk_whisper_text_config& c, int N, Workspace& ws, KKGroupBufs& g) {
  const size_t T = c.n_text_ctx, F = (size_t)N * KK_WHISPER_BEAM_FIN;
  g.cand_token = (int32_t*)ws.raw((size_t)N * KK_WHISPER_BEAM_C * 4);
  g.cand_logprob = (float*)ws.raw((size_t)N * KK_WHISPER_BEAM_C * 4);
  g.owner[0] = (int32_t*)ws.raw((size_t)N * T * 4);
  g.owner[1] = (int32_t*)ws.raw((size_t)N * T * 4);
  g.parent = (int32_t*)ws.raw((size_t)N * 4);
  g.fin_score = (float*)ws.raw(F * 4);
  g.fin_length = (int32_t*)ws.raw(F * 4);
  g.fin_tokens = (int32_t*)ws.raw(F * T * 4);
  g.fin_count = (int32_t*)ws.raw((size_t)N * 4);
  g.complete = (int32_t*)ws.raw((size_t)N * 4);
}
int groups_bound(const char* who, const kk_whisper_text* m, KKGroupBufs& g) {
  if (!m->groups_state) return kk_failf("%s: groups are not bound (kk_whisper_text_rows_groups_bind after rows_open)", who);
  Workspace gs;
  bind(gs, m->groups_state, (size_t)-1 / 2);
  plan_groups_state(m->cfg, (int)m->rows.size(), gs, g);
  return 0;
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
// One admission, behind rows_admit (one row) and rows_admit_group (rows[0] leads).  The checks both make of what is admitted, and the workspace:
int rows_admit_check(const char* who, const kk_whisper_text* m, int n, const kk_whisper_pick_params* params, void* workspace, size_t workspace_bytes, RowsWork& p) {
  const kk_whisper_text_config& c = m->cfg;
  if (n < 1 || n > c.n_text_ctx) return kk_failf("%s: %d initial tokens are outside [1, n_text_ctx = %d]", who, n, c.n_text_ctx);
  KK_TRY(check_pick_params(who, c, params));
  Workspace ws;
  bind(ws, workspace, workspace_bytes);
  plan_rows_work(c, 1, false, ws, p);
  if (ws.oom) return kk_failf("%s: workspace too small", who);
  return 0;
}
// and, everything checked, the admission: the window's cross K/V is projected ONCE (set_audio's launches with one window), into the leader's slices
// -- the other rows name them; every row gets the initial tokens, the pick parameters and bitmask, a reset pick state and no draw (greedy until
// rows_set_draw).  beam: the buffers of a beam group, whose tables are reset too, or null.  Synchronised once, at the end: the host arrays may go away.
int rows_admit_body(const char* who, kk_whisper_text* m, void* stream, const RowsState& s, const RowsWork& p, const int32_t* rows, int n_rows,
                    const float* audio_features, const int32_t* tokens, int n, const kk_whisper_pick_params* params, const uint32_t* suppress,
                    const KKGroupBufs* beam) {
  const kk_whisper_text_config& c = m->cfg;
  hipStream_t st = (hipStream_t)stream;
  for (int k = 0; k < n_rows; ++k) {  // a failure below leaves the rows unusable, not half new
    m->rows[rows[k]].admitted = false;
    m->rows[rows[k]].logit = -1;
  }
  KK_TRY(project_cross(m, st, audio_features, 1, p.t.feat, s.cross, (int)m->rows.size(), rows[0]));
  KKGroupRows gr;
  memset(&gr, 0, sizeof gr);
  for (int k = 0; k < n_rows; ++k) {
    const int row = gr.row[k] = rows[k];
    if (hipMemcpyAsync(s.init + (size_t)row * c.n_text_ctx, tokens, (size_t)n * 4, hipMemcpyHostToDevice, st) != hipSuccess) return kk_failf("%s: upload failed", who);
    KK_TRY(upload_pick_params(who, st, c, params, suppress, s.params + row, s.suppress + (size_t)row * mask_words(c)));
    if (hipMemsetAsync(s.draws + row, 0, sizeof(PickDraw), st) != hipSuccess) return kk_failf("%s: clearing the draw failed", who);
    KK_TRY(kk_op_whisper_pick_reset(stream, 1, s.rows + row, s.not_ended));
  }
  if (beam) KK_TRY(kk_launch_whisper_rows_group_reset(st, gr, n_rows, c.n_text_ctx, *beam));
  if (hipStreamSynchronize(st) != hipSuccess) return kk_failf("%s: stream sync failed", who);
  for (int k = 0; k < n_rows; ++k) {
    kk_whisper_text::Row& r = m->rows[rows[k]];
    r.admitted = true;
    r.n_init = n;
    r.at = 0;
  }
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
  plan_rows_work(m->cfg, max_round_rows, m->groups_state != nullptr, ws, p);
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
  if (hipMemsetAsync(s.draws, 0, (size_t)max_rows * sizeof(PickDraw), (hipStream_t)stream) != hipSuccess) return kk_failf("%s: clearing the draws failed", who);
  m->rows_state = (char*)state;
  m->rows.assign(max_rows, kk_whisper_text::Row());
  m->rows_logits = nullptr;
  m->groups_state = nullptr;  // groups are bound anew after every rows_open
  m->groups.clear();
  return 0;
}

extern "C" int kk_whisper_text_rows_admit(kk_whisper_text* m, void* stream, int row, const float* audio_features, const int32_t* tokens, int n,
                                          const kk_whisper_pick_params* params, const uint32_t* suppress, void* workspace, size_t workspace_bytes) {
  const char* who = "kk_whisper_text_rows_admit";
  RowsState s;
  KK_TRY(rows_bound(who, m, s));
  KK_TRY(rows_check_row(who, m, row, false));
  if (!audio_features || !tokens || !params || !workspace) return kk_failf("%s: null argument", who);
  RowsWork p;
  KK_TRY(rows_admit_check(who, m, n, params, workspace, workspace_bytes, p));
  if (m->rows[row].group >= 0) return kk_failf("%s: row %d belongs to the group led by row %d (kk_whisper_text_rows_group_release first)", who, row, m->rows[row].group);
  return rows_admit_body(who, m, stream, s, p, &row, 1, audio_features, tokens, n, params, suppress, nullptr);  // a single row: no group, bound or not
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
  KKRowItems t;
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
    t.cross[i] = it.row; t.own[i] = -1;
    R += it.count;
  }
  // groups: a group's rows step together at one position -- before its first pick the leader may run alone (its detection round)
  bool owned = false;
  for (int i = 0; i < n_items && m->groups_state; ++i) {
    const int lead = m->rows[items[i].row].group;
    if (lead < 0) continue;
    const kk_whisper_text::Group& g = m->groups[lead];
    int listed = 0;
    for (int k = 0; k < g.G; ++k) listed += seen >> g.rows[k] & 1u;
    const bool alone = listed == 1 && items[i].row == lead && g.picks == 0;
    if (listed != g.G && !alone)
      return kk_failf("%s: item %d: the group led by row %d is stepped partially (%d of its %d rows are in this round)", who, i, lead, listed, g.G);
    if (items[i].row != lead)
      for (int j = 0; j < n_items; ++j)
        if (items[j].row == lead && (items[j].pos != items[i].pos || items[j].count != items[i].count))
          return kk_failf("%s: item %d: row %d is at position %d + %d, its group's leader %d at %d + %d", who, i, items[i].row, items[i].pos, items[i].count, lead,
                          items[j].pos, items[j].count);
    t.cross[i] = lead;
    if (g.kind == KK_WHISPER_GROUP_BEAM && g.picks > 0) {
      if (items[i].from >= 0) return kk_failf("%s: item %d: row %d of a beam group is prefilled after the group's first select", who, i, items[i].row);
      t.own[i] = g.flip;  // the step reads its self keys through ITS owner row of the group's current table
      owned = true;
    }
  }
  Workspace ws;
  bind(ws, workspace, workspace_bytes);
  RowsWork p;
  plan_rows_work(c, (int)R, m->groups_state != nullptr, ws, p);
  if (ws.oom) return kk_failf("%s: workspace too small for R = %lld rows", who, R);
  if (n_out < 1 || n_out > 2 * n_items || n_out > R) return kk_failf("%s: n_out = %d is outside [1, min(2 n_items, R)]", who, n_out);
  std::vector<int> where((size_t)R, -1);  // flat row -> its row of logits_out
  bool identity = n_out == R;
  KKRowGather sel;
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
  int* item_cross = m->groups_state ? p.t.item_cross : nullptr;  // without groups every row reads its own slice: one table, as before
  KK_TRY(kk_launch_whisper_text_plan(st, t, (int)R, c.n_text_ctx, c.n_audio_ctx, s.init, s.next, p.t.item, item_cross, p.t.posr, p.t.len_self, p.t.len_cross,
                                     p.t.cache_row, p.tok));
  if (owned) {  // a round that steps a beam group: ONE more launch, however many groups, and the owned self-attention for every row (identity rows for the others)
    KKGroupBufs gb;
    KK_TRY(groups_bound(who, m, gb));
    KK_TRY(kk_launch_whisper_text_plan_owner(st, t, (int)R, c.n_text_ctx, gb.owner[0], gb.owner[1], p.own));
  }
  const TextPass run{m, st, N, N, s.self, s.cross, item_cross ? item_cross : p.t.item, p.t, owned ? p.own : nullptr};
  KK_TRY(run.embed((int)R, p.tok, p.t.posr));
  KK_TRY(run.layers((int)R, nullptr, 0, 0));
  const float* x = p.t.x;
  if (!identity) {  // a round of steps wants every row: nothing to gather
    KK_TRY(kk_launch_whisper_gather_rows(st, n_out, sel, p.t.x, D, p.t.q));
    x = p.t.q;
  }
  KK_TRY(run.logits(x, D, n_out, logits_out));
  for (int i = 0; i < n_items; ++i) {
    const kk_whisper_rows_item& it = items[i];
    kk_whisper_text::Row& r = m->rows[it.row];
    const int last = where[t.first[i] + it.count - 1];
    r.logit = last >= 0 ? last : -1;
    r.at = it.pos + it.count;
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
  KKPickSel sel;
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
  // groups: a group is picked whole; a beam group's rows offer their top-k in the same launch, and ONE select launch behind it serves
  // every listed beam group at its own position and flip
  KKGroupSel gsel;
  KKGroupBufs gb;
  memset(&gsel, 0, sizeof gsel);
  memset(&gb, 0, sizeof gb);
  int n_beam = 0;
  for (int j = 0; j < n && m->groups_state; ++j) {
    const int lead = m->rows[rows[j]].group;
    if (lead < 0) continue;
    const kk_whisper_text::Group& g = m->groups[lead];
    int listed = 0;
    for (int k = 0; k < g.G; ++k) listed += seen >> g.rows[k] & 1u;
    if (listed != g.G) return kk_failf("%s: the group led by row %d is picked partially (%d of its %d rows are listed)", who, lead, listed, g.G);
    if (g.kind != KK_WHISPER_GROUP_BEAM) continue;
    sel.topk[j] = g.G + 1;
    if (rows[j] != lead) continue;
    gsel.leader[n_beam] = lead; gsel.K[n_beam] = g.G; gsel.pos[n_beam] = m->rows[lead].at; gsel.flip[n_beam] = g.flip; gsel.max_candidates[n_beam] = g.max_candidates;
    for (int k = 0; k < g.G; ++k) {
      if (m->rows[g.rows[k]].at != m->rows[lead].at) return kk_failf("%s: row %d of the group led by row %d is at another position", who, g.rows[k], lead);
      gsel.rows[n_beam][k] = g.rows[k];
    }
    ++n_beam;
  }
  if (n_beam) KK_TRY(groups_bound(who, m, gb));
  const kk_whisper_text_config& c = m->cfg;
  KK_TRY(kk_launch_whisper_pick_rows((hipStream_t)stream, n, sel, m->rows_logits, (long long)c.n_vocab, s.params, s.suppress, (int)mask_words(c), s.draws, s.rows, s.tokens,
                                     c.n_text_ctx, s.next, gb.cand_token, gb.cand_logprob));
  if (n_beam) KK_TRY(kk_launch_whisper_rows_select((hipStream_t)stream, n_beam, gsel, gb, c.n_text_ctx, s.params, s.rows, s.tokens, s.next));
  for (int j = 0; j < n; ++j) m->rows[rows[j]].logit = -2;  // picked: the row can step on its token, and is not picked twice on the same logits
  for (int j = 0; j < n && m->groups_state; ++j) {
    const int lead = m->rows[rows[j]].group;
    if (lead != rows[j]) continue;
    kk_whisper_text::Group& g = m->groups[lead];
    if (g.picks++ == 0) g.begin = m->rows[lead].at;
    if (g.kind == KK_WHISPER_GROUP_BEAM) g.flip ^= 1;
  }
  return 0;
}

extern "C" int kk_whisper_text_rows_set_draw(kk_whisper_text* m, void* stream, int row, float temperature, uint64_t seed, uint32_t stream_id) {
  const char* who = "kk_whisper_text_rows_set_draw";
  const float inv_t = 1.0f / temperature;
  if (!(temperature > 0.f) || !std::isfinite(temperature) || !std::isfinite(inv_t))
    return kk_failf("%s: temperature must be finite and > 0 (a row picks greedily from its admission on: leave this call out)", who);
  RowsState s;
  KK_TRY(rows_bound(who, m, s));
  KK_TRY(rows_check_row(who, m, row, true));
  const PickDraw dr{inv_t, seed, stream_id};
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(s.draws + row, &dr, sizeof dr, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return kk_failf("%s: upload failed", who);  // synchronised: dr goes away
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

// ---- groups of row mode ---------------------------------------------------------------------------------------------------------------
// G rows, not necessarily adjacent, admitted and retired together on ONE cross K/V slice (the leader's, rows[0]): a beam group (G = beam_size: per-row
// top-k in the round's pick launch, one select workgroup per group, the step's self keys through the group's owner table) or a plain group (best_of:
// every row picks or draws for itself).  What they keep lives in a second caller-owned buffer; without the bind call row mode is what it was.
extern "C" size_t kk_whisper_text_rows_groups_state_bytes(const kk_whisper_text* m, int max_rows) {
  if (!m || max_rows < 1 || max_rows > KK_WHISPER_MAX_ROWS) return 0;
  Workspace ws;
  KKGroupBufs g;
  plan_groups_state(m->cfg, max_rows, ws, g);
  return ws.used + 256;
}

extern "C" int kk_whisper_text_rows_groups_bind(kk_whisper_text* m, void* stream, void* state, size_t state_bytes) {
  const char* who = "kk_whisper_text_rows_groups_bind";
  (void)stream;
  RowsState s;
  KK_TRY(rows_bound(who, m, s));
  if (!state) return kk_failf("%s: null argument", who);
  Workspace gs;
  bind(gs, state, state_bytes);
  KKGroupBufs g;
  plan_groups_state(m->cfg, (int)m->rows.size(), gs, g);
  if (gs.oom) return kk_failf("%s: state buffer too small", who);
  for (const auto& r : m->rows)
    if (r.group >= 0) return kk_failf("%s: a group is live", who);
  m->groups_state = (char*)state;  // nothing is launched: an admission resets what its group reads
  m->groups.assign(m->rows.size(), kk_whisper_text::Group());
  return 0;
}

extern "C" int kk_whisper_text_rows_admit_group(kk_whisper_text* m, void* stream, const int32_t* rows, int n_rows, int kind, const float* audio_features,
                                                const int32_t* tokens, int n, const kk_whisper_pick_params* params, const uint32_t* suppress, int max_candidates,
                                                void* workspace, size_t workspace_bytes) {
  const char* who = "kk_whisper_text_rows_admit_group";
  RowsState s;
  KK_TRY(rows_bound(who, m, s));
  KKGroupBufs gb;
  KK_TRY(groups_bound(who, m, gb));
  if (!rows || !audio_features || !tokens || !params || !workspace) return kk_failf("%s: null argument", who);
  if (n_rows < 1 || n_rows > KK_WHISPER_MAX_GROUP) return kk_failf("%s: a group of %d rows is outside [1, %d]", who, n_rows, KK_WHISPER_MAX_GROUP);
  if (kind != KK_WHISPER_GROUP_PLAIN && kind != KK_WHISPER_GROUP_BEAM) return kk_failf("%s: kind = %d is neither plain (0) nor beam (1)", who, kind);
  if (kind == KK_WHISPER_GROUP_BEAM && (max_candidates < 1 || max_candidates > KK_WHISPER_BEAM_FIN))
    return kk_failf("%s: max_candidates = %d is outside [1, %d]", who, max_candidates, KK_WHISPER_BEAM_FIN);
  unsigned seen = 0;
  for (int k = 0; k < n_rows; ++k) {
    KK_TRY(rows_check_row(who, m, rows[k], false));
    if (seen >> rows[k] & 1u) return kk_failf("%s: row %d is listed twice", who, rows[k]);
    seen |= 1u << rows[k];
    if (m->rows[rows[k]].group >= 0) return kk_failf("%s: row %d is already in the group led by row %d", who, rows[k], m->rows[rows[k]].group);
  }
  RowsWork p;
  KK_TRY(rows_admit_check(who, m, n, params, workspace, workspace_bytes, p));
  KK_TRY(rows_admit_body(who, m, stream, s, p, rows, n_rows, audio_features, tokens, n, params, suppress, kind == KK_WHISPER_GROUP_BEAM ? &gb : nullptr));
  const int lead = rows[0];
  kk_whisper_text::Group& g = m->groups[lead];
  g = kk_whisper_text::Group();
  g.live = true;
  g.kind = kind;
  g.G = n_rows;
  g.max_candidates = kind == KK_WHISPER_GROUP_BEAM ? max_candidates : 0;
  for (int k = 0; k < n_rows; ++k) {
    g.rows[k] = rows[k];
    m->rows[rows[k]].group = lead;
    m->rows[rows[k]].slot = k;
  }
  return 0;
}

extern "C" int kk_whisper_text_rows_group_release(kk_whisper_text* m, int leader) {
  const char* who = "kk_whisper_text_rows_group_release";
  if (!m) return kk_failf("%s: null model", who);
  if (!m->rows_state || !m->groups_state) return kk_failf("%s: groups are not bound (kk_whisper_text_rows_groups_bind after rows_open)", who);
  if (leader < 0 || leader >= (int)m->groups.size() || !m->groups[leader].live) return kk_failf("%s: row %d leads no group", who, leader);
  kk_whisper_text::Group& g = m->groups[leader];
  for (int k = 0; k < g.G; ++k) {
    m->rows[g.rows[k]].group = -1;
    m->rows[g.rows[k]].admitted = false;  // its cross K/V is the leader's: a released row is admitted anew before it runs again
    m->rows[g.rows[k]].logit = -1;
  }
  g.live = false;
  return 0;
}

extern "C" int kk_whisper_text_rows_group_read(kk_whisper_text* m, void* stream, int leader, int cap, int32_t* fin_count, float* fin_score, int32_t* fin_length,
                                               int32_t* fin_tokens, int32_t* live_tokens, float* live_sum, int32_t* live_length, float* kept) {
  const char* who = "kk_whisper_text_rows_group_read";
  RowsState s;
  KK_TRY(rows_bound(who, m, s));
  KKGroupBufs gb;
  KK_TRY(groups_bound(who, m, gb));
  if (leader < 0 || leader >= (int)m->groups.size() || !m->groups[leader].live) return kk_failf("%s: row %d leads no group", who, leader);
  if (!fin_count || !fin_score || !fin_length || !fin_tokens || !live_tokens || !live_sum || !live_length || cap < 1) return kk_failf("%s: bad argument", who);
  const kk_whisper_text::Group& g = m->groups[leader];
  const kk_whisper_text_config& c = m->cfg;
  hipStream_t st = (hipStream_t)stream;
  const int T = c.n_text_ctx, n = cap < T ? cap : T, G = g.G, F = g.max_candidates;
  const bool beam = g.kind == KK_WHISPER_GROUP_BEAM;
  std::vector<int32_t> tok((size_t)G * T), own((size_t)G * T);
  std::vector<kk_whisper_pick_state> rows(G);
  bool ok = true;
  *fin_count = 0;
  if (beam)
    ok = hipMemcpyAsync(fin_count, gb.fin_count + leader, 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
         hipMemcpyAsync(fin_score, gb.fin_score + (size_t)leader * KK_WHISPER_BEAM_FIN, (size_t)F * 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
         hipMemcpyAsync(fin_length, gb.fin_length + (size_t)leader * KK_WHISPER_BEAM_FIN, (size_t)F * 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
         hipMemcpy2DAsync(fin_tokens, (size_t)cap * 4, gb.fin_tokens + (size_t)leader * KK_WHISPER_BEAM_FIN * T, (size_t)T * 4, (size_t)n * 4, F, hipMemcpyDeviceToHost,
                          st) == hipSuccess;
  for (int k = 0; k < G && ok; ++k) {
    const int row = g.rows[k];
    ok = hipMemcpyAsync(tok.data() + (size_t)k * T, s.tokens + (size_t)row * T, (size_t)T * 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
         hipMemcpyAsync(rows.data() + k, s.rows + row, sizeof(kk_whisper_pick_state), hipMemcpyDeviceToHost, st) == hipSuccess &&
         (!beam || hipMemcpyAsync(own.data() + (size_t)k * T, gb.owner[g.flip] + (size_t)row * T, (size_t)T * 4, hipMemcpyDeviceToHost, st) == hipSuccess);
  }
  if (ok && kept) ok = hipMemcpyAsync(kept, s.kept + (size_t)leader * 2 * c.n_vocab, (size_t)2 * c.n_vocab * 4, hipMemcpyDeviceToDevice, st) == hipSuccess;
  if (!ok || hipStreamSynchronize(st) != hipSuccess) return kk_failf("%s: read failed", who);
  const auto slot_of = [&g](int o) {  // the group's table names decoder rows: the slot is the row's place in the group's list
    int slot = -1;
    for (int q = 0; q < g.G; ++q)
      if (g.rows[q] == o) slot = q;
    return slot;
  };
  live_prefixes(G, T, n, cap, g.begin, rows.data(), tok.data(), beam && g.picks > 0 ? own.data() : nullptr, slot_of, live_tokens, live_sum, live_length);
  return 0;
}

extern "C" int kk_whisper_text_rows_group_offers(kk_whisper_text* m, void* stream, int row, int32_t* token, float* logprob) {
  const char* who = "kk_whisper_text_rows_group_offers";
  RowsState s;
  KK_TRY(rows_bound(who, m, s));
  KKGroupBufs gb;
  KK_TRY(groups_bound(who, m, gb));
  KK_TRY(rows_check_row(who, m, row, true));
  if (!token || !logprob) return kk_failf("%s: null argument", who);
  const int lead = m->rows[row].group;
  if (lead < 0 || m->groups[lead].kind != KK_WHISPER_GROUP_BEAM || m->groups[lead].picks == 0) return kk_failf("%s: row %d has no offers (a beam row after its pick)", who, row);
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)m->groups[lead].G + 1;
  if (hipMemcpyAsync(token, gb.cand_token + (size_t)row * KK_WHISPER_BEAM_C, n * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(logprob, gb.cand_logprob + (size_t)row * KK_WHISPER_BEAM_C, n * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return kk_failf("%s: read failed", who);
  return 0;
}
