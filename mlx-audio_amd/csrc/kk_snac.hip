// SNAC codec (mlx_audio/codec/models/snac/{snac,layers,vq}.py): encode, decode, the multi-rate residual VQ.
//   decode: codes_i [B][T / stride_i] -> from_codes (gather-sum over out_proj(codebook) tables) -> depth-wise k7 -> 1x1 ->
//           n x {Snake, transposed conv k = 2s, NoiseBlock, 3 residual units dil 1 / 3 / 9} -> Snake, conv k7 to one channel, tanh
//   encode: pcm [B][N] -> conv k7 -> n x {3 residual units, Snake, strided conv k = 2s} -> depth-wise k7 ->
//           per quantiser {average pool, in_proj, cosine search, out_proj, repeat, residual update}
// Host orchestration + the kernels that exist only here (kk_snac_kernels.h).  Dense convolutions (1x1, strided, transposed) are the library's
// generic fp32 kernel (kk_conv.hip) and, for bf16 activations, the variant-4 matrix-core kernel (kk_conv_mfma4.hip).  Activations are
// frames-major channels-last [B][L][ld]; the encoder always runs in fp32 (the code-book search is an argmax).
//
// Reference semantics restated as written (file:line relative to mlx_audio/codec/models/snac/):
//   layers.py:105-121   WNConvTranspose1d never passes output_padding: Lout = (L - 1) s - 2 ceil(s / 2) + 2 s (= L s for even s, L s - 1 for odd)
//   layers.py:261-267   NoiseBlock unpacks B, C, T from a channels-last tensor: its noise is [B][1][C], one normal per item and channel
//   layers.py:226-231   ResidualUnit's crop compares channel counts: a no-op
//   layers.py:124-130   snake(x) = x + sin^2(alpha x) / (alpha + 1e-9)
//   layers.py:9-14,57   weight norm g v / |v| over the axes except 0 (folded at finalize in float64)
//   vq.py:23-54,62-77   average pool, in_proj, L2-normalised search argmax(-dist), z_e + (z_q - z_e), out_proj, repeat-interleave
//   vq.py:97-129        residual update and from_codes (quantisers added in ascending order)
#include <math.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/kokoro_hip.h"
#include "kk_common.h"
#include "kk_kernels.h"
#include "kk_host.h"
#include "kk_snac_kernels.h"

namespace {

struct PackedConv {  // generic-kernel pack [K][Cin][ldw] fp32 (+ bias); bf16 decode: the variant-4 fragment pack as well
  size_t w_off = 0, b_off = 0, wf_off = 0;
  bool has_bias = false, mfma = false;
  int Cin = 0, Cout = 0, K = 0, ldw = 0, CinP = 0, CoutP = 0;
  const float* w = nullptr;
  const float* b = nullptr;  // [CoutP] when mfma (zero padded), else [Cout]
  const bf16_t* wf = nullptr;
};
struct DwConv {  // depth-wise k7: w [C][7], b [C]
  ArenaVec w, b;
  int C = 0;
};
struct Unit {  // ResidualUnit (layers.py:208-231)
  ArenaVec a1, a2;
  DwConv dw;
  PackedConv pw;
  int dil = 1;
};
struct DecBlock {  // DecoderBlock (layers.py:270-297)
  ArenaVec alpha;
  PackedConv up, nz;
  Unit u[3];
  int stride = 1, Cin = 0, Cout = 0;
};
struct EncBlock {  // EncoderBlock (layers.py:234-253)
  Unit u[3];
  ArenaVec alpha;
  PackedConv down;
  int stride = 1, Cin = 0, Cout = 0;
};
struct Quant {  // VectorQuantize (vq.py:10-77)
  PackedConv in_proj, out_proj;
  ArenaVec cb, cbn, c2, table;  // code book [bins][cd], its rows L2-normalised, their squared norms, out_proj(code book) [bins][D] without bias
  int stride = 1;
};

}  // namespace

struct kk_snac {
  kk_snac_config cfg;
  WeightArena arena;
  bool finalized = false;
  int adt = KK_F32;  // activation dtype of DECODE
  int D = 0;         // latent_dim
  DwConv dec_dw, enc_last;
  PackedConv dec_pw, dec_last, enc_first;
  ArenaVec dec_alpha, bias_sum;
  std::vector<DecBlock> dec;
  std::vector<EncBlock> enc;
  std::vector<Quant> vq;
  DebugNotes dbg;
  std::mutex dbg_mu;
};

namespace {

struct Act {  // an activation tensor [B][rows][ld], C valid channels, dense
  void* p = nullptr;
  int rows = 0, C = 0, ld = 0, dtype = KK_F32;
  long long bs() const { return (long long)rows * ld; }
};
int pitch_of(int C, int dtype) { return dtype == KK_BF16 ? rup(C, 64) : C; }  // bf16 tensors can feed the matrix-core kernel
size_t esize(int dtype) { return dtype == KK_BF16 ? 2 : 4; }

// every dense convolution of the codec: the matrix-core kernel for bf16 tensors with a fragment pack and an eligible shape, else the generic one
int snac_conv(hipStream_t st, int B, const PackedConv& w, const Act& x, const Act& out, int pad, bool transposed, int stride, const Act* res, int* path) {
  const int Lin = x.rows, Lout = out.rows;
  if (w.mfma && x.dtype == KK_BF16 && out.dtype == KK_BF16 && x.ld >= w.CinP && kk_mfma_eligible(w.Cin, w.Cout, w.K, transposed ? KK_CONVT : KK_CONV, stride, 1)) {
    KKMfmaArgs g;
    memset(&g, 0, sizeof g);
    g.x = (const bf16_t*)x.p; g.xbs = x.bs(); g.ldx = x.ld; g.wf = w.wf; g.CinP = w.CinP; g.Cin = w.Cin; g.CoutP = w.CoutP; g.bias = w.b;
    g.out = out.p; g.obs = out.bs(); g.ldo = out.ld;
    if (res) { g.res = res->p; g.rbs = res->bs(); g.ldr = res->ld; }
    g.Cout = w.Cout; g.Kw = w.K; g.mode = transposed ? KK_CONVT : KK_CONV; g.stride = stride; g.pad = pad; g.dil = 1;
    g.Q = transposed ? kk_cdiv(Lout, stride) : Lout; g.Lo_rows = Lout;
    g.lin = KKLen{nullptr, 0, Lin}; g.lout = KKLen{nullptr, 0, Lout};
    g.in_slope = 1.f; g.scale = 1.f;
    g.slabwise = 1;
    if (path) *path = KK_SNAC_UNIT_MFMA;
    return kk_launch_conv_mfma4(g, B, KK_BF16, st);
  }
  KKConvArgs a;
  memset(&a, 0, sizeof a);
  a.x = x.p; a.xbs = x.bs(); a.ldx = x.ld;
  a.w = w.w; a.ldw = w.ldw; a.bias = w.b;
  a.out = out.p; a.obs = out.bs(); a.ldo = out.ld;
  if (res) { a.res = res->p; a.rbs = res->bs(); a.ldr = res->ld; }
  a.Cin = w.Cin; a.Cout = w.Cout; a.Kw = w.K;
  a.mode = transposed ? KK_CONVT : KK_CONV; a.stride = stride; a.pad = pad; a.dil = 1;
  a.Q = transposed ? kk_cdiv(Lout, stride) : Lout; a.Lo_rows = Lout;
  a.lin = KKLen{nullptr, 0, Lin}; a.lout = KKLen{nullptr, 0, Lout};
  a.in_slope = 1.f; a.scale = 1.f;
  if (path) *path = KK_SNAC_UNIT_GENERIC;
  return kk_launch_conv_generic(a, B, x.dtype, out.dtype, st);
}

// ResidualUnit: out = x + W snake(dw7(snake(x))) + b in two launches (tmp: [B][rows][x.ld], x's dtype).  out may not alias x or tmp.
int snac_residual_unit(hipStream_t st, int B, const Unit& u, const Act& x, const Act& tmp, const Act& out, int* path) {
  KK_TRY(snac_launch_dw_conv(x.p, x.bs(), x.ld, x.dtype, x.rows, x.C, u.dil, u.dw.w.p, u.dw.b.p, u.a1.p, u.a2.p, tmp.p, tmp.bs(), tmp.ld, B, st));
  return snac_conv(st, B, u.pw, tmp, out, 0, false, 1, &x, path);
}

// conv_transpose1d without output padding (layers.py:105-121) and the strided conv of an EncoderBlock (layers.py:243-249)
int convt_len(int L, int s) { return (L - 1) * s - 2 * ((s + 1) / 2) + 2 * s; }
int convs_len(int L, int s) { return (L + 2 * ((s + 1) / 2) - 2 * s) / s + 1; }

struct Run : Workspace {
  kk_snac* m;
  hipStream_t st;
  int B;
  Run(kk_snac* m_, hipStream_t st_, int B_, void* ws, size_t ws_bytes) : m(m_), st(st_), B(B_) {
    base = (char*)ws; cap = ws_bytes; dry = ws == nullptr;
  }
  Act act(int rows, int C, int dtype) {
    Act t;
    t.dtype = dtype; t.rows = rows; t.C = C; t.ld = pitch_of(C, dtype);
    t.p = raw((size_t)B * rows * t.ld * esize(dtype));
    return t;
  }
  // three scratch tensors of `elems` elements each; view(i, ...) shapes slot i
  char* slot[3] = {nullptr, nullptr, nullptr};
  void scratch(size_t elems, int dtype) {
    for (int i = 0; i < 3; ++i) slot[i] = (char*)raw(elems * esize(dtype));
  }
  Act view(int i, int rows, int C, int dtype) const {
    Act t;
    t.dtype = dtype; t.rows = rows; t.C = C; t.ld = pitch_of(C, dtype); t.p = slot[i];
    return t;
  }
  static int other(int a, int b) {  // a slot that is neither a nor b
    for (int i = 0; i < 3; ++i)
      if (i != a && i != b) return i;
    return 0;
  }
  void note(const std::string& name, const Act& t) {
    if (!dry) {
      std::lock_guard<std::mutex> lk(m->dbg_mu);
      m->dbg.map[name] = DebugNote{t.p, t.ld, t.bs(), t.rows, t.C, t.dtype, B};
    }
  }
  // three units from slot `cur` into `out` (a tensor outside the slots)
  int units(const Unit* u, int cur, int rows, int C, int dtype, const Act& out) {
    if (dry) return 0;
    for (int i = 0; i < 3; ++i) {
      const int t = other(cur, cur), nx = other(cur, t);
      const Act x = view(cur, rows, C, dtype), tmp = view(t, rows, C, dtype);
      const Act o = i == 2 ? out : view(nx, rows, C, dtype);
      KK_TRY(snac_residual_unit(st, B, u[i], x, tmp, o, nullptr));
      cur = nx;
    }
    return 0;
  }
};

int decode_samples(const kk_snac* m, int T) {
  int L = T;
  for (const DecBlock& b : m->dec) L = convt_len(L, b.stride);
  return L;
}
size_t decode_scratch_elems(const kk_snac* m, int B, int T) {
  const int dt = m->adt;
  size_t mx = (size_t)T * pitch_of(m->D, dt);
  int L = T;
  for (const DecBlock& b : m->dec) {
    mx = std::max(mx, (size_t)L * pitch_of(b.Cin, dt));
    L = convt_len(L, b.stride);
    mx = std::max(mx, (size_t)L * pitch_of(b.Cout, dt));
  }
  return mx * B;
}

int run_decode(Run& r, int T, const int32_t* const* codes, const float* const* noise, float* pcm) {
  kk_snac* m = r.m;
  const kk_snac_config& c = m->cfg;
  const int B = r.B, dt = m->adt;
  Act z = r.act(T, m->D, dt), y = r.act(T, c.decoder_dim, dt);
  r.scratch(decode_scratch_elems(m, B, T), dt);
  if (!r.dry) {
    SnacCodes sc;
    memset(&sc, 0, sizeof sc);
    sc.nq = c.n_vq;
    for (int i = 0; i < c.n_vq; ++i) { sc.codes[i] = codes[i]; sc.table[i] = m->vq[i].table.p; sc.stride[i] = m->vq[i].stride; }
    KK_TRY(snac_launch_from_codes(sc, c.codebook_size, m->D, T, m->bias_sum.p, z.p, z.ld, dt, B, r.st));
    r.note("z_q", z);
    const Act d0 = r.view(0, T, m->D, dt);
    KK_TRY(snac_launch_dw_conv(z.p, z.bs(), z.ld, dt, T, m->D, 1, m->dec_dw.w.p, m->dec_dw.b.p, nullptr, nullptr, d0.p, d0.bs(), d0.ld, B, r.st));
    KK_TRY(snac_conv(r.st, B, m->dec_pw, d0, y, 0, false, 1, nullptr, nullptr));
  }
  int L = T;
  for (size_t l = 0; l < m->dec.size(); ++l) {
    const DecBlock& b = m->dec[l];
    const int Lo = convt_len(L, b.stride);
    Act o = r.act(Lo, b.Cout, dt);
    if (r.oom) return kk_fail("kk_snac_decode: workspace too small");
    if (!r.dry) {
      const Act s = r.view(0, L, b.Cin, dt), u = r.view(1, Lo, b.Cout, dt);
      KK_TRY(snac_launch_snake(y.p, y.ld, dt, L, b.Cin, b.alpha.p, s.p, s.ld, B, r.st));
      KK_TRY(snac_conv(r.st, B, b.up, s, u, (b.stride + 1) / 2, true, b.stride, nullptr, nullptr));
      int cur = 1;
      if (c.noise) {
        const Act h = r.view(2, Lo, b.Cout, dt);
        KK_TRY(snac_conv(r.st, B, b.nz, u, h, 0, false, 1, nullptr, nullptr));
        KK_TRY(snac_launch_noise_mix(u.p, h.p, noise[l], dt, Lo, b.Cout, u.ld, h.p, B, r.st));  // h <- u + n h
        cur = 2;
      }
      KK_TRY(r.units(b.u, cur, Lo, b.Cout, dt, o));
      static const char* names[8] = {"block0", "block1", "block2", "block3", "block4", "block5", "block6", "block7"};
      r.note(names[l], o);
    }
    y = o;
    L = Lo;
  }
  if (r.oom) return kk_fail("kk_snac_decode: workspace too small");
  if (r.dry) return 0;
  const PackedConv& w = m->dec_last;
  return snac_launch_conv_cout1(y.p, dt, y.ld, L, w.Cin, w.K, 3, w.w, w.ldw, w.b, m->dec_alpha.p, 1, pcm, B, r.st);
}

int encode_frames(const kk_snac* m, int N) {
  int L = N;
  for (const EncBlock& b : m->enc) {
    if (L + 2 * ((b.stride + 1) / 2) < 2 * b.stride) return 0;
    L = convs_len(L, b.stride);
  }
  return L;
}
size_t encode_scratch_elems(const kk_snac* m, int B, int N) {
  size_t mx = (size_t)N * m->cfg.encoder_dim;
  int L = N;
  for (const EncBlock& b : m->enc) {
    mx = std::max(mx, (size_t)L * b.Cin);
    L = convs_len(L, b.stride);
  }
  return mx * B;
}

int run_encode(Run& r, int N, const float* pcm, int32_t* const* codes) {
  kk_snac* m = r.m;
  const kk_snac_config& c = m->cfg;
  const int B = r.B, T = encode_frames(m, N), D = m->D;
  if (T < 1) return kk_fail("kk_snac_encode: too few samples");
  for (const Quant& q : m->vq)
    if (T % q.stride != 0) return kk_failf("kk_snac_encode: %d latent frames are no multiple of the quantiser stride %d (preprocess pads the audio)", T, q.stride);
  Act y = r.act(N, c.encoder_dim, KK_F32);
  r.scratch(encode_scratch_elems(m, B, N), KK_F32);
  if (r.oom) return kk_fail("kk_snac_encode: workspace too small");
  if (!r.dry) {
    Act x;
    x.p = const_cast<float*>(pcm); x.rows = N; x.C = 1; x.ld = 1; x.dtype = KK_F32;
    KK_TRY(snac_conv(r.st, B, m->enc_first, x, y, 3, false, 1, nullptr, nullptr));
  }
  int L = N;
  for (const EncBlock& b : m->enc) {
    const int Lo = convs_len(L, b.stride);
    Act o = r.act(Lo, b.Cout, KK_F32);
    if (r.oom) return kk_fail("kk_snac_encode: workspace too small");
    if (!r.dry) {
      // (the block's input lives outside the slots: the first unit reads it in place)
      const Act t0 = r.view(0, L, b.Cin, KK_F32), r1 = r.view(1, L, b.Cin, KK_F32), r2 = r.view(2, L, b.Cin, KK_F32);
      KK_TRY(snac_residual_unit(r.st, B, b.u[0], y, t0, r1, nullptr));
      KK_TRY(snac_residual_unit(r.st, B, b.u[1], r1, t0, r2, nullptr));
      KK_TRY(snac_residual_unit(r.st, B, b.u[2], r2, t0, r1, nullptr));
      KK_TRY(snac_launch_snake(r1.p, r1.ld, KK_F32, L, b.Cin, b.alpha.p, t0.p, t0.ld, B, r.st));
      KK_TRY(snac_conv(r.st, B, b.down, t0, o, (b.stride + 1) / 2, false, b.stride, nullptr, nullptr));
    }
    y = o;
    L = Lo;
  }
  Act z = r.act(T, D, KK_F32);
  if (r.oom) return kk_fail("kk_snac_encode: workspace too small");
  if (!r.dry) {
    KK_TRY(snac_launch_dw_conv(y.p, y.bs(), y.ld, KK_F32, T, D, 1, m->enc_last.w.p, m->enc_last.b.p, nullptr, nullptr, z.p, z.bs(), z.ld, B, r.st));
    r.note("encoder", z);
  }
  Act res = z;
  for (size_t i = 0; i < m->vq.size(); ++i) {
    const Quant& q = m->vq[i];
    const int Ti = T / q.stride, cd = c.codebook_dim;
    Act pooled = r.act(Ti, D, KK_F32), ze = r.act(Ti, cd, KK_F32), zq = r.act(Ti, cd, KK_F32), zo = r.act(Ti, D, KK_F32), nres = r.act(T, D, KK_F32);
    if (r.oom) return kk_fail("kk_snac_encode: workspace too small");
    if (r.dry) continue;
    const Act* src = &res;
    if (q.stride > 1) {
      KK_TRY(snac_launch_avg_pool((const float*)res.p, T, D, q.stride, (float*)pooled.p, B, r.st));
      src = &pooled;
    }
    KK_TRY(snac_conv(r.st, B, q.in_proj, *src, ze, 0, false, 1, nullptr, nullptr));
    KK_TRY(snac_launch_vq_search((const float*)ze.p, ze.ld, cd, q.cb.p, q.cbn.p, q.c2.p, c.codebook_size, Ti, codes[i], (float*)zq.p, zq.ld, B, r.st));
    KK_TRY(snac_conv(r.st, B, q.out_proj, zq, zo, 0, false, 1, nullptr, nullptr));
    KK_TRY(snac_launch_residual_update((const float*)res.p, (const float*)zo.p, T, D, q.stride, (float*)nres.p, B, r.st));
    r.note("residual" + std::to_string(i), nres);
    res = nres;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------------------- packing
struct Packer {
  kk_snac* m;
  WeightArena& a;
  // weight norm folded in float64 (layers.py:9-14,57): g v / |v| over the axes except 0.  v [A][K][Bn], g [A]
  bool folded(const std::string& p, int A, int K, int Bn, std::vector<double>& w) {
    const HostTensor* v = a.get(p + ".weight_v", (size_t)A * K * Bn);
    const HostTensor* g = a.get(p + ".weight_g", (size_t)A);
    if (!v || !g) return false;
    w.resize((size_t)A * K * Bn);
    for (int i = 0; i < A; ++i) {
      double ss = 0;
      for (int e = 0; e < K * Bn; ++e) { const double x = v->d[(size_t)i * K * Bn + e]; ss += x * x; }
      const double nrm = sqrt(ss);
      for (int e = 0; e < K * Bn; ++e) w[(size_t)i * K * Bn + e] = (double)g->d[i] * (double)v->d[(size_t)i * K * Bn + e] / nrm;
    }
    return true;
  }
  // WNConv1d [O][K][I] or WNConvTranspose1d [I][K][O] -> [K][I][ldw] (+ the fragment pack when `mfma`)
  PackedConv conv(const std::string& p, int O, int K, int I, bool transposed, bool bias, bool mfma) {
    PackedConv c;
    std::vector<double> w;
    if (!folded(p, transposed ? I : O, K, transposed ? O : I, w)) return c;
    auto at = [&](int o, int k, int i) { return (float)(transposed ? w[((size_t)i * K + k) * O + o] : w[((size_t)o * K + k) * I + i]); };
    c.Cin = I; c.Cout = O; c.K = K; c.ldw = rup(O, 64);
    c.w_off = a.alloc((size_t)K * I * c.ldw);
    float* dst = &a.pack[c.w_off];
    for (int o = 0; o < O; ++o)
      for (int k = 0; k < K; ++k)
        for (int i = 0; i < I; ++i) dst[((size_t)k * I + i) * c.ldw + o] = at(o, k, i);
    c.mfma = mfma && O % 8 == 0 && O >= 16 && I >= 16;
    if (c.mfma) {
      c.CinP = rup(I, 64);
      c.CoutP = rup(O, 128);
      const size_t nel = (size_t)K * c.CoutP * c.CinP;
      c.wf_off = a.alloc((nel + 1) / 2);
      uint16_t* dfr = (uint16_t*)&a.pack[c.wf_off];
      for (int o = 0; o < O; ++o)
        for (int k = 0; k < K; ++k)
          for (int i = 0; i < I; ++i) dfr[kk_mfma4_pack_index(k, o, i, c.CoutP, c.CinP)] = f32_to_bf16_rne(at(o, k, i));
    }
    const int nb = c.mfma ? c.CoutP : O;
    if (bias || c.mfma) {
      c.has_bias = true;
      c.b_off = a.alloc(nb);
      if (bias) {
        const HostTensor* b = a.get(p + ".bias", (size_t)O);
        if (!b) return c;
        memcpy(&a.pack[c.b_off], b->d.data(), (size_t)O * 4);
      }
    }
    return c;
  }
  DwConv dw(const std::string& p, int C) {
    DwConv d;
    d.C = C;
    std::vector<double> w;
    if (!folded(p, C, SNAC_DW_K, 1, w)) return d;
    std::vector<float> f(w.begin(), w.end());
    d.w = a.put(f.data(), f.size());
    d.b = a.vec(p + ".bias", C);
    return d;
  }
  Unit unit(const std::string& p, int C, int dil, bool mfma) {  // p.block.layers.{0 Snake, 1 dw conv, 2 Snake, 3 1x1}
    Unit u;
    u.dil = dil;
    u.a1 = a.vec(p + ".block.layers.0.alpha", C);
    u.dw = dw(p + ".block.layers.1", C);
    u.a2 = a.vec(p + ".block.layers.2.alpha", C);
    u.pw = conv(p + ".block.layers.3", C, 1, C, false, true, mfma);
    return u;
  }
};

void resolve(kk_snac* m, PackedConv& c) {
  c.w = m->arena.dev + c.w_off;
  c.b = c.has_bias ? m->arena.dev + c.b_off : nullptr;
  c.wf = c.mfma ? (const bf16_t*)(m->arena.dev + c.wf_off) : nullptr;
}
void resolve(kk_snac* m, ArenaVec& v) { m->arena.resolve(v); }
void resolve(kk_snac* m, DwConv& d) { resolve(m, d.w); resolve(m, d.b); }
void resolve(kk_snac* m, Unit& u) { resolve(m, u.a1); resolve(m, u.a2); resolve(m, u.dw); resolve(m, u.pw); }

int check_cfg(const kk_snac_config& c) {
  const char* who = "kk_snac_create";
  if (c.attn_window_size != 0) return kk_failf("%s: attn_window_size: LocalMHA is not built (the 32 / 44 kHz checkpoints)", who);
  if (!c.depthwise) return kk_failf("%s: depthwise=False is not built", who);
  if (c.encoder_dim < 1 || c.decoder_dim < 1 || c.latent_dim < 1 || c.codebook_size < 1) return kk_failf("%s: bad dimension", who);
  if (c.codebook_dim < 1 || c.codebook_dim > SNAC_VQ_MAX_DIM) return kk_failf("%s: codebook_dim must be 1 .. %d", who, SNAC_VQ_MAX_DIM);
  if (c.n_encoder_rates < 1 || c.n_encoder_rates > 8 || c.n_decoder_rates < 1 || c.n_decoder_rates > 8 || c.n_vq < 1 || c.n_vq > SNAC_MAX_VQ)
    return kk_failf("%s: 1 .. 8 encoder rates, decoder rates and quantisers", who);
  for (int i = 0; i < c.n_encoder_rates; ++i)
    if (c.encoder_rates[i] < 1 || c.encoder_rates[i] > 64) return kk_failf("%s: bad encoder rate", who);
  for (int i = 0; i < c.n_decoder_rates; ++i)
    if (c.decoder_rates[i] < 1 || c.decoder_rates[i] > 64) return kk_failf("%s: bad decoder rate", who);
  for (int i = 0; i < c.n_vq; ++i)
    if (c.vq_strides[i] < 1) return kk_failf("%s: bad quantiser stride", who);
  if ((c.decoder_dim >> c.n_decoder_rates) < 1 || c.decoder_dim % (1 << c.n_decoder_rates) != 0) return kk_failf("%s: decoder_dim must be divisible by 2^len(decoder_rates)", who);
  return 0;
}

bool dt_ok(int d) { return d == KK_F32 || d == KK_BF16; }
bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int kk_snac_create(const kk_snac_config* cfg, kk_snac** out) {
  if (!cfg || !out) return kk_fail("kk_snac_create: null argument");
  KK_TRY(check_cfg(*cfg));
  kk_snac* m = new kk_snac();
  m->cfg = *cfg;
  m->adt = cfg->compute_dtype == KK_BF16 ? KK_BF16 : KK_F32;
  m->D = cfg->latent_dim;
  *out = m;
  return 0;
}

extern "C" void kk_snac_destroy(kk_snac* m) {
  if (!m) return;
  if (m->arena.dev) (void)hipFree(m->arena.dev);
  delete m;
}

extern "C" int kk_snac_load_tensor(kk_snac* m, const char* name, const int64_t* shape, int ndim, const float* data) {
  return kk_host_load_tensor("kk_snac_load_tensor", m ? &m->arena.host : nullptr, m && m->finalized, name, shape, ndim, data);
}

extern "C" int kk_snac_finalize(kk_snac* m, void* stream) {
  if (!m) return kk_fail("kk_snac_finalize: null model");
  if (m->finalized) return kk_fail("kk_snac_finalize: already finalized");
  const kk_snac_config& c = m->cfg;
  Packer P{m, m->arena};
  const int D = m->D, cd = c.codebook_dim, bins = c.codebook_size;
  const bool bf = m->adt == KK_BF16;
  // ---- encoder (layers.py:133-156), fp32 packs only
  {
    const std::string e = "encoder.block.layers.";
    int d = c.encoder_dim;
    m->enc_first = P.conv(e + "0", d, SNAC_DW_K, 1, false, true, false);
    m->enc.resize(c.n_encoder_rates);
    for (int l = 0; l < c.n_encoder_rates; ++l) {
      EncBlock& b = m->enc[l];
      const std::string p = e + std::to_string(l + 1) + ".block.layers.";
      b.Cin = d; b.Cout = 2 * d; b.stride = c.encoder_rates[l];
      static const int dils[3] = {1, 3, 9};
      for (int i = 0; i < 3; ++i) b.u[i] = P.unit(p + std::to_string(i), d, dils[i], false);
      b.alpha = P.a.vec(p + "3.alpha", d);
      b.down = P.conv(p + "4", 2 * d, 2 * b.stride, d, false, true, false);
      d *= 2;
    }
    if (d != D) return kk_failf("kk_snac_finalize: latent_dim %d is not encoder_dim * 2^len(encoder_rates) = %d (the quantiser reads the encoder's channels)", D, d);
    m->enc_last = P.dw(e + std::to_string(c.n_encoder_rates + 1), D);
  }
  // ---- quantiser (vq.py): packs, the normalised code book, the from_codes tables
  m->vq.resize(c.n_vq);
  std::vector<double> bsum(D, 0.0);
  for (int i = 0; i < c.n_vq; ++i) {
    Quant& q = m->vq[i];
    const std::string p = "quantizer.quantizers." + std::to_string(i);
    q.stride = c.vq_strides[i];
    q.in_proj = P.conv(p + ".in_proj", cd, 1, D, false, true, false);
    q.out_proj = P.conv(p + ".out_proj", D, 1, cd, false, true, false);
    const HostTensor* cb = P.a.get(p + ".codebook.weight", (size_t)bins * cd);
    std::vector<double> wo;
    const bool have = P.folded(p + ".out_proj", D, 1, cd, wo);
    const HostTensor* ob = P.a.get(p + ".out_proj.bias", (size_t)D);
    if (!cb || !have || !ob) continue;
    std::vector<float> cbn((size_t)bins * cd), c2(bins), table((size_t)bins * D);
    for (int r = 0; r < bins; ++r) {
      double ss = 0;
      for (int j = 0; j < cd; ++j) ss += (double)cb->d[(size_t)r * cd + j] * cb->d[(size_t)r * cd + j];
      const double nrm = std::max(sqrt(ss), 1e-12);  // normalize(): x / max(|x|, eps) (vq.py:132-135)
      double s2 = 0;
      for (int j = 0; j < cd; ++j) {
        const float v = (float)(cb->d[(size_t)r * cd + j] / nrm);
        cbn[(size_t)r * cd + j] = v;
        s2 += (double)v * v;
      }
      c2[r] = (float)s2;
      for (int o = 0; o < D; ++o) {
        double acc = 0;
        for (int j = 0; j < cd; ++j) acc += wo[(size_t)o * cd + j] * (double)cb->d[(size_t)r * cd + j];
        table[(size_t)r * D + o] = (float)acc;
      }
    }
    for (int o = 0; o < D; ++o) bsum[o] += ob->d[o];
    q.cb = P.a.put(cb->d.data(), cb->d.size());
    q.cbn = P.a.put(cbn.data(), cbn.size());
    q.c2 = P.a.put(c2.data(), c2.size());
    q.table = P.a.put(table.data(), table.size());
  }
  {
    std::vector<float> f(bsum.begin(), bsum.end());
    m->bias_sum = P.a.put(f.data(), f.size());
  }
  // ---- decoder (layers.py:159-205)
  {
    const std::string dp = "decoder.model.layers.";
    m->dec_dw = P.dw(dp + "0", D);
    m->dec_pw = P.conv(dp + "1", c.decoder_dim, 1, D, false, true, bf);
    m->dec.resize(c.n_decoder_rates);
    int out_dim = c.decoder_dim;
    for (int l = 0; l < c.n_decoder_rates; ++l) {
      DecBlock& b = m->dec[l];
      const std::string p = dp + std::to_string(l + 2) + ".block.layers.";
      b.Cin = c.decoder_dim >> l; b.Cout = c.decoder_dim >> (l + 1); b.stride = c.decoder_rates[l];
      b.alpha = P.a.vec(p + "0.alpha", b.Cin);
      b.up = P.conv(p + "1", b.Cout, 2 * b.stride, b.Cin, true, true, bf);
      int at = 2;
      if (c.noise) b.nz = P.conv(p + std::to_string(at++) + ".linear", b.Cout, 1, b.Cout, false, false, bf);
      static const int dils[3] = {1, 3, 9};
      for (int i = 0; i < 3; ++i) b.u[i] = P.unit(p + std::to_string(at++), b.Cout, dils[i], bf);
      out_dim = b.Cout;
    }
    m->dec_alpha = P.a.vec(dp + std::to_string(c.n_decoder_rates + 2) + ".alpha", out_dim);
    m->dec_last = P.conv(dp + std::to_string(c.n_decoder_rates + 3), 1, SNAC_DW_K, out_dim, false, true, false);
  }
  if (!P.a.err.empty()) return kk_failf("kk_snac_finalize: %s", P.a.err.c_str());
  KK_TRY(m->arena.upload((hipStream_t)stream, "kk_snac_finalize"));
  resolve(m, m->enc_first); resolve(m, m->enc_last); resolve(m, m->dec_dw); resolve(m, m->dec_pw); resolve(m, m->dec_last);
  resolve(m, m->dec_alpha); resolve(m, m->bias_sum);
  for (auto& b : m->enc) {
    for (auto& u : b.u) resolve(m, u);
    resolve(m, b.alpha); resolve(m, b.down);
  }
  for (auto& b : m->dec) {
    for (auto& u : b.u) resolve(m, u);
    resolve(m, b.alpha); resolve(m, b.up);
    if (c.noise) resolve(m, b.nz);
  }
  for (auto& q : m->vq) { resolve(m, q.in_proj); resolve(m, q.out_proj); resolve(m, q.cb); resolve(m, q.cbn); resolve(m, q.c2); resolve(m, q.table); }
  m->finalized = true;
  return 0;
}

extern "C" int64_t kk_snac_hop_length(const kk_snac* m) {
  if (!m) return 0;
  int64_t h = 1;
  for (int i = 0; i < m->cfg.n_encoder_rates; ++i) h *= m->cfg.encoder_rates[i];
  return h;
}

extern "C" int64_t kk_snac_decode_samples(const kk_snac* m, int T) { return (m && m->finalized && T > 0) ? decode_samples(m, T) : 0; }

extern "C" size_t kk_snac_decode_workspace_bytes(kk_snac* m, int B, int T) {
  if (!m || !m->finalized || B <= 0 || T <= 0 || (long long)B * decode_samples(m, T) * 64 > (1ll << 40)) return 0;
  Run r(m, nullptr, B, nullptr, 0);
  if (run_decode(r, T, nullptr, nullptr, nullptr) != 0) return 0;
  return r.used + 256;
}

extern "C" int kk_snac_decode(kk_snac* m, void* stream, int B, int T, const int32_t* const* codes, const float* const* noise, void* workspace,
                              size_t workspace_bytes, float* pcm_out) {
  const char* who = "kk_snac_decode";
  if (!m || !m->finalized) return kk_failf("%s: model not finalized", who);
  if (B <= 0 || T <= 0 || !codes || !workspace || !pcm_out) return kk_failf("%s: bad argument", who);
  for (int i = 0; i < m->cfg.n_vq; ++i) {
    if (!codes[i]) return kk_failf("%s: codes[%d] is null", who, i);
    if (T % m->cfg.vq_strides[i] != 0) return kk_failf("%s: %d latent frames are no multiple of the quantiser stride %d", who, T, m->cfg.vq_strides[i]);
  }
  if (m->cfg.noise) {
    if (!noise) return kk_failf("%s: the model has NoiseBlocks: noise must hold one [B][C] tensor per decoder block", who);
    for (int l = 0; l < m->cfg.n_decoder_rates; ++l)
      if (!noise[l]) return kk_failf("%s: noise[%d] is null", who, l);
  }
  if ((long long)decode_samples(m, T) < 1) return kk_failf("%s: no output samples", who);
  const size_t need = kk_snac_decode_workspace_bytes(m, B, T);
  if (need == 0 || workspace_bytes < need) return kk_failf("%s: workspace too small", who);
  { std::lock_guard<std::mutex> lk(m->dbg_mu); m->dbg.map.clear(); }
  Run r(m, (hipStream_t)stream, B, workspace, workspace_bytes);
  return run_decode(r, T, codes, noise, pcm_out);
}

extern "C" int kk_snac_encode_frames(const kk_snac* m, int N) { return (m && m->finalized && N > 0) ? encode_frames(m, N) : 0; }

extern "C" size_t kk_snac_encode_workspace_bytes(kk_snac* m, int B, int N) {
  if (!m || !m->finalized || B <= 0 || N <= 0) return 0;
  Run r(m, nullptr, B, nullptr, 0);
  if (run_encode(r, N, nullptr, nullptr) != 0) return 0;
  return r.used + 256;
}

extern "C" int kk_snac_encode(kk_snac* m, void* stream, int B, int N, const float* pcm, void* workspace, size_t workspace_bytes, int32_t* const* codes_out) {
  const char* who = "kk_snac_encode";
  if (!m || !m->finalized) return kk_failf("%s: model not finalized", who);
  if (B <= 0 || N <= 0 || !pcm || !workspace || !codes_out) return kk_failf("%s: bad argument", who);
  for (int i = 0; i < m->cfg.n_vq; ++i)
    if (!codes_out[i]) return kk_failf("%s: codes_out[%d] is null", who, i);
  const size_t need = kk_snac_encode_workspace_bytes(m, B, N);
  if (need == 0) return -1;  // (run_encode said why)
  if (workspace_bytes < need) return kk_failf("%s: workspace too small", who);
  { std::lock_guard<std::mutex> lk(m->dbg_mu); m->dbg.map.clear(); }
  Run r(m, (hipStream_t)stream, B, workspace, workspace_bytes);
  return run_encode(r, N, pcm, codes_out);
}

extern "C" int kk_snac_debug_info(kk_snac* m, const char* name, int64_t* rows, int64_t* channels) {
  if (!m || !name) return kk_fail("kk_snac_debug_info: bad argument");
  std::lock_guard<std::mutex> lk(m->dbg_mu);
  return m->dbg.info("kk_snac_debug_info", name, rows, channels);
}
extern "C" int kk_snac_debug_fetch(kk_snac* m, void* stream, const char* name, float* dst) {
  if (!m || !name || !dst) return kk_fail("kk_snac_debug_fetch: bad argument");
  std::lock_guard<std::mutex> lk(m->dbg_mu);
  return m->dbg.fetch("kk_snac_debug_fetch", name, (hipStream_t)stream, dst);
}

// ------------------------------------------------------------------------------------------------ single-kernel entry points (ABI minor 28)
// The codec's launch functions on caller-owned device buffers (tests/test_gpu_snac_kernels.py); every argument is checked here, on the host,
// before any launch.
extern "C" int kk_op_snac_dw_conv(void* stream, int B, const void* x, long long xbs, int ldx, int dtype, int L, int C, int dil, const float* w,
                                  const float* bias, const float* alpha_in, const float* alpha_out, void* out, long long obs, int ldo) {
  const char* who = "kk_op_snac_dw_conv";
  if (B <= 0 || L < 1 || C < 1 || !x || !w || !bias || !out || x == out) return kk_failf("%s: B, L, C must be positive, x / w / bias / out non-null, out != x", who);
  if (!dt_ok(dtype)) return kk_failf("%s: dtype is KK_DTYPE_F32 or KK_DTYPE_BF16", who);
  if (dil < 1 || dil > SNAC_DW_MAX_DIL) return kk_failf("%s: dil must be 1 .. %d", who, SNAC_DW_MAX_DIL);
  if (ldx < C || ldo < C || xbs < (long long)L * ldx || obs < (long long)L * ldo) return kk_failf("%s: a pitch is smaller than what it spans", who);
  return snac_launch_dw_conv(x, xbs, ldx, dtype, L, C, dil, w, bias, alpha_in, alpha_out, out, obs, ldo, B, (hipStream_t)stream);
}

extern "C" int kk_op_snac_residual_unit(void* stream, int B, const void* x, int ldx, int dtype, int L, int C, int dil, const float* dw_w,
                                        const float* dw_b, const float* alpha1, const float* alpha2, const float* pw_packed, int ldw,
                                        const void* pw_frag, int CinP, int CoutP, const float* pw_bias, void* tmp, void* out, int ldo, int* path_out) {
  const char* who = "kk_op_snac_residual_unit";
  if (path_out) *path_out = -1;
  if (B <= 0 || L < 1 || C < 1 || !x || !dw_w || !dw_b || !alpha1 || !alpha2 || !pw_packed || !pw_bias || !tmp || !out)
    return kk_failf("%s: B, L, C must be positive and every pointer but pw_frag non-null", who);
  if (out == x || out == tmp || tmp == x) return kk_failf("%s: x, tmp and out must be three tensors", who);
  if (!dt_ok(dtype)) return kk_failf("%s: dtype is KK_DTYPE_F32 or KK_DTYPE_BF16", who);
  if (dil < 1 || dil > SNAC_DW_MAX_DIL) return kk_failf("%s: dil must be 1 .. %d", who, SNAC_DW_MAX_DIL);
  if (ldx < C || ldo < C) return kk_failf("%s: a row pitch is smaller than C", who);
  if (ldw % 4 != 0 || ldw < kk_cdiv(C, 64) * 64) return kk_failf("%s: ldw must be a multiple of 4 covering C rounded up to 64", who);
  Unit u;
  u.dil = dil;
  u.a1.p = alpha1; u.a2.p = alpha2; u.dw.w.p = dw_w; u.dw.b.p = dw_b; u.dw.C = C;
  PackedConv& w = u.pw;
  w.Cin = C; w.Cout = C; w.K = 1; w.ldw = ldw; w.w = pw_packed; w.b = pw_bias; w.has_bias = true;
  if (pw_frag) {
    if (CinP % 64 != 0 || CoutP % 128 != 0 || CinP < C || CoutP < C) return kk_failf("%s: pw_frag needs CinP %% 64 == 0 >= C, CoutP %% 128 == 0 >= C (and a bias of CoutP entries)", who);
    if (dtype == KK_BF16 && (ldx % 8 || ldo % 8 || !al16(x) || !al16(out) || !al16(tmp) || !al16(pw_frag)))
      return kk_failf("%s: with pw_frag, bf16 tensors need pitches that are multiples of 8 and 16-byte aligned pointers", who);
    w.mfma = true; w.CinP = CinP; w.CoutP = CoutP; w.wf = (const bf16_t*)pw_frag;
  }
  Act ax, at, ao;
  ax.p = const_cast<void*>(x); ax.rows = L; ax.C = C; ax.ld = ldx; ax.dtype = dtype;
  at = ax; at.p = tmp;
  ao = ax; ao.p = out; ao.ld = ldo;
  return snac_residual_unit((hipStream_t)stream, B, u, ax, at, ao, path_out);
}

extern "C" int kk_op_snac_from_codes(void* stream, int B, int T, int D, int nq, const int32_t* const* codes, const int32_t* strides,
                                     const float* const* tables, int bins, const float* bias_sum, void* out, int ldo, int dtype) {
  const char* who = "kk_op_snac_from_codes";
  if (B <= 0 || T < 1 || D < 1 || bins < 1 || nq < 1 || nq > SNAC_MAX_VQ) return kk_failf("%s: B, T, D, bins must be positive, nq 1 .. %d", who, SNAC_MAX_VQ);
  if (!codes || !strides || !tables || !bias_sum || !out || !dt_ok(dtype) || ldo < D) return kk_failf("%s: null pointer, bad dtype, or ldo < D", who);
  SnacCodes sc;
  memset(&sc, 0, sizeof sc);
  sc.nq = nq;
  for (int i = 0; i < nq; ++i) {
    if (!codes[i] || !tables[i] || strides[i] < 1 || T % strides[i] != 0) return kk_failf("%s: quantiser %d: null pointer, or T is no multiple of its stride", who, i);
    sc.codes[i] = codes[i]; sc.table[i] = tables[i]; sc.stride[i] = strides[i];
  }
  return snac_launch_from_codes(sc, bins, D, T, bias_sum, out, ldo, dtype, B, (hipStream_t)stream);
}

extern "C" int kk_op_snac_vq_search(void* stream, int B, int T, const float* ze, int ldz, int cd, const float* codebook, const float* codebook_n,
                                    const float* c2, int bins, int32_t* codes, float* zq, int ldq) {
  const char* who = "kk_op_snac_vq_search";
  if (B <= 0 || T < 1 || bins < 1 || cd < 1 || cd > SNAC_VQ_MAX_DIM) return kk_failf("%s: B, T, bins must be positive, the code dimension 1 .. %d", who, SNAC_VQ_MAX_DIM);
  if (!ze || !codebook || !codebook_n || !c2 || !codes || !zq || ldz < cd || ldq < cd || zq == ze) return kk_failf("%s: null pointer, a pitch below the code dimension, or zq == ze", who);
  return snac_launch_vq_search(ze, ldz, cd, codebook, codebook_n, c2, bins, T, codes, zq, ldq, B, (hipStream_t)stream);
}

extern "C" int kk_op_snac_conv_cout1(void* stream, int B, const void* x, int dtype, int ld, int L, int Cin, int Kw, int pad, const float* w_packed,
                                     int ldw, const float* bias, const float* alpha, int tanh_out, float* out) {
  const char* who = "kk_op_snac_conv_cout1";
  if (B <= 0 || L < 1 || Cin < 1 || !x || !w_packed || !out) return kk_failf("%s: B, L, Cin must be positive, x / w_packed / out non-null", who);
  if (!dt_ok(dtype) || ld < Cin || ldw < 1 || pad < 0 || Kw < 1 || Kw > SNAC_C1_MAX_K || pad >= Kw || (tanh_out != 0 && tanh_out != 1))
    return kk_failf("%s: bad dtype, ld < Cin, ldw < 1, Kw outside 1 .. %d, pad outside [0, Kw) or tanh_out not 0 / 1", who, SNAC_C1_MAX_K);
  return snac_launch_conv_cout1(x, dtype, ld, L, Cin, Kw, pad, w_packed, ldw, bias, alpha, tanh_out, out, B, (hipStream_t)stream);
}
