// Dense convolutions of the codec handles (SNAC kk_snac.hip, BigVGAN kk_bigvgan.hip): one activation descriptor, one weight pack and one dispatch
// to the library's conv launchers -- the variant-4 matrix-core kernel (kk_conv_mfma4.hip) for bf16 tensors with a fragment pack and an eligible
// shape, the generic fp32 kernel (kk_conv.hip) otherwise.  Everything here is file-local to the .hip file that includes it.
#pragma once
#include <string.h>

#include <string>

#include "../../include/kokoro_hip.h"
#include "kk_common.h"
#include "kk_host.h"
#include "kk_kernels.h"

namespace {

struct PackedConv {  // generic-kernel pack [K][Cin][ldw] fp32 (+ bias); bf16 tensors: the variant-4 fragment pack as well
  size_t w_off = 0, b_off = 0, wf_off = 0;
  bool has_bias = false, mfma = false;
  int Cin = 0, Cout = 0, K = 0, ldw = 0, CinP = 0, CoutP = 0;
  const float* w = nullptr;
  const float* b = nullptr;  // [CoutP] when mfma (zero padded), else [Cout]
  const bf16_t* wf = nullptr;
};

struct Act {  // an activation tensor [B][rows][ld], C valid channels, dense
  void* p = nullptr;
  int rows = 0, C = 0, ld = 0, dtype = KK_F32;
  long long bs() const { return (long long)rows * ld; }
};
int pitch_of(int C, int dtype) { return dtype == KK_BF16 ? rup(C, 64) : C; }  // bf16 tensors can feed the matrix-core kernel
size_t esize(int dtype) { return dtype == KK_BF16 ? 2 : 4; }

// out = (conv(x) + bias + res) * scale (+ out when `accumulate`); *path (nullable): KK_SNAC_UNIT_MFMA / KK_SNAC_UNIT_GENERIC, the kernel that ran
int codec_conv(hipStream_t st, int B, const PackedConv& w, const Act& x, const Act& out, int pad, bool transposed, int stride, int dil, const Act* res,
               float scale, int accumulate, int* path) {
  const int Lin = x.rows, Lout = out.rows;
  if (w.mfma && x.dtype == KK_BF16 && out.dtype == KK_BF16 && x.ld >= w.CinP && kk_mfma_eligible(w.Cin, w.Cout, w.K, transposed ? KK_CONVT : KK_CONV, stride, dil)) {
    KKMfmaArgs g;
    memset(&g, 0, sizeof g);
    g.x = (const bf16_t*)x.p; g.xbs = x.bs(); g.ldx = x.ld; g.wf = w.wf; g.CinP = w.CinP; g.Cin = w.Cin; g.CoutP = w.CoutP; g.bias = w.b;
    g.out = out.p; g.obs = out.bs(); g.ldo = out.ld;
    if (res) { g.res = res->p; g.rbs = res->bs(); g.ldr = res->ld; }
    g.Cout = w.Cout; g.Kw = w.K; g.mode = transposed ? KK_CONVT : KK_CONV; g.stride = stride; g.pad = pad; g.dil = dil;
    g.Q = transposed ? kk_cdiv(Lout, stride) : Lout; g.Lo_rows = Lout;
    g.lin = KKLen{nullptr, 0, Lin}; g.lout = KKLen{nullptr, 0, Lout};
    g.in_slope = 1.f; g.scale = scale; g.accumulate = accumulate;
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
  a.mode = transposed ? KK_CONVT : KK_CONV; a.stride = stride; a.pad = pad; a.dil = dil;
  a.Q = transposed ? kk_cdiv(Lout, stride) : Lout; a.Lo_rows = Lout;
  a.lin = KKLen{nullptr, 0, Lin}; a.lout = KKLen{nullptr, 0, Lout};
  a.in_slope = 1.f; a.scale = scale; a.accumulate = accumulate;
  if (path) *path = KK_SNAC_UNIT_GENERIC;
  return kk_launch_conv_generic(a, B, x.dtype, out.dtype, st);
}

// weights at(o, k, i) -> [K][I][ldw] in the arena (+ the fragment pack when `mfma` and the shape allows it); the bias is the parameter p.bias
template <typename At>
PackedConv codec_pack(WeightArena& a, const std::string& p, int O, int K, int I, bool bias, bool mfma, At at) {
  PackedConv c;
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

void codec_resolve(const WeightArena& a, PackedConv& c) {
  c.w = a.dev + c.w_off;
  c.b = c.has_bias ? a.dev + c.b_off : nullptr;
  c.wf = c.mfma ? (const bf16_t*)(a.dev + c.wf_off) : nullptr;
}

}  // namespace
