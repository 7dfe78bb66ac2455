// Variant 4 of the bf16 MFMA implicit-GEMM convolution (see kk_conv_mfma.hip for the base design): the weight (B) fragments
// do NOT go through LDS.  W is packed in FRAGMENT ORDER at load time (kk_mfma4_pack_index), so a wave fetches the 1 KiB
// fragment of 16 output channels x 32 k of one k-step as ONE fully coalesced global_load_dwordx4, straight into the MFMA
// operand registers, one (tap, slab) iteration ahead.  Against the LDS-staged kernel that removes the W double buffer, the ds_write of W,
// 8 of the 20 ds_read_b128 per wave and iteration, and the barrier per tap: waves synchronise only when the X slab changes.
//
// bf16 MFMA implicit-GEMM convolution for frames-major tensors (gfx950, v_mfma_f32_16x16x32_bf16).
//
//   out[b][q][n] = sum_t sum_ci  W[t][n][ci] * f(X[b][q + off_t][ci])       (stride 1, any dilation)
//   transposed conv = `stride` independent phase convolutions with 2 taps each (polyphase form, see kk_conv.hip)
//   f = identity, LeakyReLU, ELU, or the fused AdaIN apply + Snake / LeakyReLU of the reference's resblocks
//
// GEMM view per workgroup: M = 192 output rows, N = 128 output channels, K = taps x Cin walked in slabs of 64 channels (slab outer, tap
// inner).  A = X rows (positions) from LDS, B = W rows (output channels) from global memory in fragment order.
//   * 4 waves as 2 x 2; a wave owns 96 x 64 outputs = 6 x 4 accumulator blocks of 16 x 16 (lane l holds rows 4 * (l / 16) .. + 3 of column
//     l % 16): 96 registers.  Per k-step (32 channels) a wave's 4 B fragments stay in registers while its 6 A fragments stream through.
//   * A fragment of lane l: row l % 16, k-group l / 16 (4 groups of 8 k), ONE ds_read_b128.  LDS rows have a 160-BYTE PITCH (XLD = 80
//     elements): 16 consecutive rows land on the even 16-byte granules and the odd k-groups on the odd ones, so the four lane groups of
//     a read are conflict-free (a 144-byte pitch, right for the older 32x32x16 fragments, collides 2-way here).  Slab: 38.7 KB.
//   * B fragment of lane l: column l % 16, k-group l / 16; pack order [tap][n block][chunk][wc][ks][ni][lane] x 16 bytes: one coalesced
//     1 KiB load per fragment, requested right behind the MFMAs of the k-step that frees its registers.
//   * the X slab [192 + halo rows][64 ch] is staged once per channel slab (kk_conv_mfma_stage.h: registers -> fused transform -> LDS) and
//     re-used by every tap as a shifted window.  Three forms: the slab-by-slab kernel (any slab count; the next slab is requested at the
//     first tap of the current one and stored between two barriers after its last tap), the WHOLE-K kernel for exactly two slabs
//     (CinP == 128: both staged in the prologue into buffers of their own, no staging in the loop -- see conv_mfma4_wholek_kernel) and
//     the RING kernel for three or more (two LDS buffers, the next slab stored behind the current one's last tap, ONE barrier per slab:
//     the Linears and the fused AdaIN + Snake layers -- see conv_mfma4_ring_kernel).
//   * all global loads are unconditional (clamped address + mask at use): a load under a data-dependent branch makes
//     hipcc wait vmcnt(0) right behind it, which serialises the loads (one HBM round trip each)
//   * epilogue (kk_conv_mfma_epilogue.h) through a 96 x 128 fp32 LDS tile per wave row, aliasing the slab: bias / activation / residual /
//     scale / accumulate / length mask on coalesced 16-byte rows, ONE rounding to bf16, optional per-tile column sums for the next
//     instance norm.
// The 16x16x32 instruction (round 3) has the FLOPs per cycle and operand bytes per FLOP of round 2's 32x32x16, but the chip holds a higher
// clock on it under load (MI355X_MICROARCH.md, DVFS give-back item 7: 1.12-1.15 x in MFMA-paced loops): -3 ... -11 % on every conv shape.
#include <stdlib.h>

#include "kk_common.h"
#include "kk_kernels.h"
#include "kk_conv_mfma_shared.h"

#define TR_NOW() 0ull
#define TR_ADD(slot, v) do { } while (0)
namespace {
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BN = 128, CK = 64;
constexpr int XLD = 80;       // elements per LDS row: the 160-byte pitch keeps the 16-row fragments' ds_read_b128 conflict-free (above)
constexpr int MAX_HALO = 50;  // (Kw-1)*dil of the largest resblock conv (k 11, dilation 5)
constexpr int CLD = BN;       // fp32 epilogue tile pitch: 128 x 128 x 4 B = exactly 64 KiB

constexpr int PS_BYTES = 2 * 3 * CK * 4;  // double-buffered AdaIN parameter table of one slab (A, B, alpha)

template <int BM>
struct Geo {
  static constexpr int XROWS = BM + MAX_HALO;
  static constexpr int XS_BYTES = XROWS * XLD * 2;
  static constexpr int MAIN_BYTES = XS_BYTES + PS_BYTES;
  static constexpr int RPP = BM / 2;  // rows per epilogue pass: one wave row group (64 or 96 rows)
  static constexpr int EPI_BYTES = RPP * CLD * 4;
  static constexpr int LDS_BYTES = MAIN_BYTES > EPI_BYTES ? MAIN_BYTES : EPI_BYTES;
  static constexpr int XREG = (XROWS * 8 + 255) / 256;  // 16-byte chunks of the slab per thread
};


union U16 {
  uint4 u;
  bf16_t h[8];
};
union U32x8 {
  uint4 u[2];
  float f[8];
};

// NRM: 0 = raw input, 1 = AdaIN + Snake while staging, 2 = AdaIN + LeakyReLU(nrm_slope; 1 = identity) while staging
// WM = 96: 192-row tile (KK_MFMA_TILE_ROWS), 2 workgroups per CU (230-256 VGPRs)
template <typename TO, int WM, int NRM>
__global__ __launch_bounds__(256, 2) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv_mfma4_kernel(KKMfmaArgs a) {
  constexpr int BM = 2 * WM, MI16 = WM / 16;
  constexpr bool ACC16 = true;  // 16 x 16 accumulator blocks (kk_conv_mfma_epilogue.h)
  constexpr int EPI = KK_EPI_GENERIC;  // the slab-by-slab kernel is the reference form: every epilogue choice at run time
  using G = Geo<BM>;
  constexpr int XREG = G::XREG;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16_t* Xs = (bf16_t*)smem;
  float* Ps = (float*)(smem + G::XS_BYTES);  // [2][3][64]
  float* Cs = (float*)smem;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int nphase = a.mode == KK_CONVT ? a.stride : 1;
  // XCD-aware tile order: the dispatcher deals workgroup ids (x fastest, then y, z) round-robin to the 8 XCDs, each with its own L2.
  // Neighbouring row tiles share their halo rows (up to 50 of 192 + 50 for k = 11, dilation 5) and the column blocks of one row tile share
  // the whole X slab, so the flat id is re-dealt: an XCD walks a contiguous run of (utterance, row tile) pairs, column blocks innermost.
  int bx, by, bz;
  {
    const int gx = gridDim.x, gy = gridDim.y, total = gx * gy * gridDim.z;
    int lid = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
    const int per = total / 8, rem = total - per * 8;
    const int xcd = lid & 7, idx = lid >> 3;
    lid = xcd * per + (xcd < rem ? xcd : rem) + idx;
    by = lid % gy;  // column blocks innermost
    const int t = lid / gy;
    bx = t % gx;
    bz = t / gx;
  }
  const int b = bz / nphase, phase = bz - b * nphase;
  const int q0 = bx * BM, n0 = by * BN;
  const int Lin = kk_len(a.lin, b), Lout = kk_len(a.lout, b);

  // taps: input row of output q for tap t is q + off0 + t*dstep ; weight slice widx0 + t*wstep
  int ntaps, off0, dstep, widx0, wstep;
  if (a.mode == KK_CONV) {
    ntaps = a.Kw; off0 = -a.pad; dstep = a.dil; widx0 = 0; wstep = 1;
  } else {
    const int k0 = (phase + a.pad) % a.stride;
    ntaps = (a.Kw - k0 + a.stride - 1) / a.stride;
    off0 = (phase + a.pad - k0) / a.stride; dstep = -1; widx0 = k0; wstep = a.stride;
  }
  const int min_off = dstep >= 0 ? off0 : off0 + (ntaps - 1) * dstep;
  const int halo = (ntaps - 1) * (dstep >= 0 ? dstep : -dstep);
  const int xrows = BM + halo;

  const int op_first = a.mode == KK_CONV ? q0 : phase + a.stride * q0;
  const bool tile_live = op_first < Lout;  // uniform over the workgroup

  const unsigned long long tr0 = TR_NOW();
  unsigned long long tr_sx = 0, tr_sw = 0;
  (void)tr0; (void)tr_sx; (void)tr_sw;
  f32x4 acc[MI16][4];
#pragma unroll
  for (int i = 0; i < MI16; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (tile_live) {
    const bf16_t* xb = a.x + (long long)b * a.xbs;
    const int nchunk = a.CinP / CK;
    const int nit = nchunk * ntaps;
    const int lin_hi = Lin > 0 ? Lin - 1 : 0;
    const int cin_real = a.Cin > 0 ? a.Cin : a.CinP;

#define KK_STG(name) name
#define KK_STG_XS Xs
#include "kk_conv_mfma_stage.h"  // xreg / preg / xok, load_x, store_p, store_x (shared with variant 2)
    // B fragments of one (tap, slab) iteration: [ks][ni], loaded from the fragment-order pack one iteration ahead.  Named
    // scalars, not an array (hipcc put a lambda-captured register array in scratch once already).
    uint4 q00, q01, q02, q03, q10, q11, q12, q13;
    const int nb = by;
    auto frag_ptr = [&](int it) __attribute__((always_inline)) -> const uint4* {
      const int chunk = it / ntaps, tap = it - chunk * ntaps;
      // pack order: [tap][n block][chunk][wc][ks][ni][lane] x 16 bytes
      const long long blk = ((long long)(widx0 + tap * wstep) * (a.CoutP / BN) + nb) * nchunk + chunk;
      return (const uint4*)a.wf + blk * 1024 + (wc * 2) * 4 * 64 + lane;
    };
    // ---- prologue
    load_x(0);
    {
      const uint4* fp = frag_ptr(0);
      q00 = fp[0 * 64]; q01 = fp[1 * 64]; q02 = fp[2 * 64]; q03 = fp[3 * 64];
      q10 = fp[4 * 64]; q11 = fp[5 * 64]; q12 = fp[6 * 64]; q13 = fp[7 * 64];
      asm volatile("" ::: "memory");
    }
    store_p(0);
    __syncthreads();
    store_x(0);
    __syncthreads();

    const int arow = wr * WM + (lane & 15);  // + mi*16 + tap shift
    const int kofs = 8 * (lane >> 4);

    for (int it = 0; it < nit; ++it) {
      const int chunk = it / ntaps, tap = it - chunk * ntaps;
      const bool last_tap = tap == ntaps - 1;
      // prefetch the next channel slab of X at the FIRST tap of this slab: it has ntaps iterations to land.  (Measured in round 2: hipcc loads the
      // slab into rotated registers under this condition and moves them into place behind vmcnt waits, i.e. it waits for the rows here.  A slab loop
      // with the request outside any condition removes those waits and is 2.5 % SLOWER on the k = 11 layers, +-0 elsewhere: vmcnt retires in order, so
      // the weight fragments requested after the rows wait for them one tap later anyway, and the second workgroup of the CU covers either stall.)
      if (tap == 0 && chunk + 1 < nchunk) load_x(chunk + 1);
      // next iteration's fragments (the last iteration re-requests its own: no branch around the loads)
      const uint4* fn = frag_ptr(it + 1 < nit ? it + 1 : it);

      const int shift = (off0 + tap * dstep) - min_off;  // row shift of this tap inside the X slab
      const bf16_t* xa = Xs + (arow + shift) * XLD + kofs;
      KK_MFMA_ITER(q00, q01, q02, q03, q10, q11, q12, q13)
      asm volatile("" ::: "memory");
      if (it + 1 < nit) {
        if (tap == 0 && chunk + 1 < nchunk) store_p(chunk + 1);  // parameter loads were issued with load_x above
        if (last_tap) {
          __syncthreads();  // all waves are done with the X slab
          store_x(chunk + 1);
          __syncthreads();
        }
      }
    }
    __syncthreads();  // main-loop LDS is dead; the epilogue tile aliases it
  }

#include "kk_conv_mfma_epilogue.h"  // (shared with variant 2)
}

// ---- the WHOLE-K form: stride-1 convolutions with CinP == 128 (the stage-1 resblocks: 24 launches, more than half of the forward's conv time).
// Two 64-channel slabs ARE the whole K of such a tile, so both are staged in the prologue -- ONE request round (parameters and rows of both slabs,
// the first weight fragments), both transforms, both slabs into LDS buffers of their own, ONE barrier -- and the main loop is nothing but
// MFMAs, A-fragment reads and the next iteration's weight requests: no slab request, no transform, no barrier, no condition around a load.
// The slab-by-slab kernel above staged slab 1 in the MIDDLE of the loop (request at tap 0, then barrier / transform by all four waves with
// this workgroup's matrix pipe idle / barrier).  Also gone:
//   * dead staging rows: XR = 7 chunks per thread and slab (224 rows) where the launch's halo (taps - 1) * dil is <= 32 -- every stage-1
//     layer except 11 taps at dilation 5 -- instead of the 8 (256 rows, 242 kept) that the largest halo needs;
//   * the final iteration's weight request (the loop above re-requests its own fragments there): that iteration is peeled.
// Iteration order (slab outer, tap inner, two k-steps), operands and epilogue are those of the slab-by-slab kernel: outputs and statistics
// partials are BIT-IDENTICAL (tests/test_gpu_conv_wholek.py compares the two forms with torch.equal).
template <int XR>
struct GeoWK {
  static constexpr int SROWS = XR == 7 ? 224 : 192 + MAX_HALO;  // rows of one slab buffer
  static constexpr int SLAB = SROWS * XLD;                      // elements
  static constexpr int XS_BYTES = 2 * SLAB * 2;
  static constexpr int MAIN_BYTES = XS_BYTES + PS_BYTES;  // 73 216 / 78 976 B: two workgroups per CU in 160 KB
  static constexpr int RPP = 96;
  static constexpr int EPI_BYTES = RPP * CLD * 4;
  static constexpr int LDS_BYTES = MAIN_BYTES > EPI_BYTES ? MAIN_BYTES : EPI_BYTES;
};

template <int NRM, int XR, int EPI>
__global__ __launch_bounds__(256, 2) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv_mfma4_wholek_kernel(KKMfmaArgs a) {
  using TO = bf16_t;
  constexpr int WM = 96, BM = 2 * WM, MI16 = WM / 16, XREG = XR;
  constexpr bool ACC16 = true;
  using G = GeoWK<XR>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16_t* Xs = (bf16_t*)smem;                 // [2 slabs][SROWS][XLD]
  float* Ps = (float*)(smem + G::XS_BYTES);  // [2 slabs][3][64]
  float* Cs = (float*)smem;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  constexpr int nphase = 1, phase = 0;
  int bx, by, b;  // XCD-aware tile order, as above
  {
    const int gx = gridDim.x, gy = gridDim.y, total = gx * gy * gridDim.z;
    int lid = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
    const int per = total / 8, rem = total - per * 8;
    const int xcd = lid & 7, idx = lid >> 3;
    lid = xcd * per + (xcd < rem ? xcd : rem) + idx;
    by = lid % gy;
    const int t = lid / gy;
    bx = t % gx;
    b = t / gx;
  }
  const int q0 = bx * BM, n0 = by * BN;
  const int Lin = kk_len(a.lin, b), Lout = kk_len(a.lout, b);
  const int ntaps = a.Kw, off0 = -a.pad, dstep = a.dil, min_off = off0;
  const int xrows = BM + (ntaps - 1) * dstep;  // <= GeoWK<XR>::SROWS (the launcher picks XR by the halo)
  const bool tile_live = q0 < Lout;            // uniform over the workgroup

  const unsigned long long tr0 = TR_NOW();
  (void)tr0;
  f32x4 acc[MI16][4];
#pragma unroll
  for (int i = 0; i < MI16; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (tile_live) {
    const bf16_t* xb = a.x + (long long)b * a.xbs;
    const int nit = 2 * ntaps;
    const int lin_hi = Lin > 0 ? Lin - 1 : 0;
    const int cin_real = a.Cin > 0 ? a.Cin : a.CinP;

    // one register set and one LDS buffer per slab: xreg_s0 / load_x_s0 / ... and xreg_s1 / load_x_s1 / ...
#define KK_STG(name) name##_s0
#define KK_STG_XS Xs
#include "kk_conv_mfma_stage.h"
#define KK_STG(name) name##_s1
#define KK_STG_XS (Xs + G::SLAB)
#include "kk_conv_mfma_stage.h"
    uint4 q00, q01, q02, q03, q10, q11, q12, q13;  // B fragments of one (tap, slab) iteration, [ks][ni], one iteration ahead
    auto frag_ptr = [&](int it) __attribute__((always_inline)) -> const uint4* {
      const int chunk = it >= ntaps ? 1 : 0, tap = it - chunk * ntaps;
      // pack order: [tap][n block][chunk][wc][ks][ni][lane] x 16 bytes
      const long long blk = ((long long)tap * (a.CoutP / BN) + by) * 2 + chunk;
      return (const uint4*)a.wf + blk * 1024 + (wc * 2) * 4 * 64 + lane;
    };
    // ---- prologue: everything a tile reads except the later weight fragments, in one request round
    load_x_s0(0);
    load_x_s1(1);
    {
      const uint4* fp = frag_ptr(0);
      q00 = fp[0 * 64]; q01 = fp[1 * 64]; q02 = fp[2 * 64]; q03 = fp[3 * 64];
      q10 = fp[4 * 64]; q11 = fp[5 * 64]; q12 = fp[6 * 64]; q13 = fp[7 * 64];
      asm volatile("" ::: "memory");
    }
    store_p_s0(0);
    store_p_s1(1);
    __syncthreads();
    store_x_s0(0);  // (slab 1's rows are still landing)
    store_x_s1(1);
    __syncthreads();

    const int arow = wr * WM + (lane & 15);  // + mi*16 + tap shift
    const int kofs = 8 * (lane >> 4);
    for (int it = 0; it + 1 < nit; ++it) {
      const int chunk = it >= ntaps ? 1 : 0, tap = it - chunk * ntaps;
      const uint4* fn = frag_ptr(it + 1);
      const bf16_t* xa = Xs + chunk * G::SLAB + (arow + tap * dstep) * XLD + kofs;
      KK_MFMA_ITER(q00, q01, q02, q03, q10, q11, q12, q13)
      asm volatile("" ::: "memory");
    }
    {  // the final iteration (slab 1, last tap): no fragment request
      const bf16_t* xa = Xs + G::SLAB + (arow + (ntaps - 1) * dstep) * XLD + kofs;
      KK_MFMA_ITER_LAST(q00, q01, q02, q03, q10, q11, q12, q13)
      asm volatile("" ::: "memory");
    }
    __syncthreads();  // main-loop LDS is dead; the epilogue tile aliases it
  }

#include "kk_conv_mfma_epilogue.h"  // (shared with variant 2 and the slab-by-slab kernel)
}

// ---- the RING form: stride-1 convolutions over three or more slabs (CinP >= 192) with a halo of at most 32 rows, for the layer classes
// where it measures faster: the Linears (k = 1, plain input: Albert, bert_encoder, the 1 x 1 shortcuts) and the fused AdaIN +
// Snake layers with 3 or 7 taps (the 3-tap layers of stage 0).  The slab-by-slab kernel above gives every
// 64-channel slab a barrier / transform-and-store by all four waves / barrier gap after its last tap.  Here:
//   * two LDS slab buffers of whole-K's geometry (224 rows each; slab c lives in buffer c & 1): slab c + 1 is unpacked, transformed and stored
//     into the other buffer right behind the MFMAs of slab c's last tap -- that buffer is free since the barrier that ended slab c - 1 -- and
//     the ONE barrier at the end of slab c publishes slab c + 1 and retires slab c.  No barrier between a slab's taps, and a wave that has
//     issued its MFMAs goes on to the store without waiting for the other three;
//   * ONE register set of XR chunks (6 for k = 1: 192 rows, else 7), requested ahead of the MFMAs of slab c's first tap (as measured: behind
//     them is 1 % slower on the fused layers).  A second set, which would give a k = 1 slab two periods to land, does not fit: 1, 60 and
//     223 spilled VGPRs in the three arrangements built;
//   * the requests are unconditional: the first tap of a slab period, the tile's last slab and its final iteration are peeled, no load sits
//     under a branch, no weight fragment is requested that nobody multiplies;
//   * the AdaIN parameters of slab c + 2 are requested at slab c's first tap and stored at its last (the table's half of slab c is free since
//     slab c was stored, one barrier ago), so that the barrier at the end of slab c publishes them ahead of slab c + 1's period, which reads them.
// Iteration order, operands and epilogue are those of the slab-by-slab kernel: outputs and statistics partials are BIT-IDENTICAL
// (tests/test_gpu_conv_ring.py).  Plain inputs with two or more taps and the polyphase transposed convs measured level or slower in this
// form (-2 ... -5 % at 3 / 5 taps plain) and stay slab by slab.
template <int NRM, int XR, int EPI>
__global__ __launch_bounds__(256, 2) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv_mfma4_ring_kernel(KKMfmaArgs a) {
  using TO = bf16_t;
  constexpr int WM = 96, BM = 2 * WM, MI16 = WM / 16, XREG = XR;
  constexpr bool ACC16 = true;
  using G = GeoWK<7>;  // two buffers of 224 rows (XR = 6 fills 192 of them)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16_t* Xs = (bf16_t*)smem;                 // [2 buffers][SROWS][XLD]
  float* Ps = (float*)(smem + G::XS_BYTES);  // [2][3][64]: the half (chunk & 1) holds slab `chunk`
  float* Cs = (float*)smem;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  constexpr bool K1 = XR == 6;  // k = 1 (the Linears): one tap, no halo, plain input -- the launcher sends nothing else here
  static_assert(!(K1 && NRM), "the one-tap schedule carries no parameter pipeline");
  constexpr int nphase = 1, phase = 0;
  int bx, by, b;  // XCD-aware tile order, as above
  {
    const int gx = gridDim.x, gy = gridDim.y, total = gx * gy * gridDim.z;
    int lid = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
    const int per = total / 8, rem = total - per * 8;
    const int xcd = lid & 7, idx = lid >> 3;
    lid = xcd * per + (xcd < rem ? xcd : rem) + idx;
    by = lid % gy;
    const int t = lid / gy;
    bx = t % gx;
    b = t / gx;
  }
  const int q0 = bx * BM, n0 = by * BN;
  const int Lin = kk_len(a.lin, b), Lout = kk_len(a.lout, b);
  const int ntaps = K1 ? 1 : a.Kw, off0 = -a.pad, dstep = K1 ? 1 : a.dil, min_off = off0;
  const int xrows = BM + (ntaps - 1) * dstep;  // <= XR * 32 (the launcher picks XR by the halo)
  const bool tile_live = q0 < Lout;            // uniform over the workgroup

  const unsigned long long tr0 = TR_NOW();
  (void)tr0;
  f32x4 acc[MI16][4];
#pragma unroll
  for (int i = 0; i < MI16; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (tile_live) {
    const bf16_t* xb = a.x + (long long)b * a.xbs;
    const int nchunk = a.CinP / CK;  // >= 3
    const int lin_hi = Lin > 0 ? Lin - 1 : 0;
    const int cin_real = a.Cin > 0 ? a.Cin : a.CinP;

    // store_x writes the buffer that `stbuf` selects
    int stbuf = 0;
#define KK_STG(name) name
#define KK_STG_XS (Xs + stbuf)
#include "kk_conv_mfma_stage.h"
    // The AdaIN parameters travel one slab ahead of the rows (below), so they have a request of their own, at the addresses load_x uses
    // (kk_conv_mfma_stage.h); the one load_x issues with the rows is overwritten before anybody reads it and drops out of the loop.
    auto load_p = [&](int chunk) __attribute__((always_inline)) -> float4 {
      if (!NRM) return make_float4(0.f, 0.f, 0.f, 0.f);
      const int which = __builtin_amdgcn_readfirstlane(tid >> 6), c = chunk * CK + (tid & 15) * 4;
      const float* base = (NRM == 1 && which == 2) ? a.nrm_alpha : (which == 1 ? a.nrm_b : a.nrm_a) + (long long)b * a.nrm_stride;
      const int off = (NRM == 1 && which == 2) ? (c + 3 < a.nrm_C ? c : 0) : c;
      return *(const float4*)(base + off);
    };
    uint4 q00, q01, q02, q03, q10, q11, q12, q13;  // B fragments of one (tap, slab) iteration, [ks][ni], one iteration ahead
    auto frag_ptr = [&](int chunk, int tap) __attribute__((always_inline)) -> const uint4* {
      // pack order: [tap][n block][chunk][wc][ks][ni][lane] x 16 bytes
      const long long blk = ((long long)tap * (a.CoutP / BN) + by) * nchunk + chunk;
      return (const uint4*)a.wf + blk * 1024 + (wc * 2) * 4 * 64 + lane;
    };
    const int arow = wr * WM + (lane & 15);  // + mi*16 + tap shift
    const int kofs = 8 * (lane >> 4);
    // one (tap, slab) iteration on slab C in buffer C & 1; the next iteration's fragments are those of (FC, FT)
#define KK_RING_ITER(C, TAP, FC, FT)                                                                            \
    {                                                                                                             \
      const uint4* fn = frag_ptr(FC, FT);                                                                         \
      const bf16_t* xa = Xs + ((C) & 1) * G::SLAB + (arow + (TAP) * dstep) * XLD + kofs;                       \
      KK_MFMA_ITER(q00, q01, q02, q03, q10, q11, q12, q13)                                                       \
      asm volatile("" ::: "memory");                                                                              \
    }

    // ---- prologue: slab 0, the parameters of slabs 0 and 1, the first weight fragments
    load_x(0);
    {
      const uint4* fp = frag_ptr(0, 0);
      q00 = fp[0 * 64]; q01 = fp[1 * 64]; q02 = fp[2 * 64]; q03 = fp[3 * 64];
      q10 = fp[4 * 64]; q11 = fp[5 * 64]; q12 = fp[6 * 64]; q13 = fp[7 * 64];
      asm volatile("" ::: "memory");
    }
    float4 pnext = load_p(1);
    store_p(0);
    if (NRM) {
      preg = pnext;
      store_p(1);
    }
    __syncthreads();
    store_x(0);
    __syncthreads();

    int c = 0;
    if (K1) {
      // ---- one tap: slab c + 1 is requested ahead of slab c's MFMAs (the fragments they multiply are in flight already, the fragments
      // requested behind it are not needed before it is stored) and stored right behind them
#pragma unroll 1
      for (; c + 1 < nchunk; ++c) {
        load_x(c + 1);
        KK_RING_ITER(c, 0, c + 1, 0)
        stbuf = ((c + 1) & 1) * G::SLAB;
        store_x(c + 1);
        __syncthreads();  // publishes slab c + 1, retires slab c
      }
    } else {
      // ---- two or more taps: slab c + 1 (and the parameters of slab c + 2) requested at slab c's first tap and stored behind its last tap
#pragma unroll 1
      for (; c + 1 < nchunk; ++c) {
        pnext = load_p(c + 2 < nchunk ? c + 2 : c + 1);
        load_x(c + 1);
        KK_RING_ITER(c, 0, c, 1)
        for (int tap = 1; tap < ntaps; ++tap) {
          const bool lt = tap + 1 == ntaps;
          KK_RING_ITER(c, tap, lt ? c + 1 : c, lt ? 0 : tap + 1)
        }
        if (NRM && c + 2 < nchunk) {
          preg = pnext;
          store_p(c + 2);
        }
        stbuf = ((c + 1) & 1) * G::SLAB;
        store_x(c + 1);
        __syncthreads();  // publishes slab c + 1 (and the parameters of slab c + 2), retires slab c
      }
    }
    // ---- the last slab: MFMAs and weight requests alone; the final iteration requests nothing
    for (int tap = 0; tap + 1 < ntaps; ++tap) KK_RING_ITER(c, tap, c, tap + 1)
    {
      const bf16_t* xa = Xs + (c & 1) * G::SLAB + (arow + (ntaps - 1) * dstep) * XLD + kofs;
      KK_MFMA_ITER_LAST(q00, q01, q02, q03, q10, q11, q12, q13)
      asm volatile("" ::: "memory");
    }
#undef KK_RING_ITER
    __syncthreads();  // main-loop LDS is dead; the epilogue tile aliases it
  }

#include "kk_conv_mfma_epilogue.h"  // (shared with variant 2 and the other forms)
}

template <int NRM, int XR, int EPI>
int launch_ring(const KKMfmaArgs& a, int B, hipStream_t st) {
  using G = GeoWK<7>;
  static KKDevOnce attr_once;
  if (attr_once.first()) {
    (void)hipFuncSetAttribute((const void*)conv_mfma4_ring_kernel<NRM, XR, EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS_BYTES);
    attr_once.done();
  }
  dim3 grid(kk_cdiv(a.Q, 192), a.CoutP / BN, B);
  hipLaunchKernelGGL((conv_mfma4_ring_kernel<NRM, XR, EPI>), grid, dim3(256), G::LDS_BYTES, st, a);
  KK_CHECK_LAUNCH();
  return 0;
}

template <int NRM, int XR, int EPI>
int launch_wholek(const KKMfmaArgs& a, int B, hipStream_t st) {
  using G = GeoWK<XR>;
  static KKDevOnce attr_once;
  if (attr_once.first()) {
    (void)hipFuncSetAttribute((const void*)conv_mfma4_wholek_kernel<NRM, XR, EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS_BYTES);
    attr_once.done();
  }
  dim3 grid(kk_cdiv(a.Q, 192), a.CoutP / BN, B);
  hipLaunchKernelGGL((conv_mfma4_wholek_kernel<NRM, XR, EPI>), grid, dim3(256), G::LDS_BYTES, st, a);
  KK_CHECK_LAUNCH();
  return 0;
}

template <typename TO, int WM, int NRM>
int launch_one(const KKMfmaArgs& a, int B, hipStream_t st) {
  using G = Geo<2 * WM>;
  static KKDevOnce attr_once;
  if (attr_once.first()) {
    (void)hipFuncSetAttribute((const void*)conv_mfma4_kernel<TO, WM, NRM>, hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS_BYTES);
    attr_once.done();
  }
  const int nphase = a.mode == KK_CONVT ? a.stride : 1;
  dim3 grid(kk_cdiv(a.Q, 2 * WM), a.CoutP / BN, B * nphase);
  hipLaunchKernelGGL((conv_mfma4_kernel<TO, WM, NRM>), grid, dim3(256), G::LDS_BYTES, st, a);
  KK_CHECK_LAUNCH();
  return 0;
}

__global__ __launch_bounds__(256) void pack_w_frag_kernel(const bf16_t* w, bf16_t* wf, int Kw, int CoutP, int CinP) {
  const long long n = (long long)Kw * CoutP * CinP;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const int k = (int)(e % CinP);
    const long long r = e / CinP;
    const int cout = (int)(r % CoutP), tap = (int)(r / CoutP);
    wf[KK_MFMA4_PACK_INDEX(tap, cout, k, CoutP, CinP)] = w[e];
  }
}
}  // namespace

// device-side re-layout [Kw][CoutP][CinP] -> fragment order (the single-kernel test entry points; the model packs on the host)
int kk_launch_pack_w_frag(const void* w, void* wf, int Kw, int CoutP, int CinP, hipStream_t st) {
  if (CinP % CK != 0 || CoutP % BN != 0) return kk_fail("pack_w_frag: CinP must be a multiple of 64 and CoutP of 128");
  hipLaunchKernelGGL(pack_w_frag_kernel, dim3(1024), dim3(256), 0, st, (const bf16_t*)w, (bf16_t*)wf, Kw, CoutP, CinP);
  KK_CHECK_LAUNCH();
  return 0;
}

// what the whole-K form takes: stride-1 convolutions whose K is exactly two 64-channel slabs, halo within the slab buffers
bool kk_mfma4_wholek_eligible(const KKMfmaArgs& a) {
  return a.mode == KK_CONV && a.stride == 1 && a.CinP == 2 * CK && a.dil >= 1 && (a.Kw - 1) * a.dil <= MAX_HALO;
}

// what the ring form takes: stride-1 convolutions over three or more slabs with a halo within its 224-row buffers, in the layer classes that
// measured faster in it in every run of every pass: the Linears (one tap, plain input) and the fused AdaIN + Snake layers with 3 or
// 7 taps.  Plain inputs with more taps and the transposed convs were level or slower; the fused AdaIN + LeakyReLU layers (3 and 5 taps) were
// 1.5 - 2.8 % faster by the median but had a run inside the reference's range in one pass each; other tap counts were not measured.
static bool ring_eligible(const KKMfmaArgs& a, int nrm) {
  if (a.mode != KK_CONV || a.stride != 1 || a.CinP < 3 * CK || a.dil < 1 || (a.Kw - 1) * a.dil > 32) return false;
  return a.Kw == 1 ? nrm == 0 : (nrm == 1 && (a.Kw == 3 || a.Kw == 7));
}

int kk_launch_conv_mfma4(const KKMfmaArgs& a, int B, int out_dtype, hipStream_t st) {
  if (a.Q <= 0 || B <= 0) return 0;
  if (!a.wf) return kk_fail("conv_mfma4: fragment-order weights missing");
  const int nrm = a.nrm_a == nullptr ? 0 : (a.nrm_act == KK_ACT_SNAKE ? 1 : 2);
  if (nrm == 1 && a.nrm_C % 4 != 0) return kk_fail("conv_mfma: the fused Snake input needs a channel count that is a multiple of 4");
  KKMfmaArgs g = a;
  if (nrm == 2 && a.nrm_act != KK_ACT_LRELU) g.nrm_slope = 1.0f;  // plain AdaIN: identity activation
  if (out_dtype != KK_BF16) return kk_fail("conv_mfma4: bf16 output only");
  // The epilogue class (kk_conv_mfma_shared.h) is compiled in for the fused Snake layers of the Kokoro generator (run_resblock1 of
  // kk_model.hip; 3 taps at both stages, 7 and 11 taps where variant 5 does not take them): first convolution of a pair (statistics),
  // second one (residual + statistics), and the last second one of a resblock, which writes or adds to the mean over the three resblocks
  // (residual + scale, read-and-add, the final LeakyReLU).  Everything else runs the generic instantiation.
  const int epi = kk_epi_mask(g);
  kk_conv_epi_last = KK_EPI_GENERIC;
#define KK_EPI_CASE(LAUNCH, MASK) \
  case (MASK):                    \
    kk_conv_epi_last = (MASK);    \
    return LAUNCH(MASK)(g, B, st);
  if (kk_mfma4_wholek_eligible(g) && !g.slabwise) {
    // chunk registers per thread and slab by the launch's halo: 7 x 32 = 224 rows cover a 192-row tile with a halo of up to 32
    const bool x7 = (g.Kw - 1) * g.dil <= 32;
    if (nrm == 1 && x7) {
      switch (epi) {
#define KK_L(E) launch_wholek<1, 7, E>
        KK_EPI_CASE(KK_L, KK_EPI_STAT)
        KK_EPI_CASE(KK_L, KK_EPI_RES | KK_EPI_STAT)
        KK_EPI_CASE(KK_L, KK_EPI_RES | KK_EPI_SCALE)
        KK_EPI_CASE(KK_L, KK_EPI_RES | KK_EPI_SCALE | KK_EPI_ACC)
        KK_EPI_CASE(KK_L, KK_EPI_RES | KK_EPI_SCALE | KK_EPI_ACC | KK_EPI_POST)
#undef KK_L
        default: break;
      }
    }
    if (nrm == 1) return x7 ? launch_wholek<1, 7, KK_EPI_GENERIC>(g, B, st) : launch_wholek<1, 8, KK_EPI_GENERIC>(g, B, st);
    if (nrm == 2) return x7 ? launch_wholek<2, 7, KK_EPI_GENERIC>(g, B, st) : launch_wholek<2, 8, KK_EPI_GENERIC>(g, B, st);
    return x7 ? launch_wholek<0, 7, KK_EPI_GENERIC>(g, B, st) : launch_wholek<0, 8, KK_EPI_GENERIC>(g, B, st);
  }
  if (!g.slabwise && ring_eligible(g, nrm)) {
    if (nrm == 1) {
      switch (epi) {
#define KK_L(E) launch_ring<1, 7, E>
        KK_EPI_CASE(KK_L, KK_EPI_STAT)
        KK_EPI_CASE(KK_L, KK_EPI_RES | KK_EPI_STAT)
        KK_EPI_CASE(KK_L, KK_EPI_RES | KK_EPI_SCALE)
#undef KK_L
        default: break;
      }
    }
    return nrm == 1 ? launch_ring<1, 7, KK_EPI_GENERIC>(g, B, st) : launch_ring<0, 6, KK_EPI_GENERIC>(g, B, st);
  }
#undef KK_EPI_CASE
  if (nrm == 1) return launch_one<bf16_t, 96, 1>(g, B, st);
  if (nrm == 2) return launch_one<bf16_t, 96, 2>(g, B, st);
  return launch_one<bf16_t, 96, 0>(g, B, st);
}
