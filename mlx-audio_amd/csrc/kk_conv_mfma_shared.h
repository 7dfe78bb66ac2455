// Helpers shared by the MFMA convolution kernels (variants 2, 4, 5).
#pragma once
#include <hip/hip_runtime.h>

namespace {
// Two floats WITHOUT the packed-f32 instructions (v_pk_fma_f32 ...): beside another wave's MFMAs on the same SIMD the packed forms run at
// about half rate (variant 5's service waves showed it first; 2-6 % per fused launch of variant 4).  The files that include this are built
// with -fno-slp-vectorize for the same reason (build.py FILE_FLAGS).
struct v2f {
  float x, y;
};
__device__ __forceinline__ v2f operator*(v2f a, v2f b) { return v2f{a.x * b.x, a.y * b.y}; }
__device__ __forceinline__ v2f& operator+=(v2f& a, v2f b) { a.x += b.x; a.y += b.y; return a; }
__device__ __forceinline__ v2f& operator*=(v2f& a, v2f b) { a.x *= b.x; a.y *= b.y; return a; }
__device__ __forceinline__ v2f fma2(v2f a, v2f b, v2f c) { return v2f{__builtin_fmaf(a.x, b.x, c.x), __builtin_fmaf(a.y, b.y, c.y)}; }
// nn.gelu (exact erf form, modules.py / transformer feed-forward)
__device__ __forceinline__ float gelu_exact(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

// Epilogue class of a launch (template parameter EPI of the fused kernels of variants 4 / 5).  KK_EPI_GENERIC keeps every choice a uniform
// runtime branch on the arguments (any activation, GELU and GELU-tanh included).  Every other value is a mask of the bits below and states
// the launch at compile time: no output activation, and residual / scale != 1 / final LeakyReLU / statistics / read-and-add exactly as the
// bits say, so that the code of the paths not taken -- the erff and tanhf expansions above all -- is not in the kernel.  The arithmetic of
// a path is the same text in both forms.  The launchers compute the mask from the arguments (kk_epi_mask) and instantiate the masks that
// the Kokoro generator launches on each kernel; everything else runs the generic instantiation.
constexpr int KK_EPI_GENERIC = -1;
constexpr int KK_EPI_RES = 1, KK_EPI_SCALE = 2, KK_EPI_POST = 4, KK_EPI_STAT = 8, KK_EPI_ACC = 16;
#define KK_EPI_ON(EPI, BIT, RUNTIME) ((EPI) < 0 ? (RUNTIME) : (((EPI) & (BIT)) != 0))
// the mask of a launch, or KK_EPI_GENERIC where a mask cannot state it (an output activation, flat rows) or the debug switch asks for it
inline int kk_epi_mask(const KKMfmaArgs& a) {
  if (kk_conv_epi_generic || a.act != KK_ACT_NONE || a.flat_T) return KK_EPI_GENERIC;
  return (a.res ? KK_EPI_RES : 0) | (a.scale != 1.0f ? KK_EPI_SCALE : 0) | (a.post_slope != 0.f && a.post_slope != 1.0f ? KK_EPI_POST : 0) |
         (a.stat_part ? KK_EPI_STAT : 0) | (a.accumulate ? KK_EPI_ACC : 0);
}

typedef float kk_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 kk_bf16x8 __attribute__((ext_vector_type(8)));

// One (tap, slab) iteration of the main loop of variants 4 / 5 on v_mfma_f32_16x16x32_bf16: two k-steps of 32 channels, the B fragments in
// named registers [ks][ni] (fragment order, kk_mfma4_pack_index).  Per k-step this wave's 4 B fragments (4 x 16 columns) stay in registers
// while the MI16 A fragments stream through from the X slab in LDS; the B registers are refilled from fn (the next iteration's fragments)
// as soon as their MFMAs are issued.  Issue order: the A fragment of row block mi + 1 is read from LDS while the 4 MFMAs of row block mi
// run, and the four global loads that refill a k-step's B registers go out right behind that k-step's MFMAs.
// Names taken from the including scope: acc (kk_f32x4 [MI16][4]), xa (this lane's row and k-group at the tap's row shift), fn, MI16, XLD.
// Macros, not functions: an always_inline function of the same body changes the kernels' register allocation.
#define KK_MFMA_KSTEP(KS, B0, B1, B2, B3)                                                                                                  \
  {                                                                                                                                          \
    const kk_bf16x8 b0 = __builtin_bit_cast(kk_bf16x8, B0), b1 = __builtin_bit_cast(kk_bf16x8, B1);                                          \
    const kk_bf16x8 b2 = __builtin_bit_cast(kk_bf16x8, B2), b3 = __builtin_bit_cast(kk_bf16x8, B3);                                          \
    _Pragma("unroll") for (int mi = 0; mi < MI16; ++mi) {                                                                                    \
      const kk_bf16x8 av = *(const kk_bf16x8*)(xa + mi * 16 * XLD + (KS) * 32);                                                              \
      acc[mi][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, b0, acc[mi][0], 0, 0, 0);                                                     \
      acc[mi][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, b1, acc[mi][1], 0, 0, 0);                                                     \
      acc[mi][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, b2, acc[mi][2], 0, 0, 0);                                                     \
      acc[mi][3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, b3, acc[mi][3], 0, 0, 0);                                                     \
    }                                                                                                                                        \
    B0 = fn[((KS) * 4 + 0) * 64];                                                                                                            \
    B1 = fn[((KS) * 4 + 1) * 64];                                                                                                            \
    B2 = fn[((KS) * 4 + 2) * 64];                                                                                                            \
    B3 = fn[((KS) * 4 + 3) * 64];                                                                                                            \
  }
#define KK_MFMA_ITER(Q00, Q01, Q02, Q03, Q10, Q11, Q12, Q13)                                                                               \
  KK_MFMA_KSTEP(0, Q00, Q01, Q02, Q03)                                                                                                     \
  KK_MFMA_KSTEP(1, Q10, Q11, Q12, Q13)                                                                                                     \
  __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                                                                                         \
  _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                                                                                         \
    _Pragma("unroll") for (int j = 0; j < MI16; ++j) {                                                                                       \
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);                                                                                     \
      if (ks * MI16 + j + 2 < 2 * MI16) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                                   \
    }                                                                                                                                        \
    __builtin_amdgcn_sched_group_barrier(0x020, 4, 0);                                                                                       \
  }
// The same iteration with NO refill of the B registers: a tile's final (tap, slab) iteration where it is peeled off the loop (the whole-K
// form of variant 4), so that no fragment set is requested that nobody multiplies.  Same MFMAs on the same operands in the same order.
#define KK_MFMA_KSTEP_LAST(KS, B0, B1, B2, B3)                                                                                             \
  {                                                                                                                                          \
    const kk_bf16x8 b0 = __builtin_bit_cast(kk_bf16x8, B0), b1 = __builtin_bit_cast(kk_bf16x8, B1);                                          \
    const kk_bf16x8 b2 = __builtin_bit_cast(kk_bf16x8, B2), b3 = __builtin_bit_cast(kk_bf16x8, B3);                                          \
    _Pragma("unroll") for (int mi = 0; mi < MI16; ++mi) {                                                                                    \
      const kk_bf16x8 av = *(const kk_bf16x8*)(xa + mi * 16 * XLD + (KS) * 32);                                                              \
      acc[mi][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, b0, acc[mi][0], 0, 0, 0);                                                     \
      acc[mi][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, b1, acc[mi][1], 0, 0, 0);                                                     \
      acc[mi][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, b2, acc[mi][2], 0, 0, 0);                                                     \
      acc[mi][3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, b3, acc[mi][3], 0, 0, 0);                                                     \
    }                                                                                                                                        \
  }
#define KK_MFMA_ITER_LAST(Q00, Q01, Q02, Q03, Q10, Q11, Q12, Q13)                                                                          \
  KK_MFMA_KSTEP_LAST(0, Q00, Q01, Q02, Q03)                                                                                                \
  KK_MFMA_KSTEP_LAST(1, Q10, Q11, Q12, Q13)                                                                                                \
  __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                                                                                         \
  _Pragma("unroll") for (int j = 0; j < 2 * MI16; ++j) {                                                                                     \
    __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);                                                                                       \
    if (j + 2 < 2 * MI16) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                                                 \
  }
}  // namespace
