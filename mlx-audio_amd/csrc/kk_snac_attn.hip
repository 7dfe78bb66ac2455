// SNAC LocalMHA, steps 3-6 (mlx_audio/codec/models/snac/attention.py:28-41): attention inside windows of 32 frames with a rotary embedding that
// restarts in every window.  Input is the q | k | v tensor [B][T][ld >= 3 D] of the to_qkv Linear, output o [B][T][ldo >= D], heads of 64 channels:
//   q'_i = rope(q_i, i), k'_j = rope(k_j, j) for positions i, j = 0 .. 31 inside the window; P = softmax(q' k'^T / 8) over the window's 32 keys;
//   o = P v.  No mask, no look-back.  A second of 44 kHz audio is ~75 such 32 x 32 x 64 problems per item; none of them shares anything.
//
// One wave per (item, window, head); the four waves of a workgroup take neighbouring heads of one window, so the rows they fetch together are
// contiguous runs of 4 x 64 channels.  Everything but v stays in registers:
//   * lane (r = lane & 31, g = lane >> 5) loads channels 16 k + 8 g + e (k = 0 .. 3, e = 0 .. 7) of row r of q and of k: 16-byte loads, and
//     exactly the operand fragment of a 32x32 matrix instruction with the contraction over channels.  Channel c and its rotary partner c + 32
//     are chunks k and k + 2 of the SAME lane, so the embedding is applied on the loaded registers (the [32][32] cos / sin table, made once
//     in float64, is read with the lane's own position r): no rotated value ever goes to memory.
//   * S^T = k' q'^T, NOT q' k'^T: the accumulator of lane (i, g) then holds 16 of the 32 scores of QUERY i (keys j = (a & 3) + 8 (a >> 2) + 4 g,
//     a = 0 .. 15) and lane (i, 1 - g) the other 16.  Row maximum and row sum are 16-register reductions plus one exchange with lane ^ 32.
//   * O^T = v^T P^T: the contraction runs over keys, and any order of the keys will do as long as both operands use the same one.  In the order
//     the accumulator already has, the P^T operand of lane (i, g) is its own registers: no LDS trip for the scores.  v^T is the one operand
//     that needs a transpose (8 keys of one channel per lane): v goes through a per-wave LDS tile, written by rows, read by columns.
//   * the accumulator of O^T has query i in lane (i, g): 1 / sum is a per-lane scalar, and a lane stores runs of 4 channels.
// bf16: v_mfma_f32_32x32x16_bf16, 4 for S^T and 2 x 2 for O^T; the embedding and the softmax in fp32; P rounded to bf16 in registers.
// fp32: the same data flow on v_mfma_f32_32x32x2_f32 (32 + 32 instructions), fp32 operands and accumulation throughout: encode ends in an
// argmax over the code book.  An item's output is a function of its own window alone, with one fixed order of operations.
#include <math.h>

#include <mutex>

#include "kk_common.h"
#include "kk_kernels.h"

namespace {
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int AT_W = 32;       // window: queries = keys
constexpr int AT_DH = 64;      // channels per head
constexpr int AT_WAVES = 4;    // heads per workgroup
constexpr int AT_VP = 72;      // LDS row pitch of the v tile in elements: 16-byte rows, and rows j, j + 4 (the two lane groups of a column read) 16
                               // (bf16) / 32 (fp32) banks apart

__device__ float snac_rope_tab[2 * AT_W * 32];  // cos [pos][freq], then sin [pos][freq]

// the lane's 32 channels of one row: u[8 k + e] = row[16 k + 8 g + e]
__device__ __forceinline__ void at_load(const float* row, int g, float* u) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const f32x4 a = *(const f32x4*)(row + 16 * k + 8 * g), b = *(const f32x4*)(row + 16 * k + 8 * g + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { u[8 * k + e] = a[e]; u[8 * k + 4 + e] = b[e]; }
  }
}
__device__ __forceinline__ void at_load(const bf16_t* row, int g, float* u) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint4 a = *(const uint4*)(row + 16 * k + 8 * g);
    const unsigned w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) { u[8 * k + 2 * e] = __uint_as_float(w[e] << 16); u[8 * k + 2 * e + 1] = __uint_as_float(w[e] & 0xFFFF0000u); }
  }
}
// u' = u cos + rot(u) sin, rot(u)[c] = -u[c + 32] (c < 32), u[c - 32] (c >= 32): channel 16 k + 8 g + e (k < 2) is u[8 k + e], its partner u[8 k + e + 16]
__device__ __forceinline__ void at_rope(float* u, const float* cs, const float* sn) {
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const float lo = u[s], hi = u[s + 16];
    u[s] = lo * cs[s] - hi * sn[s];
    u[s + 16] = hi * cs[s] + lo * sn[s];
  }
}

template <typename T>
__global__ __launch_bounds__(64 * AT_WAVES) void snac_local_attn_kernel(const T* qkv, int ld, int Tn, int H, T* out, int ldo) {
  constexpr bool BF = sizeof(T) == 2;
  __shared__ __attribute__((aligned(16))) T vs_all[AT_WAVES][AT_W * AT_VP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, g = lane >> 5;
  const int h = blockIdx.y * AT_WAVES + wave, D = H * AT_DH;
  const bool live = h < H;  // (uniform over the wave; the barrier below is reached by every wave)
  T* vs = vs_all[wave];
  const long long row0 = (long long)blockIdx.z * Tn + (long long)blockIdx.x * AT_W;
  f32x16 acc;
#pragma unroll
  for (int a = 0; a < 16; ++a) acc[a] = 0.f;
  if (live) {
    const T* base = qkv + (row0 + r) * ld + h * AT_DH;
    // v first: its trip through LDS overlaps the first product
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if constexpr (BF) {
        *(uint4*)(vs + r * AT_VP + 16 * k + 8 * g) = *(const uint4*)(base + 2 * D + 16 * k + 8 * g);
      } else {
        *(f32x4*)(vs + r * AT_VP + 16 * k + 8 * g) = *(const f32x4*)(base + 2 * D + 16 * k + 8 * g);
        *(f32x4*)(vs + r * AT_VP + 16 * k + 8 * g + 4) = *(const f32x4*)(base + 2 * D + 16 * k + 8 * g + 4);
      }
    }
    float cs[16], sn[16], q[32], kk[32];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        cs[8 * k + e] = snac_rope_tab[r * 32 + 16 * k + 8 * g + e];
        sn[8 * k + e] = snac_rope_tab[AT_W * 32 + r * 32 + 16 * k + 8 * g + e];
      }
    at_load(base, g, q);
    at_load(base + D, g, kk);
    at_rope(q, cs, sn);
    at_rope(kk, cs, sn);
    // S^T[j][i] = sum_c k'[j][c] q'[i][c]: A = k' (row j = r), B = q' (column i = r)
    if constexpr (BF) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        bf16x8 af, bfr;
#pragma unroll
        for (int e = 0; e < 8; ++e) { af[e] = (bf16_t)kk[8 * k + e]; bfr[e] = (bf16_t)q[8 * k + e]; }
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr, acc, 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int s = 0; s < 32; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kk[s], q[s], acc, 0, 0, 0);
    }
  }
  // softmax over the 32 keys of query i = r: 16 here, 16 in lane ^ 32.  exp((s - max) / 8) = exp2((s - max) * log2(e) / 8)
  float mx = acc[0];
#pragma unroll
  for (int a = 1; a < 16; ++a) mx = fmaxf(mx, acc[a]);
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  float p[16], sum = 0.f;
#pragma unroll
  for (int a = 0; a < 16; ++a) {
    p[a] = __builtin_amdgcn_exp2f((acc[a] - mx) * 0.18033688011112042f);
    sum += p[a];
  }
  sum += __shfl_xor(sum, 32);  // (a + b == b + a: both lanes of a query hold the same sum)
  const float inv = 1.0f / sum;
  __syncthreads();  // the v tile is written (each wave reads its own tile only)
  if (!live) return;
  // O^T[c][i] = sum_j v[j][c] P[i][j], the keys in the accumulator's order j(a, g) = (a & 3) + 8 (a >> 2) + 4 g: A = v^T (row c = 32 half + r), B = P^T
  f32x16 o[2];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int a = 0; a < 16; ++a) o[half][a] = 0.f;
    const T* vc = vs + 4 * g * AT_VP + 32 * half + r;
    if constexpr (BF) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        bf16x8 af, bfr;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          af[e] = vc[((e & 3) + 8 * (e >> 2) + 16 * t) * AT_VP];
          bfr[e] = (bf16_t)p[8 * t + e];
        }
        o[half] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr, o[half], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int a = 0; a < 16; ++a) o[half] = __builtin_amdgcn_mfma_f32_32x32x2f32(vc[((a & 3) + 8 * (a >> 2)) * AT_VP], p[a], o[half], 0, 0, 0);
    }
  }
  // lane (i, g) holds channels 32 half + 8 m + 4 g + (0 .. 3) of query i
  T* orow = out + (row0 + r) * ldo + h * AT_DH + 4 * g;
#pragma unroll
  for (int half = 0; half < 2; ++half)
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const float v0 = o[half][4 * m] * inv, v1 = o[half][4 * m + 1] * inv, v2 = o[half][4 * m + 2] * inv, v3 = o[half][4 * m + 3] * inv;
      T* dst = orow + 32 * half + 8 * m;
      if constexpr (BF) {
        typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
        *(bf16x4*)dst = bf16x4{(bf16_t)v0, (bf16_t)v1, (bf16_t)v2, (bf16_t)v3};
      } else {
        *(f32x4*)dst = f32x4{v0, v1, v2, v3};
      }
    }
}

// the rotary table of attention.py:46-77 without xpos: angle(i, j) = i * 10000^(-2 j / 64), in float64, once per device
int rope_table_ready() {
  static KKDevOnce once;
  static std::mutex mu;
  if (!once.first()) return 0;
  std::lock_guard<std::mutex> lk(mu);
  if (!once.first()) return 0;
  static float tab[2 * AT_W * 32];
  for (int i = 0; i < AT_W; ++i)
    for (int j = 0; j < 32; ++j) {
      const double th = (double)i * pow(10000.0, -2.0 * j / AT_DH);
      tab[i * 32 + j] = (float)cos(th);
      tab[AT_W * 32 + i * 32 + j] = (float)sin(th);
    }
  const hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(snac_rope_tab), tab, sizeof tab);  // (blocking: the table is there before any launch)
  if (e != hipSuccess) return kk_fail(hipGetErrorString(e));
  once.done();
  return 0;
}
}  // namespace

int snac_launch_local_attn(const void* qkv, int ld, int dtype, int T, int H, void* out, int ldo, int B, hipStream_t st) {
  if (rope_table_ready() != 0) return -1;
  const dim3 grid(T / AT_W, kk_cdiv(H, AT_WAVES), B);
  if (dtype == KK_BF16)
    hipLaunchKernelGGL(snac_local_attn_kernel<bf16_t>, grid, dim3(64 * AT_WAVES), 0, st, (const bf16_t*)qkv, ld, T, H, (bf16_t*)out, ldo);
  else
    hipLaunchKernelGGL(snac_local_attn_kernel<float>, grid, dim3(64 * AT_WAVES), 0, st, (const float*)qkv, ld, T, H, (float*)out, ldo);
  KK_CHECK_LAUNCH();
  return 0;
}
