// Row-table ring copies (ABI minor 13): what a continuous listener's samples take into and out of its ring, for every row in
// one launch.  The table (kk_ring_host.h) travels as a launch argument, as the resampler's does.
//   write:  ring[b][(pos[b] + i) % ring_len] = src[b][i]                       i < n[b]
//   read:   dst[b][i] = ring[b][(pos[b] + i) % ring_len]   i < n[b];   0.0f    n[b] <= i < n_total[b]
// A row whose two sides are 16-byte aligned and whose run does not wrap moves in groups of four floats; any other row goes element by
// element, the address modulo the ring by one conditional subtract.  The result is a copy either way: no arithmetic touches a sample.
#include "../../include/kokoro_hip.h"
#include "kk_host.h"
#include "kk_ring_host.h"

#define RING_MAX_BLOCKS 64  // workgroups per row; a longer row strides

template <bool READ>
__global__ __launch_bounds__(256) void ring_rows_kernel(RingRows t, const float* from, long long ldfrom, float* to, long long ldto, long long ring_len) {
  const int row = blockIdx.y, n = t.n[row], tot = t.n_total[row];
  if (tot == 0) return;  // the row sits out: nothing of it is touched
  const long long off = t.off[row];
  const float* f = from + row * ldfrom;
  float* o = to + row * ldto;
  const int stride = gridDim.x * 256, i0 = blockIdx.x * 256 + threadIdx.x;
  if (t.vec[row]) {  // groups of four: whole groups below n are copied, whole groups behind it are zeros (a read), a mixed one goes by elements
    const float* fr = READ ? f + off : f;
    float* orun = READ ? o : o + off;
    for (int g = i0; g * 4 < tot; g += stride) {
      const int i = g * 4;
      if (i + 4 <= n) {
        *reinterpret_cast<float4*>(orun + i) = *reinterpret_cast<const float4*>(fr + i);
      } else if (READ && i >= n && i + 4 <= tot) {
        *reinterpret_cast<float4*>(orun + i) = make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        for (int j = i; j < min(i + 4, tot); ++j) orun[j] = j < n ? fr[j] : 0.f;
      }
    }
    return;
  }
  for (int i = i0; i < tot; i += stride) {
    long long a = off + i;  // off < ring_len and i < n <= ring_len: one subtract
    if (a >= ring_len) a -= ring_len;
    if (READ) o[i] = i < n ? f[a] : 0.f;
    else o[a] = f[i];
  }
}

static dim3 ring_grid(const RingPlan& plan, int rows) {
  const long long blocks = (plan.longest + 1023) / 1024;
  return dim3((unsigned)(blocks < RING_MAX_BLOCKS ? blocks : RING_MAX_BLOCKS), (unsigned)rows);
}

extern "C" int kk_ring_write_rows(void* stream, int rows, const float* src, long long lds, float* ring, long long ldr, long long ring_len,
                                  const int64_t* pos, const int32_t* n) {
  const char* who = "kk_ring_write_rows";
  RingPlan plan;
  KK_TRY(ring_plan(kk_failf, who, rows, (uintptr_t)src, lds, (uintptr_t)ring, ldr, ring_len, pos, n, nullptr, &plan));
  if (plan.longest == 0) return 0;
  if (!src || !ring) return kk_failf("%s: null src or ring", who);
  hipLaunchKernelGGL(ring_rows_kernel<false>, ring_grid(plan, rows), dim3(256), 0, (hipStream_t)stream, plan.t, src, lds, ring, ldr, ring_len);
  KK_CHECK_LAUNCH();
  return 0;
}

extern "C" int kk_ring_read_rows(void* stream, int rows, const float* ring, long long ldr, long long ring_len, float* dst, long long ldd,
                                 const int64_t* pos, const int32_t* n, const int32_t* n_total) {
  const char* who = "kk_ring_read_rows";
  if (!n_total) return kk_failf("%s: null n_total", who);
  RingPlan plan;
  KK_TRY(ring_plan(kk_failf, who, rows, (uintptr_t)dst, ldd, (uintptr_t)ring, ldr, ring_len, pos, n, n_total, &plan));
  if (plan.longest == 0) return 0;
  if (!dst || !ring) return kk_failf("%s: null dst or ring", who);
  hipLaunchKernelGGL(ring_rows_kernel<true>, ring_grid(plan, rows), dim3(256), 0, (hipStream_t)stream, plan.t, ring, ldr, dst, ldd, ring_len);
  KK_CHECK_LAUNCH();
  return 0;
}
