// Row-mode voice-activity detector (ABI minor 12): endpointing and barge-in for the listening edge of CSM serving.  The
// reference's fallback detector (mlx_audio/sts/voice_pipeline.py _is_silent, _listener) as one launch per listen round:
//   frame f of a row's stream is speech iff E = sum_i x[f frame_len + i]^2 >= thr2n = threshold^2 frame_len   (rms >= threshold)
//   speech: speaking = 1, silent = 0, last_speech = f, onset = f if there was none;  silence while speaking: ++silent, and
//   silent > hang_frames ends the row at endpoint = f;  silence before any speech does nothing.
// One workgroup of 4 waves per row.  A frame's energy is ONE wave's work in ONE fixed order -- lane l runs acc = fmaf(x, x, acc) from 0.0f
// over i = l, l + 64, ... ascending, then an xor butterfly over 32, 16, 8, 4, 2, 1 adds the 64 partial sums -- so E's bits depend on the
// frame's samples alone, never on the step, the row or the neighbours.  Wave w takes new frames w, w + 4, ... of a batch of at most
// VAD_BATCH frames and leaves E in LDS; behind the barrier one lane walks the batch in frame order through the state machine.
// A NaN energy compares false and reads as silence.  The row's state stays on the device; the host mirrors the frame count with integers.
// Below the flat detector: the same energy routine over a ring, with a state machine that re-arms behind every utterance (kk_vad_ring; ABI minor 13).
#include "../../include/kokoro_hip.h"
#include "kk_host.h"
#include "kk_vad_host.h"
#include "kk_vad_ring_host.h"

static_assert(VAD_LOG == KK_VAD_LOG, "kk_vad_ring_host.h and kokoro_hip.h disagree");

// The energy of one frame, by one wave: lane l runs fmaf from 0.0f over i = l, l + 64, ... ascending, then the xor butterfly over 32 ... 1.
// The frame starts at xr[off]; RING: sample i lives at (off + i) modulo ring_len -- off < ring_len and frame_len <= ring_len, so one
// conditional subtract -- and only the address differs from the flat form: the same values enter the same chain in the same order.
template <bool RING>
__device__ static inline float vad_frame_energy(const float* xr, long long off, int fl, long long ring_len, int lane) {
  float acc = 0.f;
  for (int i = lane; i < fl; i += 64) {
    long long a = off + i;
    if (RING && a >= ring_len) a -= ring_len;
    const float v = xr[a];
    acc = fmaf(v, v, acc);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
  return acc;
}

struct VadRow {  // device state of one row
  int frame_len, hang;
  float thr2n;
  int classified, onset, last_speech, endpoint;  // what status[row] shows; -1: none
  int speaking, silent;
};

struct VadSteps {
  int32_t upto[VAD_MAX_ROWS];
};

__global__ void vad_set_row_kernel(VadRow* rows, int row, int frame_len, float thr2n, int hang) {
  if (threadIdx.x != 0) return;
  VadRow r;
  r.frame_len = frame_len, r.hang = hang, r.thr2n = thr2n;
  r.classified = 0, r.onset = -1, r.last_speech = -1, r.endpoint = -1, r.speaking = 0, r.silent = 0;
  rows[row] = r;
}

__global__ __launch_bounds__(256) void vad_rows_kernel(VadRow* rows, VadSteps steps, const float* x, long long ldx, int32_t* status, float* energy,
                                                       long long lde) {
  __shared__ float e_s[VAD_BATCH];
  __shared__ int walked_s[2];  // frames of the batch the walk classified, and whether it met the endpoint
  const int row = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int upto = steps.upto[row];
  if (upto < 0) return;  // a row that sits out: nothing of it is read
  VadRow r = rows[row];
  if (r.endpoint >= 0 || upto <= r.classified) return;  // the row has ended: state and status stay
  const int fl = r.frame_len, first = r.classified;
  const float* xr = x + row * ldx;
  for (int b0 = first; b0 < upto; b0 += VAD_BATCH) {
    const int nb = min(VAD_BATCH, upto - b0);
    for (int k = wave; k < nb; k += 4) {
      const float acc = vad_frame_energy<false>(xr, (long long)(b0 + k) * fl, fl, 0, lane);
      if (lane == 0) e_s[k] = acc;
    }
    __syncthreads();
    if (tid == 0) {
      int k = 0;
      for (; k < nb && r.endpoint < 0; ++k) {
        if (e_s[k] >= r.thr2n) {
          r.speaking = 1, r.silent = 0, r.last_speech = b0 + k;
          if (r.onset < 0) r.onset = b0 + k;
        } else if (r.speaking && ++r.silent > r.hang) {
          r.endpoint = b0 + k;
        }
      }
      r.classified = b0 + k;
      walked_s[0] = k, walked_s[1] = r.endpoint >= 0;
    }
    __syncthreads();
    const int walked = walked_s[0], ended = walked_s[1];
    if (energy)
      for (int k = tid; k < walked; k += 256) energy[row * lde + (b0 - first) + k] = e_s[k];
    __syncthreads();  // e_s and walked_s are written again by the next batch
    if (ended) break;
  }
  if (tid == 0) {
    rows[row] = r;
    int32_t* s = status + row * 4;
    s[0] = r.classified, s[1] = r.onset, s[2] = r.last_speech, s[3] = r.endpoint;
  }
}

// ---- the re-arming detector over a ring (ABI minor 13) -------------------------------------------------------------------
// A row's stream is numbered from 0 at set_row in 64-bit positions; sample p lives at x[row][p % ring_len].  The state machine is the flat
// one with the reset the reference's `while True` does behind an utterance: closing (silent > hang, or the utterance reaching max_frames:
// flag 1, "forced") appends {onset, last_speech, endpoint, flags} to the row's log of VAD_LOG records and re-arms, and the walk goes on
// with the next frame in the same launch.  The walking lane stops in front of any frame while closed - acked == VAD_LOG; a later step
// resumes from the device's own `classified`.
struct VadRingRow {
  int frame_len, hang;
  float thr2n;
  int speaking;
  long long max_frames, ring_len;
  long long classified, closed, onset, last_speech;  // what status[row] shows; -1: no open utterance
  long long silent;
};

struct VadRingSteps {
  int64_t upto[VAD_MAX_ROWS];
  int64_t acked[VAD_MAX_ROWS];
};

__global__ void vad_ring_set_row_kernel(VadRingRow* rows, int row, int frame_len, float thr2n, int hang, long long max_frames, long long ring_len) {
  if (threadIdx.x != 0) return;
  VadRingRow r;
  r.frame_len = frame_len, r.hang = hang, r.thr2n = thr2n, r.speaking = 0, r.max_frames = max_frames, r.ring_len = ring_len;
  r.classified = 0, r.closed = 0, r.onset = -1, r.last_speech = -1, r.silent = 0;
  rows[row] = r;
}

__global__ __launch_bounds__(256) void vad_ring_rows_kernel(VadRingRow* rows, VadRingSteps steps, const float* x, long long ldx, int64_t* status,
                                                            int64_t* log, float* energy, long long lde) {
  __shared__ float e_s[VAD_BATCH];
  __shared__ int walked_s[2];  // frames of the batch the walk classified, and whether it stopped in front of a full log
  const int row = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long upto = steps.upto[row], acked = steps.acked[row];
  if (upto < 0) return;  // a row that sits out: nothing of it is read
  VadRingRow r = rows[row];
  if (upto <= r.classified || r.closed - acked >= VAD_LOG) return;  // nothing new, or the log is still full: state and status stay
  const int fl = r.frame_len;
  const long long ring_len = r.ring_len;
  const float* xr = x + row * ldx;
  int64_t* lg = log + (long long)row * VAD_LOG * 4;
  for (long long b0 = r.classified; b0 < upto; b0 += VAD_BATCH) {
    const int nb = (int)min((long long)VAD_BATCH, upto - b0);
    for (int k = wave; k < nb; k += 4) {
      const long long off = ((b0 + k) * fl) % ring_len;  // the frame's first position in the ring; (b0 + k + 1) fl <= n_avail: no overflow
      const float acc = vad_frame_energy<true>(xr, off, fl, ring_len, lane);
      if (lane == 0) e_s[k] = acc;
    }
    __syncthreads();
    if (tid == 0) {
      int k = 0, stalled = 0;
      for (; k < nb; ++k) {
        if (r.closed - acked >= VAD_LOG) {
          stalled = 1;
          break;
        }
        const long long f = b0 + k;
        int close = 0, flags = 0;
        if (e_s[k] >= r.thr2n) {
          r.speaking = 1, r.silent = 0, r.last_speech = f;
          if (r.onset < 0) r.onset = f;
        } else if (r.speaking && ++r.silent > r.hang) {
          close = 1;
        }
        if (!close && r.speaking && f - r.onset + 1 == r.max_frames) close = 1, flags = 1;
        if (close) {
          int64_t* rec = lg + (r.closed % VAD_LOG) * 4;
          rec[0] = r.onset, rec[1] = r.last_speech, rec[2] = f, rec[3] = flags;
          ++r.closed;
          r.speaking = 0, r.silent = 0, r.onset = -1, r.last_speech = -1;
        }
      }
      r.classified = b0 + k;
      walked_s[0] = k, walked_s[1] = stalled;
    }
    __syncthreads();
    const int walked = walked_s[0], stalled = walked_s[1];
    if (energy)
      for (int k = tid; k < walked; k += 256) energy[row * lde + (b0 + k) % lde] = e_s[k];
    __syncthreads();  // e_s and walked_s are written again by the next batch
    if (stalled) break;
  }
  if (tid == 0) {
    rows[row] = r;
    int64_t* s = status + row * 4;
    s[0] = r.classified, s[1] = r.closed, s[2] = r.onset, s[3] = r.last_speech;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
struct kk_vad {
  VadHost host;
  VadRow* d_rows = nullptr;
};

extern "C" void kk_vad_destroy(kk_vad* v) {
  if (!v) return;
  if (v->d_rows) (void)hipFree(v->d_rows);
  delete v;
}

extern "C" int kk_vad_create(int max_rows, kk_vad** out) {
  const char* who = "kk_vad_create";
  if (!out) return kk_failf("%s: null out", who);
  *out = nullptr;
  if (max_rows < 1 || max_rows > VAD_MAX_ROWS) return kk_failf("%s: max_rows %d is outside [1, %d]", who, max_rows, VAD_MAX_ROWS);
  kk_vad* v = new kk_vad;
  v->host.fail = kk_failf;
  v->host.rows.resize(max_rows);
  if (hipMalloc((void**)&v->d_rows, sizeof(VadRow) * max_rows) != hipSuccess) {
    kk_vad_destroy(v);
    return kk_failf("%s: allocation failed", who);
  }
  *out = v;
  return 0;
}

extern "C" int kk_vad_set_row(kk_vad* v, void* stream, int row, int frame_len, float thr2n, int hang_frames) {
  const char* who = "kk_vad_set_row";
  if (!v) return kk_failf("%s: null detector", who);
  KK_TRY(v->host.check_set_row(who, row, frame_len, thr2n, hang_frames));
  hipLaunchKernelGGL(vad_set_row_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, v->d_rows, row, frame_len, thr2n, hang_frames);
  KK_CHECK_LAUNCH();
  v->host.set_row(row, frame_len, thr2n, hang_frames);
  return 0;
}

extern "C" int kk_vad_step(kk_vad* v, void* stream, const float* x, long long ldx, const int32_t* n_avail, int32_t* status, float* energy,
                           long long lde) {
  const char* who = "kk_vad_step";
  if (!v) return kk_failf("%s: null detector", who);
  VadPlan plan;
  KK_TRY(v->host.plan_step(who, n_avail, ldx, energy != nullptr, lde, &plan));
  if (plan.rows_in > 0) {
    if (!x || !status) return kk_failf("%s: null x or status", who);
    VadSteps steps;
    memcpy(steps.upto, plan.upto, sizeof steps.upto);
    hipLaunchKernelGGL(vad_rows_kernel, dim3((unsigned)v->host.rows.size()), dim3(256), 0, (hipStream_t)stream, v->d_rows, steps, x, ldx, status,
                       energy, lde);
    KK_CHECK_LAUNCH();
  }
  v->host.commit_step(n_avail, plan);
  return 0;
}

extern "C" int kk_op_vad(void* stream, const float* x, int n, int frame_len, float thr2n, int hang_frames, int32_t status_host[4], float* energy_or_null) {
  const char* who = "kk_op_vad";
  if (n < 1 || !x || !status_host) return kk_failf("%s: n must be >= 1, x and status_host not null", who);
  hipStream_t st = (hipStream_t)stream;
  kk_vad* v = nullptr;
  KK_TRY(kk_vad_create(1, &v));
  int32_t* d_status = nullptr;
  const int32_t init[4] = {0, -1, -1, -1}, n_avail = n;
  int rc = kk_vad_set_row(v, stream, 0, frame_len, thr2n, hang_frames);
  if (rc == 0 && (hipMalloc((void**)&d_status, sizeof init) != hipSuccess || hipMemcpyAsync(d_status, init, sizeof init, hipMemcpyHostToDevice, st) != hipSuccess))
    rc = kk_failf("%s: allocation failed", who);
  if (rc == 0) rc = kk_vad_step(v, stream, x, n, &n_avail, d_status, energy_or_null, n / (frame_len > 0 ? frame_len : 1));
  if (rc == 0 && hipMemcpyAsync(status_host, d_status, sizeof init, hipMemcpyDeviceToHost, st) != hipSuccess) rc = kk_failf("%s: status copy failed", who);
  if (hipStreamSynchronize(st) != hipSuccess && rc == 0) rc = kk_failf("%s: stream sync failed", who);
  if (d_status) (void)hipFree(d_status);
  kk_vad_destroy(v);
  return rc;
}

struct kk_vad_ring {
  VadRingHost host;
  VadRingRow* d_rows = nullptr;
};

extern "C" void kk_vad_ring_destroy(kk_vad_ring* v) {
  if (!v) return;
  if (v->d_rows) (void)hipFree(v->d_rows);
  delete v;
}

extern "C" int kk_vad_ring_create(int max_rows, kk_vad_ring** out) {
  const char* who = "kk_vad_ring_create";
  if (!out) return kk_failf("%s: null out", who);
  *out = nullptr;
  if (max_rows < 1 || max_rows > VAD_MAX_ROWS) return kk_failf("%s: max_rows %d is outside [1, %d]", who, max_rows, VAD_MAX_ROWS);
  kk_vad_ring* v = new kk_vad_ring;
  v->host.fail = kk_failf;
  v->host.rows.resize(max_rows);
  if (hipMalloc((void**)&v->d_rows, sizeof(VadRingRow) * max_rows) != hipSuccess) {
    kk_vad_ring_destroy(v);
    return kk_failf("%s: allocation failed", who);
  }
  *out = v;
  return 0;
}

extern "C" int kk_vad_ring_set_row(kk_vad_ring* v, void* stream, int row, int frame_len, float thr2n, int hang_frames, long long max_frames,
                                   long long ring_len) {
  const char* who = "kk_vad_ring_set_row";
  if (!v) return kk_failf("%s: null detector", who);
  KK_TRY(v->host.check_set_row(who, row, frame_len, thr2n, hang_frames, max_frames, ring_len));
  hipLaunchKernelGGL(vad_ring_set_row_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, v->d_rows, row, frame_len, thr2n, hang_frames, max_frames,
                     ring_len);
  KK_CHECK_LAUNCH();
  v->host.set_row(row, frame_len, thr2n, hang_frames, max_frames, ring_len);
  return 0;
}

extern "C" int kk_vad_ring_step(kk_vad_ring* v, void* stream, const float* x, long long ldx, const int64_t* n_avail, const int64_t* acked,
                                int64_t* status, int64_t* log, float* energy, long long lde) {
  const char* who = "kk_vad_ring_step";
  if (!v) return kk_failf("%s: null detector", who);
  VadRingPlan plan;
  KK_TRY(v->host.plan_step(who, n_avail, acked, ldx, energy != nullptr, lde, &plan));
  if (plan.rows_in > 0) {
    if (!x || !status || !log) return kk_failf("%s: null x, status or log", who);
    VadRingSteps steps;
    memcpy(steps.upto, plan.upto, sizeof steps.upto);
    memcpy(steps.acked, plan.acked, sizeof steps.acked);
    hipLaunchKernelGGL(vad_ring_rows_kernel, dim3((unsigned)v->host.rows.size()), dim3(256), 0, (hipStream_t)stream, v->d_rows, steps, x, ldx, status,
                       log, energy, lde);
    KK_CHECK_LAUNCH();
  }
  v->host.commit_step(n_avail, acked, plan);
  return 0;
}
