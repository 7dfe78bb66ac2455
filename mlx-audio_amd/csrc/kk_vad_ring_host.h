// The host half of the re-arming voice-activity detector over a ring (kk_vad_ring in kk_vad.hip; ABI minor 13): per-row counts
// in 64-bit stream positions and every refusal, with no device call, so that the bounds arithmetic can be built and run on its own under a
// host sanitizer (tools/vad_ring_host_check.cpp).  `fail` is the includer's error reporter: a printf-style message, returns non-zero.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "kk_vad_host.h"  // VAD_MAX_ROWS, VAD_MAX_FRAME, VAD_BATCH

#define VAD_LOG 8  // closed-utterance records the device keeps per row in front of the host's ack

struct VadRingPlan {  // what a step launches: per row the frame count it may classify up to (-1: the row sits out) and the records consumed
  int64_t upto[VAD_MAX_ROWS];
  int64_t acked[VAD_MAX_ROWS];
  int rows_in = 0;
};

struct VadRingHost {
  int (*fail)(const char* fmt, ...) = nullptr;
  struct Row {
    bool set = false;
    int frame_len = 0, hang = 0;
    float thr2n = 0.f;
    long long max_frames = 0, ring_len = 0;
    long long n_prev = 0;  // the n_avail of the row's last step
    long long handed = 0;  // whole frames handed to a step so far: the device's `classified` stops short of it only in front of a full log
    long long acked = 0;   // the acked of the row's last step
  };
  std::vector<Row> rows;

  int check_set_row(const char* who, int row, int frame_len, float thr2n, int hang, long long max_frames, long long ring_len) const {
    if (row < 0 || row >= (int)rows.size()) return fail("%s: row %d is outside [0, %d)", who, row, (int)rows.size());
    if (frame_len < 1 || frame_len > VAD_MAX_FRAME) return fail("%s: frame_len %d is outside [1, %d]", who, frame_len, VAD_MAX_FRAME);
    if (hang < 0) return fail("%s: hang_frames %d is negative", who, hang);
    if (max_frames < 1) return fail("%s: max_frames %lld is below 1", who, max_frames);
    if (!(thr2n >= 0.f) || isinf(thr2n)) return fail("%s: thr2n must be finite and >= 0", who);
    if (ring_len < frame_len) return fail("%s: ring_len %lld is below frame_len %d", who, ring_len, frame_len);
    return 0;
  }
  void set_row(int row, int frame_len, float thr2n, int hang, long long max_frames, long long ring_len) {
    Row& w = rows[row];
    w.set = true, w.frame_len = frame_len, w.hang = hang, w.thr2n = thr2n, w.max_frames = max_frames, w.ring_len = ring_len;
    w.n_prev = 0, w.handed = 0, w.acked = 0;
  }

  // Every refusal of a step, before anything is launched or changed.  has_energy: the caller passed an energy buffer of pitch lde.
  // A closed record takes at least one frame of its own, so a row's records never outnumber the frames handed to the device: that is
  // what `acked` is held against.  A row takes part when it has a new whole frame, or a new ack that may release a walk stalled at VAD_LOG.
  int plan_step(const char* who, const int64_t* n_avail, const int64_t* acked, long long ldx, bool has_energy, long long lde, VadRingPlan* plan) const {
    if (!n_avail || !acked || !plan) return fail("%s: null argument", who);
    if (ldx < 0 || lde < 0 || (has_energy && lde < 1)) return fail("%s: a bad row pitch", who);
    plan->rows_in = 0;
    for (int b = 0; b < VAD_MAX_ROWS; ++b) plan->upto[b] = -1, plan->acked[b] = 0;
    for (int b = 0; b < (int)rows.size(); ++b) {
      const Row& w = rows[b];
      if (!w.set) continue;  // a row without a stream sits out: its n_avail and acked are not read either
      const long long n = n_avail[b], a = acked[b];
      if (w.ring_len > ldx) return fail("%s: row %d: a ring of %lld in a row of %lld", who, b, w.ring_len, ldx);
      if (n < w.n_prev) return fail("%s: row %d: n_avail = %lld is below its previous %lld", who, b, n, w.n_prev);
      // (handed frame_len <= n_prev <= n: the product cannot overflow)
      if (n - w.ring_len > w.handed * w.frame_len)
        return fail("%s: row %d: n_avail = %lld has overwritten position %lld, which no step has seen (ring_len %lld)", who, b, n, w.handed * w.frame_len,
                    w.ring_len);
      if (a < w.acked) return fail("%s: row %d: acked = %lld is below its previous %lld", who, b, a, w.acked);
      if (a > w.handed) return fail("%s: row %d: acked = %lld, but only %lld frames were handed out before this step", who, b, a, w.handed);
      const long long upto = n / w.frame_len;
      if (upto <= w.handed && a == w.acked) continue;  // no new whole frame, and no ack that could release a stalled walk
      plan->upto[b] = upto, plan->acked[b] = a;
      ++plan->rows_in;
    }
    return 0;
  }
  void commit_step(const int64_t* n_avail, const int64_t* acked, const VadRingPlan& plan) {
    for (int b = 0; b < (int)rows.size(); ++b) {
      if (!rows[b].set) continue;
      rows[b].n_prev = n_avail[b], rows[b].acked = acked[b];
      if (plan.upto[b] >= 0) rows[b].handed = plan.upto[b];
    }
  }
};
