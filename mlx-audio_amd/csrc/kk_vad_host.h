// The host half of the row-mode voice-activity detector (kk_vad.hip; ABI minor 12): per-row counts and every refusal, with no
// device call, so that the bounds arithmetic can be built and run on its own under a host sanitizer (tools/vad_host_check.cpp).
// `fail` is the includer's error reporter (the library's kk_failf): it records a printf-style message and returns non-zero.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#define VAD_MAX_ROWS 64     // the per-step table travels as a launch argument
#define VAD_MAX_FRAME 4096  // samples per frame
#define VAD_BATCH 1024      // frame energies one pass holds in LDS

struct VadPlan {  // what a step launches: per row the frame count it classifies up to, -1 for a row that sits out
  int32_t upto[VAD_MAX_ROWS];
  int rows_in = 0;  // rows that take part
};

struct VadHost {
  int (*fail)(const char* fmt, ...) = nullptr;
  struct Row {
    bool set = false;
    int frame_len = 0, hang = 0;
    float thr2n = 0.f;
    long long n_prev = 0;      // the n_avail of the row's last step
    long long classified = 0;  // whole frames handed to the device so far (the device stops short of it only behind an endpoint)
  };
  std::vector<Row> rows;

  int check_set_row(const char* who, int row, int frame_len, float thr2n, int hang) const {
    if (row < 0 || row >= (int)rows.size()) return fail("%s: row %d is outside [0, %d)", who, row, (int)rows.size());
    if (frame_len < 1 || frame_len > VAD_MAX_FRAME) return fail("%s: frame_len %d is outside [1, %d]", who, frame_len, VAD_MAX_FRAME);
    if (hang < 0) return fail("%s: hang_frames %d is negative", who, hang);
    if (!(thr2n >= 0.f) || isinf(thr2n)) return fail("%s: thr2n must be finite and >= 0", who);
    return 0;
  }
  void set_row(int row, int frame_len, float thr2n, int hang) {
    Row& w = rows[row];
    w.set = true, w.frame_len = frame_len, w.hang = hang, w.thr2n = thr2n, w.n_prev = 0, w.classified = 0;
  }

  // Every refusal of a step, before anything is launched or changed.  has_energy: the caller passed an energy buffer of pitch lde.
  int plan_step(const char* who, const int32_t* n_avail, long long ldx, bool has_energy, long long lde, VadPlan* plan) const {
    if (!n_avail || !plan) return fail("%s: null argument", who);
    if (ldx < 0 || lde < 0) return fail("%s: a negative row pitch", who);
    plan->rows_in = 0;
    for (int b = 0; b < VAD_MAX_ROWS; ++b) plan->upto[b] = -1;
    for (int b = 0; b < (int)rows.size(); ++b) {
      const Row& w = rows[b];
      if (!w.set) continue;  // a row without a stream sits out: its n_avail is not read either
      const long long n = n_avail[b];
      if (n < w.n_prev) return fail("%s: row %d: n_avail = %lld is below its previous %lld", who, b, n, w.n_prev);
      if (n > ldx) return fail("%s: row %d: n_avail = %lld in a row of %lld", who, b, n, ldx);
      const long long upto = n / w.frame_len;
      if (upto <= w.classified) continue;  // no new whole frame
      if (has_energy && upto - w.classified > lde)
        return fail("%s: row %d: %lld new frames, the energy rows hold %lld", who, b, upto - w.classified, lde);
      plan->upto[b] = (int32_t)upto;
      ++plan->rows_in;
    }
    return 0;
  }
  void commit_step(const int32_t* n_avail, const VadPlan& plan) {
    for (int b = 0; b < (int)rows.size(); ++b) {
      if (!rows[b].set) continue;
      rows[b].n_prev = n_avail[b];
      if (plan.upto[b] >= 0) rows[b].classified = plan.upto[b];
    }
  }
};
