// The host halves of the re-arming voice-activity detector and of the row-table ring copies (mlx-audio_amd/csrc/kk_vad_ring_host.h,
// kk_ring_host.h: 64-bit stream positions, bounds arithmetic, every refusal) on their own, with no device: built with a host compiler under
// AddressSanitizer and UndefinedBehaviorSanitizer and run once.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/vad_ring_host_check.cpp -o tools/_bin/vad_ring_host_check && tools/_bin/vad_ring_host_check
#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "../mlx-audio_amd/csrc/kk_ring_host.h"
#include "../mlx-audio_amd/csrc/kk_vad_ring_host.h"

static char g_msg[512];
static int failf(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof g_msg, fmt, ap);
  va_end(ap);
  return -1;
}

static int g_bad = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, g_msg); \
      ++g_bad;                                                    \
    }                                                             \
  } while (0)

static void check_vad_ring() {
  VadRingHost h;
  h.fail = failf;
  h.rows.resize(VAD_MAX_ROWS);
  const char* who = "check";
  const int L = VAD_MAX_ROWS - 1;
  // set_row refusals
  EXPECT(h.check_set_row(who, -1, 720, 0.6f, 50, 10, 7200) != 0 && strstr(g_msg, "row"));
  EXPECT(h.check_set_row(who, VAD_MAX_ROWS, 720, 0.6f, 50, 10, 7200) != 0 && h.check_set_row(who, INT_MAX, 720, 0.6f, 50, 10, 7200) != 0);
  EXPECT(h.check_set_row(who, INT_MIN, 720, 0.6f, 50, 10, 7200) != 0);
  EXPECT(h.check_set_row(who, 0, 0, 0.6f, 50, 10, 7200) != 0 && strstr(g_msg, "frame_len"));
  EXPECT(h.check_set_row(who, 0, VAD_MAX_FRAME + 1, 0.6f, 50, 10, 7200) != 0 && h.check_set_row(who, 0, INT_MIN, 0.6f, 50, 10, 7200) != 0);
  EXPECT(h.check_set_row(who, 0, 720, 0.6f, -1, 10, 7200) != 0 && strstr(g_msg, "hang_frames"));
  EXPECT(h.check_set_row(who, 0, 720, 0.6f, 50, 0, 7200) != 0 && strstr(g_msg, "max_frames"));
  EXPECT(h.check_set_row(who, 0, 720, 0.6f, 50, LLONG_MIN, 7200) != 0);
  EXPECT(h.check_set_row(who, 0, 720, -1.f, 0, 10, 7200) != 0 && strstr(g_msg, "thr2n"));
  EXPECT(h.check_set_row(who, 0, 720, INFINITY, 0, 10, 7200) != 0 && h.check_set_row(who, 0, 720, NAN, 0, 10, 7200) != 0);
  EXPECT(h.check_set_row(who, 0, 720, 0.6f, 50, 10, 719) != 0 && strstr(g_msg, "ring_len"));
  EXPECT(h.check_set_row(who, 0, 720, 0.6f, 50, 10, LLONG_MIN) != 0);
  EXPECT(h.check_set_row(who, 0, 1, 0.f, 0, 1, 1) == 0 && h.check_set_row(who, L, VAD_MAX_FRAME, 1e30f, INT_MAX, LLONG_MAX, LLONG_MAX) == 0);
  h.set_row(0, 720, 0.6f, 50, 10, 7200);
  h.set_row(L, 1, 0.f, INT_MAX, LLONG_MAX, 1);
  // step refusals, with nothing changed
  int64_t n[VAD_MAX_ROWS], a[VAD_MAX_ROWS];
  for (int b = 0; b < VAD_MAX_ROWS; ++b) n[b] = a[b] = INT64_MIN;  // rows without a stream: never read
  VadRingPlan plan;
  n[0] = 1500, a[0] = 0, n[L] = 0, a[L] = 0;
  EXPECT(h.plan_step(who, nullptr, a, 7200, false, 0, &plan) != 0 && h.plan_step(who, n, nullptr, 7200, false, 0, &plan) != 0);
  EXPECT(h.plan_step(who, n, a, 7200, false, 0, nullptr) != 0);
  EXPECT(h.plan_step(who, n, a, -1, false, 0, &plan) != 0 && h.plan_step(who, n, a, 7200, true, 0, &plan) != 0 && h.plan_step(who, n, a, 7200, true, -1, &plan) != 0);
  EXPECT(h.plan_step(who, n, a, 7199, false, 0, &plan) != 0 && strstr(g_msg, "a ring of 7200 in a row of 7199"));
  a[0] = 1;
  EXPECT(h.plan_step(who, n, a, 7200, false, 0, &plan) != 0 && strstr(g_msg, "handed out"));  // no frame was handed out yet
  a[0] = 0;
  EXPECT(h.plan_step(who, n, a, 7200, true, 1, &plan) == 0 && plan.rows_in == 1 && plan.upto[0] == 2 && plan.acked[0] == 0 && plan.upto[1] == -1 &&
         plan.upto[L] == -1);
  EXPECT(h.rows[0].handed == 0 && h.rows[0].n_prev == 0);  // planning changes nothing
  h.commit_step(n, a, plan);
  EXPECT(h.rows[0].handed == 2 && h.rows[0].n_prev == 1500 && h.rows[0].acked == 0);
  n[0] = 1499;
  EXPECT(h.plan_step(who, n, a, 7200, false, 0, &plan) != 0 && strstr(g_msg, "previous"));
  n[0] = INT64_MIN;
  EXPECT(h.plan_step(who, n, a, 7200, false, 0, &plan) != 0);
  n[0] = 2159;  // still two whole frames and no new ack: the row sits out
  EXPECT(h.plan_step(who, n, a, 7200, false, 0, &plan) == 0 && plan.rows_in == 0 && plan.upto[0] == -1);
  h.commit_step(n, a, plan);
  EXPECT(h.rows[0].handed == 2 && h.rows[0].n_prev == 2159);
  a[0] = 3;
  EXPECT(h.plan_step(who, n, a, 7200, false, 0, &plan) != 0 && strstr(g_msg, "handed out"));
  a[0] = 2;  // a new ack alone lets the row take part: it may release a stalled walk
  EXPECT(h.plan_step(who, n, a, 7200, false, 0, &plan) == 0 && plan.rows_in == 1 && plan.upto[0] == 2 && plan.acked[0] == 2);
  h.commit_step(n, a, plan);
  a[0] = 1;
  EXPECT(h.plan_step(who, n, a, 7200, false, 0, &plan) != 0 && strstr(g_msg, "acked = 1 is below its previous 2"));
  a[0] = 2;
  // the ring: frames 0, 1 were handed out, so position 1440 is the oldest unseen one and n_avail may reach 1440 + 7200
  n[0] = 1440 + 7200;
  EXPECT(h.plan_step(who, n, a, 7200, false, 0, &plan) == 0 && plan.upto[0] == 12);
  n[0] = 1440 + 7201;
  EXPECT(h.plan_step(who, n, a, 7200, false, 0, &plan) != 0 && strstr(g_msg, "overwritten position 1440"));
  EXPECT(h.rows[0].handed == 2 && h.rows[0].n_prev == 2159 && h.rows[0].acked == 2);
  // the largest counts: a one-sample ring and frame can walk to INT64_MAX one ring at a time; a wide ring takes it in one step
  n[L] = 1;
  EXPECT(h.plan_step(who, n, a, 7200, false, 0, &plan) != 0);  // (row 0 still refuses: nothing of row L is committed either)
  n[0] = 2159;
  EXPECT(h.plan_step(who, n, a, 7200, false, 0, &plan) == 0 && plan.upto[L] == 1);
  h.commit_step(n, a, plan);
  n[L] = 3;
  EXPECT(h.plan_step(who, n, a, 7200, false, 0, &plan) != 0 && strstr(g_msg, "overwritten position 1"));
  h.set_row(L, VAD_MAX_FRAME, 0.f, 0, LLONG_MAX, LLONG_MAX);
  n[L] = INT64_MAX, a[L] = 0;
  EXPECT(h.plan_step(who, n, a, LLONG_MAX, true, 1, &plan) == 0 && plan.upto[L] == INT64_MAX / VAD_MAX_FRAME);
  VadRingPlan other;
  EXPECT(h.plan_step(who, n, a, LLONG_MAX - 1, false, 0, &other) != 0);
  h.commit_step(n, a, plan);
  EXPECT(h.rows[L].handed == INT64_MAX / VAD_MAX_FRAME && h.rows[L].n_prev == INT64_MAX);
  a[L] = INT64_MAX / VAD_MAX_FRAME;
  EXPECT(h.plan_step(who, n, a, LLONG_MAX, false, 0, &plan) == 0 && plan.acked[L] == a[L]);
  a[L] = INT64_MAX;
  EXPECT(h.plan_step(who, n, a, LLONG_MAX, false, 0, &plan) != 0);
  h.set_row(L, 1, 0.f, 0, 1, 4);  // frame 1 in a ring of 4: handed = INT64_MAX - 3 lets n_avail reach INT64_MAX without overflow
  h.rows[L].n_prev = INT64_MAX - 3, h.rows[L].handed = INT64_MAX - 3;
  n[L] = INT64_MAX, a[L] = 0;
  EXPECT(h.plan_step(who, n, a, 7200, false, 0, &plan) == 0 && plan.upto[L] == INT64_MAX);
  h.set_row(0, 8, 0.f, 0, 1, 8);  // a new stream starts from zero
  EXPECT(h.rows[0].handed == 0 && h.rows[0].n_prev == 0 && h.rows[0].acked == 0);
}

static void check_ring() {
  const char* who = "check";
  RingPlan plan;
  int64_t pos[RING_MAX_ROWS] = {0};
  int32_t n[RING_MAX_ROWS] = {0}, tot[RING_MAX_ROWS] = {0};
  const uintptr_t al = 4096, un = 4100;
  EXPECT(ring_plan(failf, who, 0, al, 64, al, 64, 64, pos, n, nullptr, &plan) != 0 && ring_plan(failf, who, RING_MAX_ROWS + 1, al, 64, al, 64, 64, pos, n, nullptr, &plan) != 0);
  EXPECT(ring_plan(failf, who, INT_MIN, al, 64, al, 64, 64, pos, n, nullptr, &plan) != 0);
  EXPECT(ring_plan(failf, who, 1, al, 64, al, 64, 64, nullptr, n, nullptr, &plan) != 0 && ring_plan(failf, who, 1, al, 64, al, 64, 64, pos, nullptr, nullptr, &plan) != 0);
  EXPECT(ring_plan(failf, who, 1, al, 64, al, 64, 65, pos, n, nullptr, &plan) != 0 && strstr(g_msg, "a ring of 65"));
  EXPECT(ring_plan(failf, who, 1, al, 64, al, 64, 0, pos, n, nullptr, &plan) != 0 && ring_plan(failf, who, 1, al, -1, al, 64, 64, pos, n, nullptr, &plan) != 0);
  n[0] = -1;
  EXPECT(ring_plan(failf, who, 1, al, 64, al, 64, 64, pos, n, nullptr, &plan) != 0 && strstr(g_msg, "negative count"));
  n[0] = 33;
  EXPECT(ring_plan(failf, who, 1, al, 64, al, 64, 32, pos, n, nullptr, &plan) != 0 && strstr(g_msg, "above ring_len"));
  EXPECT(ring_plan(failf, who, 1, al, 32, al, 64, 64, pos, n, nullptr, &plan) != 0 && strstr(g_msg, "in a row of 32"));
  tot[0] = 32;
  EXPECT(ring_plan(failf, who, 1, al, 64, al, 64, 64, pos, n, tot, &plan) != 0 && strstr(g_msg, "above n_total"));
  tot[0] = 65;
  EXPECT(ring_plan(failf, who, 1, al, 64, al, 64, 64, pos, n, tot, &plan) != 0 && strstr(g_msg, "in a row of 64"));
  tot[0] = 64, pos[0] = -1;
  EXPECT(ring_plan(failf, who, 1, al, 64, al, 64, 64, pos, n, tot, &plan) != 0 && strstr(g_msg, "negative position"));
  pos[0] = INT64_MIN;
  EXPECT(ring_plan(failf, who, 1, al, 64, al, 64, 64, pos, n, tot, &plan) != 0);
  // what is planned: aligned and not wrapping -> 16-byte accesses; anything else -> elements
  pos[0] = 64 * 1000 + 28;
  EXPECT(ring_plan(failf, who, 1, al, 64, al, 64, 64, pos, n, tot, &plan) == 0 && plan.t.off[0] == 28 && plan.t.n[0] == 33 && plan.t.n_total[0] == 64 && plan.t.vec[0] == 1 &&
         plan.longest == 64);
  pos[0] = 32;  // 32 + 33 wraps
  EXPECT(ring_plan(failf, who, 1, al, 64, al, 64, 64, pos, n, tot, &plan) == 0 && plan.t.vec[0] == 0);
  pos[0] = 29;
  EXPECT(ring_plan(failf, who, 1, al, 64, al, 64, 64, pos, n, tot, &plan) == 0 && plan.t.off[0] == 29 && plan.t.vec[0] == 0);
  pos[0] = 28;
  EXPECT(ring_plan(failf, who, 1, un, 64, al, 64, 64, pos, n, tot, &plan) == 0 && plan.t.vec[0] == 0);
  EXPECT(ring_plan(failf, who, 1, al, 64, un, 64, 64, pos, n, tot, &plan) == 0 && plan.t.vec[0] == 0);
  EXPECT(ring_plan(failf, who, 1, al, 66, al, 64, 64, pos, n, tot, &plan) == 0 && plan.t.vec[0] == 0);
  EXPECT(ring_plan(failf, who, 1, al, 64, al, 66, 64, pos, n, tot, &plan) == 0 && plan.t.vec[0] == 0);
  // a row with n_total = 0 sits out, whatever its position; the largest position and counts
  n[0] = tot[0] = 0, pos[0] = INT64_MIN;
  pos[1] = INT64_MAX, n[1] = tot[1] = INT_MAX;
  EXPECT(ring_plan(failf, who, 2, al, INT_MAX, al, LLONG_MAX, LLONG_MAX, pos, n, tot, &plan) == 0 && plan.t.n_total[0] == 0 && plan.t.off[1] == 0 && plan.longest == INT_MAX);
  EXPECT(ring_plan(failf, who, 2, al, INT_MAX, al, INT_MAX, INT_MAX, pos, n, tot, &plan) == 0 && plan.t.off[1] == INT64_MAX % INT_MAX && plan.t.vec[1] == 0);
  n[1] = tot[1] = 0;
  EXPECT(ring_plan(failf, who, 2, al, 64, al, 64, 64, pos, n, tot, &plan) == 0 && plan.longest == 0);
}

int main() {
  check_vad_ring();
  check_ring();
  if (g_bad) printf("%d checks failed\n", g_bad);
  else printf("vad_ring_host_check: all refusal paths as documented\n");
  return g_bad != 0;
}
