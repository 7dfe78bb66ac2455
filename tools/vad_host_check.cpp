// The host half of the voice-activity detector (mlx-audio_amd/csrc/kk_vad_host.h: per-row counts, bounds arithmetic, every refusal) on its
// own, with no device: built with a host compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run once.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/vad_host_check.cpp -o tools/_bin/vad_host_check && tools/_bin/vad_host_check
#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "../mlx-audio_amd/csrc/kk_vad_host.h"

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

int main() {
  VadHost h;
  h.fail = failf;
  h.rows.resize(VAD_MAX_ROWS);
  const char* who = "check";
  // set_row refusals
  EXPECT(h.check_set_row(who, -1, 720, 0.6f, 50) != 0 && strstr(g_msg, "row"));
  EXPECT(h.check_set_row(who, VAD_MAX_ROWS, 720, 0.6f, 50) != 0);
  EXPECT(h.check_set_row(who, INT_MAX, 720, 0.6f, 50) != 0 && h.check_set_row(who, INT_MIN, 720, 0.6f, 50) != 0);
  EXPECT(h.check_set_row(who, 0, 0, 0.6f, 50) != 0 && strstr(g_msg, "frame_len"));
  EXPECT(h.check_set_row(who, 0, VAD_MAX_FRAME + 1, 0.6f, 50) != 0 && h.check_set_row(who, 0, INT_MIN, 0.6f, 50) != 0);
  EXPECT(h.check_set_row(who, 0, 720, 0.6f, -1) != 0 && strstr(g_msg, "hang_frames"));
  EXPECT(h.check_set_row(who, 0, 720, -1.f, 0) != 0 && strstr(g_msg, "thr2n"));
  EXPECT(h.check_set_row(who, 0, 720, INFINITY, 0) != 0 && h.check_set_row(who, 0, 720, NAN, 0) != 0);
  EXPECT(h.check_set_row(who, 0, 1, 0.f, 0) == 0 && h.check_set_row(who, VAD_MAX_ROWS - 1, VAD_MAX_FRAME, 1e30f, INT_MAX) == 0);
  h.set_row(0, 720, 0.6f, 50);
  h.set_row(VAD_MAX_ROWS - 1, 1, 0.f, INT_MAX);
  // step refusals, with nothing changed
  int32_t n[VAD_MAX_ROWS];
  for (int b = 0; b < VAD_MAX_ROWS; ++b) n[b] = INT_MIN;  // rows without a stream: never read
  VadPlan plan;
  n[0] = 1500, n[VAD_MAX_ROWS - 1] = 0;
  EXPECT(h.plan_step(who, nullptr, 4096, false, 0, &plan) != 0 && h.plan_step(who, n, 4096, false, 0, nullptr) != 0);
  EXPECT(h.plan_step(who, n, -1, false, 0, &plan) != 0 && h.plan_step(who, n, 4096, true, -1, &plan) != 0);
  EXPECT(h.plan_step(who, n, 1499, false, 0, &plan) != 0 && strstr(g_msg, "in a row of 1499"));
  EXPECT(h.plan_step(who, n, 4096, true, 1, &plan) != 0 && strstr(g_msg, "energy"));
  EXPECT(h.plan_step(who, n, 4096, true, 2, &plan) == 0 && plan.rows_in == 1 && plan.upto[0] == 2 && plan.upto[1] == -1 && plan.upto[VAD_MAX_ROWS - 1] == -1);
  EXPECT(h.rows[0].classified == 0 && h.rows[0].n_prev == 0);  // planning changes nothing
  h.commit_step(n, plan);
  EXPECT(h.rows[0].classified == 2 && h.rows[0].n_prev == 1500);
  n[0] = 1499;
  EXPECT(h.plan_step(who, n, 4096, false, 0, &plan) != 0 && strstr(g_msg, "previous"));
  n[0] = INT_MIN;
  EXPECT(h.plan_step(who, n, 4096, false, 0, &plan) != 0);
  n[0] = 2159;  // still two whole frames: the row sits out
  EXPECT(h.plan_step(who, n, 4096, true, 0, &plan) == 0 && plan.rows_in == 0 && plan.upto[0] == -1);
  h.commit_step(n, plan);
  EXPECT(h.rows[0].classified == 2 && h.rows[0].n_prev == 2159);
  // the largest counts the ABI can carry
  n[0] = INT_MAX, n[VAD_MAX_ROWS - 1] = INT_MAX;
  EXPECT(h.plan_step(who, n, (long long)INT_MAX, true, LLONG_MAX, &plan) == 0 && plan.rows_in == 2);
  EXPECT(plan.upto[0] == INT_MAX / 720 && plan.upto[VAD_MAX_ROWS - 1] == INT_MAX);
  EXPECT(h.plan_step(who, n, (long long)INT_MAX, true, (long long)INT_MAX - 1, &plan) != 0);
  EXPECT(h.plan_step(who, n, (long long)INT_MAX - 1, false, 0, &plan) != 0);
  h.commit_step(n, plan);
  h.set_row(0, 8, 0.f, 0);  // a new stream starts from zero
  EXPECT(h.rows[0].classified == 0 && h.rows[0].n_prev == 0);
  if (g_bad) printf("%d checks failed\n", g_bad);
  else printf("vad_host_check: all refusal paths as documented\n");
  return g_bad != 0;
}
