// The host half of the row-table ring copies (kk_ring.hip; ABI minor 13): every refusal and the launch table, with no device
// call, so that the bounds arithmetic can be built and run on its own under a host sanitizer (tools/vad_ring_host_check.cpp).
// `fail` is the includer's error reporter: a printf-style message, returns non-zero.
#pragma once
#include <stdint.h>

#define RING_MAX_ROWS 64  // the table travels as a launch argument

struct RingRows {  // per row: where the run starts in the ring, its length, the length with the zero fill, and whether 16-byte accesses are safe
  int64_t off[RING_MAX_ROWS];
  int32_t n[RING_MAX_ROWS];
  int32_t n_total[RING_MAX_ROWS];
  int32_t vec[RING_MAX_ROWS];
};

struct RingPlan {
  RingRows t;
  long long longest = 0;  // the longest row of the launch, 0: nothing to do
};

// flat: the address of the flat side (src of a write, dst of a read) and its pitch ldf in floats; ring: the ring's address and pitch ldr.
// n_total: NULL for a write (the flat side holds n), the zero-filled length of a read.
static inline int ring_plan(int (*fail)(const char*, ...), const char* who, int rows, uintptr_t flat, long long ldf, uintptr_t ring, long long ldr,
                            long long ring_len, const int64_t* pos, const int32_t* n, const int32_t* n_total, RingPlan* plan) {
  if (rows < 1 || rows > RING_MAX_ROWS) return fail("%s: rows %d is outside [1, %d]", who, rows, RING_MAX_ROWS);
  if (!pos || !n || !plan) return fail("%s: null argument", who);
  if (ring_len < 1 || ring_len > ldr) return fail("%s: a ring of %lld in a row of %lld", who, ring_len, ldr);
  if (ldf < 0) return fail("%s: a negative row pitch", who);
  plan->longest = 0;
  for (int b = 0; b < RING_MAX_ROWS; ++b) plan->t.off[b] = 0, plan->t.n[b] = 0, plan->t.n_total[b] = 0, plan->t.vec[b] = 0;
  const bool flat_al = flat % 16 == 0 && ldf % 4 == 0, ring_al = ring % 16 == 0 && ldr % 4 == 0;
  for (int b = 0; b < rows; ++b) {
    const long long nb = n[b], tot = n_total ? n_total[b] : n[b];
    if (nb < 0 || tot < 0) return fail("%s: row %d: a negative count", who, b);
    if (nb > tot) return fail("%s: row %d: n = %lld is above n_total = %lld", who, b, nb, tot);
    if (tot == 0) continue;  // the row sits out: its position is not read either
    if (nb > ring_len) return fail("%s: row %d: n = %lld is above ring_len = %lld", who, b, nb, ring_len);
    if (tot > ldf) return fail("%s: row %d: %lld samples in a row of %lld", who, b, tot, ldf);
    if (pos[b] < 0) return fail("%s: row %d: a negative position %lld", who, b, (long long)pos[b]);
    const long long off = pos[b] % ring_len;
    plan->t.off[b] = off, plan->t.n[b] = (int32_t)nb, plan->t.n_total[b] = (int32_t)tot;
    plan->t.vec[b] = flat_al && ring_al && off % 4 == 0 && nb <= ring_len - off;  // both sides aligned and the run does not wrap
    if (tot > plan->longest) plan->longest = tot;
  }
  return 0;
}
