// Host-side helpers shared by the weight loaders (kk_model.hip, kk_mimi.hip).
#pragma once
#include <stdint.h>
#include <string.h>

// fp32 -> bf16 bits, round to nearest even
static inline uint16_t f32_to_bf16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
