// The host's side of the fixed-point gradient sums (sf_dev.h, "Reproducible gradient sums"), plain C++ so that sf_dev.h and the
// host plan of the NGP backward (ngp_bwd_plan.h) share it.
#pragma once
static inline float sf_fix_thr(double max_addends) {      // host: largest power of two <= 2^18 / max_addends
  float t = 262144.0f;
  while (t > 0x1p-40f && (double)t * max_addends > 262144.0) t *= 0.5f;
  return t;
}
