// api_internal.h -- what cg_api.hip (gogp_cg_*) and vecchia_api.hip (gogp_vecchia_*) take from api.hip, and the few lines
// of host code the two families share.  Private to libgogp_hip.so.
#pragma once
#include <math.h>
#include <stdio.h>

#include "handle.h"

namespace gogp {
// ---- defined in api.hip ----------------------------------------------------------------------------------------------------
// DevParams of the natural parameters ts (similarity), tn (noise)
void fill_params_theta(const gogp_handle *h, const double *ts, const double *tn, DevParams &p);
// NULL, or what is wrong with the natural parameters ts / tn
const char *theta_refusal(const gogp_handle *h, const double *ts, const double *tn);
// d LML / d log theta from the slot sums of a gradient reduction (common.h: ACC_*); out: P zeros
void assemble_gradient(const gogp_handle *h, const double *a, double dnoise, double *out);
// GOGP_OK, or GOGP_EARG for no handle (h == NULL) and, with "<who>: <why>" as the error text, for the kinds of handle both
// families refuse: precision = 32, sharded, event discounts
int refuse_handle(gogp_handle *h, const char *who);

// ---- shared host code ------------------------------------------------------------------------------------------------------
// `code`, with "<who>: <what>" as the handle's error text
inline int refuse(gogp_handle *h, const char *who, int code, const char *what) {
  return fail(h, code, (std::string(who) + ": " + what).c_str());
}

// Consecutive arrays, each rounded up to 256 bytes, out of the block at `base` (nullptr: `off` alone, the bytes it needs)
struct Carve {
  char *base;
  size_t off = 0;
  template <class T>
  T *take(size_t count) {
    char *q = base ? base + off : nullptr;
    off += (count * sizeof(T) + 255) / 256 * 256;
    return reinterpret_cast<T *>(q);
  }
};

// NULL, or what gogp_cg_set_data and gogp_vecchia_set_data refuse in a data set: X (N x D), y (N) or the noise variances v
// (N; nullptr: none) not finite, a negative variance.  *vmin (nullptr: not wanted): the smallest variance, 0 without v.
inline const char *resident_data_refusal(const double *X, const double *y, const double *v, int64_t N, int D,
                                         double *vmin = nullptr) {
  for (int64_t i = 0; i < N * D; ++i)
    if (!std::isfinite(X[i])) return "non-finite input";
  for (int64_t i = 0; i < N; ++i)
    if (!std::isfinite(y[i])) return "non-finite output";
  double lo = v ? INFINITY : 0.0;
  for (int64_t i = 0; v && i < N; ++i) {
    if (!std::isfinite(v[i]) || v[i] < 0.0) return "noise variances must be finite and >= 0";
    lo = std::min(lo, v[i]);
  }
  if (vmin) *vmin = lo;
  return nullptr;
}
}  // namespace gogp
