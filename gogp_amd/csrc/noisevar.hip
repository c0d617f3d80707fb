// noisevar.hip -- per-observation noise variances (gogp_set_noise_variances; api.hip orchestrates).
//
// The model is K = k(X, X) + s2 I + diag(v) with v_i >= 0 known per observation.  A fixed diag(v) has no derivative in
// theta, and everything behind the factorisation works from the factor, alpha and the explicit K^-1, so the feature is
// three bandwidth-bound passes:
//   nv_diag_add_kernel     A_ii += v_i behind the Gram build (Sweep::build_gram), split over the two streams the way the
//                          Gram build is: a diagonal element belongs to the stream that wrote its column;
//   nv_gradient_kernel     dLML/dv_i = 1/2 (alpha_i^2 - [K^-1]_ii), one pass over the diagonal of K^-1;
//   nv_append_fold_kernel  gogp_append_noisy: -v2 folded into the first slab's partial sums of append_gram_kernel, so
//                          that append_commit_kernel (untouched) forms S = C + diag(v2) - V^T V.
// No sums: every element is one thread's, two identical calls give the same bits.
#include "common.h"

namespace gogp {

// One thread per row i0 <= i < i1 (<= n): the diagonal element only
__global__ __launch_bounds__(256) void nv_diag_add_kernel(double *__restrict__ A, long ld, const double *__restrict__ v,
                                                          long i0, long i1) {
  const long i = i0 + (long)blockIdx.x * 256 + threadIdx.x;
  if (i < i1) A[i * (ld + 1)] += v[i];
}

// One thread per row i < n.  fma: alpha^2 - Kinv_ii is rounded once, also where the two cancel.
__global__ __launch_bounds__(256) void nv_gradient_kernel(const double *__restrict__ Kinv, long ld,
                                                          const double *__restrict__ alpha, long n,
                                                          double *__restrict__ dv) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const double a = alpha[i];
    dv[i] = 0.5 * fma(a, a, -Kinv[i * (ld + 1)]);
  }
}

// One workgroup of 64: the diagonal of the first slab's 64 x 64 part (row stride 64)
__global__ __launch_bounds__(64) void nv_append_fold_kernel(double *__restrict__ part, const double *__restrict__ v2, int m) {
  const int i = threadIdx.x;
  if (i < m) part[i * 64 + i] -= v2[i];
}

void launch_nv_diag_add(hipStream_t s_first, hipStream_t s_rest, double *A, int64_t ld, int64_t n, const double *v,
                        int64_t wcols) {
  const int64_t w = std::max<int64_t>(0, std::min(wcols, n));
  if (w > 0)
    GOGP_KLAUNCH(nv_diag_add_kernel, dim3((unsigned)((w + 255) / 256)), dim3(256), 0, s_first, A, (long)ld, v, 0L, (long)w);
  if (n > w)
    GOGP_KLAUNCH(nv_diag_add_kernel, dim3((unsigned)((n - w + 255) / 256)), dim3(256), 0, s_rest, A, (long)ld, v, (long)w,
                 (long)n);
}

void launch_nv_gradient(hipStream_t s, const double *Kinv, int64_t ld, const double *alpha, int64_t n, double *dv) {
  if (n <= 0) return;
  GOGP_KLAUNCH(nv_gradient_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, Kinv, (long)ld, alpha, (long)n, dv);
}

void launch_nv_append_fold(hipStream_t s, double *part, const double *v2, int m) {
  if (m <= 0) return;
  GOGP_KLAUNCH(nv_append_fold_kernel, dim3(1), dim3(64), 0, s, part, v2, m);
}

}  // namespace gogp
