// multi.hip -- T output columns on one factorisation (gogp_multi_*; api.hip orchestrates).
//
// Shared inputs, kernel and hyperparameters, T independent output columns Y = [y_1 .. y_T]: with A = K^-1 Y
//     lml_t = -1/2 y_t^T a_t - sum_i log L_ii - n/2 log 2 pi,        total = sum_t lml_t,
//     d total = 1/2 sum_ab (A A^T - T K^-1)_ab dK_ab.
// The solutions come from the factor (Produce's forward and ProduceGradient's backward substitution with Y^T as the
// right-hand-side rows); two kernels are new.  multi_weight_kernel forms G = T K^-1 - A A^T on the lower 64 x 64 tiles:
// the gradient reduction of grad.hip, whose weight is alpha_i alpha_j - Kinv_ij, then runs on G with a zero vector for
// alpha, as gogp_loo_gradient does.  multi_dots_kernel forms the T quadratic terms y_t^T a_t.
//
// Every sum has a fixed order (no atomics): two identical calls give the same bits.
#include "common.h"

namespace gogp {

typedef double mw_f64x4 __attribute__((ext_vector_type(4)));
// Rows of A^T per pass through LDS and the stride of one of them there.  A slice is kept as it lies in memory, one row
// of A^T (64 observations) per LDS row: a fragment read takes 16 consecutive observations of 4 consecutive rows, and
// with 80 doubles per row the rows k and k + 1 start half the banks apart -- 512 bytes in two passes, the minimum for 64
// lanes of 8 bytes; the writes run along a row.
constexpr int MW_KC = 32, MW_S = 80;

// (ti, tj), tj <= ti, of the t-th tile of a lower triangle enumerated row by row (loo.hip, pcov.hip do the same)
__device__ __forceinline__ void multi_lower_tile(int t, int &ti, int &tj) {
  ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (ti * (ti + 1) / 2 > t) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  tj = t - ti * (ti + 1) / 2;
}

// G (ldk doubles per row, as Kinv) = scale Kinv - A A^T (gogp_multi_*: scale = T; gogp_basis_*: 1) on the elements j <= i < n of the lower 64 x 64 tiles, one
// workgroup per tile (ti, tj), tj <= ti; every other element of those tiles -- i >= n, j >= n, the upper half of a
// diagonal tile -- is written as an exact zero, and nothing outside them is written.  At: T4 rows (T rounded up to a
// multiple of 4, the rows from T on zero) of ld doubles, row t = column t of A, contiguous along the observations: both
// 64-observation slices are loaded along those rows (a diagonal tile loads one) and multiplied as a SYRK with K = T4 on
// v_mfma_f64_16x16x4_f64.  Wave w owns rows 16 w .. 16 w + 15 of the tile: one A fragment and four B fragments per 4 k
// (A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][column = lane & 15]).  Of Kinv only the elements j <= i < n are
// READ: whatever its upper triangle and padding hold does not matter.  (__launch_bounds__(256, 2), as pcov_syrk_kernel:
// the accumulators stay in architectural VGPRs -- tools/codeobj_audit.py allows no AGPR.)
__global__ __launch_bounds__(256, 2) void multi_weight_kernel(const double *__restrict__ At, long ld, int T, int T4,
                                                           const double *__restrict__ Kinv, long ldk, long n,
                                                           double scale, double *__restrict__ G) {
  __shared__ double As[MW_KC * MW_S], Bs[MW_KC * MW_S];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int ti, tj;
  multi_lower_tile((int)blockIdx.x, ti, tj);
  const bool diag = ti == tj;
  const long r0 = (long)ti * 64, c0 = (long)tj * 64;
  const int fr = lane & 15, fk = lane >> 4;
  const double *Bsrc = diag ? As : Bs;
  mw_f64x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = (mw_f64x4){0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < T4; k0 += MW_KC) {
    const int kc = min(MW_KC, T4 - k0);  // a multiple of 4
    if (k0 > 0) __syncthreads();         // the previous pass's readers are done
#pragma unroll
    for (int rr = 0; rr < MW_KC / 4; ++rr) {
      const int k = w + 4 * rr;
      if (k < kc) {
        const double *row = At + (long)(k0 + k) * ld;
        As[k * MW_S + lane] = row[r0 + lane];
        if (!diag) Bs[k * MW_S + lane] = row[c0 + lane];
      }
    }
    __syncthreads();
    for (int kk = 0; kk < kc; kk += 4) {
      const double a = As[(kk + fk) * MW_S + 16 * w + fr];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bsrc[(kk + fk) * MW_S + 16 * t + fr], acc[t], 0, 0, 0);
    }
  }
  // C fragment: column = lane & 15, row = (lane >> 4) + 4 v
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const long gi = r0 + 16 * w + fk + 4 * v;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const long gj = c0 + 16 * t + fr;
      double g = 0.0;
      if (gi < n && gj <= gi) g = scale * Kinv[gi * ldk + gj] - acc[t][v];
      G[gi * ldk + gj] = g;
    }
  }
}

// dots[t] = sum_{i < n} Yt[t][i] At[t][i], one workgroup per output row t: every thread sums its elements i = tid,
// tid + 256, .. in that order, then a fixed tree over the lanes and the four waves
__global__ __launch_bounds__(256) void multi_dots_kernel(const double *__restrict__ Yt, const double *__restrict__ At,
                                                         long ld, long n, double *__restrict__ dots) {
  __shared__ double red[4];
  const double *y = Yt + (long)blockIdx.x * ld, *a = At + (long)blockIdx.x * ld;
  double t = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) t += y[i] * a[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) dots[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

void launch_multi_weight(hipStream_t s, const double *At, int64_t ld, int T, const double *Kinv, int64_t ldk, int64_t n,
                         int64_t npad, double scale, double *G) {
  const int nt = (int)(npad / 64);
  GOGP_KLAUNCH(multi_weight_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, s, At, (long)ld, T, (T + 3) / 4 * 4,
               Kinv, (long)ldk, (long)n, scale, G);
}

void launch_multi_dots(hipStream_t s, const double *Yt, const double *At, int64_t ld, int64_t n, int T, double *dots) {
  GOGP_KLAUNCH(multi_dots_kernel, dim3((unsigned)T), dim3(256), 0, s, Yt, At, (long)ld, (long)n, dots);
}

}  // namespace gogp
