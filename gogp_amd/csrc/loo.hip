// loo.hip -- leave-one-out cross-validation from the explicit K^-1 (gogp_loo, gogp_loo_gradient; api.hip orchestrates).
//
// Rasmussen & Williams section 5.4.2: with kappa_i = [K^-1]_ii and alpha = K^-1 y the held-out prediction of y_i is
//     mu_i = y_i - alpha_i / kappa_i,  sigma_i^2 = 1 / kappa_i,
//     log p_i = 1/2 log kappa_i - 1/2 alpha_i^2 / kappa_i - 1/2 log 2 pi,        L_LOO = sum_i log p_i.
// With d K^-1 = -K^-1 dK K^-1 and d alpha = -K^-1 dK alpha,
//     d L_LOO = sum_ab W_ab dK_ab,   W = 1/2 (u alpha^T + alpha u^T) - K^-1 diag(w) K^-1,
//     v_i = alpha_i / kappa_i,  u = K^-1 v,  w_i = 1/2 (1 + alpha_i^2 / kappa_i) / kappa_i.
// The kernels here form G = B B^T - u alpha^T - alpha u^T = -2 W with B = K^-1 diag(s), s_i^2 = 2 w_i (the product
// B B^T itself is one launch of the tile kernel); the gradient reduction of grad.hip, whose weight is
// alpha_i alpha_j - Kinv_ij, then runs on G with a zero vector for alpha: weight 2 W, halved by the host.
//
// Every pass is HBM-bound; every sum has a fixed order (no atomics): two identical calls give the same bits.
#include "common.h"

namespace gogp {

// One thread per row.  i < n: the three LOO quantities, v_i and s_i; n <= i < npad: v_i = s_i = 0.  part[block] = the
// block's sum of log p_i by a fixed tree (the host adds the npad / 256 block sums in order).
__global__ __launch_bounds__(256) void loo_stats_kernel(const double *__restrict__ Kinv, long ld,
                                                        const double *__restrict__ alpha, const double *__restrict__ y,
                                                        long n, double *__restrict__ mu, double *__restrict__ sigma,
                                                        double *__restrict__ logp, double *__restrict__ v,
                                                        double *__restrict__ sc, double *__restrict__ part) {
  __shared__ double red[4];
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  double lp = 0.0, vi = 0.0, si = 0.0;
  if (i < n) {
    const double kap = Kinv[i * ld + i], a = alpha[i];
    vi = a / kap;
    lp = 0.5 * log(kap) - 0.5 * a * vi - 0.9189385332046727418;  // 1/2 log 2 pi
    si = sqrt((1.0 + a * vi) / kap);
    mu[i] = y[i] - vi;
    sigma[i] = sqrt(1.0 / kap);
    logp[i] = lp;
  }
  v[i] = vi;
  sc[i] = si;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lp += __shfl_xor(lp, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = lp;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// (ti, tj), tj <= ti, of the t-th tile of a lower triangle enumerated row by row (grad.hip does the same)
__device__ __forceinline__ void lower_tile(int t, int &ti, int &tj) {
  ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (ti * (ti + 1) / 2 > t) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  tj = t - ti * (ti + 1) / 2;
}

// One pass over the lower triangle of K^-1 (npad x npad, ld), one workgroup per 64 x 64 tile (ti, tj), tj <= ti.
// Only the elements j <= i < n are READ: whatever the upper triangle and the padding hold (the factorisation's work
// area, a mirror left by the input gradient, an identity) does not matter.  The tile goes through LDS (rows padded by
// one element) and leaves twice, both times with the lanes along a row of the destination:
//   B[r0 + r][c0 + c] = t[r][c] s[c0 + c]          and, off the diagonal,  B[c0 + c][r0 + r] = t[r][c] s[r0 + r]
// so B = K^-1 diag(s) is written in full, with exact zeros in the rows and columns >= n.  The tile's share of
// u = K^-1 v -- row sums for the rows r0.., column sums for the rows c0.. -- goes to upart[tj][r0 + r] and
// upart[ti][c0 + c] (npad / 64 slots of npad doubles): every (slot, row) is written by exactly one workgroup, and
// loo_u_final_kernel adds a row's slots in slot order.
__global__ __launch_bounds__(256) void loo_scale_symv_kernel(const double *__restrict__ Kinv, long ld, long n, long npad,
                                                             const double *__restrict__ sc, const double *__restrict__ v,
                                                             double *__restrict__ B, long ldb,
                                                             double *__restrict__ upart) {
  __shared__ double tile[64][65];
  __shared__ double vr[64], vc[64];
  int ti, tj;
  lower_tile((int)blockIdx.x, ti, tj);
  const bool diag = ti == tj;
  const long r0 = (long)ti * 64, c0 = (long)tj * 64;
  const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
  const long gj = c0 + tx;
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const int r = ty * 16 + rr;
    const long gi = r0 + r;
    tile[r][tx] = (gi < n && gj < n && (!diag || tx <= r)) ? Kinv[gi * ld + gj] : 0.0;
  }
  if (tid < 64) vr[tid] = v[r0 + tid];  // (v is zero from row n on)
  else if (tid < 128) vc[tid - 64] = v[c0 + tid - 64];
  __syncthreads();
  if (diag) {  // the upper half of a diagonal tile is the mirror of its lower half
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
      const int r = ty * 16 + rr;
      if (tx > r) tile[r][tx] = tile[tx][r];
    }
    __syncthreads();
  }
  const double scol = sc[c0 + tx];
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const int r = ty * 16 + rr;
    B[(r0 + r) * ldb + c0 + tx] = tile[r][tx] * scol;
  }
  // share of u: 4 threads per row (column), 16 elements each, then a fixed two-step tree
  const int q = tid & 3, k = tid >> 2;
  double rs = 0.0;
#pragma unroll
  for (int jj = 0; jj < 16; ++jj) rs += tile[k][q * 16 + jj] * vc[q * 16 + jj];
  rs += __shfl_xor(rs, 1);
  rs += __shfl_xor(rs, 2);
  if (q == 0) upart[(long)tj * npad + r0 + k] = rs;
  if (!diag) {
    const double srow = sc[r0 + tx];
#pragma unroll
    for (int cc = 0; cc < 16; ++cc) {
      const int c = ty * 16 + cc;
      B[(c0 + c) * ldb + r0 + tx] = tile[tx][c] * srow;
    }
    double cs = 0.0;
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) cs += tile[q * 16 + jj][k] * vr[q * 16 + jj];
    cs += __shfl_xor(cs, 1);
    cs += __shfl_xor(cs, 2);
    if (q == 0) upart[(long)ti * npad + c0 + k] = cs;
  }
}

// u_i = sum over the nslot slots of upart, in slot order; zero from row n on
__global__ __launch_bounds__(256) void loo_u_final_kernel(const double *__restrict__ upart, int nslot, long n, long npad,
                                                          double *__restrict__ u) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  double t = 0.0;
  for (int k = 0; k < nslot; ++k) t += upart[(long)k * npad + i];
  u[i] = i < n ? t : 0.0;
}

// G_ij -= u_i alpha_j + alpha_i u_j on the 64 x 64 tiles of the lower triangle (alpha is taken as zero from row n on)
__global__ __launch_bounds__(256) void loo_rank2_kernel(double *__restrict__ G, long ld, long n,
                                                        const double *__restrict__ u, const double *__restrict__ alpha) {
  int ti, tj;
  lower_tile((int)blockIdx.x, ti, tj);
  const long r0 = (long)ti * 64, c0 = (long)tj * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long gj = c0 + tx;
  const double uj = u[gj], aj = gj < n ? alpha[gj] : 0.0;
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const long gi = r0 + ty * 16 + rr;  // wave-uniform
    const double ui = u[gi], ai = gi < n ? alpha[gi] : 0.0;
    G[gi * ld + gj] -= ui * aj + ai * uj;
  }
}

void launch_loo_stats(hipStream_t s, const double *Kinv, int64_t ld, const double *alpha, const double *y, int64_t n,
                      int64_t npad, double *mu, double *sigma, double *logp, double *v, double *sc, double *part) {
  GOGP_KLAUNCH(loo_stats_kernel, dim3((unsigned)(npad / 256)), dim3(256), 0, s, Kinv, (long)ld, alpha, y, (long)n, mu, sigma,
               logp, v, sc, part);
}

void launch_loo_scale_symv(hipStream_t s, const double *Kinv, int64_t ld, int64_t n, int64_t npad, const double *sc,
                           const double *v, double *B, int64_t ldb, double *upart, double *u) {
  const int nt = (int)(npad / 64);
  GOGP_KLAUNCH(loo_scale_symv_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, s, Kinv, (long)ld, (long)n,
               (long)npad, sc, v, B, (long)ldb, upart);
  GOGP_KLAUNCH(loo_u_final_kernel, dim3((unsigned)(npad / 256)), dim3(256), 0, s, (const double *)upart, nt, (long)n,
               (long)npad, u);
}

void launch_loo_rank2(hipStream_t s, double *G, int64_t ld, int64_t n, int64_t npad, const double *u, const double *alpha) {
  const int nt = (int)(npad / 64);
  GOGP_KLAUNCH(loo_rank2_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, s, G, (long)ld, (long)n, u, alpha);
}

}  // namespace gogp
