// laplace.hip -- non-Gaussian likelihoods by the Laplace approximation (gogp_laplace_*; api.hip orchestrates).
//
// Rasmussen & Williams sections 3.4 and 5.5.1, with K the handle's Gram matrix (noise on the diagonal: the latent
// nugget), f = K a the latent values and, per observation, g = dlog p/df, W = -d2log p/df2, rho = d3log p/df3 / W:
//     Newton:    sw = sqrt(W), b = W f + g, B = I + diag(sw) K diag(sw) = L L^T,
//                beta = B^-1 (sw o (K b)), a+ = b - sw o beta, damped along a + t (a+ - a) on
//                psi(a) = -1/2 a^T f + sum_i log p(y_i | f_i);
//     LML:       Z = psi(a^) - sum_i log L_ii at the mode;
//     gradient:  s_i = 1/2 (1 - [B^-1]_ii) rho_i, u = s - sw o (B^-1 (sw o (K s))),
//                G = diag(sw) B^-1 diag(sw) - u a^T - a u^T, dZ/dlog theta = 1/2 sum_ab (a a^T - G)_ab dK_ab/dlog theta
//                (the sign of s is the opposite of R&W eq. 5.23 / Alg. 5.1, which carry a sign error: DESIGN.md);
//     Produce:   mu = k*^T a, sigma^2 = k(z, z) - |L^-1 (sw o k*)|^2, then the response-scale mean.
// The factorisation, the triangular inverse, B^-1 = Y Y^T, the products with K (matrix-free, gram.hip) and the gradient
// reduction are the regression path's; the kernels here are the bandwidth-bound passes around them.
//
// Every sum and maximum has a fixed order (no atomics): two identical calls give the same bits.
#include "common.h"

namespace gogp {

// log p, g, W and rho of one observation.  pi and softplus go through e = exp(-|f|) <= 1: nothing overflows for
// |f| ~ 700, and W = e / (1 + e)^2 keeps its last bits where pi (1 - pi) would round to zero.
__device__ __forceinline__ void lap_site(int lik, double f, double y, double &lp, double &g, double &W, double &rho) {
  if (lik == GOGP_LIK_BERNOULLI_LOGIT) {
    const double e = exp(-fabs(f)), d = 1.0 / (1.0 + e);
    const double pi = f >= 0.0 ? d : e * d;
    lp = y * f - (fmax(f, 0.0) + log1p(e));
    g = y - pi;
    W = e * d * d;
    rho = 2.0 * pi - 1.0;
  } else {
    const double ef = exp(f);
    lp = y * f - ef - lgamma(y + 1.0);
    g = y - ef;
    W = ef;
    rho = -1.0;
  }
}
__device__ __forceinline__ bool lap_y_ok(int lik, double y) {
  if (lik == GOGP_LIK_BERNOULLI_LOGIT) return y == 0.0 || y == 1.0;
  return y >= 0.0 && y <= 9007199254740992.0 && y == floor(y);
}

// One thread per row.  i < n: the site functions of (f_i, y_i) and b_i = W_i f_i + g_i; n <= i < npad: zeros.  part holds
// five rows of npad / 256 block results, by fixed trees: [0] sum log p, [1] sum a_i f_i, [2] max |a_i - g_i|,
// [3] max |a_i|, [4] the first row whose y the likelihood refuses (as a double; -1: none).
__global__ __launch_bounds__(256) void lap_site_kernel(int lik, const double *__restrict__ f, const double *__restrict__ y,
                                                       const double *__restrict__ a, long n, double *__restrict__ g,
                                                       double *__restrict__ W, double *__restrict__ sw,
                                                       double *__restrict__ b, double *__restrict__ rho,
                                                       double *__restrict__ part) {
  __shared__ double red[5][4];
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int nb = gridDim.x;
  double lp = 0.0, af = 0.0, res = 0.0, am = 0.0, bad = INFINITY;
  double gi = 0.0, Wi = 0.0, ri = 0.0, bi = 0.0;
  if (i < n) {
    const double fi = f[i], yi = y[i], ai = a[i];
    if (lap_y_ok(lik, yi)) {
      lap_site(lik, fi, yi, lp, gi, Wi, ri);
      bi = Wi * fi + gi;
      af = ai * fi;
      res = fabs(ai - gi);
      am = fabs(ai);
    } else {
      bad = (double)i;
    }
  }
  g[i] = gi;
  W[i] = Wi;
  sw[i] = sqrt(Wi);
  b[i] = bi;
  rho[i] = ri;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lp += __shfl_xor(lp, o);
    af += __shfl_xor(af, o);
    res = fmax(res, __shfl_xor(res, o));
    am = fmax(am, __shfl_xor(am, o));
    bad = fmin(bad, __shfl_xor(bad, o));
  }
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    red[0][w] = lp, red[1][w] = af, red[2][w] = res, red[3][w] = am, red[4][w] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[0 * nb + blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    part[1 * nb + blockIdx.x] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    part[2 * nb + blockIdx.x] = fmax(fmax(red[2][0], red[2][1]), fmax(red[2][2], red[2][3]));
    part[3 * nb + blockIdx.x] = fmax(fmax(red[3][0], red[3][1]), fmax(red[3][2], red[3][3]));
    const double bd = fmin(fmin(red[4][0], red[4][1]), fmin(red[4][2], red[4][3]));
    part[4 * nb + blockIdx.x] = bd == INFINITY ? -1.0 : bd;
  }
}

// One workgroup, one thread: the block results in block order.  out[0] = sum log p, out[1] = sum a f, out[2] = max
// |a - g|, out[3] = max |a|, out[4] = the first refused row or -1.
__global__ void lap_site_finish_kernel(const double *__restrict__ part, int nb, double *__restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double lp = 0.0, af = 0.0, res = 0.0, am = 0.0, bad = -1.0;
  for (int k = 0; k < nb; ++k) {
    lp += part[0 * nb + k];
    af += part[1 * nb + k];
    res = fmax(res, part[2 * nb + k]);
    am = fmax(am, part[3 * nb + k]);
    if (bad < 0.0 && part[4 * nb + k] >= 0.0) bad = part[4 * nb + k];
  }
  out[0] = lp, out[1] = af, out[2] = res, out[3] = am, out[4] = bad;
}

// A (lower 64-tiles of the column tiles [tc0, tc1), ld) := diag(sw) A diag(sw) + I on the elements i, j < n; the padding
// keeps the identity the Gram kernel wrote.  One workgroup per 64 x 64 tile (grid: row tiles x column tiles); the
// tiles above the diagonal are left alone.
__global__ __launch_bounds__(256) void lap_scale_gram_kernel(double *__restrict__ A, long ld, long n,
                                                             const double *__restrict__ sw, int tc0) {
  const int tr = blockIdx.x + tc0, tc = blockIdx.y + tc0;
  if (tr < tc) return;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long gj = (long)tc * 64 + tx;
  if (gj >= n) return;
  const double sj = sw[gj];
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const long gi = (long)tr * 64 + ty * 16 + rr;  // wave-uniform
    if (gi < n) {
      const double k = sw[gi] * A[gi * ld + gj] * sj;
      A[gi * ld + gj] = gi == gj ? 1.0 + k : k;
    }
  }
}

// out_i = q_i r_i (p == nullptr) or p_i - q_i r_i, i < n; zero from row n on
__global__ __launch_bounds__(256) void lap_vec_kernel(const double *__restrict__ p, const double *__restrict__ q,
                                                      const double *__restrict__ r, long n, double *__restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  double v = 0.0;
  if (i < n) v = p ? p[i] - q[i] * r[i] : q[i] * r[i];
  out[i] = v;
}

// at = a + t (a1 - a), ft = f + t (f1 - f) on the rows i < n; zero from row n on
__global__ __launch_bounds__(256) void lap_interp_kernel(const double *__restrict__ a, const double *__restrict__ a1,
                                                         const double *__restrict__ f, const double *__restrict__ f1,
                                                         double t, long n, double *__restrict__ at,
                                                         double *__restrict__ ft) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  double av = 0.0, fv = 0.0;
  if (i < n) {
    av = a[i] + t * (a1[i] - a[i]);
    fv = f[i] + t * (f1[i] - f[i]);
  }
  at[i] = av;
  ft[i] = fv;
}

// s_i = 1/2 (1 - [B^-1]_ii) rho_i on the rows i < n; zero from row n on
__global__ __launch_bounds__(256) void lap_s_kernel(const double *__restrict__ Binv, long ld, const double *__restrict__ rho,
                                                    long n, double *__restrict__ s) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  s[i] = i < n ? 0.5 * (1.0 - Binv[i * ld + i]) * rho[i] : 0.0;
}

// (ti, tj), tj <= ti, of the t-th tile of a lower triangle enumerated row by row (loo.hip does the same)
__device__ __forceinline__ void lap_lower_tile(int t, int &ti, int &tj) {
  ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (ti * (ti + 1) / 2 > t) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  tj = t - ti * (ti + 1) / 2;
}

// The symmetric product t = B^-1 v from the lower triangle of B^-1 (ld), one workgroup per 64 x 64 tile: the leaner
// sibling of loo_scale_symv_kernel, which also writes a scaled copy of the matrix.  Only the elements j <= i < n are
// read.  The tile's row sums go to upart[tj][r0 + r], its column sums (off the diagonal) to upart[ti][c0 + c]: every
// (slot, row) of the npad / 64 slots x npad rows is written exactly once -- for a row of tile t by the row sums of the
// tiles (t, slot) where slot <= t and by the column sums of the tiles (slot, t) where slot > t -- so lap_u_kernel, which
// adds all the slots of a row in slot order, reads nothing that this launch did not write.
__global__ __launch_bounds__(256) void lap_symv_kernel(const double *__restrict__ Binv, long ld, long n, long npad,
                                                       const double *__restrict__ v, double *__restrict__ upart) {
  __shared__ double tile[64][65];
  __shared__ double vr[64], vc[64];
  int ti, tj;
  lap_lower_tile((int)blockIdx.x, ti, tj);
  const bool diag = ti == tj;
  const long r0 = (long)ti * 64, c0 = (long)tj * 64;
  const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
  const long gj = c0 + tx;
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const int r = ty * 16 + rr;
    const long gi = r0 + r;
    tile[r][tx] = (gi < n && gj < n && (!diag || tx <= r)) ? Binv[gi * ld + gj] : 0.0;
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
  // 4 threads per row (column), 16 elements each, then a fixed two-step tree
  const int q = tid & 3, k = tid >> 2;
  double rs = 0.0;
#pragma unroll
  for (int jj = 0; jj < 16; ++jj) rs += tile[k][q * 16 + jj] * vc[q * 16 + jj];
  rs += __shfl_xor(rs, 1);
  rs += __shfl_xor(rs, 2);
  if (q == 0) upart[(long)tj * npad + r0 + k] = rs;
  if (!diag) {
    double cs = 0.0;
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) cs += tile[q * 16 + jj][k] * vr[q * 16 + jj];
    cs += __shfl_xor(cs, 1);
    cs += __shfl_xor(cs, 2);
    if (q == 0) upart[(long)ti * npad + c0 + k] = cs;
  }
}

// u_i = s_i - sw_i t_i with t_i the sum over the nslot slots of upart in slot order; zero from row n on
__global__ __launch_bounds__(256) void lap_u_kernel(const double *__restrict__ upart, int nslot, long n, long npad,
                                                    const double *__restrict__ s, const double *__restrict__ sw,
                                                    double *__restrict__ u) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  double t = 0.0;
  for (int k = 0; k < nslot; ++k) t += upart[(long)k * npad + i];
  u[i] = i < n ? s[i] - sw[i] * t : 0.0;
}

// In place on the lower 64 x 64 tiles of B^-1 (ld): G_ab = sw_a [B^-1]_ab sw_b - u_a a_b - a_a u_b on the elements
// b <= a < n -- the ones the gradient reduction reads -- and exact zeros on the rest of those tiles (multi_weight_kernel
// leaves its tiles the same way).  Every element depends on its own old value only.
__global__ __launch_bounds__(256) void lap_weight_kernel(double *__restrict__ G, long ld, long n,
                                                         const double *__restrict__ sw, const double *__restrict__ u,
                                                         const double *__restrict__ a) {
  int ti, tj;
  lap_lower_tile((int)blockIdx.x, ti, tj);
  const long r0 = (long)ti * 64, c0 = (long)tj * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long gj = c0 + tx;
  const bool cj = gj < n;
  const double swj = cj ? sw[gj] : 0.0, uj = cj ? u[gj] : 0.0, aj = cj ? a[gj] : 0.0;
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const long gi = r0 + ty * 16 + rr;  // wave-uniform
    double g = 0.0;
    if (gi < n && gj <= gi) g = sw[gi] * G[gi * ld + gj] * swj - u[gi] * aj - a[gi] * uj;
    G[gi * ld + gj] = g;
  }
}

// KsT (rows x ld) := KsT diag(sw) on the columns < npad (sw is zero from column n on, as KsT is)
__global__ __launch_bounds__(256) void lap_colscale_kernel(double *__restrict__ KsT, long ld, long npad,
                                                           const double *__restrict__ sw) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= npad) return;
  KsT[(long)blockIdx.y * ld + j] *= sw[j];
}

// 32-point Gauss-Hermite rule (weight exp(-x^2)): the positive nodes and their weights; the rule is symmetric
__constant__ double LAP_GH_X[16] = {
    1.94840741569399345e-01, 5.84978765435932413e-01, 9.76500463589682788e-01, 1.37037641095287177e+00,
    1.76765410946320145e+00, 2.16949918360611216e+00, 2.57724953773231746e+00, 2.99249082500237407e+00,
    3.41716749281857091e+00, 3.85375548547144486e+00, 4.30554795335119866e+00, 4.77716450350259603e+00,
    5.27555098651588050e+00, 5.81222594951591365e+00, 6.40949814926966077e+00, 7.12581390983072804e+00};
__constant__ double LAP_GH_W[16] = {
    3.75238352592802471e-01, 2.77458142302529964e-01, 1.51269734076642320e-01, 6.04581309559126881e-02,
    1.75534288315734380e-02, 3.65489032665442621e-03, 5.36268365527972049e-04, 5.41658406181999070e-05,
    3.65058512956237819e-06, 1.57416779254558817e-07, 4.09883216477087927e-09, 5.93329146339667624e-11,
    4.21501021132641555e-13, 1.19734401709285026e-15, 9.23173653651825780e-19, 7.31067642738409573e-23};

__device__ __forceinline__ double lap_logistic(double f) {
  const double e = exp(-fabs(f)), d = 1.0 / (1.0 + e);
  return f >= 0.0 ? d : e * d;
}

// The response-scale prediction from the latent mu and sigma.  Poisson: exp(mu + sigma^2 / 2).  Bernoulli:
// 1/sqrt(pi) sum_k w_k logistic(mu + sqrt(2) sigma x_k), the node pairs +-x_k added from the outermost (smallest
// weights) inwards.
__global__ __launch_bounds__(256) void lap_mean_kernel(int lik, const double *__restrict__ mu,
                                                       const double *__restrict__ sigma, long m,
                                                       double *__restrict__ mean) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const double mj = mu[j], sj = sigma[j];
  if (lik == GOGP_LIK_POISSON_LOG) {
    mean[j] = exp(mj + 0.5 * sj * sj);
    return;
  }
  const double c = 1.4142135623730951 * sj;
  double acc = 0.0;
  for (int k = 15; k >= 0; --k)
    acc += LAP_GH_W[k] * (lap_logistic(mj + c * LAP_GH_X[k]) + lap_logistic(mj - c * LAP_GH_X[k]));
  mean[j] = acc * 0.56418958354775629;  // 1 / sqrt(pi)
}

void launch_lap_site(hipStream_t s, int lik, const double *f, const double *y, const double *a, int64_t n, int64_t npad,
                     double *g, double *W, double *sw, double *b, double *rho, double *part, double *out) {
  const int nb = (int)(npad / 256);
  GOGP_KLAUNCH(lap_site_kernel, dim3((unsigned)nb), dim3(256), 0, s, lik, f, y, a, (long)n, g, W, sw, b, rho, part);
  GOGP_KLAUNCH(lap_site_finish_kernel, dim3(1), dim3(64), 0, s, (const double *)part, nb, out);
}

void launch_lap_scale_gram(hipStream_t s_first, hipStream_t s_rest, double *A, int64_t ld, int64_t n, int64_t npad,
                           const double *sw, int64_t wcols) {
  const int nt = (int)(npad / 64);
  int w = (int)(wcols / 64);
  if (w > nt) w = nt;
  if (w > 0)  // block columns [0, w): every row tile
    GOGP_KLAUNCH(lap_scale_gram_kernel, dim3((unsigned)nt, (unsigned)w), dim3(256), 0, s_first, A, (long)ld, (long)n, sw, 0);
  if (nt > w)  // the remaining triangle
    GOGP_KLAUNCH(lap_scale_gram_kernel, dim3((unsigned)(nt - w), (unsigned)(nt - w)), dim3(256), 0, s_rest, A, (long)ld,
                 (long)n, sw, w);
}

void launch_lap_vec(hipStream_t s, const double *p, const double *q, const double *r, int64_t n, int64_t npad, double *out) {
  GOGP_KLAUNCH(lap_vec_kernel, dim3((unsigned)(npad / 256)), dim3(256), 0, s, p, q, r, (long)n, out);
}

void launch_lap_interp(hipStream_t s, const double *a, const double *a1, const double *f, const double *f1, double t,
                       int64_t n, int64_t npad, double *at, double *ft) {
  GOGP_KLAUNCH(lap_interp_kernel, dim3((unsigned)(npad / 256)), dim3(256), 0, s, a, a1, f, f1, t, (long)n, at, ft);
}

void launch_lap_weight_vectors(hipStream_t s, const double *Binv, int64_t ld, const double *rho, int64_t n, int64_t npad,
                               double *sv) {
  GOGP_KLAUNCH(lap_s_kernel, dim3((unsigned)(npad / 256)), dim3(256), 0, s, Binv, (long)ld, rho, (long)n, sv);
}

void launch_lap_symv_u(hipStream_t s, const double *Binv, int64_t ld, int64_t n, int64_t npad, const double *v,
                       const double *sv, const double *sw, double *upart, double *u) {
  const int nt = (int)(npad / 64);
  GOGP_KLAUNCH(lap_symv_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, s, Binv, (long)ld, (long)n, (long)npad, v,
               upart);
  GOGP_KLAUNCH(lap_u_kernel, dim3((unsigned)(npad / 256)), dim3(256), 0, s, (const double *)upart, nt, (long)n, (long)npad,
               sv, sw, u);
}

void launch_lap_weight(hipStream_t s, double *G, int64_t ld, int64_t n, int64_t npad, const double *sw, const double *u,
                       const double *a) {
  const int nt = (int)(npad / 64);
  GOGP_KLAUNCH(lap_weight_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, s, G, (long)ld, (long)n, sw, u, a);
}

void launch_lap_colscale(hipStream_t s, double *KsT, int64_t ld, int64_t rows, int64_t npad, const double *sw) {
  for (int64_t r0 = 0; r0 < rows; r0 += 32768)  // (the grid's y extent ends at 65535)
    GOGP_KLAUNCH(lap_colscale_kernel, dim3((unsigned)(npad / 256), (unsigned)std::min<int64_t>(32768, rows - r0)), dim3(256),
                 0, s, KsT + r0 * ld, (long)ld, (long)npad, sw);
}

void launch_lap_mean(hipStream_t s, int lik, const double *mu, const double *sigma, int64_t m, double *mean) {
  GOGP_KLAUNCH(lap_mean_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, lik, mu, sigma, (long)m, mean);
}

}  // namespace gogp
