// basis.hip -- explicit basis functions: a linear mean h(x)^T beta with beta integrated out under a flat prior
// (gogp_basis_*; api.hip orchestrates; Rasmussen & Williams section 2.7; DESIGN.md section 4, "Explicit basis functions").
//
// H is n x p, kept as H^T: one basis column per row of ld doubles, contiguous along the observations.  With K the
// handle's Gram matrix (noise included) and alpha = K^-1 y:
//     W = K^-1 H         A = H^T W = L_A L_A^T       g = H^T alpha       beta = A^-1 g      alpha~ = alpha - W beta
//     Q = W L_A^-T       G = K^-1 - [Q | alpha~][Q | alpha~]^T           (multi_weight_kernel forms G, scale 1)
// Five kernels: basis_symm_kernel (W from the explicit symmetric K^-1, on v_mfma_f64_16x16x4_f64 -- the hot path; its
// slabs' partial sums are added by basis_symm_sum_kernel), basis_gram_kernel ([A | g], slabs added by basis_gram_sum_kernel),
// basis_finish_kernel (L_A, log|A|, beta, g^T beta, A^-1 and an info word), basis_cols_kernel ([Q | alpha~]^T) and
// basis_predict_kernel (the correction of Produce's mean and deviation).
//
// Every sum has a fixed order (no atomics): two identical calls give the same bits.
#include <algorithm>

#include "common.h"

namespace gogp {

typedef double bs_f64x4 __attribute__((ext_vector_type(4)));
// LDS strides.  The 64 x 64 tile of K^-1 lies as S[j][i] (j: summed observation, i: output observation), 80 doubles per
// row: a B fragment takes 16 consecutive i of 4 consecutive j, and rows j, j + 1 start half the banks apart (multi.hip:
// MW_S).  The slice of H^T lies transposed, Hs[j][c], 32 basis columns per pass and 48 doubles per row: an A fragment
// takes 16 consecutive c of 4 consecutive j, rows again half the banks apart.  40960 + 24576 bytes: the 64 KiB of a
// workgroup exactly, two workgroups per CU.
constexpr int BS_SS = 80, BS_HC = 32, BS_HS = 48;

// cc (a multiple of 4, <= 32) basis columns from c0 on of the 64 observations from j0 on into Hs[j][c]; columns >= p and
// observations >= n as zeros
__device__ __forceinline__ void bs_load_h(double *Hs, const double *__restrict__ Ht, long ld, int c0, int cc, int p, long j0,
                                          long n, int w, int lane) {
#pragma unroll 2
  for (int rr = 0; rr < BS_HC / 4; ++rr) {
    const int c = w + 4 * rr;
    if (c < cc) {
      const long gj = j0 + lane;
      Hs[lane * BS_HS + c] = (c0 + c < p && gj < n) ? Ht[(long)(c0 + c) * ld + gj] : 0.0;
    }
  }
}
// the 64 summed observations of one tile against the cc basis columns in Hs, into the accumulators BASE (columns 0 .. 15
// of the pass) and BASE + 1 (16 .. 31, where cc > 16); the columns from cc on were not loaded and count as zeros
template <int BASE>
__device__ __forceinline__ void bs_pass(bs_f64x4 (&acc)[4], const double *Ss, const double *Hs, int cc, int w, int fr,
                                        int fk) {
  const double *sp = Ss + fk * BS_SS + 16 * w + fr, *hp = Hs + fk * BS_HS + fr;
  if (cc > 16) {  // (uniform)
    const bool m1 = 16 + fr < cc;
#pragma unroll 4
    for (int kk = 0; kk < 64; kk += 4) {
      const double b = sp[kk * BS_SS], a0 = hp[kk * BS_HS], a1 = m1 ? hp[kk * BS_HS + 16] : 0.0;
      acc[BASE] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[BASE], 0, 0, 0);
      acc[BASE + 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[BASE + 1], 0, 0, 0);
    }
  } else {
    const bool m0 = fr < cc;
#pragma unroll 4
    for (int kk = 0; kk < 64; kk += 4) {
      const double b = sp[kk * BS_SS], a0 = m0 ? hp[kk * BS_HS] : 0.0;
      acc[BASE] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[BASE], 0, 0, 0);
    }
  }
}

// part (slab blockIdx.y; p4 rows of ld doubles each) [c][i] = sum_{j in the slab's 64-tiles} Ht[c][j] S(j, i) for the 64
// observations i of tile blockIdx.x, S = the symmetric K^-1 of which only the elements j <= i < n are READ: a tile J > I
// is read as stored (K^-1[J, I]), a tile J < I transposed through LDS (from K^-1[I, J]), the diagonal tile mirrored from
// its lower half.  Rows and columns >= n of S and columns >= n and rows >= p of Ht count as exact zeros, whatever the
// arrays hold there.  Wave w owns the observations 16 w .. 16 w + 15 of the tile and all p4 <= 64 basis columns, 32 of them
// per pass through LDS (bs_pass, with compile-time accumulator indices): one B fragment (S) and up to two A fragments (H^T)
// per 4 j and pass, A[row = c = lane & 15][k = j = lane >> 4], B[k = j = lane >> 4]
// [column = i = lane & 15], C[row = c = (lane >> 4) + 4 v][column = i = lane & 15] (the maps of multi.hip).
// (__launch_bounds__(256, 2): the 16 accumulator register pairs stay in architectural VGPRs.)
__global__ __launch_bounds__(256, 2) void basis_symm_kernel(const double *__restrict__ Kinv, long ldk, long n,
                                                          const double *__restrict__ Ht, long ld, int p, int p4,
                                                          int nt, int nslab, double *__restrict__ part) {
  __shared__ double Ss[64 * BS_SS], Hs[64 * BS_HS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const int it = (int)blockIdx.x, slab = (int)blockIdx.y;
  const long i0 = (long)it * 64;
  const int jt0 = (int)((long)nt * slab / nslab), jt1 = (int)((long)nt * (slab + 1) / nslab);
  bs_f64x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = (bs_f64x4){0.0, 0.0, 0.0, 0.0};
  for (int jt = jt0; jt < jt1; ++jt) {
    const long j0 = (long)jt * 64;
    if (jt > jt0) __syncthreads();  // the previous tile's readers are done
    // the tile of S: a tile below the diagonal of K^-1 (J > I) as stored, row j0 + r; one above it from its mirror image,
    // row i0 + r of K^-1 written down a column of Ss; the diagonal tile both ways from its lower half
    const bool stored = jt > it, diag = jt == it;
    const long rbase = stored ? j0 : i0, cbase = stored ? i0 : j0;
#pragma unroll 2
    for (int rr = 0; rr < 16; ++rr) {
      const int r = w + 4 * rr;
      const long gr = rbase + r, gc = cbase + lane;
      const bool half = !diag || lane <= r;
      const double v = (half && gr < n && gc < n) ? Kinv[gr * ldk + gc] : 0.0;
      if (half && (stored || diag)) Ss[r * BS_SS + lane] = v;
      if (half && !stored) Ss[lane * BS_SS + r] = v;
    }
    bs_load_h(Hs, Ht, ld, 0, min(BS_HC, p4), p, j0, n, w, lane);
    __syncthreads();
    bs_pass<0>(acc, Ss, Hs, min(BS_HC, p4), w, fr, fk);
    if (p4 > BS_HC) {   // the second 32 basis columns
      __syncthreads();  // the first pass's readers are done
      bs_load_h(Hs, Ht, ld, BS_HC, p4 - BS_HC, p, j0, n, w, lane);
      __syncthreads();
      bs_pass<2>(acc, Ss, Hs, p4 - BS_HC, w, fr, fk);
    }
  }
  double *out = part + (long)slab * p4 * ld;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int c = 16 * t + fk + 4 * v;
      if (c < p4) out[(long)c * ld + i0 + 16 * w + fr] = acc[t][v];
    }
  }
}

// Wt (p4 rows of ld doubles) = the slabs' partial sums added in slab order; exact zeros at the columns >= n (up to
// ld) and the rows >= p
__global__ __launch_bounds__(256) void basis_symm_sum_kernel(const double *__restrict__ part, int nslab, long ld, long n,
                                                             long ncol, int p, int p4, double *__restrict__ Wt) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)blockIdx.y;
  if (i >= ld) return;
  double t = 0.0;
  if (c < p && i < n && i < ncol)
    for (int s = 0; s < nslab; ++s) t += part[((long)s * p4 + c) * ld + i];
  Wt[(long)c * ld + i] = t;
}

// part (slab blockIdx.x; p (p + 1) doubles each) [a][b] = sum over the slab's observations i < n of Ht[a][i] Bt[b][i],
// Bt = Wt for b < p and alpha for b == p.  32 observations per pass through LDS; thread e, e + 256, .. owns the element
// e = a (p + 1) + b and sums its observations in index order.
constexpr int BG_CH = 32, BG_S = 33, BG_PER = (64 * 65 + 255) / 256;
__global__ __launch_bounds__(256) void basis_gram_kernel(const double *__restrict__ Ht, const double *__restrict__ Wt,
                                                         long ld, const double *__restrict__ alpha, long n, int p,
                                                         long slab_len, double *__restrict__ part) {
  __shared__ double Hs[64 * BG_S], Bs[65 * BG_S];
  const int tid = threadIdx.x, p1 = p + 1, total = p * p1;
  const long b0 = (long)blockIdx.x * slab_len, b1 = min(n, b0 + slab_len);
  double acc[BG_PER];
#pragma unroll
  for (int q = 0; q < BG_PER; ++q) acc[q] = 0.0;
  for (long i0 = b0; i0 < b1; i0 += BG_CH) {
    if (i0 > b0) __syncthreads();
    for (int e = tid; e < (2 * p + 1) * BG_CH; e += 256) {
      const int row = e / BG_CH, k = e % BG_CH;
      const long gi = i0 + k;
      double v = 0.0;
      if (gi < b1) v = row < p ? Ht[(long)row * ld + gi] : row < 2 * p ? Wt[(long)(row - p) * ld + gi] : alpha[gi];
      if (row < p)
        Hs[row * BG_S + k] = v;
      else
        Bs[(row - p) * BG_S + k] = v;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < BG_PER; ++q) {
      const int e = tid + 256 * q;
      if (e < total) {
        const double *hr = Hs + (e / p1) * BG_S, *br = Bs + (e % p1) * BG_S;
        double t = acc[q];
        for (int k = 0; k < BG_CH; ++k) t += hr[k] * br[k];
        acc[q] = t;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < BG_PER; ++q) {
    const int e = tid + 256 * q;
    if (e < total) part[(long)blockIdx.x * total + e] = acc[q];
  }
}
__global__ __launch_bounds__(256) void basis_gram_sum_kernel(const double *__restrict__ part, int nslab, int total,
                                                             double *__restrict__ Ag) {
  const int e = (int)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  double t = 0.0;
  for (int s = 0; s < nslab; ++s) t += part[(long)s * total + e];
  Ag[e] = t;
}

// One workgroup; Ag = [A | g], p rows of p + 1 doubles, of A the lower triangle is read.  In LDS: the Cholesky factor
// L_A in the lower triangle, then the strict lower triangle of L_A^-1 transposed into the strict upper one (its diagonal
// in a vector).  Out: LA (p x p, zeros above the diagonal), Ainv (p x p, symmetric), beta (p), scal[0] = log|A|,
// scal[1] = g^T beta (= |L_A^-1 g|^2), info[0] = 0 or the first pivot (+ 1) that is not positive and finite -- the other
// outputs are then not written.
__global__ __launch_bounds__(256) void basis_finish_kernel(const double *__restrict__ Ag, int p, double *__restrict__ LA,
                                                           double *__restrict__ Ainv, double *__restrict__ beta,
                                                           double *__restrict__ scal, long long *__restrict__ info) {
  __shared__ double As[64 * 65], dinv[64], gs[64], zs[64];
  __shared__ int bad;
  const int tid = threadIdx.x, p1 = p + 1;
  for (int e = tid; e < p * p; e += 256) {
    const int i = e / p, j = e % p;
    As[i * 65 + j] = j <= i ? Ag[i * p1 + j] : 0.0;
  }
  if (tid < p) gs[tid] = Ag[tid * p1 + p];
  if (tid == 0) bad = 0;
  __syncthreads();
  for (int k = 0; k < p; ++k) {
    if (tid == 0) {
      const double d = As[k * 65 + k];
      if (!(d > 0.0) || !isfinite(d))
        bad = k + 1;
      else
        As[k * 65 + k] = sqrt(d);
    }
    __syncthreads();
    if (bad) break;  // uniform: read behind the barrier
    const double lkk = As[k * 65 + k];
    for (int i = k + 1 + tid; i < p; i += 256) As[i * 65 + k] /= lkk;
    __syncthreads();
    const int m = p - k - 1;  // the trailing lower triangle, rows and columns k + 1 ..
    for (int e = tid; e < m * m; e += 256) {
      const int i = k + 1 + e / m, j = k + 1 + e % m;
      if (j <= i) As[i * 65 + j] -= As[i * 65 + k] * As[j * 65 + k];
    }
    __syncthreads();
  }
  if (bad) {
    if (tid == 0) info[0] = bad;
    return;
  }
  for (int e = tid; e < p * p; e += 256) {
    const int i = e / p, j = e % p;
    LA[e] = j <= i ? As[i * 65 + j] : 0.0;
  }
  // column j of Li = L_A^-1 by forward substitution, one thread each: Li(i, j), i > j, at As[j][i]
  if (tid < p) {
    const int j = tid;
    const double dj = 1.0 / As[j * 65 + j];
    dinv[j] = dj;
    for (int i = j + 1; i < p; ++i) {
      double s = As[i * 65 + j] * dj;
      for (int k = j + 1; k < i; ++k) s += As[i * 65 + k] * As[j * 65 + k];
      As[j * 65 + i] = -s / As[i * 65 + i];
    }
  }
  __syncthreads();
  // z = Li g, beta = Li^T z
  if (tid < p) {
    const int i = tid;
    double s = dinv[i] * gs[i];
    for (int k = 0; k < i; ++k) s += As[k * 65 + i] * gs[k];
    zs[i] = s;
  }
  __syncthreads();
  if (tid < p) {
    const int a = tid;
    double s = dinv[a] * zs[a];
    for (int k = a + 1; k < p; ++k) s += As[a * 65 + k] * zs[k];
    beta[a] = s;
  }
  // A^-1 = Li^T Li: (a, b), b <= a, = sum_{k >= a} Li(k, a) Li(k, b)
  for (int e = tid; e < p * p; e += 256) {
    const int a = e / p, b = e % p;
    if (b > a) continue;
    double s = dinv[a] * (a == b ? dinv[a] : As[b * 65 + a]);
    for (int k = a + 1; k < p; ++k) s += As[a * 65 + k] * As[b * 65 + k];
    Ainv[a * p + b] = s;
    Ainv[b * p + a] = s;
  }
  if (tid == 0) {
    double ld = 0.0, q = 0.0;
    for (int k = 0; k < p; ++k) {
      ld += log(As[k * 65 + k]);
      q += zs[k] * zs[k];
    }
    scal[0] = 2.0 * ld;
    scal[1] = q;
    info[0] = 0;
  }
}

// Ct: (p + 1) rounded up to a multiple of 4 rows of ld doubles.  Rows c < p: Q^T = L_A^-1 W^T by forward substitution
// down the rows, one thread per observation (it reads back the rows it wrote itself); row p: alpha~ = alpha - W beta;
// the rows behind it and every column >= n (up to ld): exact zeros.
__global__ __launch_bounds__(256) void basis_cols_kernel(const double *__restrict__ Wt, long ld, long n, int p,
                                                         const double *__restrict__ LA, const double *__restrict__ beta,
                                                         const double *__restrict__ alpha, double *Ct) {
  __shared__ double Ls[64 * 64], bs[64];
  const int tid = threadIdx.x;
  for (int e = tid; e < p * p; e += 256) Ls[e] = LA[e];
  if (tid < p) bs[tid] = beta[tid];
  __syncthreads();
  const long i = (long)blockIdx.x * 256 + tid;
  if (i >= ld) return;
  const int rows = (p + 1 + 3) / 4 * 4;
  if (i >= n) {
    for (int c = 0; c < rows; ++c) Ct[(long)c * ld + i] = 0.0;
    return;
  }
  double at = alpha[i];
  for (int c = 0; c < p; ++c) {
    const double wv = Wt[(long)c * ld + i];
    double s = wv;
    for (int k = 0; k < c; ++k) s -= Ls[c * p + k] * Ct[(long)k * ld + i];
    Ct[(long)c * ld + i] = s / Ls[c * p + c];
    at -= wv * bs[c];
  }
  Ct[(long)p * ld + i] = at;
  for (int c = p + 1; c < rows; ++c) Ct[(long)c * ld + i] = 0.0;
}

// Per test point j < m, one thread each: R_j = Hz[j] - KW[j] (Hz m x p row-major; KW = Kstar^T W, ldkw doubles per row),
// mu[j] = mu0[j] + R_j beta, sigma[j] = sqrt(prior[j] - q[j] + R_j A^-1 R_j^T): the variance is not clamped before the
// root (solve.hip: sigma_kernel)
__global__ __launch_bounds__(64) void basis_predict_kernel(const double *__restrict__ Hz, const double *__restrict__ KW,
                                                           long ldkw, long m, int p, const double *__restrict__ beta,
                                                           const double *__restrict__ Ainv, const double *__restrict__ mu0,
                                                           const double *__restrict__ prior, const double *__restrict__ q,
                                                           double *__restrict__ mu, double *__restrict__ sigma) {
  __shared__ double Ai[64 * 64], bs[64];
  const int tid = threadIdx.x;
  for (int e = tid; e < p * p; e += 64) Ai[e] = Ainv[e];
  if (tid < p) bs[tid] = beta[tid];
  __syncthreads();
  const long j = (long)blockIdx.x * 64 + tid;
  if (j >= m) return;
  const double *hz = Hz + j * p, *kw = KW + j * ldkw;
  double dm = 0.0, dv = 0.0;
  for (int a = 0; a < p; ++a) {
    const double ra = hz[a] - kw[a];
    dm += ra * bs[a];
    double t = 0.0;
    for (int b = 0; b < p; ++b) t += Ai[a * p + b] * (hz[b] - kw[b]);
    dv += ra * t;
  }
  mu[j] = mu0[j] + dm;
  if (sigma) sigma[j] = sqrt(prior[j] - q[j] + dv);
}

// the slabs of the J range of basis_symm_kernel for n observations: enough workgroups to fill the GPU at small n, at
// most BASIS_SYMM_SLABS_MAX and at most one per 64-tile
int basis_symm_slabs(int64_t n) {
  const int nt = (int)((n + 63) / 64);
  return std::max(1, std::min(std::min(nt, BASIS_SYMM_SLABS_MAX), 1024 / nt));
}
int basis_gram_slabs(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(BASIS_GRAM_SLABS_MAX, (n + 255) / 256)); }

void launch_basis_symm(hipStream_t s, const double *Kinv, int64_t ldk, int64_t n, int64_t npad, const double *Ht, int64_t ld,
                       int p, double *part, double *Wt) {
  const int nt = (int)((n + 63) / 64), nslab = basis_symm_slabs(n), p4 = (p + 3) / 4 * 4;
  GOGP_KLAUNCH(basis_symm_kernel, dim3((unsigned)nt, (unsigned)nslab), dim3(256), 0, s, Kinv, (long)ldk, (long)n, Ht, (long)ld,
               p, p4, nt, nslab, part);
  GOGP_KLAUNCH(basis_symm_sum_kernel, dim3((unsigned)((ld + 255) / 256), (unsigned)p4), dim3(256), 0, s,
               (const double *)part, nslab, (long)ld, (long)n, (long)nt * 64, p, p4, Wt);
  (void)npad;
}

void launch_basis_gram(hipStream_t s, const double *Ht, const double *Wt, int64_t ld, const double *alpha, int64_t n, int p,
                       double *part, double *Ag) {
  const int nslab = basis_gram_slabs(n), total = p * (p + 1);
  const int64_t slab_len = ((n + nslab - 1) / nslab + BG_CH - 1) / BG_CH * BG_CH;
  GOGP_KLAUNCH(basis_gram_kernel, dim3((unsigned)nslab), dim3(256), 0, s, Ht, Wt, (long)ld, alpha, (long)n, p, (long)slab_len,
               part);
  GOGP_KLAUNCH(basis_gram_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const double *)part, nslab,
               total, Ag);
}

void launch_basis_finish(hipStream_t s, const double *Ag, int p, double *LA, double *Ainv, double *beta, double *scal,
                         long long *info) {
  GOGP_KLAUNCH(basis_finish_kernel, dim3(1), dim3(256), 0, s, Ag, p, LA, Ainv, beta, scal, info);
}

void launch_basis_cols(hipStream_t s, const double *Wt, int64_t ld, int64_t n, int p, const double *LA, const double *beta,
                       const double *alpha, double *Ct) {
  GOGP_KLAUNCH(basis_cols_kernel, dim3((unsigned)((ld + 255) / 256)), dim3(256), 0, s, Wt, (long)ld, (long)n, p, LA, beta,
               alpha, Ct);
}

void launch_basis_predict(hipStream_t s, const double *Hz, const double *KW, int64_t ldkw, int64_t m, int p,
                          const double *beta, const double *Ainv, const double *mu0, const double *prior, const double *q,
                          double *mu, double *sigma) {
  if (m <= 0) return;
  GOGP_KLAUNCH(basis_predict_kernel, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, s, Hz, KW, (long)ldkw, (long)m, p, beta,
               Ainv, mu0, prior, q, mu, sigma);
}

}  // namespace gogp
