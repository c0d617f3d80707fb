// blockcv.hip -- leave-block-out cross-validation from the explicit K^-1 (gogp_blockcv, gogp_blockcv_gradient; api.hip
// orchestrates).  The "leave-out-k" form of Rasmussen & Williams section 5.4.2: the rows are cut into F consecutive
// blocks B_f = [start[f], start[f + 1]) of 1 .. 128 rows.  With Q = K^-1, alpha = Q y and, per block, Q_BB = C C^T
// (lower Cholesky), X = C^-1, w = X alpha_B, v_B = X^T w (= Q_BB^-1 alpha_B), Sigma_B = Q_BB^-1 = X^T X:
//     mu_B = y_B - v_B,  sigma_i = sqrt((Sigma_B)_ii)  (the norm of column i of X),
//     logp_f = -1/2 |w|^2 + sum_i log C_ii - |B| / 2 log 2 pi  = log p(y_B | every other block).
// With v the stacked v_B, u = Q v and M = blockdiag(Sigma_B + v_B v_B^T),
//     d sum_f logp_f = sum_ab W_ab dK_ab,   W = 1/2 (u alpha^T + alpha u^T) - 1/2 Q M Q,
// and M_B = S_B S_B^T for S_B = X^T + gamma v_B w^T, gamma = (sqrt(1 + |w|^2) - 1) / |w|^2 = 1 / (sqrt(1 + |w|^2) + 1)
// (the second form is exact at w = 0 and loses nothing near it).  So G = Bm Bm^T - u alpha^T - alpha u^T = -2 W with
// Bm = Q blockdiag(S_B): the matrix gogp_loo_gradient hands to the gradient reduction, which blocks of one row
// reproduce (C = sqrt(kappa), S = sqrt((1 + alpha^2 / kappa) / kappa) = s_i of loo.hip).
//
// Grouping (blockcv_pack: a host function of `start` alone): consecutive blocks are packed greedily, in order, into
// groups of at most 128 columns.  A group's diagonal piece of K^-1 with the entries between different blocks replaced by
// exact zeros, padded with the identity to 128, is block diagonal, and so are its factor and its inverse: ONE in-LDS
// factorisation (potrf128_lds, invert128_lds of diag256.hip, compiled into this translation unit's own namespace)
// serves every block of the group.
//
// Every sum has a fixed order (no atomics): two identical calls give the same bits.
#define GOGP_NS gogp_bcv
#define GOGP_DIAG256_DEVICE_ONLY
#include "diag256.hip"

namespace gogp_bcv {

// ---- 1. the group kernel: one workgroup (512 threads) per group ---------------------------------------------------------
// bstart: the F + 1 block starts; gfirst: the ngroups + 1 first blocks of the groups.  Group g holds the columns
// c0 = bstart[gfirst[g]] .. c1 = bstart[gfirst[g + 1]] of K^-1, m = c1 - c0 <= 128 of them.  Only the elements
// j <= i < n of Kinv are READ (loo.hip: loo_scale_symv_kernel says what the rest may hold).  Written: mu, sigma, v and
// ones (= 1.0) at the rows c0 .. c1 - 1, logp at the group's blocks, the group's 128 x 128 S_g (S_B on its diagonal
// blocks, exact zeros elsewhere, padding included) at Sg + g * 128 * 128, and info[g] = first failing pivot's global
// row + 1, or 0.  A group that fails writes info[g] alone.
__global__ __launch_bounds__(NT) void blockcv_groups_kernel(const double *__restrict__ Kinv, long ld,
                                                            const double *__restrict__ alpha, const double *__restrict__ y,
                                                            const long long *__restrict__ bstart,
                                                            const long long *__restrict__ gfirst, double *__restrict__ mu,
                                                            double *__restrict__ sigma, double *__restrict__ v,
                                                            double *__restrict__ ones, double *__restrict__ logp,
                                                            double *__restrict__ Sg, long long *__restrict__ info) {
  __shared__ __attribute__((aligned(16))) double S[128 * SLD];
  __shared__ __attribute__((aligned(16))) double G[GSIZE];
  __shared__ double rinv_s[8 * 16];
  __shared__ double as[128], ws[128], vs[128], lc[128], gm[128];  // alpha, w, v, log C_ii, gamma of the column's block
  __shared__ int bs[129];                                         // the group's block starts, relative to c0
  __shared__ int lo[128], hi[128], bid[128];                      // column -> its block [lo, hi) and the block's index
  __shared__ long long info_s;
  const int tid = threadIdx.x;
  const long g = blockIdx.x;
  const long f0 = gfirst[g], f1 = gfirst[g + 1];
  const int nb = (int)(f1 - f0);
  const long c0 = bstart[f0];
  const int m = (int)(bstart[f1] - c0);
  if (tid <= nb && tid < 129) bs[tid] = (int)(bstart[f0 + tid] - c0);
  if (tid == 0) info_s = 0;
  __syncthreads();
  if (tid < 128) {
    int b = -1, l = tid, h = tid + 1;  // the padding: blocks of one row
    if (tid < m) {
      b = 0;
      while (bs[b + 1] <= tid) ++b;  // (bs[nb] = m > tid)
      l = bs[b];
      h = bs[b + 1];
    }
    bid[tid] = b;
    lo[tid] = l;
    hi[tid] = h;
    as[tid] = tid < m ? alpha[c0 + tid] : 0.0;
  }
  __syncthreads();
  // ---- the group's block-diagonal piece of K^-1, lower triangle; rows / columns >= m: identity ---------------------------
  for (int idx = tid; idx < 128 * 128; idx += NT) {
    const int i = idx >> 7, j = idx & 127;
    double k = 0.0;
    if (j <= i) {
      if (i < m) {
        if (lo[i] == lo[j]) k = Kinv[(c0 + i) * ld + c0 + j];
      } else {
        k = (i == j) ? 1.0 : 0.0;
      }
    }
    S[i * SLD + j] = k;
  }
  __syncthreads();
  potrf128_lds(S, G, rinv_s, tid, c0, c0 + m, &info_s);  // (ends with a barrier)
  const long long bad = info_s;
  if (bad != 0) {  // workgroup-uniform: this group stops here
    if (tid == 0) info[g] = bad;
    return;
  }
  if (tid == 0) info[g] = 0;
  if (tid < 128) lc[tid] = tid < m ? log(S[tid * SLD + tid]) : 0.0;
  __syncthreads();  // the inverse starts by overwriting the diagonal blocks
  invert128_lds(S, G, tid);  // S = X = C^-1 (lower, block diagonal); ends with a barrier
  // ---- w = X alpha_B: row tid / 4, a quarter of the row's block each, added in a fixed order ------------------------------
  {
    const int i = tid >> 2, p = tid & 3;
    double a = 0.0;
    for (int k = lo[i] + p; k <= i; k += 4) a += S[i * SLD + k] * as[k];
    a += __shfl_xor(a, 1);
    a += __shfl_xor(a, 2);
    if (p == 0) ws[i] = a;
  }
  __syncthreads();
  // ---- v = X^T w and the column norms of X: column tid / 4 over the rows of its block --------------------------------------
  {
    const int j = tid >> 2, p = tid & 3;
    double a = 0.0, q = 0.0;
    for (int k = j + p; k < hi[j]; k += 4) {
      const double x = S[k * SLD + j];
      a += x * ws[k];
      q += x * x;
    }
    a += __shfl_xor(a, 1);
    a += __shfl_xor(a, 2);
    q += __shfl_xor(q, 1);
    q += __shfl_xor(q, 2);
    if (p == 0) {
      vs[j] = a;
      if (j < m) {
        mu[c0 + j] = y[c0 + j] - a;
        sigma[c0 + j] = sqrt(q);
        v[c0 + j] = a;
        ones[c0 + j] = 1.0;
      }
    }
  }
  // ---- per block: |w|^2 and sum log C_ii, by every column of the block in the same order (the same bits) -------------------
  if (tid < 128) {
    double w2 = 0.0, sl = 0.0;
    for (int k = lo[tid]; k < hi[tid]; ++k) {
      w2 += ws[k] * ws[k];
      sl += lc[k];
    }
    gm[tid] = 1.0 / (sqrt(1.0 + w2) + 1.0);
    if (tid < m && tid == lo[tid])
      logp[f0 + bid[tid]] = -0.5 * w2 + sl - (double)(hi[tid] - lo[tid]) * 0.9189385332046727418;  // 1/2 log 2 pi
  }
  __syncthreads();
  // ---- S_g: (S_B)_ij = X_ji + gamma v_i w_j inside a block, exact zeros elsewhere ----------------------------------------
  double *out = Sg + g * (128L * 128L);
  for (int idx = tid; idx < 128 * 128; idx += NT) {
    const int i = idx >> 7, j = idx & 127;
    double s = 0.0;
    if (i < m && j < m && lo[i] == lo[j]) s = (j >= i ? S[j * SLD + i] : 0.0) + gm[i] * vs[i] * ws[j];
    out[idx] = s;
  }
}

// ---- 2. the block multiply: Bm = Q blockdiag(S_g), in place, on v_mfma_f64_16x16x4_f64 --------------------------------
// Workgroup (x, g): rows r0 = 64 x .. r0 + 63 of Q (r0 < n <= the rows of Q), columns c0 .. c0 + m - 1 of group g.  S_g
// goes through LDS in two halves of 64 k rows (two workgroups per CU; rows 144 doubles apart: the fragment reads of two k
// rows land on disjoint halves of the banks);
// wave w owns the rows r0 + 16 w .. + 15: it reads its 16 x m piece of Q into registers as the A fragments of the 32
// k-steps (plain 8-byte loads: a group starts at any column, so no wider alignment holds), multiplies, and stores the
// piece back -- nobody else reads or writes these elements, and every load of the wave precedes its first store.  The
// columns >= m of the 128-wide product are not read (their A fragments are zeros) and not written.
constexpr int BLD = 144;
__global__ __launch_bounds__(256, 2) void blockcv_apply_kernel(double *__restrict__ Q, long ld,
                                                               const long long *__restrict__ bstart,
                                                               const long long *__restrict__ gfirst,
                                                               const double *__restrict__ Sg) {
  __shared__ __attribute__((aligned(16))) double Bs[64 * BLD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const long g = blockIdx.y;
  const long c0 = bstart[gfirst[g]];
  const int m = (int)(bstart[gfirst[g + 1]] - c0);
  const double *src = Sg + g * (128L * 128L);
  const double *row = Q + ((long)blockIdx.x * 64 + w * 16 + fr) * ld + c0;
  double a[32];
#pragma unroll
  for (int ks = 0; ks < 32; ++ks) {
    const int k = ks * 4 + fk;
    const double q = row[k < m ? k : m - 1];  // (every load is issued: no branch around it, one wait for all)
    a[ks] = k < m ? q : 0.0;
  }
  f64x4 acc[8];
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) acc[ct] = (f64x4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    if (half) __syncthreads();  // every wave is done with the first half
    for (int idx = tid; idx < 64 * 64; idx += 256) {
      const int k = idx >> 6, j2 = (idx & 63) * 2;
      *reinterpret_cast<f64x2 *>(Bs + k * BLD + j2) = *reinterpret_cast<const f64x2 *>(src + (half * 64 + k) * 128 + j2);
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      const double *bp = Bs + (ks * 4 + fk) * BLD + fr;
#pragma unroll
      for (int ct = 0; ct < 8; ++ct) acc[ct] = mfma(a[half * 16 + ks], bp[ct * 16], acc[ct]);
    }
  }
  // C[row fk + 4 v][column ct * 16 + fr]
  double *dst = Q + ((long)blockIdx.x * 64 + w * 16 + fk) * ld + c0 + fr;
#pragma unroll
  for (int ct = 0; ct < 8; ++ct)
    if (ct * 16 + fr < m) {
#pragma unroll
      for (int vv = 0; vv < 4; ++vv) dst[(long)(4 * vv) * ld + ct * 16] = acc[ct][vv];
    }
}

}  // namespace gogp_bcv

namespace gogp {

int blockcv_pack(const int64_t *start, int64_t F, int64_t *first) {
  if (F <= 0) {
    first[0] = 0;
    return 0;
  }
  int g = 0;
  int64_t cols = 0;
  first[0] = 0;
  for (int64_t f = 0; f < F; ++f) {
    const int64_t len = start[f + 1] - start[f];
    if (cols + len > 128) {
      first[++g] = f;
      cols = 0;
    }
    cols += len;
  }
  first[g + 1] = F;
  return g + 1;
}

void launch_blockcv_groups(hipStream_t s, const double *Kinv, int64_t ld, const double *alpha, const double *y,
                           const int64_t *bstart, const int64_t *gfirst, int ngroups, double *mu, double *sigma, double *v,
                           double *ones, double *logp, double *Sg, long long *info) {
  GOGP_KLAUNCH(gogp_bcv::blockcv_groups_kernel, dim3((unsigned)ngroups), dim3(gogp_bcv::NT), 0, s, Kinv, (long)ld, alpha, y,
               reinterpret_cast<const long long *>(bstart), reinterpret_cast<const long long *>(gfirst), mu, sigma, v, ones,
               logp, Sg, info);
}

void launch_blockcv_apply(hipStream_t s, double *Q, int64_t ld, int64_t n, const int64_t *bstart, const int64_t *gfirst,
                          int ngroups, const double *Sg) {
  GOGP_KLAUNCH(gogp_bcv::blockcv_apply_kernel, dim3((unsigned)((n + 63) / 64), (unsigned)ngroups), dim3(256), 0, s, Q, (long)ld,
               reinterpret_cast<const long long *>(bstart), reinterpret_cast<const long long *>(gfirst), Sg);
}

}  // namespace gogp
