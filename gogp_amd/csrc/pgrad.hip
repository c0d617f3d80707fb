// pgrad.hip -- the derivatives of the forecast with respect to the test points (gogp_produce_gradient).
//
// No reference counterpart: gp.GP.Produce (gp/gp.go:322-360) returns mu and sigma only.  With k*_j = k(X, z_j),
// alpha = K^-1 y and w_j = K^-1 k*_j = L^-T (L^-1 k*_j):
//     d mu_j    / d z_jd =      sum_i alpha_i dk(z_j, x_i)/dz_jd
//     d sigma_j / d z_jd = (-2  sum_i w_ij    dk(z_j, x_i)/dz_jd) / (2 sigma_j)
// (k(z, z) is the sum of the output scales: no z in it).  Produce's forward substitution leaves V^T = Kstar^T L^-T, one
// test point per row (api.hip: produce_solve_t).  Two device parts are added here:
//   1. bwd_panel_kernel: the plain (NN) product  C (+)= -/+ A B  for a skinny A (the test points' rows), on
//      v_mfma_f64_16x16x4_f64 -- the steps of the block BACKWARD substitution W^T = V^T L^-1, which walks the column
//      panels from last to first: W^T[:, p] = R[:, p] inv(L_pp) (B = the block inverse the forward solve uses, lower
//      triangular), then R[:, j] -= W^T[:, p] L[p, j] for the columns j left of the panel (B = rows of the factor as
//      they are stored: the A B^T tile kernel cannot take them).
//   2. pgrad_kernel / pgrad_final_kernel: both sums above in one pass over X.
#ifndef GOGP_EV  // first pass: the whole file, the kernels without event discounts
#include <algorithm>

#include "kern_eval.h"

#define GOGP_EV 0
#define GOGP_EVN(name) name
namespace gogp {

typedef double pg_f64x4 __attribute__((ext_vector_type(4)));

// C (16 MT rows x 64 columns per workgroup) = A B (sub == 0) or C - A B (sub == 1); A: rows x K (lda), B: K x ncols
// (ldb), all row-major.  tri: B is lower triangular against the columns (B[k][j] == 0 for k < j, element by element:
// a block inverse with its zero upper half), so a workgroup starts at k = its first column.
// One wave per 16 columns: its B fragments are loaded from global memory straight in the MFMA operand layout (lane l:
// B[k + (l >> 4)][j + (l & 15)]; every element of B is needed by exactly one wave, once) -- a panel row of L is
// streamed once per group of 64 test points.  A, which the four waves share, goes through LDS in chunks of KC columns.
// The next chunk's loads are in flight behind the MFMAs of the current one.  grid: (ncols / 64, row groups of 16 MT).
template <int MT>
__global__ __launch_bounds__(256, 2) void bwd_panel_kernel(const double *__restrict__ A, long lda,
                                                          const double *__restrict__ B, long ldb, double *C, long ldc,
                                                          int K, int tri, int sub) {
  constexpr int KC = 32, AS = KC + 1;
  __shared__ double As[16 * MT * AS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int j0 = blockIdx.x * 64;
  A += (long)blockIdx.y * (16 * MT) * lda;
  C += (long)blockIdx.y * (16 * MT) * ldc + j0;
  B += j0 + 16 * w;
  // staging map of A: chunk (16 MT) x 32: thread: row tid >> 2, 8 consecutive k from (tid & 3) * 8
  const int ar = tid >> 2, ak = (tid & 3) * 8;
  const int fr = lane & 15, fk = lane >> 4;
  double ra[8], rb[KC / 4];
  auto gload = [&](int k0) {
    if (ar < 16 * MT) {
#pragma unroll
      for (int i = 0; i < 8; ++i) ra[i] = A[(long)ar * lda + k0 + ak + i];
    }
#pragma unroll
    for (int kk = 0; kk < KC / 4; ++kk) rb[kk] = B[(long)(k0 + 4 * kk + fk) * ldb + fr];
  };
  pg_f64x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = (pg_f64x4){0.0, 0.0, 0.0, 0.0};
  const int kbeg = tri ? j0 : 0;
  if (kbeg < K) gload(kbeg);
  for (int k0 = kbeg; k0 < K; k0 += KC) {
    __syncthreads();  // the previous chunk's readers are done
    if (ar < 16 * MT) {
#pragma unroll
      for (int i = 0; i < 8; ++i) As[ar * AS + ak + i] = ra[i];
    }
    double b[KC / 4];
#pragma unroll
    for (int kk = 0; kk < KC / 4; ++kk) b[kk] = rb[kk];
    __syncthreads();
    if (k0 + KC < K) gload(k0 + KC);
#pragma unroll
    for (int kk = 0; kk < KC / 4; ++kk) {
#pragma unroll
      for (int t = 0; t < MT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(As[(16 * t + fr) * AS + 4 * kk + fk], b[kk], acc[t], 0, 0, 0);
    }
  }
  // C fragment: column = lane & 15, row = (lane >> 4) + 4 v
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      double *c = C + (long)(16 * t + fk + 4 * v) * ldc + 16 * w + fr;
      *c = sub ? *c - acc[t][v] : acc[t][v];
    }
}

void launch_bwd_panel(hipStream_t s, int64_t rows16, const double *A, int64_t lda, const double *B, int64_t ldb,
                      double *C, int64_t ldc, int64_t ncols, int K, bool tri, bool sub) {
  if (rows16 <= 0 || ncols <= 0 || K <= 0) return;
  const unsigned nx = (unsigned)(ncols / 64);
#define GOGP_LAUNCH_BP(MTV, GROUPS)                                                                              \
  GOGP_KLAUNCH(bwd_panel_kernel<MTV>, dim3(nx, (unsigned)(GROUPS)), dim3(256), 0, s, A, (long)lda, B, (long)ldb, C, \
               (long)ldc, K, tri ? 1 : 0, sub ? 1 : 0)
  if (rows16 == 1) GOGP_LAUNCH_BP(1, 1);
  else if (rows16 == 2) GOGP_LAUNCH_BP(2, 1);
  else GOGP_LAUNCH_BP(4, (rows16 + 3) / 4);
#undef GOGP_LAUNCH_BP
}

constexpr int PG_TJ = 4;  // test points per workgroup of pgrad_kernel
#endif

// Partial sums of both derivative sums: workgroup (jb, slab) takes the PG_TJ test points from jb * PG_TJ and the
// `tps` 64-row tiles of X from slab * tps; thread (r = tid >> 2, q = tid & 3) owns the pair (row r of the tile, test
// point q).  The X tile is staged in LDS as xgrad_kernel stages it.  dk/dz is formed once per pair (unit weight) and
// enters both sums.  The sums over the rows are taken in a fixed order (lanes, then waves) and written -- no atomics --
// to part[0 / 1][slab][j][d]; pgrad_final_kernel adds the slabs.  Dimensions d0 .. d0 + DMAX - 1 per launch.
// GOGP_EV = 1 (pgrad_kernel_ev): one event mask per point, the pair's derivative is multiplied by the pair's discount.
template <int DMAX>
__global__ __launch_bounds__(256) void GOGP_EVN(pgrad_kernel)(const DevParams *__restrict__ Pp,
                                                              const double *__restrict__ X, long n,
                                                              const double *__restrict__ Z, long m,
                                                              const double *__restrict__ alpha,
                                                              const double *__restrict__ Wt, long ld, int tps,
                                                              double *__restrict__ part, int d0) {
  extern __shared__ double sm[];
  const DevParams &P = *Pp;
  const int D = P.ndim;
  double *Xi = sm;                      // [64][D]
  double *Zj = Xi + 64 * D;             // [PG_TJ][D]
  double *red = Zj + PG_TJ * D;         // [4 waves][PG_TJ][2 DMAX]
  unsigned long long *Mi = reinterpret_cast<unsigned long long *>(red + 4 * PG_TJ * 2 * DMAX);  // GOGP_EV: [64] row masks
  const int tid = threadIdx.x, r = tid >> 2, q = tid & 3;
  const long j = (long)blockIdx.x * PG_TJ + q;
  const long nslab = gridDim.y;
  for (int idx = tid; idx < PG_TJ * D; idx += 256) {
    const int qq = idx / D, d = idx - qq * D;
    const long jj = (long)blockIdx.x * PG_TJ + qq;
    Zj[idx] = (jj < m) ? Z[jj * D + d] : 0.0;
  }
  __syncthreads();
  const double *zj = Zj + q * D;
  const unsigned long long mz = GOGP_EV ? event_mask(P, zj[P.ev_axis]) : 0ull;
  double sa[DMAX], sw[DMAX];
#pragma unroll
  for (int d = 0; d < DMAX; ++d) sa[d] = sw[d] = 0.0;
  for (int t = 0; t < tps; ++t) {
    const long i0 = ((long)blockIdx.y * tps + t) * 64;
    if (i0 >= n) break;
    __syncthreads();
    for (int idx = tid; idx < 64 * D; idx += 256) {
      const int rr = idx / D, d = idx - rr * D;
      Xi[idx] = (i0 + rr < n) ? X[(i0 + rr) * D + d] : 0.0;
    }
    if (GOGP_EV && tid < 64) Mi[tid] = event_mask(P, (i0 + tid < n) ? X[(i0 + tid) * D + P.ev_axis] : 0.0);
    __syncthreads();
    if (i0 + r < n && j < m) {
      double g[DMAX];
#pragma unroll
      for (int d = 0; d < DMAX; ++d) g[d] = 0.0;
      const double *xi = Xi + r * D;
      double wa = alpha[i0 + r], ww = Wt[j * ld + i0 + r];
      if (GOGP_EV) {
        const double disc = event_discount(P, mz, Mi[r]);
        wa *= disc;
        ww *= disc;
      }
      simil_xgrad_accum<DMAX>(
          P, [&](int d) { return zj[d]; }, [&](int d) { return xi[d]; }, 1.0, g, d0);
#pragma unroll
      for (int d = 0; d < DMAX; ++d) {
        sa[d] += wa * g[d];
        sw[d] += ww * g[d];
      }
    }
  }
  // rows of one test point within a wave: lanes that differ in bits 2 .. 5
  const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    double a = sa[d], b = sw[d];
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) {
      a += __shfl_xor(a, o);
      b += __shfl_xor(b, o);
    }
    if (lane < PG_TJ) {
      red[(wv * PG_TJ + lane) * 2 * DMAX + d] = a;
      red[(wv * PG_TJ + lane) * 2 * DMAX + DMAX + d] = b;
    }
  }
  __syncthreads();
  if (tid < PG_TJ * 2 * DMAX) {
    const int qq = tid / (2 * DMAX), e = tid - qq * 2 * DMAX, which = e / DMAX, d = e - which * DMAX;
    const long jj = (long)blockIdx.x * PG_TJ + qq;
    if (jj < m && d0 + d < D) {
      double v = 0.0;
      for (int k = 0; k < 4; ++k) v += red[(k * PG_TJ + qq) * 2 * DMAX + e];
      part[(((long)which * nslab + blockIdx.y) * m + jj) * D + d0 + d] = v;
    }
  }
}

#if !GOGP_EV  // second pass: pgrad_kernel again, with event discounts, as pgrad_kernel_ev
#undef GOGP_EV
#undef GOGP_EVN
#define GOGP_EV 1
#define GOGP_EVN(name) name##_ev
#include "pgrad.hip"
#undef GOGP_EV
#undef GOGP_EVN
#define GOGP_EV 0
#define GOGP_EVN(name) name

// dmu[j][d] = sum over the slabs (in order) of the alpha sums; dsigma[j][d] = -2 (the same of the w sums) / (2 sigma_j):
// sigma is not clamped (gogp_produce does not either), so a row with s_j <= 0 is what the division yields
__global__ __launch_bounds__(256) void pgrad_final_kernel(const double *__restrict__ part, int nslab, long m, int D,
                                                          const double *__restrict__ sigma, double *__restrict__ dmu,
                                                          double *__restrict__ dsigma) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= m * D) return;
  double a = 0.0, b = 0.0;
  for (int sl = 0; sl < nslab; ++sl) {
    a += part[(long)sl * m * D + idx];
    b += part[((long)nslab + sl) * m * D + idx];
  }
  dmu[idx] = a;
  dsigma[idx] = (-2.0 * b) / (2.0 * sigma[idx / D]);
}

int pgrad_slabs(int64_t npad, int64_t m, int *tps_out) {
  const int tiles = (int)(npad / 64);
  const int64_t mblk = (m + PG_TJ - 1) / PG_TJ;
  int nslab = (int)std::min<int64_t>(tiles, std::max<int64_t>(1, 1024 / mblk));
  const int tps = (tiles + nslab - 1) / nslab;
  nslab = (tiles + tps - 1) / tps;
  if (tps_out) *tps_out = tps;
  return nslab;
}

void launch_pgrad(hipStream_t s, const DevParams *p, int ndim, const double *X, int64_t n, int64_t npad,
                  const double *Z, int64_t m, const double *alpha, const double *Wt, int64_t ld, const double *sigma,
                  double *part, double *dmu, double *dsigma, bool ev) {
  int tps = 1;
  const int nslab = pgrad_slabs(npad, m, &tps);
  const dim3 grid((unsigned)((m + PG_TJ - 1) / PG_TJ), (unsigned)nslab);
#define GOGP_LAUNCH_PG(KERNEL, DM, D0)                                                                              \
  do {                                                                                                              \
    const size_t lds = (size_t)((64 + PG_TJ) * ndim + 4 * PG_TJ * 2 * DM) * sizeof(double) + 64 * sizeof(unsigned long long); \
    GOGP_KLAUNCH(KERNEL<DM>, grid, dim3(256), lds, s, p, X, (long)n, Z, (long)m, alpha, Wt, (long)ld, tps, part, D0); \
  } while (0)
  // more than 16 dimensions: passes of 16 (three DMAX-vectors of doubles per thread: 16 keeps the instance inside the
  // register limits of the code-object audit without an allow-list entry, as launch_xgrad's event instances)
  if (ev) {
    if (ndim <= 4) GOGP_LAUNCH_PG(pgrad_kernel_ev, 4, 0);
    else if (ndim <= 8) GOGP_LAUNCH_PG(pgrad_kernel_ev, 8, 0);
    else
      for (int d0 = 0; d0 < ndim; d0 += 16) GOGP_LAUNCH_PG(pgrad_kernel_ev, 16, d0);
  } else if (ndim <= 4) GOGP_LAUNCH_PG(pgrad_kernel, 4, 0);
  else if (ndim <= 8) GOGP_LAUNCH_PG(pgrad_kernel, 8, 0);
  else
    for (int d0 = 0; d0 < ndim; d0 += 16) GOGP_LAUNCH_PG(pgrad_kernel, 16, d0);
#undef GOGP_LAUNCH_PG
  GOGP_KLAUNCH(pgrad_final_kernel, dim3((unsigned)((m * ndim + 255) / 256)), dim3(256), 0, s, part, nslab, (long)m, ndim,
               sigma, dmu, dsigma);
}

}  // namespace gogp
#undef GOGP_EV
#undef GOGP_EVN
#endif
