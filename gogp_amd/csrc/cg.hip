// cg.hip -- the kernels of the iterative exact GP (gogp_cg_*; cg_api.hip orchestrates; include/gogp_hip.h states the
// iteration; DESIGN.md section 4, "Iterative (CG)"): matrix-free preconditioned conjugate gradients on
// K^ = k(X, X) + sigma^2 I + diag(v), up to CG_MAX_T = 64 systems in lock-step.
//
//   kmm_kernel            the hot path: Out[t][i] = sum_j k(a_i, b_j) V[t][j] (+ diag_i V[t][i]) on v_mfma_f64_16x16x4_f64.
//                         A workgroup takes 64 rows (16 per wave) and a slab of 64-column tiles.  Per step of 4 columns
//                         lane (fr = lane & 15, fk = lane >> 4) evaluates k(a_{fr}, b_{fk}) with simil_value -- its A
//                         operand, which never touches LDS or memory -- and V[16 g + fr][j + fk] is the B operand of
//                         column group g: one evaluation feeds up to four MFMAs (64 right-hand sides).  The slabs'
//                         partial sums are added in slab order by kmm_finish_kernel.
//   cg_dots_kernel, cg_dots_final_kernel   T dot products in two stages, every sum in a fixed order; the final kernel
//                         also takes the iteration's per-column decisions (CgDotMode): a = rho / p^T q, the freeze test
//                         |r| <= tol |b|, beta = rho' / rho.
//   cg_update_xr_kernel, cg_update_p_kernel, cg_scale_kernel   the fused vector updates; a frozen column is not touched.
//   cg_diag_kernel .. cg_precond_kernel   the preconditioner P = L L^T + D by Woodbury's identity (common.h).
//   cg_probe_kernel, cg_grad_kernel       the LML's gradient (gogp_cg_lml_gradient): the probes z = D^1/2 (Ls xi1 + xi2), and
//                         the pair reduction of W = alpha alpha^T - (1/t) sum u_s w_s^T against theta dk/dtheta -- the
//                         product's mirror image: the matrix cores form the weights, the lanes evaluate the derivative.
//   cg_lanczos_quadrature (host)          e_1^T log(T) e_1 of a column's Lanczos tridiagonal, from its a and beta.
//
// Kernel boundaries are the only synchronisation: no atomics, no spin-waits, vector stores only; the order of every
// sum depends on the sizes alone -- never on T --, so two identical calls return identical bits and a column has the
// same bits alone as inside a block of 64.
#include <algorithm>
#include <cmath>
#include <vector>

#include "kern_eval.h"

namespace gogp {

typedef double cg_f64x4 __attribute__((ext_vector_type(4)));

namespace {
// the workgroup's sum of v in a fixed tree (256 threads); thread 0 returns with it
__device__ __forceinline__ double cg_block_sum(double v, double *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();  // an earlier use of red is read
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
}  // namespace

// ---- the product ----------------------------------------------------------------------------------------------------------
// Work item w = blockIdx.x + q gridDim.x: row tile w / nslab, slab w % nslab (column tiles slab * tps .. ).  Dynamic LDS:
// As[64][DS], Bs[64][DS] (DS = ndim | 1: the 16 rows a wave reads lie in different banks), Vs[64][VS] (VS = 16 ng + 1).
__global__ __launch_bounds__(256, 2) void kmm_kernel(const DevParams *__restrict__ Pp, const double *__restrict__ A, long rows,
                                                  const double *__restrict__ B, long cols, const double *__restrict__ V,
                                                  long ldv, int T, const double *__restrict__ diag, int nslab, int tps,
                                                  long nitems, long rpad, double *__restrict__ part) {
  extern __shared__ double sm[];
  const DevParams &P = *Pp;
  const int D = P.ndim;
  const int DS = D | 1;
  const int ng = (T + 15) >> 4;  // column groups of 16 right-hand sides (uniform)
  const int VS = 16 * ng + 1;
  double *As = sm, *Bs = sm + 64 * DS, *Vs = Bs + 64 * DS;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const long ctiles = (cols + 63) >> 6;
  for (long item = blockIdx.x; item < nitems; item += gridDim.x) {
    const long rt = item / nslab;
    const int slab = (int)(item - rt * nslab);
    const long r0 = rt * 64;
    __syncthreads();  // the previous item's reads of As are done
    for (int idx = tid; idx < 64 * D; idx += 256) {
      const int r = idx / D, d = idx - r * D;
      As[r * DS + d] = (r0 + r < rows) ? A[(r0 + r) * D + d] : 0.0;
    }
    const long gi = r0 + 16 * w + fr;
    const double *arow = As + (16 * w + fr) * DS;
    cg_f64x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = cg_f64x4{0.0, 0.0, 0.0, 0.0};
    const long t1 = std::min<long>(ctiles, (long)(slab + 1) * tps);
    for (long ct = (long)slab * tps; ct < t1; ++ct) {
      const long c0 = ct * 64;
      __syncthreads();  // the previous tile's reads of Bs and Vs are done (and As is staged)
      for (int idx = tid; idx < 64 * D; idx += 256) {
        const int r = idx / D, d = idx - r * D;
        Bs[r * DS + d] = (c0 + r < cols) ? B[(c0 + r) * D + d] : 0.0;
      }
      for (int idx = tid; idx < 64 * 16 * ng; idx += 256) {
        const int j = idx & 63, t = idx >> 6;
        Vs[j * VS + t] = (t < T && c0 + j < cols) ? V[(long)t * ldv + c0 + j] : 0.0;
      }
      __syncthreads();
      for (int jj = 0; jj < 64; jj += 4) {
        const long gj = c0 + jj + fk;
        double k = 0.0;
        if (gi < rows && gj < cols) {
          const double *brow = Bs + (jj + fk) * DS;
          k = simil_value(
              P, [&](int d) { return arow[d]; }, [&](int d) { return brow[d]; });
          if (diag && gi == gj) k += diag[gi];
        }
        const double *vp = Vs + (jj + fk) * VS + fr;
        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(k, vp[0], acc[0], 0, 0, 0);
        if (ng > 1) acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(k, vp[16], acc[1], 0, 0, 0);
        if (ng > 2) acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(k, vp[32], acc[2], 0, 0, 0);
        if (ng > 3) acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(k, vp[48], acc[3], 0, 0, 0);
      }
    }
    // C fragment: column (right-hand side) = lane & 15, row = (lane >> 4) + 4 v
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int t = 16 * g + fr;
      if (t < T) {
        double *dst = part + ((long)slab * T + t) * rpad + r0 + 16 * w + fk;
#pragma unroll
        for (int v = 0; v < 4; ++v) dst[4 * v] = acc[g][v];
      }
    }
  }
}

// Out[t][i] = sum_slab part[slab][t][i] in slab order for i < rows, 0 for rows <= i < ldo
__global__ __launch_bounds__(256) void kmm_finish_kernel(const double *__restrict__ part, int nslab, int T, long rpad,
                                                         long rows, double *__restrict__ Out, long ldo) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int t = blockIdx.y;
  if (i >= ldo) return;
  double s = 0.0;
  if (i < rows)
    for (int q = 0; q < nslab; ++q) s += part[((long)q * T + t) * rpad + i];
  Out[(long)t * ldo + i] = s;
}

// ---- dot products and the per-column decisions -------------------------------------------------------------------------------
// part[t * gridDim.x + b] = sum over workgroup b's elements i = (b + q gridDim.x) 256 + tid of A[t][i] B[t][i]
__global__ __launch_bounds__(256) void cg_dots_kernel(const double *__restrict__ A, const double *__restrict__ B, long ld,
                                                      long n, double *__restrict__ part) {
  __shared__ double red[4];
  const int t = blockIdx.y;
  const double *a = A + (long)t * ld, *b = B + (long)t * ld;
  double s = 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) s += a[i] * b[i];
  s = cg_block_sum(s, red);
  if (threadIdx.x == 0) part[(long)t * gridDim.x + blockIdx.x] = s;
}

// Column t = blockIdx.x: dot = the nb partials, thread tid its k = tid, tid + 256, .. in that order, then the fixed tree.
//   CG_DOT_PLAIN  out[t] = dot
//   CG_DOT_BNORM  |b|^2 = dot; rr = dot; iterations = 0; the column is frozen from the start iff dot == 0 (b = 0)
//   CG_DOT_RHO0   rho = dot                                                   (r^T z before the first iteration)
//   CG_DOT_PQ     p^T q = dot; a live column: a = rho / dot, or -- dot not positive and finite -- marked bad and frozen
//                 with a = 0; a frozen column: a = 0
//   CG_DOT_RR     a live column: rr = dot, iterations = it, frozen iff sqrt(dot) <= tol sqrt(|b|^2)
//   CG_DOT_BETA   a live column: beta = dot / rho, rho = dot; a frozen one: beta = 0
// out (may be nullptr in the other modes) receives the dot product in every mode.  hist (may be nullptr): the column's a
// (mode CG_DOT_PQ) and beta (mode CG_DOT_BETA) of iteration `it` as just decided, rows 2 (it - 1) and 2 (it - 1) + 1 of
// CG_MAX_T doubles.
__global__ __launch_bounds__(256) void cg_dots_final_kernel(const double *__restrict__ part, int nb, int mode, int it,
                                                            double tol, double *__restrict__ out, double *__restrict__ sc,
                                                            int *__restrict__ st, double *__restrict__ hist) {
  __shared__ double red[4];
  const int t = blockIdx.x;
  double s = 0.0;
  for (int k = threadIdx.x; k < nb; k += 256) s += part[(long)t * nb + k];
  s = cg_block_sum(s, red);
  if (threadIdx.x != 0) return;
  if (out) out[t] = s;
  if (mode == CG_DOT_PLAIN) return;
  double *rho = sc + CG_SC_RHO * CG_MAX_T, *a = sc + CG_SC_A * CG_MAX_T, *beta = sc + CG_SC_BETA * CG_MAX_T;
  double *bn = sc + CG_SC_BNORM2 * CG_MAX_T, *rr = sc + CG_SC_RR * CG_MAX_T, *pq = sc + CG_SC_PQ * CG_MAX_T;
  int *frozen = st + CG_ST_FROZEN * CG_MAX_T, *iters = st + CG_ST_ITERS * CG_MAX_T, *bad = st + CG_ST_BAD * CG_MAX_T;
  if (mode == CG_DOT_BNORM) {
    bn[t] = s, rr[t] = s;
    rho[t] = 0.0, a[t] = 0.0, beta[t] = 0.0, pq[t] = 0.0;
    iters[t] = 0, bad[t] = 0;
    frozen[t] = (s == 0.0) ? 1 : 0;
    return;
  }
  const bool live = frozen[t] == 0;
  if (mode == CG_DOT_RHO0) {
    rho[t] = s;
  } else if (mode == CG_DOT_PQ) {
    pq[t] = s;
    if (!live) {
      a[t] = 0.0;
    } else if (s > 0.0 && s < INFINITY) {
      a[t] = rho[t] / s;
    } else {
      a[t] = 0.0, bad[t] = 1, frozen[t] = 1;
    }
    if (hist) hist[(long)(2 * (it - 1)) * CG_MAX_T + t] = a[t];
  } else if (mode == CG_DOT_RR) {
    if (live) {
      rr[t] = s, iters[t] = it;
      if (sqrt(s) <= tol * sqrt(bn[t])) frozen[t] = 1;
    }
  } else {  // CG_DOT_BETA
    if (live) {
      beta[t] = s / rho[t];
      rho[t] = s;
    } else {
      beta[t] = 0.0;
    }
    if (hist) hist[(long)(2 * (it - 1) + 1) * CG_MAX_T + t] = beta[t];
  }
}

// status[0] = live columns, status[1] = first bad column + 1 (0: none); one wave
__global__ __launch_bounds__(64) void cg_status_kernel(int T, int *__restrict__ st) {
  const int t = threadIdx.x;
  const bool in = t < T;
  const unsigned long long live = __ballot(in && st[CG_ST_FROZEN * CG_MAX_T + t] == 0);
  const unsigned long long bad = __ballot(in && st[CG_ST_BAD * CG_MAX_T + t] != 0);
  if (t == 0) {
    st[CG_ST_STATUS * CG_MAX_T + 0] = __popcll(live);
    st[CG_ST_STATUS * CG_MAX_T + 1] = bad ? __builtin_ctzll(bad) + 1 : 0;
  }
}

// ---- the fused vector updates --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cg_update_xr_kernel(double *__restrict__ x, double *__restrict__ r,
                                                           const double *__restrict__ p, const double *__restrict__ q,
                                                           long ld, long n, const double *__restrict__ sc,
                                                           const int *__restrict__ st) {
  const int t = blockIdx.y;
  if (st[CG_ST_FROZEN * CG_MAX_T + t]) return;  // (uniform) a frozen column keeps its bits
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double a = sc[CG_SC_A * CG_MAX_T + t];
  const long e = (long)t * ld + i;
  x[e] += a * p[e];
  r[e] -= a * q[e];
}

__global__ __launch_bounds__(256) void cg_update_p_kernel(double *__restrict__ p, const double *__restrict__ z, long ld,
                                                          long n, const double *__restrict__ sc,
                                                          const int *__restrict__ st) {
  const int t = blockIdx.y;
  if (st[CG_ST_FROZEN * CG_MAX_T + t]) return;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double beta = sc[CG_SC_BETA * CG_MAX_T + t];
  const long e = (long)t * ld + i;
  p[e] = z[e] + beta * p[e];
}

__global__ __launch_bounds__(256) void cg_scale_kernel(const double *__restrict__ in, const double *__restrict__ w,
                                                       const double *__restrict__ sub, long ld, long n,
                                                       double *__restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long e = (long)blockIdx.y * ld + i;
  double v = in[e];
  if (w) v *= w[i];
  if (sub) v -= sub[e];
  out[e] = v;
}

// ---- the preconditioner ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cg_diag_kernel(const DevParams *__restrict__ Pp, const double *__restrict__ v, long n,
                                                      long npad, double *__restrict__ d, double *__restrict__ dis) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= npad) return;
  if (i < n) {
    const double di = Pp->noise_var + (v ? v[i] : 0.0);
    d[i] = di;
    dis[i] = 1.0 / sqrt(di);
  } else {
    d[i] = 0.0, dis[i] = 0.0;
  }
}

__global__ __launch_bounds__(256) void cg_scale_factor_kernel(double *__restrict__ Lt, long ldn, long n,
                                                              const double *__restrict__ dis) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) Lt[(long)blockIdx.y * ldn + i] *= dis[i];
}

// One workgroup per 16 x 16 tile (bi >= bj) of C = I + Ls^T Ls: wave w sums the rows i = 16 q + 4 w' .. of its share in
// order on the matrix cores, the four waves' sums are added in wave order; both triangles are written.
__global__ __launch_bounds__(256, 2) void cg_capacitance_kernel(const double *__restrict__ Ls, long ldn, long n, int r, int rp,
                                                             double *__restrict__ C) {
  __shared__ double red[4][256];
  int bi = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
  while (bi * (bi + 1) / 2 > (int)blockIdx.x) --bi;
  while ((bi + 1) * (bi + 2) / 2 <= (int)blockIdx.x) ++bi;
  const int bj = blockIdx.x - bi * (bi + 1) / 2;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const int ka = 16 * bi + fr, kb = 16 * bj + fr;
  const double *ca = Ls + (long)ka * ldn, *cb = Ls + (long)kb * ldn;
  cg_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  for (long i0 = 4 * w; i0 < n; i0 += 16) {
    const long i = i0 + fk;
    const bool in = i < n;
    const double a = (in && ka < r) ? ca[i] : 0.0, b = (in && kb < r) ? cb[i] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) red[w][(fk + 4 * v) * 16 + fr] = acc[v];  // [row of tile bi][column of tile bj]
  __syncthreads();
  const int rr = tid >> 4, cc = tid & 15;
  const int k1 = 16 * bi + rr, k2 = 16 * bj + cc;
  double s = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
  if (k1 == k2) s += 1.0;
  C[(long)k1 * rp + k2] = s;
  C[(long)k2 * rp + k1] = s;
}

// part[slab][t][k] = sum over the slab's rows i of Ls[i][k] dis_i R[t][i]: one workgroup per (16 columns k, 16 right-hand
// sides, slab); wave w takes the steps i = i_begin + 16 q + 4 w of the slab, the waves are added in wave order
__global__ __launch_bounds__(256, 2) void cg_lst_kernel(const double *__restrict__ Ls, long ldn, long n, int r, int rp,
                                                     const double *__restrict__ dis, const double *__restrict__ R, long ld,
                                                     int T, long rows_per_slab, double *__restrict__ part) {
  __shared__ double red[4][256];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const int k = 16 * blockIdx.x + fr, t = 16 * blockIdx.y + fr;
  const int T16 = 16 * gridDim.y;
  const long ib = (long)blockIdx.z * rows_per_slab, ie = std::min<long>(n, ib + rows_per_slab);
  const double *ca = Ls + (long)k * ldn, *rb = R + (long)t * ld;
  cg_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  for (long i0 = ib + 4 * w; i0 < ie; i0 += 16) {
    const long i = i0 + fk;
    const bool in = i < ie;
    const double a = (in && k < r) ? ca[i] : 0.0, b = (in && t < T) ? rb[i] * dis[i] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) red[w][(fk + 4 * v) * 16 + fr] = acc[v];  // [k of the tile][t of the tile]
  __syncthreads();
  const int kk = tid >> 4, tt = tid & 15;
  const double s = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
  part[((long)blockIdx.z * T16 + 16 * blockIdx.y + tt) * rp + 16 * blockIdx.x + kk] = s;
}

__global__ __launch_bounds__(256) void cg_lst_finish_kernel(const double *__restrict__ part, int nslab, int T16, int rp,
                                                            double *__restrict__ W) {
  const int k = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
  if (k >= rp) return;
  double s = 0.0;
  for (int q = 0; q < nslab; ++q) s += part[((long)q * T16 + t) * rp + k];
  W[(long)t * rp + k] = s;
}

// Y[t][k] = sum_{k' < r} Cinv[k][k'] W[t][k'] in index order
__global__ __launch_bounds__(256) void cg_small_mm_kernel(const double *__restrict__ Cinv, int r, int rp,
                                                          const double *__restrict__ W, double *__restrict__ Y) {
  const int k = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
  if (k >= rp) return;
  double s = 0.0;
  if (k < r) {
    const double *c = Cinv + (long)k * rp, *wv = W + (long)t * rp;
    for (int q = 0; q < r; ++q) s += c[q] * wv[q];
  }
  Y[(long)t * rp + k] = s;
}

// Z[t][i] = dis_i (dis_i R[t][i] - sum_{k < r} Ls[i][k] Y[t][k]) for the four right-hand sides 4 blockIdx.y ..
__global__ __launch_bounds__(256) void cg_precond_kernel(const double *__restrict__ Ls, long ldn, long n, int r, int rp,
                                                         const double *__restrict__ dis, const double *__restrict__ R,
                                                         const double *__restrict__ Y, long ld, int T,
                                                         double *__restrict__ Z) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int t0 = 4 * blockIdx.y;
  // the rows of Y of right-hand sides beyond T are never read: their index is clamped and their sum dropped
  const double *y0 = Y + (long)t0 * rp, *y1 = Y + (long)std::min(t0 + 1, T - 1) * rp;
  const double *y2 = Y + (long)std::min(t0 + 2, T - 1) * rp, *y3 = Y + (long)std::min(t0 + 3, T - 1) * rp;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  const double *col = Ls + i;
  for (int k = 0; k < r; ++k, col += ldn) {
    const double l = col[0];
    s0 += l * y0[k], s1 += l * y1[k], s2 += l * y2[k], s3 += l * y3[k];
  }
  const double di = dis[i];
  const double sv[4] = {s0, s1, s2, s3};
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (t0 + u < T) {
      const long e = (long)(t0 + u) * ld + i;
      Z[e] = di * (di * R[e] - sv[u]);
    }
}

// ---- the LML's gradient: probes and the pair reduction ---------------------------------------------------------------------------
// Z[t][i] = sqrt(d_i) (sum_{k < r} Ls[i][k] Xi[t][n + k] + Xi[t][i]) ~ N(0, L L^T + D) for standard normal Xi: the four
// right-hand sides 4 blockIdx.y .. per pass over the row of Ls, as cg_precond_kernel takes them
__global__ __launch_bounds__(256) void cg_probe_kernel(const double *__restrict__ Ls, long ldn, long n, int r,
                                                       const double *__restrict__ d, const double *__restrict__ Xi, long ldxi,
                                                       long ld, int T, double *__restrict__ Z) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int t0 = 4 * blockIdx.y;
  // rows of Xi beyond T are never read: their index is clamped and their sum dropped
  const double *x0 = Xi + (long)t0 * ldxi, *x1 = Xi + (long)std::min(t0 + 1, T - 1) * ldxi;
  const double *x2 = Xi + (long)std::min(t0 + 2, T - 1) * ldxi, *x3 = Xi + (long)std::min(t0 + 3, T - 1) * ldxi;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  const double *col = Ls + i;
  for (int k = 0; k < r; ++k, col += ldn) {
    const double l = col[0];
    s0 += l * x0[n + k], s1 += l * x1[n + k], s2 += l * x2[n + k], s3 += l * x3[n + k];
  }
  const double sd = sqrt(d[i]);
  const double sv[4] = {s0 + x0[i], s1 + x1[i], s2 + x2[i], s3 + x3[i]};
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (t0 + u < T) Z[(long)(t0 + u) * ld + i] = sd * sv[u];
}

// partials[b][slot] = sum over the 64 x 64 tiles (row tile ti, column tile tj; t = ti ntc + tj) b * per .. of workgroup b of
//     (scale sum_{s < S} A[s][i] B[s][j]) theta_p dk(x_i, x_j)/dtheta_p,        i, j < n,
// in the slot layout of grad.hip (common.h: ACC_*; the trace slot takes the weights of the pairs i == j).  The mirror image
// of kmm_kernel: there a lane evaluates the kernel and the matrix cores multiply, here the matrix cores form the weights
// and the lanes evaluate the derivative.  Wave w takes the rows 16 w .. 16 w + 15 of the tile and its four 16 x 16
// sub-tiles c in turn: ceil(S / 4) v_mfma_f64_16x16x4_f64 (A operand scale A[4 k + fk][i_fr], B operand B[4 k + fk][j_fr],
// both from LDS, the A tile staged once per row tile; rows s >= S and elements >= n are exact zeros and never read)
// leave the weights of the pairs (row fk + 4 v, column fr), v < 4, in the lane's C fragment, which go through
// simil_grad_accum in the order c, v.  A lane's order of pairs and the block's tree depend on n alone, never on S.
// Dynamic LDS: Xa[64][DS], Xb[64][DS] (DS = ndim | 1), As[S4][64], Bs[S4][64] (S4 = S rounded up to 4; element (s, j) at
// column j ^ 16 (s & 1): the rows fk, fk + 1 that half a wave reads lie in different banks), red[4][NACC].
// ARD dimensions ard0 .. ard0 + ARD_D - 1 per pass, the pass with ard0 == 0 writing every slot and a later one only its own
// (sparse_grad_kernel).  Tiles are counted in 32 bits: n < 2^21.
constexpr int CG_GRAD_BLOCKS_MAX = 2048;

template <int ARD_D>
__global__ __launch_bounds__(256, 2) void cg_grad_kernel(const DevParams *__restrict__ Pp, const double *__restrict__ X,
                                                         int n, const double *__restrict__ A,
                                                         const double *__restrict__ B, long ld, int S, double scale,
                                                         int ntc, int ntiles, int per, double *__restrict__ partials,
                                                         int ard0) {
  extern __shared__ double sm[];
  const DevParams &P = *Pp;
  const int D = P.ndim;
  const int DS = D | 1;
  const int nsteps = (S + 3) >> 2;
  double *Xa = sm, *Xb = sm + 64 * DS, *As = Xb + 64 * DS;
  double *Bs = As + 4 * nsteps * 64;
  double *red = Bs + 4 * nsteps * 64;  // [4][NACC]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;

  double acc[ACC_TRACE + 1];
#pragma unroll
  for (int q = 0; q <= ACC_TRACE; ++q) acc[q] = 0.0;
  double ard[ARD_D > 0 ? ARD_D : 1];
#pragma unroll
  for (int q = 0; q < (ARD_D > 0 ? ARD_D : 1); ++q) ard[q] = 0.0;

  const int tb = blockIdx.x * per, te = min(ntiles, tb + per);
  int have_ti = -1;
  for (int t = tb; t < te; ++t) {
    const int ti = t / ntc, tj = t - ti * ntc;
    const int r0 = ti * 64, c0 = tj * 64;
    __syncthreads();  // the previous tile's readers are done
    if (ti != have_ti) {  // (uniform)
      have_ti = ti;
      for (int idx = tid; idx < 64 * D; idx += 256) {
        const int r = idx / D, d = idx - r * D;
        Xa[r * DS + d] = (r0 + r < n) ? X[(long)(r0 + r) * D + d] : 0.0;
      }
      for (int idx = tid; idx < 4 * nsteps * 64; idx += 256) {
        const int s = idx >> 6, j = idx & 63;
        As[s * 64 + (j ^ ((s & 1) << 4))] = (s < S && r0 + j < n) ? scale * A[(long)s * ld + r0 + j] : 0.0;
      }
    }
    for (int idx = tid; idx < 64 * D; idx += 256) {
      const int r = idx / D, d = idx - r * D;
      Xb[r * DS + d] = (c0 + r < n) ? X[(long)(c0 + r) * D + d] : 0.0;
    }
    for (int idx = tid; idx < 4 * nsteps * 64; idx += 256) {
      const int s = idx >> 6, j = idx & 63;
      Bs[s * 64 + (j ^ ((s & 1) << 4))] = (s < S && c0 + j < n) ? B[(long)s * ld + c0 + j] : 0.0;
    }
    __syncthreads();
    const double *ap = As + fk * 64 + ((16 * w + fr) ^ ((fk & 1) << 4));
    for (int c = 0; c < 4; ++c) {
      cg_f64x4 wt = {0.0, 0.0, 0.0, 0.0};
      const double *bp = Bs + fk * 64 + ((16 * c + fr) ^ ((fk & 1) << 4));
      for (int k = 0; k < nsteps; ++k) wt = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[k * 256], bp[k * 256], wt, 0, 0, 0);
      // C fragment: column = lane & 15, row = (lane >> 4) + 4 v
      const int gj = c0 + 16 * c + fr;
      const double *xb = Xb + (16 * c + fr) * DS;
      // (one copy of the derivative's code: four inlined ones are over the audit's limit of SGPR spills)
#pragma nounroll
      for (int v = 0; v < 4; ++v) {
        const int r = 16 * w + fk + 4 * v;
        const int gi = r0 + r;
        if (gi < n && gj < n) {
          const double wgt = v == 0 ? wt[0] : v == 1 ? wt[1] : v == 2 ? wt[2] : wt[3];
          const double *xa = Xa + r * DS;
          simil_grad_accum<ARD_D>(
              P, [&](int d) { return xa[d]; }, [&](int d) { return xb[d]; }, wgt, acc, ard, ard0);
          if (gi == gj) acc[ACC_TRACE] += wgt;
        }
      }
    }
  }

  // ---- block reduction: wave shuffles, then 4 waves through LDS (sparse_grad_kernel) -------------
  __syncthreads();
#pragma unroll
  for (int q = 0; q <= ACC_TRACE; ++q) {
    double v = acc[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) red[w * NACC + q] = v;
  }
  if (ARD_D > 0) {
#pragma unroll
    for (int q = 0; q < (ARD_D > 0 ? ARD_D : 1); ++q) {
      double v = ard[q];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
      if (lane == 0) red[w * NACC + ACC_ARD0 + q] = v;
    }
  }
  __syncthreads();
  if (tid < NACC) {
    const bool base = tid <= ACC_TRACE, mine = tid >= ACC_ARD0 && tid < ACC_ARD0 + ARD_D;
    double v = 0.0;
    if (base || mine) v = red[tid] + red[NACC + tid] + red[2 * NACC + tid] + red[3 * NACC + tid];
    if (ard0 == 0) partials[(long)blockIdx.x * NACC + tid] = v;
    else if (mine && tid + ard0 < NACC) partials[(long)blockIdx.x * NACC + tid + ard0] = v;
  }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
// Slabs of column tiles: about 2048 work items where the row tiles alone do not give them; a function of the sizes only
int kmm_slabs(int64_t rows, int64_t cols) {
  const int64_t rt = std::max<int64_t>(1, (rows + 63) / 64), ct = std::max<int64_t>(1, (cols + 63) / 64);
  const int64_t want = (2048 + rt - 1) / rt;
  return (int)std::max<int64_t>(1, std::min<int64_t>({want, ct, (int64_t)KMM_SLABS_MAX}));
}

constexpr size_t KMM_LDS_CAP = (size_t)(2 * 64 * (GOGP_MAX_NDIM | 1) + 64 * 65) * sizeof(double);

void launch_kmm(hipStream_t s, const DevParams *p, int ndim, const double *A, int64_t rows, const double *B, int64_t cols,
                const double *V, int64_t ldv, int T, const double *diag, int nslab, int max_blocks, double *part,
                double *Out, int64_t ldo) {
  const long rt = (long)((rows + 63) / 64), ct = (long)((cols + 63) / 64);
  const long rpad = rt * 64;
  const int tps = (int)((ct + nslab - 1) / nslab);
  const long nitems = rt * nslab;
  long grid = std::min<long>(nitems, 1L << 20);
  if (max_blocks > 0) grid = std::min<long>(grid, max_blocks);
  const int ng = (T + 15) / 16;
  const size_t lds = (size_t)(2 * 64 * (ndim | 1) + 64 * (16 * ng + 1)) * sizeof(double);
  // more than 64 KB (from 29 dimensions on with 64 right-hand sides) is said to the runtime before the launch (gram.hip)
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&kmm_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)KMM_LDS_CAP);
  GOGP_KLAUNCH(kmm_kernel, dim3((unsigned)grid), dim3(256), lds, s, p, A, (long)rows, B, (long)cols, V, (long)ldv, T, diag,
               nslab, tps, nitems, rpad, part);
  GOGP_KLAUNCH(kmm_finish_kernel, dim3((unsigned)((ldo + 255) / 256), (unsigned)T), dim3(256), 0, s,
               (const double *)part, nslab, T, rpad, (long)rows, Out, (long)ldo);
}

int cg_dot_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 2047) / 2048, 512)); }

void launch_cg_dots(hipStream_t s, const double *A, const double *B, int64_t ld, int64_t n, int T, int mode, int it,
                    double tol, double *part, double *out, CgState cs, double *hist) {
  const int nb = cg_dot_blocks(n);
  GOGP_KLAUNCH(cg_dots_kernel, dim3((unsigned)nb, (unsigned)T), dim3(256), 0, s, A, B, (long)ld, (long)n, part);
  GOGP_KLAUNCH(cg_dots_final_kernel, dim3((unsigned)T), dim3(256), 0, s, (const double *)part, nb, mode, it, tol, out, cs.sc,
               cs.st, hist);
}

void launch_cg_update_xr(hipStream_t s, double *x, double *r, const double *p, const double *q, int64_t ld, int64_t n, int T,
                         CgState cs) {
  GOGP_KLAUNCH(cg_update_xr_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)T), dim3(256), 0, s, x, r, p, q, (long)ld,
               (long)n, (const double *)cs.sc, (const int *)cs.st);
}

void launch_cg_update_p(hipStream_t s, double *p, const double *z, int64_t ld, int64_t n, int T, CgState cs) {
  GOGP_KLAUNCH(cg_update_p_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)T), dim3(256), 0, s, p, z, (long)ld, (long)n,
               (const double *)cs.sc, (const int *)cs.st);
}

void launch_cg_scale(hipStream_t s, const double *in, const double *w, const double *sub, int64_t ld, int64_t n, int T,
                     double *out) {
  GOGP_KLAUNCH(cg_scale_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)T), dim3(256), 0, s, in, w, sub, (long)ld,
               (long)n, out);
}

void launch_cg_status(hipStream_t s, int T, CgState cs) {
  GOGP_KLAUNCH(cg_status_kernel, dim3(1), dim3(64), 0, s, T, cs.st);
}

void launch_cg_diag(hipStream_t s, const DevParams *p, const double *v, int64_t n, int64_t npad, double *d, double *dis) {
  GOGP_KLAUNCH(cg_diag_kernel, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, s, p, v, (long)n, (long)npad, d, dis);
}

void launch_cg_scale_factor(hipStream_t s, double *Lt, int64_t ldn, int64_t n, int r, const double *dis) {
  if (r < 1) return;
  GOGP_KLAUNCH(cg_scale_factor_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)r), dim3(256), 0, s, Lt, (long)ldn,
               (long)n, dis);
}

void launch_cg_capacitance(hipStream_t s, const double *Ls, int64_t ldn, int64_t n, int r, int rp, double *C) {
  const int nt = rp / 16;
  GOGP_KLAUNCH(cg_capacitance_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, s, Ls, (long)ldn, (long)n, r, rp,
               C);
}

// slabs of rows of the skinny transposed product: 4096 rows each, 256 at most; a function of n only
int cg_lst_slabs(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 4095) / 4096, 256)); }

void launch_cg_lst(hipStream_t s, const double *Ls, int64_t ldn, int64_t n, int r, int rp, const double *dis,
                   const double *R, int64_t ld, int T, double *part, double *W) {
  const int nslab = cg_lst_slabs(n);
  const long rps = (((long)n + nslab - 1) / nslab + 15) / 16 * 16;
  const int tg = (T + 15) / 16;
  GOGP_KLAUNCH(cg_lst_kernel, dim3((unsigned)(rp / 16), (unsigned)tg, (unsigned)nslab), dim3(256), 0, s, Ls, (long)ldn,
               (long)n, r, rp, dis, R, (long)ld, T, rps, part);
  GOGP_KLAUNCH(cg_lst_finish_kernel, dim3((unsigned)((rp + 255) / 256), (unsigned)T), dim3(256), 0, s, (const double *)part,
               nslab, 16 * tg, rp, W);
}

void launch_cg_small_mm(hipStream_t s, const double *Cinv, int r, int rp, const double *W, int T, double *Y) {
  GOGP_KLAUNCH(cg_small_mm_kernel, dim3((unsigned)((rp + 255) / 256), (unsigned)T), dim3(256), 0, s, Cinv, r, rp, W, Y);
}

void launch_cg_precond(hipStream_t s, const double *Ls, int64_t ldn, int64_t n, int r, int rp, const double *dis,
                       const double *R, const double *Y, int64_t ld, int T, double *Z) {
  GOGP_KLAUNCH(cg_precond_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)((T + 3) / 4)), dim3(256), 0, s, Ls,
               (long)ldn, (long)n, r, rp, dis, R, Y, (long)ld, T, Z);
}

void launch_cg_probes(hipStream_t s, const double *Ls, int64_t ldn, int64_t n, int r, const double *d, const double *Xi,
                      int64_t ldxi, int64_t ld, int T, double *Z) {
  GOGP_KLAUNCH(cg_probe_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)((T + 3) / 4)), dim3(256), 0, s, Ls, (long)ldn,
               (long)n, r, d, Xi, (long)ldxi, (long)ld, T, Z);
}

// workgroups of the pair reduction: one per 64 x 64 tile up to CG_GRAD_BLOCKS_MAX, then runs of consecutive tiles; a function
// of n only
int cg_grad_blocks(int64_t n) {
  const int64_t rt = std::max<int64_t>(1, (n + 63) / 64);
  return (int)std::min<int64_t>(rt * rt, CG_GRAD_BLOCKS_MAX);
}

template <int AD>
static void cgg_launch(int blocks, hipStream_t s, int ndim, const DevParams *p, const double *X, int n, const double *A,
                       const double *B, long ld, int S, double scale, int ntc, int ntiles, int per, double *partials,
                       int ard0) {
  const int ds = ndim | 1;
  const size_t lds = (size_t)(128 * ds + (S + 3) / 4 * 4 * 128 + 4 * NACC) * sizeof(double);
  if (lds > 64 * 1024)  // raised explicitly, per launch (the attribute belongs to the function on the current device)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&cg_grad_kernel<AD>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)((128 * (GOGP_MAX_NDIM | 1) + CG_MAX_T * 128 + 4 * NACC) * sizeof(double)));
  GOGP_KLAUNCH(cg_grad_kernel<AD>, dim3((unsigned)blocks), dim3(256), lds, s, p, X, n, A, B, ld, S, scale, ntc, ntiles, per,
               partials, ard0);
}

void launch_cg_grad(hipStream_t s, const DevParams *p, int ndim, int ard_dims, const double *X, int64_t n, const double *A,
                    const double *B, int64_t ld, int S, double scale, double *partials, double *out, bool accumulate) {
  if (n <= 0 || n >= (1 << 21) || S <= 0) return;  // (tiles are counted in 32 bits; the callers refuse such an n)
  const int ntc = (int)((n + 63) / 64), ntiles = ntc * ntc;
  const int blocks = cg_grad_blocks(n);
  const int per = (ntiles + blocks - 1) / blocks;
  // the rows in passes of CG_MAX_T, each summed behind the one before it; ARD dimensions in passes of 8 accumulators
  // (launch_sparse_grad: the 16-accumulator instance is over the audit's limit of SGPR spills)
  for (int s0 = 0; s0 < S; s0 += CG_MAX_T) {
    const int cnt = std::min(CG_MAX_T, S - s0);
    const double *a = A + (long)s0 * ld, *b = B + (long)s0 * ld;
    if (ard_dims <= 0)
      cgg_launch<0>(blocks, s, ndim, p, X, (int)n, a, b, (long)ld, cnt, scale, ntc, ntiles, per, partials, 0);
    else
      for (int a0 = 0; a0 < ard_dims; a0 += 8)
        cgg_launch<8>(blocks, s, ndim, p, X, (int)n, a, b, (long)ld, cnt, scale, ntc, ntiles, per, partials, a0);
    launch_sparse_grad_final(s, partials, blocks, out, accumulate || s0 > 0);
  }
}

// rho0 e_1^T log(T) e_1 = rho0 sum_j tau_j^2 log lambda_j of the symmetric tridiagonal T_kk = 1 / a_k + beta_{k-1} / a_{k-1},
// T_{k,k+1} = sqrt(beta_k) / a_k (k < m): the implicit QL sweep (EISPACK tql2), its rotations applied to the first row of
// the eigenvector matrix alone -- O(m^2).  m < 1: 0.  NaN where T is not positive definite or the sweep does not settle.
double cg_lanczos_quadrature(const double *a, const double *beta, int64_t stride, int m, double rho0) {
  if (m < 1) return 0.0;
  std::vector<double> d((size_t)m), e((size_t)m, 0.0), z((size_t)m, 0.0);
  for (int k = 0; k < m; ++k) {
    const double ak = a[(int64_t)k * stride];
    d[k] = 1.0 / ak + (k > 0 ? beta[(int64_t)(k - 1) * stride] / a[(int64_t)(k - 1) * stride] : 0.0);
    if (k + 1 < m) e[k] = sqrt(beta[(int64_t)k * stride]) / ak;  // couples k and k + 1
  }
  z[0] = 1.0;
  for (int l = 0; l < m; ++l) {
    for (int iter = 0;; ++iter) {
      int mm = l;
      for (; mm < m - 1; ++mm) {
        const double dd = fabs(d[mm]) + fabs(d[mm + 1]);
        if (fabs(e[mm]) + dd == dd) break;
      }
      if (mm == l) break;
      if (iter == 120) return NAN;
      double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
      double r = hypot(g, 1.0);
      g = d[mm] - d[l] + e[l] / (g + copysign(r, g));
      double sn = 1.0, cs = 1.0, p = 0.0;
      int i = mm - 1;
      for (; i >= l; --i) {
        double f = sn * e[i];
        const double b = cs * e[i];
        r = hypot(f, g);
        e[i + 1] = r;
        if (r == 0.0) {
          d[i + 1] -= p;
          e[mm] = 0.0;
          break;
        }
        sn = f / r, cs = g / r;
        g = d[i + 1] - p;
        r = (d[i] - g) * sn + 2.0 * cs * b;
        p = sn * r;
        d[i + 1] = g + p;
        g = cs * r - b;
        f = z[i + 1];
        z[i + 1] = sn * z[i] + cs * f;
        z[i] = cs * z[i] - sn * f;
      }
      if (r == 0.0 && i >= l) continue;
      d[l] -= p;
      e[l] = g;
      e[mm] = 0.0;
    }
  }
  // (the sum runs in index order of the sweep's output: a function of the coefficients alone)
  double sum = 0.0;
  for (int k = 0; k < m; ++k) {
    if (!(d[k] > 0.0)) return NAN;
    sum += z[k] * z[k] * log(d[k]);
  }
  return rho0 * sum;
}

}  // namespace gogp
