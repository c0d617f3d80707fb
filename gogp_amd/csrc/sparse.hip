// sparse.hip -- the kernels of the inducing-point approximation (gogp_sparse_*; api.hip orchestrates).
//
// Collapsed variational bound of Titsias (2009) on M inducing points U for N observations (X, y):
//     Kuu + eps I = L L^T,   V = L^-1 k(U, X)  (M x N),   B = I + V V^T / s2,   r = V y,   g = B^-1 r,
//     F = -N/2 log 2 pi - 1/2 log|B| - N/2 log s2 - y^T y / (2 s2) + r^T g / (2 s2^2) - (t0 - s2 (tr B - M)) / (2 s2).
// The data goes through in chunks of rows; a chunk's V^T (rows x Mp, row-major) is what Produce's forward substitution
// leaves with the chunk's rows as test points.  Three kernels carry the O(N M^2) and O(N M) work:
//   sparse_syrk_kernel   B_acc (lower 64-tiles of Mp x Mp) += Vt^T Vt and r += Vt^T y_chunk on v_mfma_f64_16x16x4_f64;
//   sparse_grad_kernel   sum over (observation f, inducing point u) of (Wt[f][u] + y_f m_u / s2^2) dk(x_f, u_u)/dlog theta
//                        into the NACC slot layout of common.h;
//   sparse_ugrad_kernel  the same pairs and weights on dk(u_u, x_f)/du_u: the (U, X) part of d bound / d U.
// The rest are the element-wise passes over the M x M matrices and the M vectors.
// Multi-output (gogp_sparse_multi_*: T columns Y on the same pass; DESIGN.md section 4, "Sparse multi-output") adds
//   sparse_xty_kernel    R^T (T x Mp) += Yc^T Vt on the same MFMA and LDS layout, K split into slabs added in order,
// and small kernels for T and S with Gamma Gamma^T, the per-output dots, the padded chunk of Y and Produce's sigma.
//
// Every sum has a fixed order (no atomics): two identical calls give the same bits.
#include <algorithm>

#include "kern_eval.h"

namespace gogp {

typedef double sp_f64x4 __attribute__((ext_vector_type(4)));
// Rows of Vt per pass through LDS and the stride of one of them there: the layout of multi.hip's multi_weight_kernel,
// whose operand is k-major too -- a slice is kept as it lies in memory, one row of Vt (64 inducing points) per LDS row;
// a fragment read takes 16 consecutive columns of 4 consecutive rows, and with 80 doubles per row the rows k and k + 1
// start half the banks apart; the writes run along a row.
constexpr int SS_KC = 32, SS_S = 80;

__device__ __forceinline__ void sparse_lower_tile(int t, int &ti, int &tj) {
  ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (ti * (ti + 1) / 2 > t) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  tj = t - ti * (ti + 1) / 2;
}

// Bacc (ldb doubles per row) += Vt^T Vt on the whole 64 x 64 tiles (ti, tj), tj <= ti, one workgroup per tile, and -- the
// workgroups of the diagonal tiles -- r[j] += sum_k Vt[k][j] y[k].  Vt: `rows` rows of ld doubles; rows >= `rows` are never read, columns >= M are read and replaced by exact zeros, so whatever the
// padding holds the padded elements of Bacc and r receive += 0.  k runs in row order, in passes of SS_KC rows through
// LDS; wave w owns rows 16 w .. 16 w + 15 of the tile: one A fragment and four B fragments per 4 k
// (A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][column = lane & 15]).  (__launch_bounds__(256, 2), as
// multi_weight_kernel: the accumulators stay in architectural VGPRs.)
__global__ __launch_bounds__(256, 2) void sparse_syrk_kernel(const double *__restrict__ Vt, long ld, long rows, long M,
                                                             const double *__restrict__ y, double *__restrict__ Bacc,
                                                             long ldb, double *__restrict__ r) {
  __shared__ double As[SS_KC * SS_S], Bs[SS_KC * SS_S], ys[SS_KC];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int ti, tj;
  sparse_lower_tile((int)blockIdx.x, ti, tj);
  const bool diag = ti == tj;
  const long r0 = (long)ti * 64, c0 = (long)tj * 64;
  const int fr = lane & 15, fk = lane >> 4;
  const double *Bsrc = diag ? As : Bs;
  const bool alive = r0 + lane < M, blive = c0 + lane < M;
  sp_f64x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = (sp_f64x4){0.0, 0.0, 0.0, 0.0};
  double racc = 0.0;
  for (long k0 = 0; k0 < rows; k0 += SS_KC) {
    if (k0 > 0) __syncthreads();  // the previous pass's readers are done
#pragma unroll
    for (int rr = 0; rr < SS_KC / 4; ++rr) {
      const int k = w + 4 * rr;
      const bool klive = k0 + k < rows;
      const double *row = Vt + (k0 + k) * ld;
      As[k * SS_S + lane] = (klive && alive) ? row[r0 + lane] : 0.0;
      if (!diag) Bs[k * SS_S + lane] = (klive && blive) ? row[c0 + lane] : 0.0;
    }
    if (diag && tid < SS_KC) ys[tid] = (k0 + tid < rows) ? y[k0 + tid] : 0.0;
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < SS_KC; kk += 4) {
      const double a = As[(kk + fk) * SS_S + 16 * w + fr];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bsrc[(kk + fk) * SS_S + 16 * t + fr], acc[t], 0, 0, 0);
    }
    if (diag && w == 0) {
      for (int k = 0; k < SS_KC; ++k) racc += As[k * SS_S + lane] * ys[k];
    }
  }
  // C fragment: column = lane & 15, row = (lane >> 4) + 4 v
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const long gi = r0 + 16 * w + fk + 4 * v;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const long gj = c0 + 16 * t + fr;
      Bacc[gi * ldb + gj] += acc[t][v];
    }
  }
  if (diag && w == 0) r[r0 + lane] += racc;
}

void launch_sparse_syrk(hipStream_t s, const double *Vt, int64_t ld, int64_t rows, int64_t M, int64_t Mp, const double *y,
                        double *Bacc, int64_t ldb, double *r) {
  if (rows <= 0) return;
  const int nt = (int)(Mp / 64);
  GOGP_KLAUNCH(sparse_syrk_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, s, Vt, (long)ld, (long)rows, (long)M,
               y, Bacc, (long)ldb, r);
}

// ---- multi-output: R^T (+)= Yc^T Vt ---------------------------------------------------------------------------------------
// part[slab] (ldp doubles per row) = Yc^T Vt over the rows of the slab, on the 64 x 64 tile (output tile blockIdx.y,
// inducing tile blockIdx.x): part[slab][t][j] = sum_k Yc[k][t] Vt[k][j], k in [slab * rps, min(rows, (slab + 1) * rps)).
// Vt as sparse_syrk_kernel takes it, Yc: rows x T with ldy doubles per row; both k-major, so both slices are kept as they
// lie in memory (sparse_syrk_kernel's LDS layout and fragment maps; the A operand is the slice of Yc, so the C fragment's
// consecutive columns are consecutive inducing points and the stores run along a row of R^T).  Rows >= `rows` are never
// read; columns >= M of Vt and >= T of Yc are replaced by exact zeros on the way into LDS, so the padded elements of
// the tile receive exact zeros.  rps is a multiple of SS_KC.  Every element of the tile is written: the partials need no
// clearing, and sparse_xty_final_kernel adds the slabs in index order.
__global__ __launch_bounds__(256, 2) void sparse_xty_kernel(const double *__restrict__ Vt, long ld, long rows, long M,
                                                            const double *__restrict__ Y, long ldy, long T, long rps,
                                                            double *__restrict__ part, long ldp, long slab_stride) {
  __shared__ double As[SS_KC * SS_S], Bs[SS_KC * SS_S];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long c0 = (long)blockIdx.x * 64, t0 = (long)blockIdx.y * 64;
  const long kb = (long)blockIdx.z * rps, ke = kb + rps < rows ? kb + rps : rows;
  const int fr = lane & 15, fk = lane >> 4;
  const bool alive = t0 + lane < T, blive = c0 + lane < M;
  sp_f64x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = (sp_f64x4){0.0, 0.0, 0.0, 0.0};
  for (long k0 = kb; k0 < ke; k0 += SS_KC) {
    if (k0 > kb) __syncthreads();  // the previous pass's readers are done
#pragma unroll
    for (int rr = 0; rr < SS_KC / 4; ++rr) {
      const int k = w + 4 * rr;
      const bool klive = k0 + k < ke;
      As[k * SS_S + lane] = (klive && alive) ? Y[(k0 + k) * ldy + t0 + lane] : 0.0;
      Bs[k * SS_S + lane] = (klive && blive) ? Vt[(k0 + k) * ld + c0 + lane] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < SS_KC; kk += 4) {
      const double a = As[(kk + fk) * SS_S + 16 * w + fr];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs[(kk + fk) * SS_S + 16 * t + fr], acc[t], 0, 0, 0);
    }
  }
  // C fragment: column = lane & 15, row = (lane >> 4) + 4 v
  double *out = part + (long)blockIdx.z * slab_stride;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const long gi = t0 + 16 * w + fk + 4 * v;
#pragma unroll
    for (int t = 0; t < 4; ++t) out[gi * ldp + c0 + 16 * t + fr] = acc[t][v];
  }
}

// Rt[t][j] += the slabs' sums in index order, t < tt, j < mc
__global__ __launch_bounds__(256) void sparse_xty_final_kernel(const double *__restrict__ part, int nslab, long slab_stride,
                                                               long ldp, long tt, long mc, double *__restrict__ Rt,
                                                               long ldr) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
  if (j >= mc || t >= tt) return;
  double v = 0.0;
  for (int sl = 0; sl < nslab; ++sl) v += part[(long)sl * slab_stride + t * ldp + j];
  Rt[t * ldr + j] += v;
}

// The slabs of launch_sparse_xty and the rows of one (*rps_out, a multiple of SS_KC): a function of (rows, M, T) alone.
// The grid (tiles x slabs) stays near SX_BLOCKS workgroups, two per CU's SIMD pair, and a slab has SX_ROWS_MIN rows at
// least, so that a workgroup's epilogue stays small beside its k loop.
constexpr int SX_BLOCKS = 1024, SX_ROWS_MIN = 256;
static int64_t sx_most(int64_t M, int64_t T) {
  const int64_t tiles = std::max<int64_t>(1, ((M + 63) / 64) * ((T + 63) / 64));
  return std::max<int64_t>(1, SX_BLOCKS / tiles);
}
int sparse_xty_slabs(int64_t rows, int64_t M, int64_t T, int64_t *rps_out) {
  const int64_t most = sx_most(M, T);
  const int64_t per = ((rows + most - 1) / most + SS_KC - 1) / SS_KC * SS_KC;
  const int64_t rps = std::max<int64_t>(SX_ROWS_MIN, per);
  if (rps_out) *rps_out = rps;
  return (int)std::max<int64_t>(1, (rows + rps - 1) / rps);
}
// An upper bound of sparse_xty_slabs(r, M, T) over every r <= rows, monotone in the rows: a slab has SX_ROWS_MIN rows
// at least, so the count is at most ceil(r / SX_ROWS_MIN); with rps == SX_ROWS_MIN, r <= SX_ROWS_MIN * most, so that is
// within `most`, and with rps >= ceil(r / most) the count ceil(r / rps) is within `most` too.
int sparse_xty_slabs_bound(int64_t rows, int64_t M, int64_t T) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((rows + SX_ROWS_MIN - 1) / SX_ROWS_MIN, sx_most(M, T)));
}
// doubles of the partials of one launch of up to `rows` rows
size_t sparse_xty_part_doubles(int64_t rows, int64_t M, int64_t T) {
  return (size_t)sparse_xty_slabs_bound(rows, M, T) * (size_t)((T + 63) / 64 * 64) * (size_t)((M + 63) / 64 * 64);
}

void launch_sparse_xty(hipStream_t s, const double *Vt, int64_t ld, int64_t rows, int64_t M, const double *Y, int64_t ldy,
                       int64_t T, double *part, double *Rt, int64_t ldr) {
  if (rows <= 0 || M <= 0 || T <= 0) return;
  int64_t rps = 0;
  const int nslab = sparse_xty_slabs(rows, M, T, &rps);
  const long mc = (long)((M + 63) / 64 * 64), tt = (long)((T + 63) / 64 * 64);
  GOGP_KLAUNCH(sparse_xty_kernel, dim3((unsigned)(mc / 64), (unsigned)(tt / 64), (unsigned)nslab), dim3(256), 0, s, Vt,
               (long)ld, (long)rows, (long)M, Y, (long)ldy, (long)T, (long)rps, part, mc, tt * mc);
  GOGP_KLAUNCH(sparse_xty_final_kernel, dim3((unsigned)((mc + 255) / 256), (unsigned)tt), dim3(256), 0, s, part, nslab,
               tt * mc, mc, tt, mc, Rt, (long)ldr);
}

// ---- the rectangular pair reduction ----------------------------------------------------------------------------------
// partials[b][slot] = sum over the 64 x 64 tiles (64 rows f of the chunk x 64 inducing points u) that workgroup b walks of
//     (Wt[f][u] + y_f m_u s4) theta_p dk(x_f, u_u)/dtheta_p,        f < rows, u < M,
// in the slot layout of grad.hip (common.h: ACC_*; the trace slot stays zero: a cross-covariance carries no noise).  The
// thread (tx, ty) takes inducing point tx of the tile and the rows 16 ty .. 16 ty + 15, as the generic instance of
// grad_reduce_kernel does, through simil_grad_accum; ARD dimensions ard0 .. ard0 + ARD_D - 1 per pass, the pass with
// ard0 == 0 writing every slot and a later one only its own.
template <int ARD_D>
__global__ __launch_bounds__(256) void sparse_grad_kernel(const DevParams *__restrict__ Pp, const double *__restrict__ X,
                                                          long rows, const double *__restrict__ U, long M,
                                                          const double *__restrict__ Wt, long ldw,
                                                          const double *__restrict__ y, const double *__restrict__ mvec,
                                                          double s4, int ntc, int ntiles, double *__restrict__ partials,
                                                          int ard0) {
  extern __shared__ double sm[];
  const DevParams &P = *Pp;
  const int D = P.ndim;
  double *Ri = sm;             // [64][D]
  double *CjT = sm + 64 * D;   // [D][64]
  double *yi = CjT + 64 * D;   // [64]
  double *mj = yi + 64;        // [64]
  double *red = mj + 64;       // [4][NACC]
  const int tid = threadIdx.x;
  const int tx = tid & 63, ty = tid >> 6;

  double acc[ACC_TRACE + 1];
#pragma unroll
  for (int q = 0; q <= ACC_TRACE; ++q) acc[q] = 0.0;
  double ard[ARD_D > 0 ? ARD_D : 1];
#pragma unroll
  for (int q = 0; q < (ARD_D > 0 ? ARD_D : 1); ++q) ard[q] = 0.0;

  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int ti = t / ntc, tj = t - ti * ntc;
    const long r0 = (long)ti * 64, c0 = (long)tj * 64;
    __syncthreads();  // previous tile's readers are done
    for (int idx = tid; idx < 64 * D; idx += 256) {
      const int r = idx / D, d = idx - r * D;
      Ri[idx] = (r0 + r < rows) ? X[(r0 + r) * D + d] : 0.0;
    }
    for (int idx = tid; idx < 64 * D; idx += 256) {
      const int d = idx >> 6, r = idx & 63;
      CjT[idx] = (c0 + r < M) ? U[(c0 + r) * D + d] : 0.0;
    }
    if (tid < 64) yi[tid] = (r0 + tid < rows) ? y[r0 + tid] : 0.0;
    else if (tid < 128) mj[tid - 64] = (c0 + tid - 64 < M) ? mvec[c0 + tid - 64] * s4 : 0.0;
    __syncthreads();
    const long gj = c0 + tx;
    const double *cj = CjT + tx;
    const double mjv = mj[tx];
    for (int rr = 0; rr < 16; ++rr) {
      const int r = ty * 16 + rr;
      const long gi = r0 + r;
      if (gi < rows && gj < M) {
        const double wgt = Wt[gi * ldw + gj] + yi[r] * mjv;
        const double *ri = Ri + r * D;
        simil_grad_accum<ARD_D>(
            P, [&](int d) { return ri[d]; }, [&](int d) { return cj[d * 64]; }, wgt, acc, ard, ard0);
      }
    }
  }

  // ---- block reduction: wave shuffles, then 4 waves through LDS (grad.hip) -------------
  __syncthreads();
  const int lane = tid & 63, wid = tid >> 6;
#pragma unroll
  for (int q = 0; q <= ACC_TRACE; ++q) {
    double v = acc[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) red[wid * NACC + q] = v;
  }
  if (ARD_D > 0) {
#pragma unroll
    for (int q = 0; q < (ARD_D > 0 ? ARD_D : 1); ++q) {
      double v = ard[q];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
      if (lane == 0) red[wid * NACC + ACC_ARD0 + q] = v;
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

// out[q] (+)= sum over blocks of partials[b][q] in index order per thread, then a fixed tree; one workgroup per slot
__global__ __launch_bounds__(256) void sparse_grad_final_kernel(const double *__restrict__ partials, int nblocks,
                                                                double *__restrict__ out, int accumulate) {
  __shared__ double red[4];
  const int q = blockIdx.x;
  double v = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 256) v += partials[(long)b * NACC + q];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double sum = red[0] + red[1] + red[2] + red[3];
    out[q] = accumulate ? out[q] + sum : sum;
  }
}

int sparse_grad_blocks(int64_t rows, int64_t M) {
  const long ntiles = (long)((rows + 63) / 64) * (long)((M + 63) / 64);
  return (int)(ntiles < SPARSE_GRAD_BLOCKS_MAX ? (ntiles > 0 ? ntiles : 1) : SPARSE_GRAD_BLOCKS_MAX);
}

void launch_sparse_grad_final(hipStream_t s, const double *partials, int blocks, double *out, bool accumulate) {
  GOGP_KLAUNCH(sparse_grad_final_kernel, dim3(NACC), dim3(256), 0, s, partials, blocks, out, accumulate ? 1 : 0);
}

template <int AD>
static void sg_launch(int blocks, hipStream_t s, int ndim, const DevParams *p, const double *X, long rows, const double *U,
                      long M, const double *Wt, long ldw, const double *y, const double *mvec, double s4, int ntc,
                      int ntiles, double *partials, int ard0) {
  const size_t lds = (size_t)(128 * ndim + 128 + 4 * NACC) * sizeof(double);
  if (lds > 64 * 1024)  // D > 61: raised explicitly, per launch (the attribute belongs to the function on the current device)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&sparse_grad_kernel<AD>),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)((128 * GOGP_MAX_NDIM + 128 + 4 * NACC) * sizeof(double)));
  GOGP_KLAUNCH(sparse_grad_kernel<AD>, dim3(blocks), dim3(256), lds, s, p, X, rows, U, M, Wt, ldw, y, mvec, s4, ntc, ntiles,
               partials, ard0);
}

void launch_sparse_grad(hipStream_t s, const DevParams *p, int ndim, int ard_dims, const double *X, int64_t rows,
                        const double *U, int64_t M, const double *Wt, int64_t ldw, const double *y, const double *mvec,
                        double s4, double *partials, double *out, bool accumulate) {
  if (rows <= 0 || M <= 0) return;
  const int ntc = (int)((M + 63) / 64), ntiles = (int)((rows + 63) / 64) * ntc;
  const int blocks = sparse_grad_blocks(rows, M);
  // ARD dimensions in passes of 8 accumulators (the 16-accumulator instance of this kernel is over the audit's limit of
  // SGPR spills)
  if (ard_dims <= 0)
    sg_launch<0>(blocks, s, ndim, p, X, (long)rows, U, (long)M, Wt, (long)ldw, y, mvec, s4, ntc, ntiles, partials, 0);
  else
    for (int a0 = 0; a0 < ard_dims; a0 += 8)
      sg_launch<8>(blocks, s, ndim, p, X, (long)rows, U, (long)M, Wt, (long)ldw, y, mvec, s4, ntc, ntiles, partials, a0);
  launch_sparse_grad_final(s, partials, blocks, out, accumulate);
}

// ---- the derivative in the inducing points: the (U, X) pairs ---------------------------------------------------------
// part[slab][u][d] = sum over the rows f of the slab's 64-row tiles of (Wt[f][u] + y_f m_u s4) dk(u_u, x_f)/du_ud,
// f < rows, u < M, d0 <= d < min(D, d0 + DMAX).  Workgroup (column tile of 64 inducing points, slab of `tps` row tiles);
// the thread (tx, ty) owns inducing point c0 + tx -- a wave reads a row of Wt along its 64 lanes -- and the rows
// 16 ty .. 16 ty + 15 of every tile, through simil_xgrad_accum with xa = the inducing point.  The U tile is staged once,
// transposed ([D][64]: the lanes read consecutive doubles), the X tile [64][D] per row tile (a wave reads one address).
// The four ty sums are added through LDS, which takes the place of the tiles once they are read, as
// ((ty 0 + ty 1) + ty 2) + ty 3; sparse_ugrad_final_kernel adds the slabs in index order.  No atomics.
constexpr int SU_TPS_MIN = 4;  // row tiles per slab at least: one staging of the U tile and one row of partials per 256 rows

template <int DMAX>
__global__ __launch_bounds__(256) void sparse_ugrad_kernel(const DevParams *__restrict__ Pp, const double *__restrict__ X,
                                                           long rows, const double *__restrict__ U, long M,
                                                           const double *__restrict__ Wt, long ldw,
                                                           const double *__restrict__ y, const double *__restrict__ mvec,
                                                           double s4, int tps, double *__restrict__ part, int d0) {
  extern __shared__ double sm[];
  const DevParams &P = *Pp;
  const int D = P.ndim;
  double *Xi = sm;             // [64][D]
  double *UjT = sm + 64 * D;   // [D][64]
  double *yi = UjT + 64 * D;   // [64]
  double *red = sm;            // [3][DMAX][64], after the last tile
  const int tid = threadIdx.x;
  const int tx = tid & 63, ty = tid >> 6;
  const long c0 = (long)blockIdx.x * 64, gj = c0 + tx;
  const bool live = gj < M;
  const int ntr = (int)((rows + 63) / 64);
  const int t0 = (int)blockIdx.y * tps, t1 = t0 + tps < ntr ? t0 + tps : ntr;

  for (int idx = tid; idx < 64 * D; idx += 256) {
    const int d = idx >> 6, r = idx & 63;
    UjT[idx] = (c0 + r < M) ? U[(c0 + r) * D + d] : 0.0;
  }
  const double mjv = live ? mvec[gj] * s4 : 0.0;
  // (from dimension d0: the pass's own coordinates lie at constant offsets -- as uj[d * 64], d = d0 + q, hipcc keeps the
  // 16 offsets of an instance in SGPRs across the pair loop and spills them)
  const double *uj = UjT + d0 * 64 + tx;
  // per-thread addresses (in VGPRs: the kernel's arguments need not stay live in SGPRs across the pair loop)
  const double *wp = Wt + (long)t0 * 64 * ldw + (ty * 16) * ldw + gj;  // row 16 ty of the tile, column gj
  double *pp = part + ((long)blockIdx.y * M + gj) * D + d0;
  double acc[DMAX];
#pragma unroll
  for (int q = 0; q < DMAX; ++q) acc[q] = 0.0;

  for (int t = t0; t < t1; ++t, wp += 64 * ldw) {
    const long r0 = (long)t * 64;
    const int nr = rows - r0 < 64 ? (int)(rows - r0) : 64;  // live rows of the tile
    __syncthreads();  // previous tile's readers are done
    for (int idx = tid; idx < 64 * D; idx += 256) Xi[idx] = (idx < nr * D) ? X[r0 * D + idx] : 0.0;
    if (tid < 64) yi[tid] = (tid < nr) ? y[r0 + tid] : 0.0;
    __syncthreads();
    if (live) {
      const int rend = nr - ty * 16 < 16 ? nr - ty * 16 : 16;
      const double *xi = Xi + (ty * 16) * D;
      const double *w = wp;
      for (int rr = 0; rr < rend; ++rr, xi += D, w += ldw) {
        const double wgt = *w + yi[ty * 16 + rr] * mjv;
        simil_xgrad_accum<DMAX>(
            P, [&](int d) { return uj[(d - d0) * 64]; }, [&](int d) { return xi[d]; }, wgt, acc, d0);
      }
    }
  }

  __syncthreads();  // the tiles are read: their place takes the sums
  if (ty > 0) {
#pragma unroll
    for (int q = 0; q < DMAX; ++q) red[((ty - 1) * DMAX + q) * 64 + tx] = acc[q];
  }
  __syncthreads();
  if (ty == 0 && live) {
#pragma unroll
    for (int q = 0; q < DMAX; ++q)
      if (d0 + q < D)
        pp[q] = ((acc[q] + red[q * 64 + tx]) + red[(DMAX + q) * 64 + tx]) + red[(2 * DMAX + q) * 64 + tx];
  }
}

// dU[u][d] (+)= the slabs' sums in index order
__global__ __launch_bounds__(256) void sparse_ugrad_final_kernel(const double *__restrict__ part, int nslab, long md,
                                                                 double *__restrict__ dU, int accumulate) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= md) return;
  double v = 0.0;
  for (int sl = 0; sl < nslab; ++sl) v += part[(long)sl * md + idx];
  dU[idx] = accumulate ? dU[idx] + v : v;
}

// The slabs of launch_sparse_ugrad and the row tiles of one (*tps_out): a function of (rows, M) alone.  The grid
// (column tiles x slabs) stays within SPARSE_GRAD_BLOCKS_MAX workgroups, as sparse_grad_blocks caps its own.
int sparse_ugrad_slabs(int64_t rows, int64_t M, int *tps_out) {
  const int64_t ntr = (rows + 63) / 64, ntc = (M + 63) / 64;
  const int64_t most = std::max<int64_t>(1, SPARSE_GRAD_BLOCKS_MAX / std::max<int64_t>(1, ntc));
  const int64_t tps = std::max<int64_t>(SU_TPS_MIN, (ntr + most - 1) / most);
  if (tps_out) *tps_out = (int)tps;
  return (int)std::max<int64_t>(1, (ntr + tps - 1) / tps);
}

// An upper bound of sparse_ugrad_slabs(r, M) over every r <= rows: what a buffer of partials shared by launches of up
// to `rows` rows holds.  The slab count itself is not monotone in the rows: beyond SU_TPS_MIN * most row tiles the slabs
// grow longer and their number falls, so a ragged last chunk may take more slabs than the full chunks before it.  With
// tps == SU_TPS_MIN the count is ceil(ntr / SU_TPS_MIN) and ntr <= SU_TPS_MIN * most; with tps = ceil(ntr / most) it is
// ceil(ntr / ceil(ntr / most)) <= most.
int sparse_ugrad_slabs_bound(int64_t rows, int64_t M) {
  const int64_t ntr = (rows + 63) / 64, ntc = (M + 63) / 64;
  const int64_t most = std::max<int64_t>(1, SPARSE_GRAD_BLOCKS_MAX / std::max<int64_t>(1, ntc));
  return (int)std::max<int64_t>(1, std::min<int64_t>((ntr + SU_TPS_MIN - 1) / SU_TPS_MIN, most));
}

template <int DM>
static void su_launch(dim3 grid, hipStream_t s, int ndim, const DevParams *p, const double *X, long rows, const double *U,
                      long M, const double *Wt, long ldw, const double *y, const double *mvec, double s4, int tps,
                      double *part, int d0) {
  auto doubles = [](int nd) { return (size_t)std::max(128 * nd + 64, 3 * DM * 64); };
  const size_t lds = doubles(ndim) * sizeof(double);
  if (lds > 64 * 1024)  // D = 64: raised explicitly, per launch (the attribute belongs to the function on the current device)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&sparse_ugrad_kernel<DM>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)(doubles(GOGP_MAX_NDIM) * sizeof(double)));
  GOGP_KLAUNCH(sparse_ugrad_kernel<DM>, grid, dim3(256), lds, s, p, X, rows, U, M, Wt, ldw, y, mvec, s4, tps, part, d0);
}

void launch_sparse_ugrad(hipStream_t s, const DevParams *p, int ndim, const double *X, int64_t rows, const double *U,
                         int64_t M, const double *Wt, int64_t ldw, const double *y, const double *mvec, double s4,
                         double *part, double *dU, bool accumulate) {
  if (rows <= 0 || M <= 0) return;
  int tps = 1;
  const int nslab = sparse_ugrad_slabs(rows, M, &tps);
  const dim3 grid((unsigned)((M + 63) / 64), (unsigned)nslab);
  // instances of 4 / 8 / 16 accumulators, passes of 16 beyond (launch_xgrad's event instances: inside the register
  // limits of the code-object audit)
#define GOGP_LAUNCH_SU(DM, D0) \
  su_launch<DM>(grid, s, ndim, p, X, (long)rows, U, (long)M, Wt, (long)ldw, y, mvec, s4, tps, part, D0)
  if (ndim <= 4) GOGP_LAUNCH_SU(4, 0);
  else if (ndim <= 8) GOGP_LAUNCH_SU(8, 0);
  else
    for (int d0 = 0; d0 < ndim; d0 += 16) GOGP_LAUNCH_SU(16, d0);
#undef GOGP_LAUNCH_SU
  const long md = (long)M * ndim;
  GOGP_KLAUNCH(sparse_ugrad_final_kernel, dim3((unsigned)((md + 255) / 256)), dim3(256), 0, s, part, nslab, md, dU,
               accumulate ? 1 : 0);
}

// ---- element-wise passes over the Mp x Mp matrices ---------------------------------------------------------------------
// B (full, both triangles) = I + Bacc / s2 from the lower 64-tiles of Bacc
__global__ __launch_bounds__(256) void sparse_finish_b_kernel(const double *__restrict__ Bacc, long Mp, double inv_s2,
                                                              double *__restrict__ B) {
  const long i = blockIdx.y, j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= Mp) return;
  const long a = i > j ? i : j, b = i > j ? j : i;
  B[i * Mp + j] = (i == j ? 1.0 : 0.0) + Bacc[a * Mp + b] * inv_s2;
}
// dst = the upper triangle of src (diagonal included), exact zeros below it
__global__ __launch_bounds__(256) void sparse_copy_upper_kernel(const double *__restrict__ src, long Mp,
                                                                double *__restrict__ dst) {
  const long i = blockIdx.y, j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= Mp) return;
  dst[i * Mp + j] = j >= i ? src[i * Mp + j] : 0.0;
}
// T = I - Binv - g g^T s4 and S = 2 I - B - Binv - g g^T s4
__global__ __launch_bounds__(256) void sparse_weights_kernel(const double *__restrict__ B, const double *__restrict__ Binv,
                                                             const double *__restrict__ g, long Mp, double s4,
                                                             double *__restrict__ T, double *__restrict__ S) {
  const long i = blockIdx.y, j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= Mp) return;
  const double e = i == j ? 1.0 : 0.0, bi = Binv[i * Mp + j], gg = g[i] * g[j] * s4;
  T[i * Mp + j] = e - bi - gg;
  S[i * Mp + j] = 2.0 * e - B[i * Mp + j] - bi - gg;
}
// out[0] = sum_i 2 log C_ii, out[1] = tr B - M, out[2] = tr Binv, out[3] = r^T g, out[4] = g^T g over i < M: one
// workgroup, every thread its elements i = tid, tid + 256, .. in that order, then a fixed tree
__global__ __launch_bounds__(256) void sparse_scalars_kernel(const double *__restrict__ C, const double *__restrict__ B,
                                                             const double *__restrict__ Binv, const double *__restrict__ r,
                                                             const double *__restrict__ g, long M, long Mp,
                                                             double *__restrict__ out) {
  __shared__ double red[4][5];
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (long i = threadIdx.x; i < M; i += 256) {
    v[0] += 2.0 * log(C[i * Mp + i]);
    v[1] += B[i * Mp + i] - 1.0;
    v[2] += Binv[i * Mp + i];
    v[3] += r[i] * g[i];
    v[4] += g[i] * g[i];
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    double t = v[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = t;
  }
  __syncthreads();
  if (threadIdx.x < 5) out[threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
// out[0] = sum_{i < n} y_i^2, the same summation
__global__ __launch_bounds__(256) void sparse_sumsq_kernel(const double *__restrict__ y, long n, double *__restrict__ out) {
  __shared__ double red[4];
  double t = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) t += y[i] * y[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (red[0] + red[1]) + (red[2] + red[3]);
}
// Produce: mu_j = dot_j / s2 and sigma_j = sqrt(prior_j - q_j + sum_i A[j][i] V[j][i]) (unclamped, as gogp_produce), one
// wave per test point, the lanes' sums in column order, then a fixed tree
__global__ __launch_bounds__(256) void sparse_predict_kernel(const double *__restrict__ A, const double *__restrict__ V, long ld,
                                                             long ncols, long m, const double *__restrict__ prior,
                                                             const double *__restrict__ q, const double *__restrict__ dot,
                                                             double inv_s2, double *__restrict__ mu,
                                                             double *__restrict__ sigma) {
  const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= m) return;
  const int lane = threadIdx.x & 63;
  double t = 0.0;
  for (long i = lane; i < ncols; i += 64) t += A[j * ld + i] * V[j * ld + i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
  if (lane == 0) {
    mu[j] = dot[j] * inv_s2;
    sigma[j] = sqrt(prior[j] - q[j] + t);
  }
}

// ---- multi-output: the small kernels ------------------------------------------------------------------------------------
// Tm = nT (I - Binv) - GG s4 and S = nT (2 I - B - Binv) - GG s4, GG = Gamma Gamma^T, nT = the number of outputs
__global__ __launch_bounds__(256) void sparse_multi_weights_kernel(const double *__restrict__ B,
                                                                   const double *__restrict__ Binv,
                                                                   const double *__restrict__ GG, long Mp, double nT,
                                                                   double s4, double *__restrict__ Tm,
                                                                   double *__restrict__ S) {
  const long i = blockIdx.y, j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= Mp) return;
  const double e = i == j ? 1.0 : 0.0, bi = Binv[i * Mp + j], gg = GG[i * Mp + j] * s4;
  Tm[i * Mp + j] = nT * (e - bi) - gg;
  S[i * Mp + j] = nT * (2.0 * e - B[i * Mp + j] - bi) - gg;
}
// out[t] = r_t^T gamma_t and out[tstride + t] = gamma_t^T gamma_t over i < M, the rows t of Rt and Gt (ld doubles per
// row): one workgroup per output, every thread its elements i = tid, tid + 256, .. in that order, then a fixed tree
__global__ __launch_bounds__(256) void sparse_multi_dots_kernel(const double *__restrict__ Rt, const double *__restrict__ Gt,
                                                                long ld, long M, int tstride, double *__restrict__ out) {
  __shared__ double red[4][2];
  const long t = blockIdx.x;
  double a = 0.0, c = 0.0;
  for (long i = threadIdx.x; i < M; i += 256) {
    const double g = Gt[t * ld + i];
    a += Rt[t * ld + i] * g;
    c += g * g;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o);
    c += __shfl_xor(c, o);
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = a, red[threadIdx.x >> 6][1] = c;
  __syncthreads();
  if (threadIdx.x < 2)
    out[threadIdx.x * tstride + t] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
// out[t] = sum_{i < n} Y[i][t]^2 (Y: n x T, ldy doubles per row), the same summation, one workgroup per output
__global__ __launch_bounds__(256) void sparse_multi_sumsq_kernel(const double *__restrict__ Y, long ldy, long n,
                                                                 double *__restrict__ out) {
  __shared__ double red[4];
  const long t = blockIdx.x;
  double v = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) v += Y[i * ldy + t] * Y[i * ldy + t];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) out[t] = (red[0] + red[1]) + (red[2] + red[3]);
}
// Yp (rpad rows of ldp doubles) = the chunk's rows of Y (rows x T, ldy doubles per row), exact zeros in the rows from
// `rows` on and the columns T .. kp - 1: the A operand of the second pass's rank-T launch
__global__ __launch_bounds__(256) void sparse_multi_pad_kernel(const double *__restrict__ Y, long ldy, long rows, long T,
                                                               long kp, double *__restrict__ Yp, long ldp) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x, i = idx / kp, k = idx - i * kp;  // idx < rpad * kp: the grid
  Yp[i * ldp + k] = (i < rows && k < T) ? Y[i * ldy + k] : 0.0;
}
// Produce: sigma_j of sparse_predict_kernel alone (the outputs share it; their means come from one product)
__global__ __launch_bounds__(256) void sparse_multi_sigma_kernel(const double *__restrict__ A, const double *__restrict__ V,
                                                                 long ld, long ncols, long m,
                                                                 const double *__restrict__ prior,
                                                                 const double *__restrict__ q, double *__restrict__ sigma) {
  const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= m) return;
  const int lane = threadIdx.x & 63;
  double t = 0.0;
  for (long i = lane; i < ncols; i += 64) t += A[j * ld + i] * V[j * ld + i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
  if (lane == 0) sigma[j] = sqrt(prior[j] - q[j] + t);
}

void launch_sparse_multi_weights(hipStream_t s, const double *B, const double *Binv, const double *GG, int64_t Mp, int T,
                                 double s4, double *Tm, double *S) {
  GOGP_KLAUNCH(sparse_multi_weights_kernel, dim3((unsigned)(Mp / 256), (unsigned)Mp), dim3(256), 0, s, B, Binv, GG, (long)Mp,
               (double)T, s4, Tm, S);
}
void launch_sparse_multi_dots(hipStream_t s, const double *Rt, const double *Gt, int64_t ld, int64_t M, int T, int tstride,
                              double *out) {
  if (T <= 0) return;
  GOGP_KLAUNCH(sparse_multi_dots_kernel, dim3((unsigned)T), dim3(256), 0, s, Rt, Gt, (long)ld, (long)M, tstride, out);
}
void launch_sparse_multi_sumsq(hipStream_t s, const double *Y, int64_t ldy, int64_t n, int T, double *out) {
  if (T <= 0) return;
  GOGP_KLAUNCH(sparse_multi_sumsq_kernel, dim3((unsigned)T), dim3(256), 0, s, Y, (long)ldy, (long)n, out);
}
void launch_sparse_multi_pad(hipStream_t s, const double *Y, int64_t ldy, int64_t rows, int64_t T, int64_t kp, int64_t rpad,
                             double *Yp, int64_t ldp) {
  if (rpad <= 0 || kp <= 0 || (rpad * kp) % 256) return;  // (rpad a multiple of 128 and kp of 16: whole workgroups)
  GOGP_KLAUNCH(sparse_multi_pad_kernel, dim3((unsigned)(rpad * kp / 256)), dim3(256), 0, s, Y, (long)ldy, (long)rows,
               (long)T, (long)kp, Yp, (long)ldp);
}
void launch_sparse_multi_sigma(hipStream_t s, const double *A, const double *V, int64_t ld, int64_t ncols, int64_t m,
                               const double *prior, const double *q, double *sigma) {
  if (m <= 0) return;
  GOGP_KLAUNCH(sparse_multi_sigma_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, s, A, V, (long)ld, (long)ncols, (long)m,
               prior, q, sigma);
}

void launch_sparse_finish_b(hipStream_t s, const double *Bacc, int64_t Mp, double inv_s2, double *B) {
  GOGP_KLAUNCH(sparse_finish_b_kernel, dim3((unsigned)(Mp / 256), (unsigned)Mp), dim3(256), 0, s, Bacc, (long)Mp, inv_s2, B);
}
void launch_sparse_copy_upper(hipStream_t s, const double *src, int64_t Mp, double *dst) {
  GOGP_KLAUNCH(sparse_copy_upper_kernel, dim3((unsigned)(Mp / 256), (unsigned)Mp), dim3(256), 0, s, src, (long)Mp, dst);
}
void launch_sparse_weights(hipStream_t s, const double *B, const double *Binv, const double *g, int64_t Mp, double s4,
                           double *T, double *S) {
  GOGP_KLAUNCH(sparse_weights_kernel, dim3((unsigned)(Mp / 256), (unsigned)Mp), dim3(256), 0, s, B, Binv, g, (long)Mp, s4, T,
               S);
}
void launch_sparse_scalars(hipStream_t s, const double *C, const double *B, const double *Binv, const double *r,
                           const double *g, int64_t M, int64_t Mp, double *out) {
  GOGP_KLAUNCH(sparse_scalars_kernel, dim3(1), dim3(256), 0, s, C, B, Binv, r, g, (long)M, (long)Mp, out);
}
void launch_sparse_sumsq(hipStream_t s, const double *y, int64_t n, double *out) {
  GOGP_KLAUNCH(sparse_sumsq_kernel, dim3(1), dim3(256), 0, s, y, (long)n, out);
}
void launch_sparse_predict(hipStream_t s, const double *A, const double *V, int64_t ld, int64_t ncols, int64_t m,
                           const double *prior, const double *q, const double *dot, double inv_s2, double *mu,
                           double *sigma) {
  if (m <= 0) return;
  GOGP_KLAUNCH(sparse_predict_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, s, A, V, (long)ld, (long)ncols, (long)m,
               prior, q, dot, inv_s2, mu, sigma);
}

}  // namespace gogp
