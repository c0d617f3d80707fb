// hessian.hip -- the Hessian of the LML in the log hyperparameters (gogp_lml_hessian); no reference counterpart.
//
// With K_i = dK/dlog theta_i, K_ij the second derivative, alpha = K^-1 y and W = alpha alpha^T - K^-1:
//     H_ij = 1/2 tr(W K_ij) - (K_i alpha)^T K^-1 (K_j alpha) + 1/2 tr(K^-1 K_i K^-1 K_j).
// Everything is linear in the derivative matrices, so the work is done per SLOT -- one occurrence of a parameter in one
// term: the term's value (its output scale: theta dK/dtheta = the term itself), a length, an ARD length, the period --
// and the host folds the slot Hessian into the P x P one (a parameter shared by two terms is the sum of its slots).
// The noise parameter has K_n = dnoise I: M_n = dnoise K^-1 is never formed, its traces come from K^-1 directly.
//
//   hess_kmm_kernel   M_s = K^-1 K_s on v_mfma_f64_16x16x4_f64 for a group of up to 3 slots of one term.  A 64 x 64
//                     tile of every M_s per workgroup, four waves of 64 x 16 outputs.  The tile of K^-1 (64 x 16 per k-step)
//                     goes through LDS -- read from the STORED lower half whichever side of the diagonal it lies on, XOR-
//                     swizzled and fetched with ds_read_b64 as dgemm.hip does.  K_s is never in memory: the rows of X of
//                     the k-step and of the tile's columns sit in LDS and every lane evaluates the four entries of its own
//                     B fragment, ONE radial evaluation (distance, exp / sincos, polynomial) for all slots of the group,
//                     which then share the A fragments and have an accumulator set each (32 VGPRs; hess_eval.h: hess_group_max).
//   hess_pair_kernel  sum_ij W_ij K_st,ij for two groups of one term over the lower 64-tiles of K^-1 (the LML gradient's
//                     reduction with second derivatives); W is formed on the fly.
//   hess_kvec_kernel  b_s = K_s alpha, matrix-free;  hess_matvec_kernel: c_s = M_s alpha = K^-1 b_s.
//   hess_trdot_kernel tr(M_s M_t) = sum_ab M_s[a][b] M_t[b][a] per pair of 64-tiles (the first operand may be the
//                     symmetric K^-1 itself, from its stored half: the noise parameter's traces).
//   hess_quad_kernel  alpha^T K^-1 alpha, |alpha|^2, tr K^-1, |K^-1|_F^2.
// Every sum has a fixed order (shuffle trees, then hess_sum_kernel over the workgroups' partials in index order) and
// nothing is added atomically: two identical calls return identical bits.
#include <math.h>

#include <algorithm>

#include "api_internal.h"
#include "hess_eval.h"

namespace gogp {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// ---- LDS tile of K^-1: dgemm.hip's layout (rows of 16 doubles, the 16-B chunk index XORed with (row >> 1) & 7) ----------
__device__ __forceinline__ int hess_lds_off(int row, int k) {
  return row * GEMM_BK + ((((k >> 1) ^ ((row >> 1) & 7)) << 1) | (k & 1));
}
template <int OFF>
__device__ __forceinline__ double hess_lds_read_b64(unsigned addr) {
  double v;
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF) : "memory");
  return v;
}
// the compiler does not count an inline-asm read in lgkmcnt: wait for all of them and pin the fragments behind the wait
__device__ __forceinline__ void hess_lds_wait(double (&a)[4]) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]));
}
__device__ __forceinline__ unsigned hess_lds_address(const double *p) {
  return (unsigned)(size_t)(__attribute__((address_space(3))) const double *)p;
}

// One k-step's operands from global memory into registers: 4 elements of the 64 x 16 tile of K^-1 (rows r0.., columns
// k0..; zero from row / column n on) and up to 4 of the 16 rows of X.  A tile left of the diagonal is read along its rows;
// one on or right of it along its COLUMNS, i.e. along the rows of the stored mirror image.
__device__ __forceinline__ void hess_stage_load(const double *__restrict__ Kinv, long ld, const double *__restrict__ X,
                                                int D, long n, long r0, long k0, int tid, double (&ast)[4],
                                                double (&xst)[4]) {
  if (k0 + GEMM_BK <= r0) {
    const long gi = r0 + (tid >> 2), gk = k0 + (tid & 3) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) ast[e] = (gi < n && gk + e < n) ? Kinv[gi * ld + gk + e] : 0.0;
  } else {
    const long gk = k0 + (tid >> 4), gi = r0 + (tid & 15) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long i = gi + e;
      ast[e] = (i < n && gk < n) ? (i >= gk ? Kinv[i * ld + gk] : Kinv[gk * ld + i]) : 0.0;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long idx = k0 * D + tid + 256 * q;
    xst[q] = (tid + 256 * q < GEMM_BK * D && idx < n * D) ? X[idx] : 0.0;
  }
}
__device__ __forceinline__ void hess_stage_store(double *At, double *Xk, int D, long r0, long k0, int tid,
                                                 const double (&ast)[4], const double (&xst)[4]) {
  if (k0 + GEMM_BK <= r0) {
    const int r = tid >> 2, kq = (tid & 3) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) At[hess_lds_off(r, kq + e)] = ast[e];
  } else {
    const int kk = tid >> 4, rq = (tid & 15) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) At[hess_lds_off(rq + e, kk)] = ast[e];
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (tid + 256 * q < GEMM_BK * D) Xk[tid + 256 * q] = xst[q];
}

// M_q (64 x 64 tile (ti, tj) of slot q, at M + q * mstride, leading dimension ldm) = K^-1 K_q for the slots q < grp.n.
// Whole tiles are written: exact zeros in the rows and columns from n on.  Dynamic LDS: (64 * 16 + 16 D + 64 (D | 1))
// doubles.  Kinv: only the elements j <= i < n are read.  X: n rows of D doubles.
template <int G, bool PER>
__global__ __launch_bounds__(256, 2) void hess_kmm_kernel(const DevParams *__restrict__ Pp, HessGroup grp,
                                                          const double *__restrict__ X, const double *__restrict__ Kinv,
                                                          long ld, long n, int nt, double *__restrict__ M, long ldm,
                                                          long mstride) {
  extern __shared__ __attribute__((aligned(16))) double hess_lds[];
  const DevParams &P = *Pp;
  const int D = P.ndim, Ds = D | 1;
  double *At = hess_lds, *Xk = At + 64 * GEMM_BK, *Xb = Xk + GEMM_BK * D;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ti = blockIdx.x / nt, tj = blockIdx.x - ti * nt;
  const long r0 = (long)ti * 64, c0 = (long)tj * 64;
  for (int e = tid; e < 64 * D; e += 256) {
    const int b = e / D, d = e - b * D;
    Xb[b * Ds + d] = c0 + b < n ? X[(c0 + b) * D + d] : 0.0;
  }
  const int frow = lane & 15, fk = lane >> 4;
  // byte address of the A fragment (m = 0) of k-group kk; the m steps are immediate offsets (16 rows = 2048 bytes)
  unsigned afrag[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) afrag[kk] = hess_lds_address(At) + 8u * (unsigned)hess_lds_off(frow, kk * 4 + fk);
  const int bcol = wid * 16 + frow;  // the lane's column of the tile: its B fragment's
  const bool bok = c0 + bcol < n;
  const double *xbp = Xb + bcol * Ds;

  f64x4 acc[G][4];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[g][m] = (f64x4){0.0, 0.0, 0.0, 0.0};

  const int nk = (int)((n + GEMM_BK - 1) / GEMM_BK);  // K^-1 is zero from column n on
  double ast[4], xst[4];
  hess_stage_load(Kinv, ld, X, D, n, r0, 0, tid, ast, xst);
  hess_stage_store(At, Xk, D, r0, 0, tid, ast, xst);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const long k0 = (long)kt * GEMM_BK;
    const bool more = kt + 1 < nk;
    if (more) hess_stage_load(Kinv, ld, X, D, n, r0, k0 + GEMM_BK, tid, ast, xst);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      double a[4];
      a[0] = hess_lds_read_b64<0>(afrag[kk]);
      a[1] = hess_lds_read_b64<2048>(afrag[kk]);
      a[2] = hess_lds_read_b64<4096>(afrag[kk]);
      a[3] = hess_lds_read_b64<6144>(afrag[kk]);
      // the lane's entry (k, column) of every K_q of the group, while the fragment reads are in flight
      const int krow = kk * 4 + fk;
      const double *xkp = Xk + krow * D;
      double bv[G];
      hess_first<G, PER>(P, grp, [&](int d) { return xkp[d]; }, [&](int d) { return xbp[d]; }, bv);
      const bool ok = bok && k0 + krow < n;
#pragma unroll
      for (int g = 0; g < G; ++g) bv[g] = ok ? bv[g] : 0.0;
      hess_lds_wait(a);
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[g][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], bv[g], acc[g][m], 0, 0, 0);
    }
    __syncthreads();  // every wave has read this step's operands
    if (more) hess_stage_store(At, Xk, D, r0, k0 + GEMM_BK, tid, ast, xst);
    __syncthreads();
  }
  // C fragment of v_mfma_f64_16x16x4_f64: column = lane & 15, row = (lane >> 4) + 4 * register
  double *Mt = M + (r0 + fk) * ldm + c0 + bcol;
#pragma unroll
  for (int g = 0; g < G; ++g)
    if (g < grp.n)
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int v = 0; v < 4; ++v) Mt[(long)g * mstride + (long)(m * 16 + 4 * v) * ldm] = acc[g][m][v];
}

// ---- the small kernels --------------------------------------------------------------------------------------------------
// (ti, tj), tj <= ti, of the t-th tile of a lower triangle enumerated row by row (loo.hip does the same)
__device__ __forceinline__ void hess_lower_tile(int t, int &ti, int &tj) {
  ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (ti * (ti + 1) / 2 > t) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  tj = t - ti * (ti + 1) / 2;
}

// out[q] (q < NV) = the sum of v[q] over the 256 threads: a shuffle tree per wave, then the waves in order
template <int NV>
__device__ __forceinline__ void hess_block_sum(double (&v)[NV], double *red /* 4 * NV doubles of LDS */, double *out) {
#pragma unroll
  for (int q = 0; q < NV; ++q)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o);
  const int tid = threadIdx.x;
  if ((tid & 63) == 0)
#pragma unroll
    for (int q = 0; q < NV; ++q) red[(tid >> 6) * NV + q] = v[q];
  __syncthreads();
  if (tid < NV) out[tid] = (red[tid] + red[NV + tid]) + (red[2 * NV + tid] + red[3 * NV + tid]);
}

// part[block][0 .. HESS_NMOM) = the sums of hess_moments over the block's lower 64-tile with the weight alpha_i alpha_j -
// Kinv_ij, j <= i < n, the pairs off the diagonal counted twice.  Dynamic LDS: 64 (D | 1) doubles (the tile's columns of X).
template <bool PER>
__global__ __launch_bounds__(256) void hess_pair_kernel(const DevParams *__restrict__ Pp, HessGroup ga, HessGroup gb,
                                                        const double *__restrict__ X, const double *__restrict__ alpha,
                                                        const double *__restrict__ Kinv, long ld, long n,
                                                        double *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double hess_lds[];
  __shared__ double red[4 * HESS_NMOM];
  const DevParams &P = *Pp;
  const int D = P.ndim, Ds = D | 1;
  int ti, tj;
  hess_lower_tile((int)blockIdx.x, ti, tj);
  const long r0 = (long)ti * 64, c0 = (long)tj * 64;
  const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
  for (int e = tid; e < 64 * D; e += 256) {
    const int b = e / D, d = e - b * D;
    hess_lds[b * Ds + d] = c0 + b < n ? X[(c0 + b) * D + d] : 0.0;
  }
  __syncthreads();
  const long j = c0 + tx;
  const double aj = j < n ? alpha[j] : 0.0;
  const double *xbp = hess_lds + tx * Ds;
  double acc[HESS_NMOM];
#pragma unroll
  for (int q = 0; q < HESS_NMOM; ++q) acc[q] = 0.0;
  for (int rr = 0; rr < 16; ++rr) {
    const long i = r0 + ty * 16 + rr;  // wave-uniform
    if (i >= n) break;
    if (j > i || j >= n) continue;
    const double w = (alpha[i] * aj - Kinv[i * ld + j]) * (j < i ? 2.0 : 1.0);
    const double *xap = X + i * D;
    hess_moments<PER>(P, ga, gb, [&](int d) { return xap[d]; }, [&](int d) { return xbp[d]; }, w, acc);
  }
  hess_block_sum<HESS_NMOM>(acc, red, part + (long)blockIdx.x * HESS_NMOM);
}

// b_q[i] = sum_{j < n} K_q(x_i, x_j) alpha_j for the slots q < g.n (row q of b, ldb doubles each; zero from row n on up
// to the grid's 64 * gridDim.x).  64 rows per workgroup; wave w takes the columns j = w (mod 4), in order.
template <bool PER>
__global__ __launch_bounds__(256) void hess_kvec_kernel(const DevParams *__restrict__ Pp, HessGroup g,
                                                        const double *__restrict__ X, const double *__restrict__ alpha,
                                                        long n, double *__restrict__ b, long ldb) {
  extern __shared__ __attribute__((aligned(16))) double hess_lds[];
  constexpr int G = HESS_G;
  __shared__ double red[4][G][64];
  const DevParams &P = *Pp;
  const int D = P.ndim, Ds = D | 1;
  const int tid = threadIdx.x, tx = tid & 63, w = tid >> 6;
  const long i0 = (long)blockIdx.x * 64, i = i0 + tx;
  for (int e = tid; e < 64 * D; e += 256) {
    const int r = e / D, d = e - r * D;
    hess_lds[r * Ds + d] = i0 + r < n ? X[(i0 + r) * D + d] : 0.0;
  }
  __syncthreads();
  const double *xap = hess_lds + tx * Ds;
  double acc[G];
#pragma unroll
  for (int q = 0; q < G; ++q) acc[q] = 0.0;
  for (long j = w; j < n; j += 4) {  // wave-uniform
    const double *xbp = X + j * D;
    const double aj = alpha[j];
    double k1[G];
    hess_first<G, PER>(P, g, [&](int d) { return xap[d]; }, [&](int d) { return xbp[d]; }, k1);
#pragma unroll
    for (int q = 0; q < G; ++q) acc[q] += k1[q] * aj;
  }
#pragma unroll
  for (int q = 0; q < G; ++q) red[w][q][tx] = acc[q];
  __syncthreads();
  if (w == 0)
#pragma unroll
    for (int q = 0; q < G; ++q)
      if (q < g.n) b[(long)q * ldb + i] = i < n ? (red[0][q][tx] + red[1][q][tx]) + (red[2][q][tx] + red[3][q][tx]) : 0.0;
}

// c_s[a] = sum_{b < n} M_s[a][b] alpha_b: one wave per row a (gridDim.x * 4 rows), blockIdx.y = s
__global__ __launch_bounds__(256) void hess_matvec_kernel(const double *__restrict__ M, long ldm, long mstride,
                                                          const double *__restrict__ alpha, long n, double *__restrict__ c,
                                                          long ldc) {
  const int lane = threadIdx.x & 63;
  const long a = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const double *row = M + (long)blockIdx.y * mstride + a * ldm;
  double t = 0.0;
  if (a < n)
    for (long b = lane; b < n; b += 64) t += row[b] * alpha[b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
  if (lane == 0) c[(long)blockIdx.y * ldc + a] = t;
}

// dots[s * (S + 1) + t] = b_s . c_t for s <= t < S (zero below the diagonal), dots[s * (S + 1) + S] = alpha . c_s;
// grid (S, S + 1)
__global__ __launch_bounds__(256) void hess_dots_kernel(const double *__restrict__ b, const double *__restrict__ c, long ldv,
                                                        const double *__restrict__ alpha, long n, int S,
                                                        double *__restrict__ dots) {
  __shared__ double red[4];
  const int s = blockIdx.x, t = blockIdx.y;
  const double *u = t == S ? alpha : b + (long)s * ldv;
  const double *v = c + (long)(t == S ? s : t) * ldv;
  double acc[1] = {0.0};
  if (t >= s)
    for (long i = threadIdx.x; i < n; i += 256) acc[0] += u[i] * v[i];
  hess_block_sum<1>(acc, red, dots + (long)s * (S + 1) + t);
}

// part[pair][tile (ta, tb)] = sum_{a in ta, b in tb, both < n} A[a][b] B[b][a] with, for pair p = blockIdx.y, B = slot
// pairs[2 p + 1] of M and A = slot pairs[2 p] of M or, pairs[2 p] < 0, the symmetric K^-1 from its stored lower half.
__global__ __launch_bounds__(256) void hess_trdot_kernel(const double *__restrict__ M, long ldm, long mstride,
                                                         const double *__restrict__ Kinv, long ld, long n, int nt,
                                                         const int *__restrict__ pairs, double *__restrict__ part) {
  __shared__ double tile[64][65];
  __shared__ double red[4];
  const int sa = pairs[2 * blockIdx.y], sb = pairs[2 * blockIdx.y + 1];
  const int ta = blockIdx.x / nt, tb = blockIdx.x - ta * nt;
  const long a0 = (long)ta * 64, b0 = (long)tb * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const double *B = M + (long)sb * mstride;
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const int r = ty * 16 + rr;
    tile[r][tx] = (b0 + r < n && a0 + tx < n) ? B[(b0 + r) * ldm + a0 + tx] : 0.0;
  }
  __syncthreads();
  const long b = b0 + tx;
  double acc[1] = {0.0};
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const int r = ty * 16 + rr;
    const long a = a0 + r;
    double v = 0.0;
    if (a < n && b < n) v = sa >= 0 ? M[(long)sa * mstride + a * ldm + b] : (a >= b ? Kinv[a * ld + b] : Kinv[b * ld + a]);
    acc[0] += v * tile[tx][r];
  }
  hess_block_sum<1>(acc, red, part + (long)blockIdx.y * nt * nt + blockIdx.x);
}

// part[block][0 .. 3] over the block's lower 64-tile: alpha^T K^-1 alpha and |K^-1|_F^2 (pairs off the diagonal counted
// twice), |alpha|^2 and tr K^-1 (diagonal tiles)
__global__ __launch_bounds__(256) void hess_quad_kernel(const double *__restrict__ Kinv, long ld,
                                                        const double *__restrict__ alpha, long n, double *__restrict__ part) {
  __shared__ double red[16];
  int ti, tj;
  hess_lower_tile((int)blockIdx.x, ti, tj);
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long j = (long)tj * 64 + tx;
  const double aj = j < n ? alpha[j] : 0.0;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int rr = 0; rr < 16; ++rr) {
    const long i = (long)ti * 64 + ty * 16 + rr;
    if (i >= n || j > i) continue;
    const double k = Kinv[i * ld + j], ai = alpha[i], m = j < i ? 2.0 : 1.0;
    acc[0] += m * ai * k * aj;
    acc[1] += m * k * k;
    if (i == j) acc[2] += ai * ai, acc[3] += k;
  }
  hess_block_sum<4>(acc, red, part + (long)blockIdx.x * 4);
}

// out[v] = sum_b part[b * sb + v * sv], b < nb: thread t adds b = t, t + 256, .. in order, then a fixed tree; grid = values
__global__ __launch_bounds__(256) void hess_sum_kernel(const double *__restrict__ part, long nb, long sb, long sv,
                                                       double *__restrict__ out) {
  __shared__ double red[4];
  const double *p = part + (long)blockIdx.x * sv;
  double acc[1] = {0.0};
  for (long b = threadIdx.x; b < nb; b += 256) acc[0] += p[b * sb];
  hess_block_sum<1>(acc, red, out + blockIdx.x);
}

// ---- launchers -----------------------------------------------------------------------------------------------------------
static HessGroup hess_group(int term, int nslot, const int *type, const int *dim) {
  HessGroup g = {};
  g.term = term;
  g.n = nslot;
  for (int q = 0; q < nslot; ++q) g.type[q] = type[q], g.dim[q] = dim[q];
  return g;
}
static size_t hess_x_lds(int ndim) { return (size_t)64 * (ndim | 1) * sizeof(double); }

void launch_hess_kmm(hipStream_t s, const DevParams *p, int ndim, bool periodic, int term, int nslot, const int *type,
                     const int *dim, const double *X, const double *Kinv, int64_t ld, int64_t n, int64_t npad, double *M,
                     int64_t ldm, int64_t mstride) {
  const HessGroup g = hess_group(term, nslot, type, dim);
  const int nt = (int)(npad / 64);
  const size_t lds = (size_t)(64 * GEMM_BK + GEMM_BK * ndim) * sizeof(double) + hess_x_lds(ndim);
  // the instance with as many accumulator sets as the group has slots
  void (*k[2][HESS_G])(const DevParams *, HessGroup, const double *, const double *, long, long, int, double *, long, long) = {
      {hess_kmm_kernel<1, false>, hess_kmm_kernel<2, false>, hess_kmm_kernel<3, false>},
      {hess_kmm_kernel<1, true>, hess_kmm_kernel<2, true>, nullptr}};  // hess_eval.h: hess_group_max
  if (nslot < 1 || nslot > hess_group_max(periodic)) return;
  GOGP_KLAUNCH(k[periodic][nslot - 1], dim3((unsigned)(nt * nt)), dim3(256), lds, s, p, g, X, Kinv, (long)ld, (long)n, nt, M,
               (long)ldm, (long)mstride);
}

void launch_hess_pair(hipStream_t s, const DevParams *p, int ndim, bool periodic, int term, int na, const int *type_a,
                      const int *dim_a, int nb, const int *type_b, const int *dim_b, const double *X, const double *alpha,
                      const double *Kinv, int64_t ld, int64_t n, int64_t npad, double *part, double *out) {
  const HessGroup ga = hess_group(term, na, type_a, dim_a), gb = hess_group(term, nb, type_b, dim_b);
  const int nt = (int)(npad / 64), blocks = nt * (nt + 1) / 2;
  GOGP_KLAUNCH(periodic ? hess_pair_kernel<true> : hess_pair_kernel<false>, dim3((unsigned)blocks), dim3(256),
               hess_x_lds(ndim), s, p, ga, gb, X, alpha, Kinv, (long)ld, (long)n, part);
  GOGP_KLAUNCH(hess_sum_kernel, dim3(HESS_NMOM), dim3(256), 0, s, part, (long)blocks, (long)HESS_NMOM, 1L, out);
}

void launch_hess_kvec(hipStream_t s, const DevParams *p, int ndim, bool periodic, int term, int nslot, const int *type,
                      const int *dim, const double *X, const double *alpha, int64_t n, int64_t npad, double *b, int64_t ldb) {
  const HessGroup g = hess_group(term, nslot, type, dim);
  GOGP_KLAUNCH(periodic ? hess_kvec_kernel<true> : hess_kvec_kernel<false>, dim3((unsigned)(npad / 64)), dim3(256),
               hess_x_lds(ndim), s, p, g, X, alpha, (long)n, b, (long)ldb);
}

void launch_hess_matvec(hipStream_t s, const double *M, int64_t ldm, int64_t mstride, const double *alpha, int64_t n,
                        int64_t npad, int S, double *c, int64_t ldc) {
  GOGP_KLAUNCH(hess_matvec_kernel, dim3((unsigned)(npad / 4), (unsigned)S), dim3(256), 0, s, M, (long)ldm, (long)mstride, alpha,
               (long)n, c, (long)ldc);
}

void launch_hess_dots(hipStream_t s, const double *b, const double *c, int64_t ldv, const double *alpha, int64_t n, int S,
                      double *dots) {
  GOGP_KLAUNCH(hess_dots_kernel, dim3((unsigned)S, (unsigned)(S + 1)), dim3(256), 0, s, b, c, (long)ldv, alpha, (long)n, S,
               dots);
}

void launch_hess_quad(hipStream_t s, const double *Kinv, int64_t ld, const double *alpha, int64_t n, int64_t npad,
                      double *part, double *out) {
  const int64_t nt = npad / 64, ntl = nt * (nt + 1) / 2;
  GOGP_KLAUNCH(hess_quad_kernel, dim3((unsigned)ntl), dim3(256), 0, s, Kinv, (long)ld, alpha, (long)n, part);
  GOGP_KLAUNCH(hess_sum_kernel, dim3(4), dim3(256), 0, s, (const double *)part, (long)ntl, 4L, 1L, out);
}

void launch_hess_traces(hipStream_t s, const double *M, int64_t ldm, int64_t mstride, const double *Kinv, int64_t ld,
                        int64_t n, int64_t npad, const int *pairs, int npairs, double *part, double *out) {
  const int64_t nt = npad / 64;
  for (int p0 = 0; p0 < npairs; p0 += HESS_TCHUNK) {
    const int np = std::min(HESS_TCHUNK, npairs - p0);
    GOGP_KLAUNCH(hess_trdot_kernel, dim3((unsigned)(nt * nt), (unsigned)np), dim3(256), 0, s, M, (long)ldm, (long)mstride, Kinv,
                 (long)ld, (long)n, (int)nt, pairs + 2 * p0, part);
    GOGP_KLAUNCH(hess_sum_kernel, dim3((unsigned)np), dim3(256), 0, s, (const double *)part, (long)(nt * nt), 1L,
                 (long)(nt * nt), out + p0);
  }
}

}  // namespace gogp

// ---- gogp_lml_hessian ------------------------------------------------------------------------------------------------------
using namespace gogp;

namespace {
struct Slot {
  int term, type, dim, param;
};
struct Group {
  int term, first, n;  // slots first .. first + n - 1
};
}  // namespace

extern "C" int gogp_lml_hessian(gogp_handle *h, double *H) {
  if (!h || !H) return fail(h, GOGP_EARG, "lml_hessian: NULL");
  const char *why = h->prec == 32          ? "precision = 32 handles"
                    : h->grad_prec == 32   ? "gradient_precision = 32 (a float K^-1)"
                    : h->ev()              ? "event discounts"
                    : h->dist              ? "sharded handles"
                                           : nullptr;
  if (why) return refuse(h, "lml_hessian", GOGP_EARG, (std::string(why) + " are not supported").c_str());
  const int P = h->P, D = h->D;
  for (int i = 0; i < P * P; ++i) H[i] = 0.0;
  if (h->n == 0) return GOGP_OK;
  if (!h->factored) return refuse(h, "lml_hessian", GOGP_ESTATE, "nothing absorbed");
  HIPCHK(h, hipSetDevice(h->device));

  // the slots: every occurrence of a similarity parameter, term by term, in groups (hess_eval.h: hess_group_max) that share an evaluation
  std::vector<Slot> slots;
  std::vector<Group> groups;
  const gogp_desc &d = h->desc;
  for (int t = 0; t < d.nterms; ++t) {
    const gogp_term &T = d.terms[t];
    const int first = (int)slots.size();
    if (T.scale_idx >= 0) slots.push_back({t, HESS_VALUE, 0, T.scale_idx});
    if (T.ard)
      for (int j = 0; j < D; ++j) slots.push_back({t, HESS_ARD, j, T.len_idx + j});
    else
      slots.push_back({t, HESS_LEN, 0, T.len_idx});
    if (T.kind == GOGP_K_PERIODIC) slots.push_back({t, HESS_PERIOD, 0, T.period_idx});
    const int gmax = hess_group_max(T.kind == GOGP_K_PERIODIC);
    for (int q = first; q < (int)slots.size(); q += gmax) groups.push_back({t, q, std::min(gmax, (int)slots.size() - q)});
  }
  const int S = (int)slots.size(), NG = (int)groups.size();
  std::vector<int> type(S), dim(S);
  for (int q = 0; q < S; ++q) type[q] = slots[q].type, dim[q] = slots[q].dim;
  // pairs of groups of one term (second derivatives), pairs of slots (traces; -1: K^-1 itself, the noise parameter's)
  std::vector<std::pair<int, int>> gpairs;
  for (int a = 0; a < NG; ++a)
    for (int b = a; b < NG; ++b)
      if (groups[a].term == groups[b].term) gpairs.push_back({a, b});
  std::vector<int> tpairs;
  for (int a = 0; a < S; ++a)
    for (int b = a; b < S; ++b) tpairs.push_back(a), tpairs.push_back(b);
  for (int b = 0; b < S; ++b) tpairs.push_back(-1), tpairs.push_back(b);
  const int NT = (int)tpairs.size() / 2;

  int rc = regression_kinv_alpha(h);
  if (rc != GOGP_OK) return rc;
  hipStream_t s = h->s;
  const int64_t n = h->n, npad = h->npad, ld = npad;
  const int64_t nt = npad / 64, ntl = nt * (nt + 1) / 2;
  const size_t mat = (size_t)npad * (size_t)npad;
  Carve cv{nullptr};
  auto layout = [&](Carve &c, double *&M, double *&bv, double *&cvv, double *&part, double *&res, int *&tp) {
    M = c.take<double>((size_t)S * mat);
    bv = c.take<double>((size_t)S * npad);
    cvv = c.take<double>((size_t)S * npad);
    part = c.take<double>(std::max<size_t>((size_t)ntl * HESS_NMOM, (size_t)std::min(NT, HESS_TCHUNK) * nt * nt));
    res = c.take<double>((size_t)gpairs.size() * HESS_NMOM + 4 + (size_t)S * (S + 1) + NT);
    tp = c.take<int>(tpairs.size());
  };
  double *M, *bv, *cvv, *part, *res;
  int *tp;
  layout(cv, M, bv, cvv, part, res, tp);
  const size_t need = cv.off;
  if (h->hess_ws.bytes < need) {  // the M_s are 8 npad^2 bytes per slot: ask before allocating, never thrash
    h->hess_ws.release();
    size_t free_b = 0, total_b = 0;
    HIPCHK(h, hipMemGetInfo(&free_b, &total_b));
    if (need > free_b) {
      char buf[200];
      snprintf(buf, sizeof buf, "needs %zu bytes of device memory (%d matrices of %zu), %zu are free", need, S,
               mat * sizeof(double), free_b);
      return refuse(h, "lml_hessian", GOGP_ENOMEM, buf);
    }
  }
  rc = h->hess_ws.reserve(h, need);
  if (rc != GOGP_OK) return rc;
  cv = Carve{h->hess_ws.as<char>()};
  layout(cv, M, bv, cvv, part, res, tp);
  double *r_pair = res, *r_quad = r_pair + gpairs.size() * HESS_NMOM, *r_dots = r_quad + 4,
         *r_tr = r_dots + (size_t)S * (S + 1);
  const size_t nres = (size_t)(r_tr + NT - res);
  HIPCHK(h, hipMemcpyAsync(tp, tpairs.data(), tpairs.size() * sizeof(int), hipMemcpyHostToDevice, s));

  for (const Group &g : groups) {
    const int *ty = type.data() + g.first, *dm = dim.data() + g.first;
    const bool per = d.terms[g.term].kind == GOGP_K_PERIODIC;
    launch_hess_kmm(s, h->devP, D, per, g.term, g.n, ty, dm, h->dX, h->bufA, ld, n, npad, M + (size_t)g.first * mat, npad,
                    (int64_t)mat);
    launch_hess_kvec(s, h->devP, D, per, g.term, g.n, ty, dm, h->dX, h->alpha, n, npad, bv + (size_t)g.first * npad, npad);
  }
  for (size_t k = 0; k < gpairs.size(); ++k) {
    const Group &a = groups[gpairs[k].first], &b = groups[gpairs[k].second];
    launch_hess_pair(s, h->devP, D, d.terms[a.term].kind == GOGP_K_PERIODIC, a.term, a.n, type.data() + a.first,
                     dim.data() + a.first, b.n, type.data() + b.first, dim.data() + b.first, h->dX, h->alpha, h->bufA, ld, n,
                     npad, part, r_pair + k * HESS_NMOM);
  }
  launch_hess_quad(s, h->bufA, ld, h->alpha, n, npad, part, r_quad);
  launch_hess_matvec(s, M, npad, (int64_t)mat, h->alpha, n, npad, S, cvv, npad);
  launch_hess_dots(s, bv, cvv, npad, h->alpha, n, S, r_dots);
  launch_hess_traces(s, M, npad, (int64_t)mat, h->bufA, ld, n, npad, tp, NT, part, r_tr);
  std::vector<double> hres(nres);
  HIPCHK(h, hipMemcpyAsync(hres.data(), res, nres * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());

  // the slot Hessian (upper triangle), the noise parameter as slot S
  const double *hp = hres.data(), *hq = hp + (r_quad - res), *hd = hp + (r_dots - res), *ht = hp + (r_tr - res);
  const double dn = h->nn > 0 ? h->hostP->dnoise : 0.0;
  std::vector<double> Hs((size_t)(S + 1) * (S + 1), 0.0);
  for (size_t k = 0; k < gpairs.size(); ++k) {
    const Group &a = groups[gpairs[k].first], &b = groups[gpairs[k].second];
    const double *m = hp + k * HESS_NMOM;  // hess_eval.h: hess_moments
    constexpr int G = HESS_G;
    for (int qa = 0; qa < a.n; ++qa)
      for (int qb = 0; qb < b.n; ++qb) {
        const int sa = a.first + qa, sb = b.first + qb;
        if (sa > sb) continue;
        const int ta = type[sa], tb = type[sb];
        double v;
        if (ta == HESS_VALUE)
          v = tb == HESS_VALUE ? m[0] : m[1 + G + qb];
        else if (tb == HESS_VALUE)
          v = m[1 + qa];
        else
          v = m[1 + 5 * G + qa * G + qb] + (sa == sb ? m[1 + 2 * G + qa] : 0.0) + (ta == HESS_PERIOD ? m[1 + 4 * G + qb] : 0.0) +
              (tb == HESS_PERIOD && sa != sb ? m[1 + 3 * G + qa] : 0.0);
        Hs[(size_t)sa * (S + 1) + sb] = 0.5 * v;
      }
  }
  int tix = 0;
  for (int a = 0; a < S; ++a)
    for (int b = a; b < S; ++b, ++tix) Hs[(size_t)a * (S + 1) + b] += 0.5 * ht[tix] - hd[(size_t)a * (S + 1) + b];
  for (int b = 0; b < S; ++b, ++tix) Hs[(size_t)b * (S + 1) + S] = dn * (0.5 * ht[tix] - hd[(size_t)b * (S + 1) + S]);
  Hs[(size_t)S * (S + 1) + S] = dn * (hq[2] - hq[3]) + dn * dn * (0.5 * hq[1] - hq[0]);
  // ... folded into the parameters: H_ij = sum over the slots of i and of j, the upper triangle mirrored
  auto param = [&](int q) { return q < S ? slots[q].param : h->ns; };
  const int SN = h->nn > 0 ? S + 1 : S;
  for (int a = 0; a < SN; ++a)
    for (int b = a; b < SN; ++b) {
      const int i = std::min(param(a), param(b)), j = std::max(param(a), param(b));
      const double v = Hs[(size_t)a * (S + 1) + b];
      H[i * P + j] += (a != b && i == j) ? 2.0 * v : v;
    }
  for (int i = 0; i < P; ++i)
    for (int j = 0; j < i; ++j) H[i * P + j] = H[j * P + i];
  return GOGP_OK;
}
