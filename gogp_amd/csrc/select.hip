// select.hip -- greedy conditional-variance selection of inducing points (gogp_sparse_select_inducing; api.hip
// orchestrates): a partial Cholesky factorisation of k(X, X) with diagonal pivoting (Burt, Rasmussen & van der Wilk,
// 2019 / 2020).  X: N x D, the similarity k at theta (the noise does not enter), a cap M and a tolerance tol >= 0:
//
//     d_i = k(x_i, x_i)                                      i < N
//     for j = 0 .. M-1:
//         p = the LOWEST index among the maximisers of d      (ties: lowest index; all d equal at j = 0, so piv[0] = 0)
//         if not (d_p > tol): stop, m = j                     (also stops on NaN)
//         piv[j] = p,  pv[j] = d_p
//         l_i = (k(x_i, x_p) - sum_{t<j} L[i][t] L[p][t]) / sqrt(d_p)   for rows not yet selected
//         l_p = sqrt(d_p);  l_i = 0 exactly for rows selected earlier
//         L[:, j] = l;  d_i -= l_i^2;  d_p = 0 exactly (selected rows keep d = 0)
//     m = number of steps taken;  trace = sum_i d_i  (= tr K - |L|_F^2 = t0 - tr Qff for U = X[piv])
//
// pv is non-increasing up to rounding; L[piv] is lower triangular with diagonal sqrt(pv) and equals chol(k(U, U)) in
// pivot order; L L^T reproduces K exactly on the selected rows and columns.
//
// The factor lies column-major on the device: Lt, column t at Lt + t * ldn, ldn = N rounded up to 256; the rows N ..
// ldn - 1 of a column are never written or read.  One step is one launch and one bandwidth-bound pass: thread i reads
// Lt[t][i] for t < j (a wave reads 512 contiguous bytes per column) and the new column is one contiguous store.  Kernel
// boundaries are the only synchronisation: no spin, no hand-off between workgroups inside a launch, no atomics, and every
// sum has a fixed order, so two runs return identical bits.
//   select_init_kernel   d, the cleared selection mask and the first per-workgroup partial maxima;
//   select_step_kernel   step j: every workgroup reduces the previous launch's partial maxima (value, index) to (p, d_p)
//                        for itself -- at most SELECT_BLOCKS_MAX pairs through L2, cheaper than a second launch --, stages
//                        row p of the factor and x_p in LDS, updates its rows (grid-stride) and writes its partial
//                        maximum of the new d for the next step into the other half of the double-buffered array;
//                        workgroup 0 records piv[j], pv[j] and the step count;
//   select_final_kernel  trace = sum d in index order per thread and a fixed tree, U = X[piv].
// A step whose predecessor recorded no pivot (piv[j - 1] < 0, as cleared before the run), or that finds the stop
// condition itself, returns without writing: the host enqueues the steps without a round trip per step and looks at
// the step count every SELECT_SYNC_STEPS launches to skip the rest.
#include <algorithm>

#include "kern_eval.h"

namespace gogp {

namespace {
// a is a better pivot candidate than b: NaN first (the run stops on it), then the larger value, then the lower index
__device__ __forceinline__ bool sel_better(double av, long long ai, double bv, long long bi) {
  const bool an = av != av, bn = bv != bv;
  if (an != bn) return an;
  if (!an && av != bv) return av > bv;
  return ai < bi;
}
__device__ __forceinline__ void sel_take(double &v, long long &i, double ov, long long oi) {
  if (sel_better(ov, oi, v, i)) v = ov, i = oi;
}
constexpr long long SEL_NONE = 0x7fffffffffffffffLL;  // the index of "no candidate" (value -inf): loses against every row

// the workgroup's best of the threads' (v, i): wave shuffles, then the four waves through LDS in wave order; every
// thread returns with the result
__device__ __forceinline__ void sel_block_best(double &v, long long &i, double *rv, long long *ri) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const long long oi = __shfl_xor(i, o);
    sel_take(v, i, ov, oi);
  }
  __syncthreads();  // an earlier use of rv / ri is read
  if ((threadIdx.x & 63) == 0) rv[threadIdx.x >> 6] = v, ri[threadIdx.x >> 6] = i;
  __syncthreads();
  v = rv[0], i = ri[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) sel_take(v, i, rv[w], ri[w]);
}
}  // namespace

// d_i = k(x_i, x_i) (d0 given: d0_i, the hook's override), sel_i = 0 and part[b] = the best of workgroup b's rows
// i = (b + q gridDim.x) 256 + tid, q = 0, 1, ..
__global__ __launch_bounds__(256) void select_init_kernel(const DevParams *__restrict__ Pp, const double *__restrict__ X,
                                                          long N, const double *__restrict__ d0, double *__restrict__ d,
                                                          unsigned char *__restrict__ sel, SelPair *__restrict__ part) {
  __shared__ double rv[4];
  __shared__ long long ri[4];
  const DevParams &P = *Pp;
  const int D = P.ndim;
  double bv = -INFINITY;
  long long bi = SEL_NONE;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
    const double *xi = X + i * D;
    const double di = d0 ? d0[i] : simil_value(P, [&](int q) { return xi[q]; }, [&](int q) { return xi[q]; });
    d[i] = di;
    sel[i] = 0;
    sel_take(bv, bi, di, i);
  }
  sel_block_best(bv, bi, rv, ri);
  if (threadIdx.x == 0) part[blockIdx.x].v = bv, part[blockIdx.x].i = bi;
}

// Step j (see the head of the file).  pin: gridDim.x pairs of the previous launch, pout: this one's.  Dynamic LDS:
// j doubles of the pivot row, then ndim doubles of x_p.
__global__ __launch_bounds__(256) void select_step_kernel(const DevParams *__restrict__ Pp, const double *__restrict__ X,
                                                          long N, double *__restrict__ Lt, long ldn, int j, double tol,
                                                          double *__restrict__ d, unsigned char *__restrict__ sel,
                                                          const SelPair *__restrict__ pin, SelPair *__restrict__ pout,
                                                          long long *__restrict__ piv, double *__restrict__ pv,
                                                          long long *__restrict__ state) {
  extern __shared__ double sm[];
  __shared__ double rv[4];
  __shared__ long long ri[4];
  if (j > 0 && piv[j - 1] < 0) return;  // an earlier step stopped (written by the previous launch, or never)
  const DevParams &P = *Pp;
  const int D = P.ndim;
  const int tid = threadIdx.x;
  double *Lp = sm, *xp = sm + j;

  // ---- the pivot: larger value first, then lower index ------------------------------------------------------------------
  double dp = -INFINITY;
  long long p = SEL_NONE;
  for (int q = tid; q < (int)gridDim.x; q += 256) sel_take(dp, p, pin[q].v, pin[q].i);
  sel_block_best(dp, p, rv, ri);
  if (!(dp > tol)) return;  // every workgroup finds the same pair: the whole grid returns
  if (blockIdx.x == 0 && tid == 0) piv[j] = p, pv[j] = dp, state[0] = j + 1;

  // ---- row p of the factor (a strided gather of j elements) and x_p -------------------------------------------------------
  for (int t = tid; t < j; t += 256) Lp[t] = Lt[(long)t * ldn + p];
  if (tid < D) xp[tid] = X[p * D + tid];
  __syncthreads();
  const double sq = sqrt(dp);

  double bv = -INFINITY;
  long long bi = SEL_NONE;
  for (long i = (long)blockIdx.x * 256 + tid; i < N; i += (long)gridDim.x * 256) {
    double li, di;
    if (i == p) {
      li = sq, di = 0.0;
      sel[i] = 1;
    } else if (sel[i]) {
      li = 0.0, di = 0.0;
    } else {
      const double *xi = X + i * D;
      const double kv = simil_value(P, [&](int q) { return xi[q]; }, [&](int q) { return xp[q]; });
      // eight interleaved partial sums (t mod 8), each in column order, added in a fixed tree: the loads are independent
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;
      const double *col = Lt + i;
      int t = 0;
      for (; t + 8 <= j; t += 8, col += 8 * ldn) {
        const double a0 = col[0], a1 = col[ldn], a2 = col[2 * ldn], a3 = col[3 * ldn];
        const double a4 = col[4 * ldn], a5 = col[5 * ldn], a6 = col[6 * ldn], a7 = col[7 * ldn];
        s0 += a0 * Lp[t], s1 += a1 * Lp[t + 1], s2 += a2 * Lp[t + 2], s3 += a3 * Lp[t + 3];
        s4 += a4 * Lp[t + 4], s5 += a5 * Lp[t + 5], s6 += a6 * Lp[t + 6], s7 += a7 * Lp[t + 7];
      }
      if (t < j) s0 += col[0] * Lp[t];
      if (t + 1 < j) s1 += col[ldn] * Lp[t + 1];
      if (t + 2 < j) s2 += col[2 * ldn] * Lp[t + 2];
      if (t + 3 < j) s3 += col[3 * ldn] * Lp[t + 3];
      if (t + 4 < j) s4 += col[4 * ldn] * Lp[t + 4];
      if (t + 5 < j) s5 += col[5 * ldn] * Lp[t + 5];
      if (t + 6 < j) s6 += col[6 * ldn] * Lp[t + 6];
      const double dot = ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7));
      li = (kv - dot) / sq;
      di = d[i] - li * li;
    }
    Lt[(long)j * ldn + i] = li;
    d[i] = di;
    sel_take(bv, bi, di, i);
  }
  sel_block_best(bv, bi, rv, ri);
  if (tid == 0) pout[blockIdx.x].v = bv, pout[blockIdx.x].i = bi;
}

// trace[0] = sum_{i < N} d_i: one workgroup, every thread its elements i = tid, tid + 256, .. in that order, then a
// fixed tree; U[jj] = X[piv[jj]] for jj < m = state[0] (U == nullptr: no gather)
__global__ __launch_bounds__(256) void select_final_kernel(const double *__restrict__ X, long N, int D,
                                                           const double *__restrict__ d, const long long *__restrict__ piv,
                                                           const long long *__restrict__ state, double *__restrict__ trace,
                                                           double *__restrict__ U) {
  __shared__ double red[4];
  double t = 0.0;
  for (long i = threadIdx.x; i < N; i += 256) t += d[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) trace[0] = (red[0] + red[1]) + (red[2] + red[3]);
  if (!U) return;
  const long md = (long)state[0] * D;
  for (long e = threadIdx.x; e < md; e += 256) {
    const long jj = e / D, q = e - jj * D;
    U[e] = X[piv[jj] * D + q];
  }
}

int select_blocks(int64_t N, int max_blocks) {
  const int64_t nb = std::max<int64_t>(1, std::min<int64_t>((N + 255) / 256, SELECT_BLOCKS_MAX));
  return (int)(max_blocks > 0 && max_blocks < nb ? max_blocks : nb);
}

size_t select_layout(char *base, int64_t N, int64_t M, int ndim, SelectBufs *b) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char *q = base ? base + off : nullptr;
    off += (bytes + 255) / 256 * 256;
    return q;
  };
  const int64_t ldn = (N + 255) / 256 * 256;
  b->ldn = ldn;
  b->d = reinterpret_cast<double *>(take((size_t)ldn * sizeof(double)));
  b->part = reinterpret_cast<SelPair *>(take(2 * (size_t)SELECT_BLOCKS_MAX * sizeof(SelPair)));
  b->piv = reinterpret_cast<long long *>(take((size_t)M * sizeof(long long)));
  b->pv = reinterpret_cast<double *>(take((size_t)M * sizeof(double)));
  b->state = reinterpret_cast<long long *>(take(sizeof(long long)));
  b->trace = reinterpret_cast<double *>(take(sizeof(double)));
  b->U = reinterpret_cast<double *>(take((size_t)M * ndim * sizeof(double)));
  b->sel = reinterpret_cast<unsigned char *>(take((size_t)ldn));
  return off;
}

void launch_select_init(hipStream_t s, const DevParams *p, const double *X, int64_t N, int blocks, const double *d0,
                        const SelectBufs &b) {
  GOGP_KLAUNCH(select_init_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p, X, (long)N, d0, b.d, b.sel, b.part);
}

void launch_select_step(hipStream_t s, const DevParams *p, int ndim, const double *X, int64_t N, int blocks, int j,
                        double tol, const SelectBufs &b) {
  const SelPair *pin = b.part + (size_t)(j & 1) * SELECT_BLOCKS_MAX;
  SelPair *pout = b.part + (size_t)((j + 1) & 1) * SELECT_BLOCKS_MAX;
  const size_t lds = (size_t)(j + ndim) * sizeof(double);  // j <= 4095, ndim <= 64: within 64 KiB
  GOGP_KLAUNCH(select_step_kernel, dim3((unsigned)blocks), dim3(256), lds, s, p, X, (long)N, b.Lt, (long)b.ldn, j, tol, b.d,
               b.sel, pin, pout, b.piv, b.pv, b.state);
}

void launch_select_final(hipStream_t s, const double *X, int64_t N, int ndim, const SelectBufs &b, bool gather) {
  GOGP_KLAUNCH(select_final_kernel, dim3(1), dim3(256), 0, s, X, (long)N, ndim, (const double *)b.d,
               (const long long *)b.piv, (const long long *)b.state, b.trace, gather ? b.U : nullptr);
}

hipError_t select_run(hipStream_t s, const DevParams *p, int ndim, const double *X, int64_t N, int64_t M, double tol,
                      int max_blocks, const double *d0, const SelectBufs &b, int64_t *m_out) {
  const int blocks = select_blocks(N, max_blocks);
  const int64_t steps = std::min(M, N);  // a step beyond N finds every row selected and stops
  hipError_t e = hipMemsetAsync(b.piv, 0xff, (size_t)M * sizeof(long long), s);  // -1: no pivot recorded
  if (e == hipSuccess) e = hipMemsetAsync(b.state, 0, sizeof(long long), s);
  if (e != hipSuccess) return e;
  launch_select_init(s, p, X, N, blocks, d0, b);
  long long taken = 0;
  for (int64_t j = 0; j < steps; ++j) {
    launch_select_step(s, p, ndim, X, N, blocks, (int)j, tol, b);
    if ((j + 1) % SELECT_SYNC_STEPS == 0 && j + 1 < steps) {
      e = hipMemcpyAsync(&taken, b.state, sizeof taken, hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) return e;
      if (taken < j + 1) break;  // stopped: the remaining steps would return at once
    }
  }
  launch_select_final(s, X, N, ndim, b, true);
  e = hipMemcpyAsync(&taken, b.state, sizeof taken, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess) e = hipGetLastError();
  *m_out = taken;
  return e;
}

}  // namespace gogp
