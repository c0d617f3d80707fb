// remove.hip -- the kernels of gogp_remove (api.hip): the observations S = {s_1 < ... < s_m} leave a factored process of n
// without a new factorisation.  No reference counterpart (the reference refactorises every step: tutorial/tutorial.go:118-142).
//
//   L[kept, :] L[kept, :]^T = K[kept, kept]  and  Lt = L[kept, kept] is lower triangular with a positive diagonal, so
//   K[kept, kept] = Lt Lt^T + W W^T,  W = L[kept, S]:  a gather and a rank-m UPDATE (a sum, never a downdate).
// The update is a sequence of Householder reflectors from the right on [Lt | W], one per column k, acting on
// (l_kk, w_k1 .. w_km) -- orthogonal, hence backward stable -- that annihilate row k of W:
//   ss = |w_k|^2,  r = +sqrt(l_kk^2 + ss),  v0 = -ss / (l_kk + r)   (Parlett: no cancellation, l_kk > 0),
//   u = w_k / v0,  tau = -v0 / r;   row i > k:  t = tau (l_ik + u . w_i),  l_ik -= t,  w_i -= t u;   l_kk = r.
// ss == 0 exactly is the identity (tau = 0): the columns left of the first removed index, the padding, the zero tops
// of the columns of W.
//   remove_gather_kernel   Lt at the final leading dimension from the old factor (one workgroup per new row; identity
//                          padding; the old factor is only read), through the map new index -> old index
//   remove_rows_kernel     the same map on the rows of X and on y
//   remove_w_kernel        up to REMOVE_W columns of W, column-major, zero above each column's first affected row
//   remove_snap_kernel     the diagonal 128-blocks of Lt before a pass (a block step reads its block from this copy:
//                          the workgroup that writes the new block back races with nobody)
//   remove_block_kernel<MW> one 128-column step: every workgroup regenerates the block's 128 reflectors in LDS from the
//                          snapshot and the block's rows of W (redundant, identical in every workgroup); workgroup 0
//                          writes the new diagonal block, workgroup g > 0 applies the reflectors to its 256 rows below:
//                          a thread owns one row and keeps its w (MW doubles) in registers, reads u as LDS broadcasts,
//                          and the factor entries of its row pass through an LDS tile 8 columns at a time so that
//                          the global traffic stays row-contiguous.
// m > MW goes in passes, each against the factor the previous one left (Lt Lt^T + W1 W1^T + W2 W2^T is a sum).
// Every sum runs in index order inside one thread: no atomics, the same bits on every run.
#include "common.h"

namespace gogp {

namespace {
constexpr int RB = 128;       // columns per step
constexpr int RCH = 8;        // columns staged per LDS tile
constexpr int RLD = RCH + 1;  // its row stride (doubles): 32 consecutive rows fall on 32 distinct even banks
}  // namespace

__global__ __launch_bounds__(256) void remove_gather_kernel(const double *__restrict__ src, long ld0,
                                                            const int *__restrict__ map, long n1, double *__restrict__ dst,
                                                            long ld1) {
  const long i = blockIdx.x;
  const long ce = (i | (PANEL - 1)) + 1;  // the end of row i's diagonal 256-block: <= npad1 = ld1
  if (i < n1) {
    const double *row = src + (long)map[i] * ld0;
    for (long c = threadIdx.x; c < ce; c += 256) dst[i * ld1 + c] = (c <= i) ? row[map[c]] : 0.0;
  } else {
    for (long c = threadIdx.x; c < ce; c += 256) dst[i * ld1 + c] = (c == i) ? 1.0 : 0.0;
  }
}

__global__ __launch_bounds__(256) void remove_rows_kernel(const double *__restrict__ src, const int *__restrict__ map, long n1,
                                                          int width, double *__restrict__ dst) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n1 * width) return;
  const long i = idx / width;
  const int d = (int)(idx - i * width);
  dst[idx] = src[(long)map[i] * width + d];
}

// W[j][i] = L[map[i]][rem[j]] for j < mc, rows r0 <= i < npad1 (zero: i >= n1, rem[j] > map[i], mc <= j < mw)
__global__ __launch_bounds__(256) void remove_w_kernel(const double *__restrict__ src, long ld0, const int *__restrict__ map,
                                                       const int *__restrict__ rem, int mc, int mw, long r0, long n1,
                                                       long npad1, double *__restrict__ W) {
  const long i = r0 + (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= npad1) return;
  const long oi = (i < n1) ? map[i] : -1;
  for (int j = 0; j < mw; ++j) {
    double v = 0.0;
    if (j < mc && rem[j] < oi) v = src[oi * ld0 + rem[j]];
    W[(long)j * npad1 + i] = v;
  }
}

// snap[b] (128 x 128) = the diagonal block of L at row / column 128 (b0 + b)
__global__ __launch_bounds__(256) void remove_snap_kernel(const double *__restrict__ L, long ld, int b0, double *__restrict__ snap) {
  const long k0 = (long)(b0 + blockIdx.x) * RB;
  double *out = snap + (long)(b0 + blockIdx.x) * RB * RB;
  for (int idx = threadIdx.x; idx < RB * RB; idx += 256) {
    const int c = idx >> 7, r = idx & 127;  // column-major: the thread that owns row r reads a column with its neighbours
    out[idx] = (c <= r) ? L[(k0 + r) * ld + k0 + c] : 0.0;
  }
}

template <int MW>
__global__ __launch_bounds__(256) void remove_block_kernel(double *__restrict__ L, long ld, const double *__restrict__ snap,
                                                           double *__restrict__ W, long ldw, long kb, long n1) {
  __shared__ double U[RB * MW];
  __shared__ double tau[RB];
  __shared__ double Ls[256 * RLD];
  const int t = threadIdx.x;
  const int g = blockIdx.x;
  double w[MW];
  // ---- the block's reflectors: thread t < 128 owns row kb + t of [Lt | W] -------------------------------------------
  {
    const long i = kb + t;  // < npad1 = ldw for t < 128
#pragma unroll
    for (int j = 0; j < MW; ++j) w[j] = (t < RB) ? W[(long)j * ldw + i] : 0.0;
  }
  const double *D = snap + (kb / RB) * (long)(RB * RB);
  // the row's entries of the diagonal block, RCH columns at a time in registers, the next ones on their way meanwhile
  double ac[RCH], an[RCH];
#pragma unroll
  for (int kk = 0; kk < RCH; ++kk) ac[kk] = (t < RB) ? D[kk * RB + t] : 0.0;
  for (int c0 = 0; c0 < RB; c0 += RCH) {
#pragma unroll
    for (int kk = 0; kk < RCH; ++kk) an[kk] = (t < RB && c0 + RCH < RB) ? D[(c0 + RCH + kk) * RB + t] : 0.0;
#pragma unroll
    for (int kk = 0; kk < RCH; ++kk) {
      const int k = c0 + kk;
      if (t == k) {
        double ss = 0.0;
#pragma unroll
        for (int j = 0; j < MW; ++j) ss = fma(w[j], w[j], ss);
        double tk = 0.0;
        if (ss != 0.0) {
          const double a = ac[kk];
          const double r = sqrt(fma(a, a, ss));
          const double v0 = -ss / (a + r);
          const double iv = 1.0 / v0;
          tk = -v0 / r;
          ac[kk] = r;
#pragma unroll
          for (int j = 0; j < MW; ++j) U[k * MW + j] = w[j] * iv;
        } else {
#pragma unroll
          for (int j = 0; j < MW; ++j) U[k * MW + j] = 0.0;
        }
        tau[k] = tk;
      }
      __syncthreads();
      const double tk = tau[k];  // workgroup-uniform
      if (tk != 0.0 && t > k && t < RB) {
        double s = ac[kk];
#pragma unroll
        for (int j = 0; j < MW; ++j) s = fma(U[k * MW + j], w[j], s);
        s *= tk;
        ac[kk] -= s;
#pragma unroll
        for (int j = 0; j < MW; ++j) w[j] = fma(-s, U[k * MW + j], w[j]);
      }
    }
    if (g == 0 && t < RB) {  // the new diagonal block (its rows of W are zero from here on and are not read again)
#pragma unroll
      for (int kk = 0; kk < RCH; ++kk)
        if (c0 + kk <= t) L[(kb + t) * ld + kb + c0 + kk] = ac[kk];
    }
#pragma unroll
    for (int kk = 0; kk < RCH; ++kk) ac[kk] = an[kk];
  }
  if (g == 0) return;
  // ---- the rows below: thread t owns row i ---------------------------------------------------------------------------
  const long i0 = kb + RB + (long)(g - 1) * 256;
  const long i = i0 + t;
  const bool live = i < n1;
#pragma unroll
  for (int j = 0; j < MW; ++j) w[j] = live ? W[(long)j * ldw + i] : 0.0;
  // the tile's next RCH columns are on their way (in registers) while the current ones are worked on
  const int pr = t / RCH, pc = t - pr * RCH;  // element q of this thread: row pr + q * (256 / RCH), column pc
  double pre[RCH];
#pragma unroll
  for (int q = 0; q < RCH; ++q) {
    const long r = i0 + pr + q * (256 / RCH);
    pre[q] = (r < n1) ? L[r * ld + kb + pc] : 0.0;
  }
  for (int c0 = 0; c0 < RB; c0 += RCH) {
    __syncthreads();  // the previous tile has been written back (the first: the reflectors are complete)
#pragma unroll
    for (int q = 0; q < RCH; ++q) Ls[(pr + q * (256 / RCH)) * RLD + pc] = pre[q];
    __syncthreads();
    if (c0 + RCH < RB) {
#pragma unroll
      for (int q = 0; q < RCH; ++q) {
        const long r = i0 + pr + q * (256 / RCH);
        pre[q] = (r < n1) ? L[r * ld + kb + c0 + RCH + pc] : 0.0;
      }
    }
    for (int kk = 0; kk < RCH; ++kk) {
      const int k = c0 + kk;
      const double tk = tau[k];
      if (tk != 0.0) {
        double s = Ls[t * RLD + kk];
#pragma unroll
        for (int j = 0; j < MW; ++j) s = fma(U[k * MW + j], w[j], s);
        s *= tk;
        Ls[t * RLD + kk] -= s;
#pragma unroll
        for (int j = 0; j < MW; ++j) w[j] = fma(-s, U[k * MW + j], w[j]);
      }
    }
    __syncthreads();
    for (int idx = t; idx < 256 * RCH; idx += 256) {
      const int r = idx / RCH, c = idx - r * RCH;
      if (i0 + r < n1) L[(i0 + r) * ld + kb + c0 + c] = Ls[r * RLD + c];
    }
  }
  if (live) {
#pragma unroll
    for (int j = 0; j < MW; ++j) W[(long)j * ldw + i] = w[j];
  }
}

void launch_remove_gather(hipStream_t s, const double *src, int64_t ld0, const int *map, int64_t n1, double *dst,
                          int64_t npad1) {
  GOGP_KLAUNCH(remove_gather_kernel, dim3((unsigned)npad1), dim3(256), 0, s, src, (long)ld0, map, (long)n1, dst, (long)npad1);
}

void launch_remove_rows(hipStream_t s, const double *src, const int *map, int64_t n1, int width, double *dst) {
  if (n1 * width <= 0) return;
  GOGP_KLAUNCH(remove_rows_kernel, dim3((unsigned)((n1 * width + 255) / 256)), dim3(256), 0, s, src, map, (long)n1, width, dst);
}

void launch_remove_w(hipStream_t s, const double *src, int64_t ld0, const int *map, const int *rem, int mc, int mw, int64_t r0,
                     int64_t n1, int64_t npad1, double *W) {
  GOGP_KLAUNCH(remove_w_kernel, dim3((unsigned)((npad1 - r0 + 255) / 256)), dim3(256), 0, s, src, (long)ld0, map, rem, mc, mw,
               (long)r0, (long)n1, (long)npad1, W);
}

void launch_remove_snap(hipStream_t s, const double *L, int64_t ld, int b0, int nb, double *snap) {
  if (nb <= 0) return;
  GOGP_KLAUNCH(remove_snap_kernel, dim3((unsigned)nb), dim3(256), 0, s, L, (long)ld, b0, snap);
}

void launch_remove_block(hipStream_t s, double *L, int64_t ld, const double *snap, double *W, int mw, int64_t kb, int64_t n1) {
  const int64_t below = n1 - (kb + RB);
  const unsigned grid = 1u + (below > 0 ? (unsigned)((below + 255) / 256) : 0u);
  if (mw == REMOVE_W_SMALL)
    GOGP_KLAUNCH(remove_block_kernel<REMOVE_W_SMALL>, dim3(grid), dim3(256), 0, s, L, (long)ld, snap, W, (long)ld, (long)kb,
                 (long)n1);
  else
    GOGP_KLAUNCH(remove_block_kernel<REMOVE_W>, dim3(grid), dim3(256), 0, s, L, (long)ld, snap, W, (long)ld, (long)kb,
                 (long)n1);
}

}  // namespace gogp
