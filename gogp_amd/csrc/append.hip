// append.hip -- the kernels of gogp_append (api.hip): m <= 64 observations join a factored process of n without a new
// factorisation.  No reference counterpart (the reference refactorises every step: tutorial/tutorial.go:118-142).
//
//   K = [K11 B^T; B C],  K11 = L11 L11^T  =>  L21 = B L11^-T = V^T,  S = C - V^T V,  L22 = chol(S),
//   z2 = L22^-1 (y2 - V^T z1).
// V = L11^-1 B^T comes from the persistent substitution kernel (trsm_small.hip), which leaves it in its workspace in
// the layout of the kernel instance that ran (common.h: TsSolution).  Two kernels follow it:
//   append_gram_kernel    one workgroup per 256 rows of V: its part of V^T V on v_mfma_f64_16x16x4_f64 (wave w owns
//                         tile row w, the tiles left of and on the diagonal), its part of V^T z, and its columns of
//                         the new factor rows (the transpose of V).  A workgroup sums its own rows in index order and
//                         writes to a slot of its own: nothing depends on the order the workgroups run in.
//   append_commit_kernel  one workgroup: the parts summed in slab order, S = C - sum with C from kern_eval.h, the
//                         Cholesky factor of S in LDS (pivot criterion !(d > 0), as pivot16.h), z2, and -- only when S
//                         was positive definite -- L22 and z2 written out.
#include "kern_eval.h"

namespace gogp {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// row stride of the staged rows of V in LDS (doubles): 640 B, half a turn of the 64 banks, so that the two k-quads a
// half-wave reads (16 lanes x 8 B each) fall on disjoint banks
constexpr int AG_LD = 80;
constexpr int AC_LD = 65;

struct GramArgs {
  TsSolution v[2];
  int m0, m;
  long npc, n;
  const double *z;
  double *part;
  double *Lnew;
  long ld;
};

__device__ __forceinline__ double sol_at(const TsSolution &s, long k, int j) {
  if (s.kind == TS_SOL_PAIRED) return static_cast<const double *>(s.p)[((k >> 1) * s.width + j) * 2 + (k & 1)];
  if (s.kind == TS_SOL_COMPACT) return static_cast<const double *>(s.p)[k * s.width + j];
  if (s.kind == TS_SOL_ROWS) return static_cast<const double *>(s.p)[(long)j * s.width + k];
  const u32x4 g = static_cast<const u32x4 *>(s.p)[k];
  return __hiloint2double((int)g.w, (int)g.y);
}

}  // namespace

// (two workgroups per compute unit: with a budget of 256 registers hipcc keeps the MFMA accumulators in VGPRs)
__global__ __launch_bounds__(256, 2) void append_gram_kernel(GramArgs g) {
  __shared__ double Vs[64 * AG_LD];
  __shared__ double zs[64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fk = lane >> 4;
  const int slab = blockIdx.x;
  const int nt = (g.m + 15) >> 4;
  f64x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = (f64x4){0.0, 0.0, 0.0, 0.0};
  double dot = 0.0;
  for (int sub = 0; sub < 4; ++sub) {
    const long k0 = (long)slab * PANEL + sub * 64;  // k0 + 63 < npc: the grid is npc / 256 workgroups
    __syncthreads();  // everybody is done with the previous 64 rows
    for (int idx = tid; idx < 64 * 64; idx += 256) {
      const int j = idx & 63, k = idx >> 6;
      double x = 0.0;
      if (j < g.m) x = (j < g.m0) ? sol_at(g.v[0], k0 + k, j) : sol_at(g.v[1], k0 + k, j - g.m0);
      Vs[k * AG_LD + j] = x;
    }
    if (tid < 64) zs[tid] = g.z[k0 + tid];
    __syncthreads();
    // the new factor rows: L21[j][k] = V[k][j], the lanes along k (consecutive addresses of a row of L)
    for (int idx = tid; idx < 64 * g.m; idx += 256) {
      const int j = idx >> 6, k = idx & 63;
      if (k0 + k < g.n) g.Lnew[(long)j * g.ld + k0 + k] = Vs[k * AG_LD + j];
    }
    if (w < nt) {
      for (int ks = 0; ks < 16; ++ks) {
        const int k = 4 * ks + fk;
        const double a = Vs[k * AG_LD + 16 * w + fr];
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) {
          if (tj <= w) {
            const double b = Vs[k * AG_LD + 16 * tj + fr];
            acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[tj], 0, 0, 0);
          }
        }
      }
    }
    if (tid < 64) {
      for (int k = 0; k < 64; ++k) dot = fma(Vs[k * AG_LD + tid], zs[k], dot);
    }
  }
  double *P = g.part + (long)slab * APPEND_PART;
  if (w < nt) {
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
      if (tj <= w) {
#pragma unroll
        for (int v = 0; v < 4; ++v) P[(16 * w + fk + 4 * v) * 64 + 16 * tj + fr] = acc[tj][v];
      }
    }
  }
  if (tid < 64) P[64 * 64 + tid] = dot;
}

template <bool EV>
__global__ __launch_bounds__(256) void append_commit_kernel(const DevParams *__restrict__ Pp, const double *__restrict__ X2,
                                                            const double *__restrict__ y2, int m, long n,
                                                            const double *__restrict__ part, int nslab,
                                                            double *__restrict__ Lnew, long ld, double *__restrict__ z2out,
                                                            long long *info) {
  __shared__ double S[64 * AC_LD];
  __shared__ double r[64];
  __shared__ int bad_s;
  const DevParams &P = *Pp;
  const int D = P.ndim;
  const int tid = threadIdx.x;
  for (int idx = tid; idx < 64 * 64; idx += 256) {
    const int i = idx >> 6, j = idx & 63;
    if (i < m && j <= i) {
      double s = 0.0;
      for (int q = 0; q < nslab; ++q) s += part[(long)q * APPEND_PART + i * 64 + j];
      const double *xi = X2 + (long)i * D, *xj = X2 + (long)j * D;
      double c = simil_value(
          P, [&](int d) { return xi[d]; }, [&](int d) { return xj[d]; });
      if (EV) c *= event_discount(P, event_mask(P, xi[P.ev_axis]), event_mask(P, xj[P.ev_axis]));
      if (i == j) c += P.noise_var;
      S[i * AC_LD + j] = c - s;
    }
  }
  if (tid < m) {
    double s = 0.0;
    for (int q = 0; q < nslab; ++q) s += part[(long)q * APPEND_PART + 64 * 64 + tid];
    r[tid] = y2[tid] - s;
  }
  if (tid == 0) bad_s = 64;
  __syncthreads();
  // right-looking Cholesky of S (m <= 64) in LDS
  for (int j = 0; j < m; ++j) {
    const double d = S[j * AC_LD + j];
    if (tid == 0 && !(d > 0.0) && bad_s == 64) bad_s = j;
    const double l = sqrt(d);
    __syncthreads();  // everybody has read the pivot
    if (tid == 0) S[j * AC_LD + j] = l;
    if (tid > j && tid < m) S[tid * AC_LD + j] /= l;
    __syncthreads();
    const int t = m - j - 1;
    for (int idx = tid; idx < t * t; idx += 256) {
      const int ii = idx / t, cc = idx - ii * t;
      if (cc <= ii) {
        const int i = j + 1 + ii, c = j + 1 + cc;
        S[i * AC_LD + c] = fma(-S[i * AC_LD + j], S[c * AC_LD + j], S[i * AC_LD + c]);
      }
    }
    __syncthreads();
  }
  if (bad_s < 64) {  // workgroup-uniform: nothing of the failed block is written
    if (tid == 0 && *info == 0) *info = (long long)(n + bad_s + 1);
    return;
  }
  for (int j = 0; j < m; ++j) {
    if (tid == 0) r[j] = r[j] / S[j * AC_LD + j];
    __syncthreads();
    if (tid > j && tid < m) r[tid] = fma(-S[tid * AC_LD + j], r[j], r[tid]);
    __syncthreads();
  }
  for (int idx = tid; idx < m * m; idx += 256) {
    const int i = idx / m, j = idx - i * m;
    Lnew[(long)i * ld + n + j] = (j <= i) ? S[i * AC_LD + j] : 0.0;
  }
  if (tid < m) z2out[tid] = r[tid];
}

__global__ __launch_bounds__(256) void append_identity_rows_kernel(double *__restrict__ L, long ld, long r0, long ncols) {
  const long r = r0 + blockIdx.x;
  for (long c = threadIdx.x; c < ncols; c += 256) L[r * ld + c] = (c == r) ? 1.0 : 0.0;
}

__global__ __launch_bounds__(256) void append_restride_kernel(const double *__restrict__ src, long ld0, long npad0,
                                                              double *__restrict__ dst, long ld1) {
  const long i = blockIdx.x;
  const long ce = (i | (PANEL - 1)) + 1;  // the end of row i's diagonal 256-block: <= npad1 <= ld1; <= npad0 for i < npad0
  if (i < npad0) {
    for (long c = threadIdx.x; c < ce; c += 256) dst[i * ld1 + c] = src[i * ld0 + c];
  } else {
    for (long c = threadIdx.x; c < ce; c += 256) dst[i * ld1 + c] = (c == i) ? 1.0 : 0.0;
  }
}

void launch_append_gram(hipStream_t s, TsSolution v0, TsSolution v1, int m0, int m, int64_t npc, int64_t n,
                        const double *z, double *part, double *Lnew, int64_t ld) {
  GramArgs g;
  g.v[0] = v0;
  g.v[1] = v1;
  g.m0 = m0;
  g.m = m;
  g.npc = (long)npc;
  g.n = (long)n;
  g.z = z;
  g.part = part;
  g.Lnew = Lnew;
  g.ld = (long)ld;
  GOGP_KLAUNCH(append_gram_kernel, dim3((unsigned)(npc / PANEL)), dim3(256), 0, s, g);
}

void launch_append_commit(hipStream_t s, const DevParams *p, const double *X2, const double *y2, int m, int64_t n,
                          const double *part, int nslab, double *Lnew, int64_t ld, double *z2out, long long *info,
                          bool ev) {
  if (ev)
    GOGP_KLAUNCH(append_commit_kernel<true>, dim3(1), dim3(256), 0, s, p, X2, y2, m, (long)n, part, nslab, Lnew, (long)ld,
                 z2out, info);
  else
    GOGP_KLAUNCH(append_commit_kernel<false>, dim3(1), dim3(256), 0, s, p, X2, y2, m, (long)n, part, nslab, Lnew, (long)ld,
                 z2out, info);
}

void launch_append_identity_rows(hipStream_t s, double *L, int64_t ld, int64_t r0, int64_t r1, int64_t ncols) {
  if (r1 <= r0) return;
  GOGP_KLAUNCH(append_identity_rows_kernel, dim3((unsigned)(r1 - r0)), dim3(256), 0, s, L, (long)ld, (long)r0, (long)ncols);
}

void launch_append_restride(hipStream_t s, const double *src, int64_t ld0, int64_t npad0, double *dst, int64_t ld1,
                            int64_t npad1) {
  GOGP_KLAUNCH(append_restride_kernel, dim3((unsigned)npad1), dim3(256), 0, s, src, (long)ld0, (long)npad0, dst, (long)ld1);
}

}  // namespace gogp
