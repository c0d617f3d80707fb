// pcov.hip -- the joint predictive covariance at the test points (gogp_produce_covariance, gogp_produce_samples).
//
// No reference counterpart: gp.GP.Produce forms Kstar^T K^-1 Kstar in full (gp/gp.go:341-342) and keeps its diagonal
// (:356).  Produce's forward substitution leaves V^T = Kstar^T L^-T in Vt, one test point per row (api.hip:
// produce_solve_t); the covariance is  cov[i][j] = k(z_i, z_j) - V_i . V_j : one product Vt Vt^T with a small output
// (m x m) and a long K (npad).  Two device parts:
//   1. pcov_syrk_kernel: split-K SYRK on v_mfma_f64_16x16x4_f64.  Workgroup (pair, slab) forms the 64 x 64 tile of the
//      lower-triangle tile pair `pair` over the columns of its slab and writes it to a slot of its own.
//   2. pcov_final_kernel (_ev: with event discounts): sums the slabs in slab order -- no atomics --, subtracts them from
//      k(z_i, z_j) and writes cov[i][j] and cov[j][i] from the same value.
#ifndef GOGP_EV  // first pass: the whole file, the kernels without event discounts
#include <algorithm>

#include "kern_eval.h"

#define GOGP_EV 0
#define GOGP_EVN(name) name
namespace gogp {

typedef double pc_f64x4 __attribute__((ext_vector_type(4)));
// k-chunk in LDS and its row stride: with 36 doubles a fragment read (16 rows x 4 k, 512 bytes) spreads evenly over the
// banks -- two passes, the minimum for 64 lanes of 8 bytes
constexpr int PC_KC = 32, PC_AS = PC_KC + 4;

// tile pair p = ti (ti + 1) / 2 + tj, tj <= ti
__device__ __forceinline__ void pcov_pair(int p, int &ti, int &tj) {
  int t = (int)((sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);
  while ((t + 1) * (t + 2) / 2 <= p) ++t;
  while (t * (t + 1) / 2 > p) --t;
  ti = t;
  tj = p - t * (t + 1) / 2;
}

// part[slab][pair][64][64] = V[ti rows, slab columns] V[tj rows, slab columns]^T.  V: row-major, one test point per row,
// contiguous along k.  Rows >= m and columns beyond the slab (or ncols) are masked, not assumed zero.  Both operands go
// through LDS in chunks of PC_KC columns (thread: row tid >> 2, 8 consecutive k: 64 contiguous bytes), a diagonal pair
// loads one.  Wave w owns rows 16 w .. 16 w + 15 of the tile: one A fragment and four B fragments per 4 k.  The next
// chunk's loads are in flight behind the MFMAs of the current one.  grid: (pairs, slabs).
__global__ __launch_bounds__(256, 2) void pcov_syrk_kernel(const double *__restrict__ V, long ld, long m, long ncols, int cps,
                                                           double *__restrict__ part) {
  __shared__ double As[64 * PC_AS], Bs[64 * PC_AS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int ti, tj;
  pcov_pair((int)blockIdx.x, ti, tj);
  const bool diag = ti == tj;
  const long kb = (long)blockIdx.y * cps, ke = min(kb + (long)cps, ncols);
  const int ar = tid >> 2, ak = (tid & 3) * 8;
  const long rowa = (long)ti * 64 + ar, rowb = (long)tj * 64 + ar;
  const bool oka = rowa < m, okb = !diag && rowb < m;
  const double *pa = V + (oka ? rowa : 0) * ld + ak, *pb = V + (okb ? rowb : 0) * ld + ak;
  double ra[8], rb[8];
  auto gload1 = [&](const double *p, bool ok, long k0, double *r) {
    if (ok && k0 + ak + 8 <= ke) {
      const double2 *q = reinterpret_cast<const double2 *>(p + k0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double2 v = q[i];
        r[2 * i] = v.x;
        r[2 * i + 1] = v.y;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) r[i] = (ok && k0 + ak + i < ke) ? p[k0 + i] : 0.0;
    }
  };
  auto gload = [&](long k0) {
    gload1(pa, oka, k0, ra);
    if (!diag) gload1(pb, okb, k0, rb);
  };
  pc_f64x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = (pc_f64x4){0.0, 0.0, 0.0, 0.0};
  const int fr = lane & 15, fk = lane >> 4;
  const double *Bsrc = diag ? As : Bs;
  if (kb < ke) gload(kb);
  for (long k0 = kb; k0 < ke; k0 += PC_KC) {
    __syncthreads();  // the previous chunk's readers are done
#pragma unroll
    for (int i = 0; i < 8; ++i) As[ar * PC_AS + ak + i] = ra[i];
    if (!diag) {
#pragma unroll
      for (int i = 0; i < 8; ++i) Bs[ar * PC_AS + ak + i] = rb[i];
    }
    __syncthreads();
    if (k0 + PC_KC < ke) gload(k0 + PC_KC);
#pragma unroll
    for (int kk = 0; kk < PC_KC / 4; ++kk) {
      const double a = As[(16 * w + fr) * PC_AS + 4 * kk + fk];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bsrc[(16 * t + fr) * PC_AS + 4 * kk + fk], acc[t], 0, 0, 0);
    }
  }
  // C fragment: column = lane & 15, row = (lane >> 4) + 4 v
  double *slot = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 4096;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int v = 0; v < 4; ++v) slot[(16 * w + fk + 4 * v) * 64 + 16 * t + fr] = acc[t][v];
}

// samples[s][j] = mu[j] + G[s][j]  (G: ldg doubles per row, samples compact ns x m)
__global__ __launch_bounds__(256) void pcov_add_mu_kernel(const double *__restrict__ G, long ldg,
                                                          const double *__restrict__ mu, long ns, long m,
                                                          double *__restrict__ out) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ns * m) return;
  const long s = idx / m, j = idx - s * m;
  out[idx] = mu[j] + G[s * ldg + j];
}
#endif

// Rows 4 y .. 4 y + 3 (y = blockIdx.y) of tile pair (ti, tj) of out (mo x mo, ldo doubles per row; mo >= m), one element
// per thread: for i, j < m
//     out[i][j] = out[j][i] = k(z_i, z_j) - sum over the slabs, in slab order, of part[slab][pair][i][j]  (+ diag_add, i == j)
// and rows / columns m .. mo - 1 are those of the identity (the padding of the factorisation of gogp_produce_samples).
// The value is formed once, for i >= j, and stored to both places.  The slabs' values are fetched eight at a time and
// added in slab order: with few test points one tile pair has npad / 256 slabs, and 16 workgroups per pair with
// independent loads in flight keep that sum from costing more than the product.  nslab == 0 (no observations): the
// prior Gram matrix.  GOGP_EV = 1 (pcov_final_kernel_ev): k carries the pair's event discount.  No noise term.
// grid: (the lower tile pairs of mo, 16).
__global__ __launch_bounds__(256) void GOGP_EVN(pcov_final_kernel)(const DevParams *__restrict__ Pp,
                                                                   const double *__restrict__ Z, long m,
                                                                   const double *__restrict__ part, int nslab,
                                                                   long npairs, double diag_add,
                                                                   double *__restrict__ out, long mo, long ldo) {
  const DevParams &P = *Pp;
  const int D = P.ndim;
  const int tid = threadIdx.x;
  int ti, tj;
  pcov_pair((int)blockIdx.x, ti, tj);
  const int r = 4 * (int)blockIdx.y + (tid >> 6), c = tid & 63;
  const long i = (long)ti * 64 + r, j = (long)tj * 64 + c;
  if (j > i || i >= mo) return;
  double v;
  if (i < m) {  // then j <= i < m
    const double *zi = Z + i * D, *zj = Z + j * D;
    v = simil_value(
        P, [&](int d) { return zi[d]; }, [&](int d) { return zj[d]; });
    if (GOGP_EV) v *= event_discount(P, event_mask(P, zi[P.ev_axis]), event_mask(P, zj[P.ev_axis]));
    const double *ps = part + (long)blockIdx.x * 4096 + r * 64 + c;
    const long ss = npairs * 4096;
    double q = 0.0;
    int sl = 0;
    for (; sl + 8 <= nslab; sl += 8) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = ps[(sl + u) * ss];
#pragma unroll
      for (int u = 0; u < 8; ++u) q += t[u];
    }
    for (; sl < nslab; ++sl) q += ps[sl * ss];
    v -= q;
    if (i == j) v += diag_add;
  } else {
    v = (i == j) ? 1.0 : 0.0;
  }
  out[i * ldo + j] = v;
  if (i != j) out[j * ldo + i] = v;
}

#if !GOGP_EV  // second pass: pcov_final_kernel again, with event discounts, as pcov_final_kernel_ev
#undef GOGP_EV
#undef GOGP_EVN
#define GOGP_EV 1
#define GOGP_EVN(name) name##_ev
#include "pcov.hip"
#undef GOGP_EV
#undef GOGP_EVN
#define GOGP_EV 0
#define GOGP_EVN(name) name

// Slabs of the columns of Vt: PCOV_WG_PER_CU workgroups per CU where the problem allows it, and a slab is a whole number
// of 256-column panels -- never shorter than 256 columns (8 chunks: below that a workgroup is all prologue).  Four per
// CU, not one: a workgroup is one wave per SIMD, whose MFMAs wait for its own LDS reads and barriers, and 136 tile pairs
// (m = 1024) x 2 slabs = 272 workgroups on 256 CUs left 16 CUs with twice the work (N = 16384: 857 us, measured).
constexpr int PCOV_WG_PER_CU = 4;
int pcov_slabs(int64_t npad, int64_t m, int ncu, int *cols_per_slab) {
  const int64_t tiles = (m + 63) / 64, pairs = tiles * (tiles + 1) / 2;
  const int64_t panels = std::max<int64_t>(1, npad / PANEL);
  int64_t nslab = std::min<int64_t>(panels, std::max<int64_t>(1, ((int64_t)PCOV_WG_PER_CU * ncu + pairs - 1) / pairs));
  const int64_t pps = (panels + nslab - 1) / nslab;
  nslab = (panels + pps - 1) / pps;
  if (cols_per_slab) *cols_per_slab = (int)(pps * PANEL);
  return (int)nslab;
}

void launch_pcov(hipStream_t s, const DevParams *p, const double *Z, int64_t m, const double *Vt, int64_t ld,
                 int64_t npad, int ncu, double *part, double diag_add, double *out, int64_t mo, int64_t ldo, bool ev) {
  const int64_t tiles = (m + 63) / 64, pairs = tiles * (tiles + 1) / 2;
  int nslab = 0, cps = 0;
  if (Vt && npad > 0) {
    nslab = pcov_slabs(npad, m, ncu, &cps);
    GOGP_KLAUNCH(pcov_syrk_kernel, dim3((unsigned)pairs, (unsigned)nslab), dim3(256), 0, s, Vt, (long)ld, (long)m,
                 (long)npad, cps, part);
  }
  const int64_t otiles = (mo + 63) / 64, opairs = otiles * (otiles + 1) / 2;
  if (ev)
    GOGP_KLAUNCH(pcov_final_kernel_ev, dim3((unsigned)opairs, 16), dim3(256), 0, s, p, Z, (long)m, part, nslab, (long)pairs,
                 diag_add, out, (long)mo, (long)ldo);
  else
    GOGP_KLAUNCH(pcov_final_kernel, dim3((unsigned)opairs, 16), dim3(256), 0, s, p, Z, (long)m, part, nslab, (long)pairs,
                 diag_add, out, (long)mo, (long)ldo);
}

void launch_pcov_add_mu(hipStream_t s, const double *G, int64_t ldg, const double *mu, int64_t ns, int64_t m, double *out) {
  if (ns <= 0 || m <= 0) return;
  GOGP_KLAUNCH(pcov_add_mu_kernel, dim3((unsigned)((ns * m + 255) / 256)), dim3(256), 0, s, G, (long)ldg, mu, (long)ns,
               (long)m, out);
}

}  // namespace gogp
#undef GOGP_EV
#undef GOGP_EVN
#endif
