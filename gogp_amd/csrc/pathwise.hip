// pathwise.hip -- pathwise posterior samples (gogp_pathwise_*; include/gogp_hip.h; DESIGN.md section 4, "Pathwise samples").
// No reference counterpart.  By Matheron's rule (Wilson et al. 2020) a posterior draw is a FUNCTION
//     f_s(z) = phi(z)^T w_s + k(z, X) v_s,      v_s = K^^-1 (y - Phi(X) w_s - eps_s),      phi_r(z) = amp_r cos(Omega_r . z + phase_r)
// fixed once (gogp_pathwise_create: the feature product at X, the residual columns, the handle's two substitutions) and then
// evaluated, and differentiated in z, at any number of points for O(N) each (gogp_pathwise_eval).
//
//   pw_feature_kernel<DG>   Out[s][i] = sum_r phi_r(z_i) W[r][s] (DG = 0) or its derivative in z_d for the DG dimensions from
//                           DG blockIdx.z (DG > 0): two chained products on v_mfma_f64_16x16x4_f64 with no LDS round trip
//                           between them.  Stage one forms the phases TRANSPOSED, Pt[r][i] = sum_d Omega[r][d] z_i[d] (A =
//                           Omega: lane (fr = lane & 15, fk = lane >> 4) holds Omega[r = fr][d = fk]; B = Z^T; K = ndim padded
//                           to 4): its C fragment leaves Pt[r = fk + 4 v][i = fr] in accumulator element v -- which is the A
//                           operand layout A[i = fr][k = fk] of stage two for the k-step over the features 4 v .. 4 v + 3.  So
//                           the lane adds the phase, takes amp cos (or -amp sin Omega[r][d]) of its four elements and issues
//                           them as the A operands of four k-steps of out[i][s] += phi[i][r] W[r][s], W from LDS as kmm_kernel
//                           stages V.  A wave takes 16 points, a workgroup 64 and a slab of 64-feature tiles.
//   pw_crossgrad_kernel<DG> G[s][i][d] = sum_j dk(z_i, x_j)/dz_d V[s][j] for the DG dimensions from DG blockIdx.z: kmm_kernel's
//                           tiling; per k-step a lane evaluates the radial derivative of its pair once (simil_xgrad_accum,
//                           the closed forms of pgrad.hip) and the DG A operands come out of it; DG x ceil(S / 16) accumulator
//                           fragments.
//   pw_finish_kernel        adds the slabs' partial sums of one or two products in slab order
//   pw_residual_kernel      the right-hand sides y - F_X[s] - sqrt(sigma^2 + v_i) Xi[s]
//
// Kernel boundaries are the only synchronisation: no atomics; the order of every sum depends on the sizes alone, never on
// S, so identical calls give identical bits and a column has the same bits alone as among 64.
#include <algorithm>
#include <string>

#include "api_internal.h"
#include "kern_eval.h"

namespace gogp {

typedef double pw_f64x4 __attribute__((ext_vector_type(4)));

// Workgroup (blockIdx.x, blockIdx.y): point tile, slab (feature tiles slab * tps ..).  Dynamic LDS:
// Zs[64][DS], Os[64][DS] (DS = (ndim rounded up to 4) | 1, zero from column ndim on), Ws[64][VS] (VS = 16 ng + 1), phases
// and amplitudes of the tile (amp = 0 from feature R on).  part: [slab][s][i] (DG = 0) or [slab][s][i][d].
template <int DG>
__global__ __launch_bounds__(256, 2) void pw_feature_kernel(const double *__restrict__ Om, const double *__restrict__ ph,
                                                           const double *__restrict__ am, int R, int D,
                                                           const double *__restrict__ Z, long m, const double *__restrict__ W,
                                                           int S, int tps, double *__restrict__ part) {
  extern __shared__ double sm[];
  constexpr int NQ = DG > 0 ? DG : 1;
  const int D4 = (D + 3) & ~3, DS = D4 | 1;
  const int ng = (S + 15) >> 4;  // column groups of 16 samples (uniform)
  const int VS = 16 * ng + 1;
  double *Zs = sm, *Os = Zs + 64 * DS, *Ws = Os + 64 * DS, *phs = Ws + 64 * VS, *ams = phs + 64;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const int dq = DG * (int)blockIdx.z;  // first dimension of this pass
  const int ftiles = (R + 63) >> 6;
  const int slab = blockIdx.y;
  const long rpad = (long)gridDim.x * 64;
  {
    const long r0 = (long)blockIdx.x * 64;
    for (int idx = tid; idx < 64 * D4; idx += 256) {
      const int r = idx / D4, d = idx - r * D4;
      Zs[r * DS + d] = (r0 + r < m && d < D) ? Z[(r0 + r) * D + d] : 0.0;
    }
    pw_f64x4 acc[NQ][4];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[q][g] = pw_f64x4{0.0, 0.0, 0.0, 0.0};
    const double *zrow = Zs + (16 * w + fr) * DS + fk;
    const int t1 = min(ftiles, (slab + 1) * tps);
    for (int ft = slab * tps; ft < t1; ++ft) {
      const int f0 = ft * 64;
      __syncthreads();  // the previous tile's reads of Os, Ws, phs, ams are done (and Zs is staged)
      for (int idx = tid; idx < 64 * D4; idx += 256) {
        const int r = idx / D4, d = idx - r * D4;
        Os[r * DS + d] = (f0 + r < R && d < D) ? Om[(long)(f0 + r) * D + d] : 0.0;
      }
      for (int idx = tid; idx < 64 * 16 * ng; idx += 256) {
        const int j = idx / (16 * ng), t = idx - j * (16 * ng);
        Ws[j * VS + t] = (t < S && f0 + j < R) ? W[(long)(f0 + j) * S + t] : 0.0;
      }
      if (tid < 64) {
        phs[tid] = (f0 + tid < R) ? ph[f0 + tid] : 0.0;
        ams[tid] = (f0 + tid < R) ? am[f0 + tid] : 0.0;
      }
      __syncthreads();
      for (int fb = 0; fb < 64; fb += 16) {
        // stage one: the lane's four phases Pt[feature fb + fk + 4 v][point 16 w + fr]
        pw_f64x4 p = {0.0, 0.0, 0.0, 0.0};
        const double *orow = Os + (fb + fr) * DS + fk;
        for (int d0 = 0; d0 < D4; d0 += 4) p = __builtin_amdgcn_mfma_f64_16x16x4f64(orow[d0], zrow[d0], p, 0, 0, 0);
        // stage two: k-step v covers the features fb + 4 v .. fb + 4 v + 3, the lane's own being fb + fk + 4 v
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int f = fb + fk + 4 * v;
          const double arg = p[v] + phs[f];
          const double *bp = Ws + f * VS + fr;
          double a[NQ];
          if (DG == 0) {
            a[0] = ams[f] * cos(arg);
          } else {
            const double base = -ams[f] * sin(arg);
#pragma unroll
            for (int q = 0; q < NQ; ++q) a[q] = (dq + q < D) ? base * Os[f * DS + dq + q] : 0.0;
          }
#pragma unroll
          for (int q = 0; q < NQ; ++q) {
            acc[q][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], bp[0], acc[q][0], 0, 0, 0);
            if (ng > 1) acc[q][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], bp[16], acc[q][1], 0, 0, 0);
            if (ng > 2) acc[q][2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], bp[32], acc[q][2], 0, 0, 0);
            if (ng > 3) acc[q][3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], bp[48], acc[q][3], 0, 0, 0);
          }
        }
      }
    }
    // C fragment: column (sample) = lane & 15, row (point) = (lane >> 4) + 4 v; padded rows and samples store nothing
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int t = 16 * g + fr;
      if (t >= S) continue;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const long i = r0 + 16 * w + fk + 4 * v;
        if (i >= m) continue;
        double *dst = part + ((long)slab * S + t) * rpad * (DG > 0 ? D : 1) + i * (DG > 0 ? D : 1);
#pragma unroll
        for (int q = 0; q < NQ; ++q)
          if (DG == 0 || dq + q < D) dst[DG > 0 ? dq + q : 0] = acc[q][g][v];
      }
    }
  }
}

// kmm_kernel's work split and staging (As: the Z tile, Bs: the X tile, both with the odd row stride DS = ndim | 1; Vs), with
// DG A operands per evaluated pair.  part: [slab][s][i][d].
template <int DG>
__global__ __launch_bounds__(256, 2) void pw_crossgrad_kernel(const DevParams *__restrict__ Pp, const double *__restrict__ Z,
                                                             long m, const double *__restrict__ X, long n,
                                                             const double *__restrict__ V, long ldv, int S, int tps,
                                                             double *__restrict__ part) {
  extern __shared__ double sm[];
  const DevParams &P = *Pp;
  const int D = P.ndim;
  const int DS = D | 1;
  const int ng = (S + 15) >> 4;
  const int VS = 16 * ng + 1;
  double *As = sm, *Bs = sm + 64 * DS, *Vs = Bs + 64 * DS;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const int dq = DG * (int)blockIdx.z;
  const long ctiles = (n + 63) >> 6;
  const int slab = blockIdx.y;
  const long rpad = (long)gridDim.x * 64;
  {
    const long r0 = (long)blockIdx.x * 64;
    for (int idx = tid; idx < 64 * D; idx += 256) {
      const int r = idx / D, d = idx - r * D;
      As[r * DS + d] = (r0 + r < m) ? Z[(r0 + r) * D + d] : 0.0;
    }
    const long gi = r0 + 16 * w + fr;
    const double *arow = As + (16 * w + fr) * DS;
    pw_f64x4 acc[DG][4];
#pragma unroll
    for (int q = 0; q < DG; ++q)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[q][g] = pw_f64x4{0.0, 0.0, 0.0, 0.0};
    const long t1 = std::min<long>(ctiles, (long)(slab + 1) * tps);
    for (long ct = (long)slab * tps; ct < t1; ++ct) {
      const long c0 = ct * 64;
      __syncthreads();  // the previous tile's reads of Bs and Vs are done (and As is staged)
      for (int idx = tid; idx < 64 * D; idx += 256) {
        const int r = idx / D, d = idx - r * D;
        Bs[r * DS + d] = (c0 + r < n) ? X[(c0 + r) * D + d] : 0.0;
      }
      for (int idx = tid; idx < 64 * 16 * ng; idx += 256) {
        const int j = idx & 63, t = idx >> 6;
        Vs[j * VS + t] = (t < S && c0 + j < n) ? V[(long)t * ldv + c0 + j] : 0.0;
      }
      __syncthreads();
#pragma nounroll
      for (int jj = 0; jj < 64; jj += 4) {
        const long gj = c0 + jj + fk;
        double a[DG];
#pragma unroll
        for (int q = 0; q < DG; ++q) a[q] = 0.0;
        if (gi < m && gj < n) {
          const double *brow = Bs + (jj + fk) * DS;
          simil_xgrad_accum<DG>(
              P, [&](int d) { return arow[d]; }, [&](int d) { return brow[d]; }, 1.0, a, dq);
        }
        const double *vp = Vs + (jj + fk) * VS + fr;
#pragma unroll
        for (int q = 0; q < DG; ++q) {
          acc[q][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], vp[0], acc[q][0], 0, 0, 0);
          if (ng > 1) acc[q][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], vp[16], acc[q][1], 0, 0, 0);
          if (ng > 2) acc[q][2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], vp[32], acc[q][2], 0, 0, 0);
          if (ng > 3) acc[q][3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], vp[48], acc[q][3], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int t = 16 * g + fr;
      if (t >= S) continue;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const long i = r0 + 16 * w + fk + 4 * v;
        if (i >= m) continue;
        double *dst = part + (((long)slab * S + t) * rpad + i) * D;
#pragma unroll
        for (int q = 0; q < DG; ++q)
          if (dq + q < D) dst[dq + q] = acc[q][g][v];
      }
    }
  }
}

// Out[t][i] = sum of pa's na slabs, then of pb's nb slabs (pb == nullptr: none), each in slab order, for i < rows; both
// [slab][t][rpad]
__global__ __launch_bounds__(256) void pw_finish_kernel(const double *__restrict__ pa, int na, const double *__restrict__ pb,
                                                        int nb, int T, long rpad, long rows, double *__restrict__ Out,
                                                        long ldo) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int t = blockIdx.y;
  if (i >= rows) return;
  double s = 0.0;
  for (int q = 0; q < na; ++q) s += pa[((long)q * T + t) * rpad + i];
  if (pb)
    for (int q = 0; q < nb; ++q) s += pb[((long)q * T + t) * rpad + i];
  Out[(long)t * ldo + i] = s;
}

// Rhs[t][i] = y_i - FX[t][i] - sqrt(noise_var + v_i) Xi[t][i] for t < S, i < n; 0 elsewhere in the `rows` rows of npad
__global__ __launch_bounds__(256) void pw_residual_kernel(const DevParams *__restrict__ Pp, const double *__restrict__ y,
                                                          const double *__restrict__ nv, const double *__restrict__ FX,
                                                          long ldf, const double *__restrict__ Xi, long n, long npad, int S,
                                                          double *__restrict__ Rhs) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int t = blockIdx.y;
  if (i >= npad) return;
  double r = 0.0;
  if (t < S && i < n) r = y[i] - FX[(long)t * ldf + i] - sqrt(Pp->noise_var + (nv ? nv[i] : 0.0)) * Xi[(long)t * n + i];
  Rhs[(long)t * npad + i] = r;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
// dimensions per pass of the two gradient kernels: the largest group whose DG x 4 accumulator fragments keep the instance
// inside the register audit without an allow-list entry ("Pathwise samples")
constexpr int PW_DG = 4;
static int pw_dg(int ndim) { return ndim >= PW_DG ? PW_DG : ndim >= 2 ? 2 : 1; }

constexpr size_t PW_LDS_CAP = (size_t)(2 * 64 * (GOGP_MAX_NDIM | 1) + 64 * 65 + 128) * sizeof(double);

template <int DG>
static void pw_feature_launch(hipStream_t s, dim3 grid, size_t lds, const double *Om, const double *ph, const double *am, int R,
                              int D, const double *Z, long m, const double *W, int S, int tps, double *part) {
  if (lds > 64 * 1024)  // said to the runtime before the launch (launch_kmm)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&pw_feature_kernel<DG>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)PW_LDS_CAP);
  GOGP_KLAUNCH(pw_feature_kernel<DG>, grid, dim3(256), lds, s, Om, ph, am, R, D, Z, m, W, S, tps, part);
}

int pw_feature_slabs(int64_t m, int R) { return kmm_slabs(m, R); }

void launch_pw_features(hipStream_t s, int ndim, const double *Om, const double *ph, const double *am, int R, const double *Z,
                        int64_t m, const double *W, int S, bool grad, int nslab, double *part) {
  const unsigned rt = (unsigned)((m + 63) / 64);
  const int ft = (R + 63) / 64, tps = (ft + nslab - 1) / nslab;
  const int d4 = (ndim + 3) & ~3, ng = (S + 15) / 16;
  const size_t lds = (size_t)(2 * 64 * (d4 | 1) + 64 * (16 * ng + 1) + 128) * sizeof(double);
  const int dg = pw_dg(ndim);
#define GOGP_PW_F(DGV, GZ) \
  pw_feature_launch<DGV>(s, dim3(rt, (unsigned)nslab, (unsigned)(GZ)), lds, Om, ph, am, R, ndim, Z, (long)m, W, S, tps, part)
  if (!grad) GOGP_PW_F(0, 1);
  else if (dg == 1) GOGP_PW_F(1, ndim);
  else if (dg == 2) GOGP_PW_F(2, (ndim + 1) / 2);
  else GOGP_PW_F(PW_DG, (ndim + PW_DG - 1) / PW_DG);
#undef GOGP_PW_F
}

template <int DG>
static void pw_crossgrad_launch(hipStream_t s, dim3 grid, size_t lds, const DevParams *p, const double *Z, long m, const double *X,
                                long n, const double *V, long ldv, int S, int tps, double *part) {
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&pw_crossgrad_kernel<DG>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)PW_LDS_CAP);
  GOGP_KLAUNCH(pw_crossgrad_kernel<DG>, grid, dim3(256), lds, s, p, Z, m, X, n, V, ldv, S, tps, part);
}

void launch_pw_crossgrad(hipStream_t s, const DevParams *p, int ndim, const double *Z, int64_t m, const double *X, int64_t n,
                         const double *V, int64_t ldv, int S, int nslab, double *part) {
  const unsigned rt = (unsigned)((m + 63) / 64);
  const long ct = (long)((n + 63) / 64);
  const int tps = (int)((ct + nslab - 1) / nslab);
  const int ng = (S + 15) / 16;
  const size_t lds = (size_t)(2 * 64 * (ndim | 1) + 64 * (16 * ng + 1)) * sizeof(double);
  const int dg = pw_dg(ndim);
#define GOGP_PW_C(DGV, GZ) \
  pw_crossgrad_launch<DGV>(s, dim3(rt, (unsigned)nslab, (unsigned)(GZ)), lds, p, Z, (long)m, X, (long)n, V, (long)ldv, S, tps, part)
  if (dg == 1) GOGP_PW_C(1, ndim);
  else if (dg == 2) GOGP_PW_C(2, (ndim + 1) / 2);
  else GOGP_PW_C(PW_DG, (ndim + PW_DG - 1) / PW_DG);
#undef GOGP_PW_C
}

void launch_pw_finish(hipStream_t s, const double *pa, int na, const double *pb, int nb, int T, int64_t rpad, int64_t rows,
                      double *Out, int64_t ldo) {
  GOGP_KLAUNCH(pw_finish_kernel, dim3((unsigned)((rows + 255) / 256), (unsigned)T), dim3(256), 0, s, pa, na, pb, nb, T,
               (long)rpad, (long)rows, Out, (long)ldo);
}

}  // namespace gogp

// ---- gogp_pathwise_* -----------------------------------------------------------------------------------------------------------
using namespace gogp;

// A set of S draws: everything gogp_pathwise_eval reads is the object's own copy, nothing of the handle's
struct gogp_paths {
  int device = 0, D = 0, S = 0, R = 0;
  int64_t n = 0, ldv = 0;
  char *own = nullptr;  // one block: the parameters, X, V, Omega, phase, amp, W
  DevParams *P = nullptr;
  double *X = nullptr, *V = nullptr, *Om = nullptr, *ph = nullptr, *am = nullptr, *W = nullptr;
  char *ws = nullptr;  // the scratch of gogp_pathwise_eval, grown on demand
  size_t ws_bytes = 0;
};

namespace {
// the object's block (base == nullptr: the bytes alone)
size_t paths_layout(gogp_paths *p, char *base) {
  Carve c{base};
  p->P = c.take<DevParams>(1);
  p->X = c.take<double>((size_t)p->n * p->D);
  p->V = c.take<double>((size_t)p->S * p->ldv);
  p->Om = c.take<double>((size_t)p->R * p->D);
  p->ph = c.take<double>((size_t)p->R);
  p->am = c.take<double>((size_t)p->R);
  p->W = c.take<double>((size_t)p->R * p->S);
  return c.off;
}
bool all_finite(const double *a, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (!std::isfinite(a[i])) return false;
  return true;
}
}  // namespace

extern "C" int gogp_pathwise_create(gogp_handle *h, int32_t R, const double *Omega, const double *phase, const double *amp,
                                    int32_t S, const double *W, const double *Xi, gogp_paths **out) {
  if (!h) return GOGP_EARG;
  if (!Omega || !phase || !amp || !W || !Xi || !out) return fail(h, GOGP_EARG, "pathwise_create: NULL");
  *out = nullptr;
  const char *why = h->prec == 32          ? "precision = 32 handles"
                    : h->grad_prec == 32   ? "gradient_precision = 32"
                    : h->ev()              ? "event discounts"
                    : h->dist              ? "sharded handles"
                                           : nullptr;
  if (why) return refuse(h, "pathwise_create", GOGP_EARG, (std::string(why) + " are not supported").c_str());
  if (S < 1 || S > GOGP_CG_MAX_RHS) return refuse(h, "pathwise_create", GOGP_EARG, "need 1 <= S <= GOGP_CG_MAX_RHS");
  if (R < 1 || R > GOGP_PATHWISE_MAX_R) return refuse(h, "pathwise_create", GOGP_EARG, "need 1 <= R <= GOGP_PATHWISE_MAX_R");
  if (h->n < 1 || !h->factored) return refuse(h, "pathwise_create", GOGP_ESTATE, "nothing absorbed");
  const int D = h->D;
  const int64_t n = h->n, npad = h->npad;
  if (!all_finite(Omega, (size_t)R * D) || !all_finite(phase, R) || !all_finite(amp, R) || !all_finite(W, (size_t)R * S) ||
      !all_finite(Xi, (size_t)S * n))
    return refuse(h, "pathwise_create", GOGP_EARG, "non-finite features or normals");
  HIPCHK(h, hipSetDevice(h->device));

  gogp_paths *p = new gogp_paths;
  p->device = h->device, p->D = D, p->S = S, p->R = R, p->n = n, p->ldv = npad;
  const size_t own = paths_layout(p, nullptr);
  // the call's scratch: Xi, the feature product's partial sums and F_X, the right-hand sides (one tile row)
  const int nslab = pw_feature_slabs(n, R);
  const int64_t rpad = (n + 63) / 64 * 64;
  Carve sc{nullptr};
  auto scratch = [&](Carve &c, double *&xi, double *&part, double *&fx, double *&rhs) {
    xi = c.take<double>((size_t)S * n);
    part = c.take<double>((size_t)nslab * S * rpad);
    fx = c.take<double>((size_t)S * npad);
    rhs = c.take<double>((size_t)TILE * npad);
  };
  double *xi, *part, *fx, *rhs;
  scratch(sc, xi, part, fx, rhs);
  size_t free_b = 0, total_b = 0;
  hipError_t e = hipMemGetInfo(&free_b, &total_b);
  if (e == hipSuccess && own + sc.off > free_b) {
    delete p;
    char buf[200];
    snprintf(buf, sizeof buf, "needs %zu bytes of device memory (%zu kept, %zu of scratch), %zu are free", own + sc.off, own,
             sc.off, free_b);
    return refuse(h, "pathwise_create", GOGP_ENOMEM, buf);
  }
  char *tmp = nullptr;
  if (e == hipSuccess) e = hipMalloc(&p->own, own);
  if (e == hipSuccess) e = hipMalloc(&tmp, sc.off);
  int rc = GOGP_OK;
  if (e == hipSuccess) {
    paths_layout(p, p->own);
    sc = Carve{tmp};
    scratch(sc, xi, part, fx, rhs);
    hipStream_t s = h->s;
    const size_t db = sizeof(double);
    e = hipMemcpyAsync(p->Om, Omega, (size_t)R * D * db, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p->ph, phase, (size_t)R * db, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p->am, amp, (size_t)R * db, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p->W, W, (size_t)R * S * db, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(xi, Xi, (size_t)S * n * db, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p->X, h->dX, (size_t)n * D * db, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p->P, h->devP, sizeof(DevParams), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) {
      launch_pw_features(s, D, p->Om, p->ph, p->am, R, p->X, n, p->W, S, false, nslab, part);
      launch_pw_finish(s, part, nslab, nullptr, 0, S, rpad, n, fx, npad);
      GOGP_KLAUNCH(pw_residual_kernel, dim3((unsigned)((npad + 255) / 256), (unsigned)TILE), dim3(256), 0, s,
                   (const DevParams *)p->P, (const double *)h->dy, (const double *)(h->nv_set ? h->nv : nullptr),
                   (const double *)fx, (long)npad, (const double *)xi, (long)n, (long)npad, (int)S, rhs);
      rc = factor_solve_rows(h, rhs, S, p->V);  // V[s] = K^^-1 rhs[s], rows of npad (zero from column n on)
      if (rc == GOGP_OK) e = hipStreamSynchronize(s);
      if (rc == GOGP_OK && e == hipSuccess) e = hipGetLastError();
    }
  }
  (void)hipFree(tmp);
  if (e != hipSuccess || rc != GOGP_OK) {
    (void)hipFree(p->own);
    delete p;
    if (rc != GOGP_OK) return rc;
    h->err = std::string("pathwise_create: ") + hipGetErrorString(e);
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? GOGP_ENOMEM : GOGP_EHIP;
  }
  *out = p;
  return GOGP_OK;
}

extern "C" int gogp_pathwise_get_v(gogp_paths *p, double *V) {
  if (!p || !V) return GOGP_EARG;
  if (hipSetDevice(p->device) != hipSuccess) return GOGP_EHIP;
  const size_t row = (size_t)p->n * sizeof(double);
  return hipMemcpy2D(V, row, p->V, (size_t)p->ldv * sizeof(double), row, (size_t)p->S, hipMemcpyDeviceToHost) == hipSuccess
             ? GOGP_OK
             : GOGP_EHIP;
}

extern "C" int gogp_pathwise_destroy(gogp_paths *p) {
  if (!p) return GOGP_OK;
  (void)hipSetDevice(p->device);
  (void)hipFree(p->own);
  (void)hipFree(p->ws);
  delete p;
  return GOGP_OK;
}

// Points per pass of gogp_pathwise_eval: 16384, fewer with derivatives where S * ndim is large (their partial sums are
// S * ndim doubles per point and slab)
static int64_t pw_chunk(int S, int D, bool grad) {
  if (!grad) return 16384;
  const int64_t c = ((int64_t)1 << 24) / ((int64_t)S * D) / 64 * 64;
  return std::max<int64_t>(64, std::min<int64_t>(16384, c));
}

extern "C" int gogp_pathwise_eval(gogp_paths *p, const double *Z, int64_t m, double *F, double *dF) {
  if (!p || !Z || !F || m < 1) return GOGP_EARG;
  const int D = p->D, S = p->S, R = p->R;
  const int64_t n = p->n;
  if (!all_finite(Z, (size_t)m * D)) return GOGP_EARG;
  if (hipSetDevice(p->device) != hipSuccess) return GOGP_EHIP;
  const bool grad = dF != nullptr;
  const int64_t mc = std::min(m, pw_chunk(S, D, grad)), mlast = m % mc;
  // slabs x padded rows of a pass's partial sums: the full passes' and the last, shorter one's (the slabs of a pass depend
  // on its points and on R / n alone)
  auto rows_f = [&](int64_t mj) { return (size_t)pw_feature_slabs(mj, R) * (size_t)((mj + 63) / 64 * 64); };
  auto rows_k = [&](int64_t mj) { return (size_t)kmm_slabs(mj, n) * (size_t)((mj + 63) / 64 * 64); };
  const size_t rf = std::max(rows_f(mc), mlast ? rows_f(mlast) : 0), rk = std::max(rows_k(mc), mlast ? rows_k(mlast) : 0);
  const size_t gd = grad ? (size_t)D : 0;
  Carve c{nullptr};
  double *dz, *pf, *pk, *fo, *pgf, *pgk, *go;
  auto layout = [&](Carve &cv) {
    dz = cv.take<double>((size_t)mc * D);
    pf = cv.take<double>(rf * S);
    pk = cv.take<double>(rk * S);
    fo = cv.take<double>((size_t)S * mc);
    pgf = cv.take<double>(rf * S * gd);
    pgk = cv.take<double>(rk * S * gd);
    go = cv.take<double>((size_t)S * mc * gd);
  };
  layout(c);
  if (p->ws_bytes < c.off) {  // ask before allocating
    (void)hipFree(p->ws);
    p->ws = nullptr, p->ws_bytes = 0;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return GOGP_EHIP;
    if (c.off > free_b) return GOGP_ENOMEM;
    if (hipMalloc(&p->ws, c.off) != hipSuccess) {
      (void)hipGetLastError();
      return GOGP_ENOMEM;
    }
    p->ws_bytes = c.off;
  }
  c = Carve{p->ws};
  layout(c);
  hipStream_t s = 0;
  const size_t db = sizeof(double);
  for (int64_t j0 = 0; j0 < m; j0 += mc) {
    const int64_t mj = std::min(mc, m - j0), rp = (mj + 63) / 64 * 64;
    const int nsf = pw_feature_slabs(mj, R), nsk = kmm_slabs(mj, n);
    hipError_t e = hipMemcpyAsync(dz, Z + j0 * D, (size_t)mj * D * db, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return GOGP_EHIP;
    // F = Phi(Z) W + k(Z, X) V: the feature slabs, then the cross term's, each in slab order
    launch_pw_features(s, D, p->Om, p->ph, p->am, R, dz, mj, p->W, S, false, nsf, pf);
    launch_kmm(s, p->P, D, dz, mj, p->X, n, p->V, p->ldv, S, nullptr, nsk, 0, pk, fo, mj);
    launch_pw_finish(s, pf, nsf, pk, nsk, S, rp, mj, fo, mj);
    if (grad) {
      launch_pw_features(s, D, p->Om, p->ph, p->am, R, dz, mj, p->W, S, true, nsf, pgf);
      launch_pw_crossgrad(s, p->P, D, dz, mj, p->X, n, p->V, p->ldv, S, nsk, pgk);
      launch_pw_finish(s, pgf, nsf, pgk, nsk, S, rp * D, mj * D, go, mj * D);
    }
    e = hipMemcpy2DAsync(F + j0, (size_t)m * db, fo, (size_t)mj * db, (size_t)mj * db, (size_t)S, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && grad)
      e = hipMemcpy2DAsync(dF + j0 * D, (size_t)m * D * db, go, (size_t)mj * D * db, (size_t)mj * D * db, (size_t)S,
                           hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return GOGP_EHIP;
    }
  }
  return GOGP_OK;
}
