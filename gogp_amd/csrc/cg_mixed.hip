// cg_mixed.hip -- the float-evaluated product of the iterative exact GP (option "cg_precision" = 32; cg_api.hip runs the
// rounds; include/gogp_hip.h states the scheme; DESIGN.md section 4, "Iterative (CG): float-evaluated product").
//
//   kmm32_kernel<KIND, DP>   Out[t][i] = sum_j c f~(a_i, b_j) V[t][j] (+ diag_i V[t][i]): kmm_kernel's work split (64 rows per
//                            workgroup, 16 per wave, a slab of 64-column tiles, lane (fr, fk) supplying one k(a_fr, b_fk) as
//                            the A operand of v_mfma_f64_16x16x4_f64, up to four column groups of 16 right-hand sides, the
//                            partials [slab][t][rpad] added by kmm_finish_kernel) with the similarity f~ evaluated in SINGLE
//                            precision.  The scales c_t, the diagonal, V, the accumulators and the partials stay fp64: a float
//                            value is converted and multiplied by c_t in fp64, so an entry is off by c_t times the float
//                            evaluation error of f alone.
//
// Staging: every coordinate is centred in fp64, x_d - centre_d, and then rounded to float, so that inputs with a large
// common offset keep their differences; V lies in LDS as doubles.  Two instantiations, chosen from the descriptor and D:
//   fast     (KIND = the radial kind, DP = D padded to 4, 8 or 16): one radial term, D <= 16.  Staging stores
//            u_d = (x_d - centre_d) / l_d, scaled in fp64 and then rounded, zero from D on; a pair is sum_d (ua_d - ub_d)^2
//            and one radial function.  The lane's row stays in DP registers for the whole row tile (read once per tile with
//            the plain stride DP: sixteen rows share banks at DP = 8 and 16, outside the pair loop); the column's row is
//            DP / 4 16-byte LDS reads that the sixteen lanes of a column share.  The 16 column steps of a tile run in
//            groups of four whose evaluations are issued one group AHEAD of their MFMAs: four independent exp chains overlap
//            each other and the matrix cores.
//   generic  (DP = 0): any descriptor the fp64 product takes -- a float restatement of simil_value.  Float copies of 1 / l,
//            the periodic terms' frequency in revolutions, the kinds and the scales are made once per workgroup, in LDS;
//            rows of A and B with the odd stride D | 1 floats (the 16 rows a wave reads lie in different banks).
// Radial kinds go through the hardware exp2 (log2 e folded into the constant) and the hardware sqrt; Periodic through the
// hardware sine on the fractional part of |delta| / (2 p), its argument in revolutions.  k~(a, b) and k~(b, a) run through the
// same operations on (a - b)^2 or |a - b|: K~ is symmetric bit for bit.
//
// Rows and columns beyond the sizes are staged as zeros and V as zero there: they contribute exact zeros without a test
// per pair; padded output rows are stored as zeros.  The diagonal is added in fp64 when the fragment is stored, by the slab
// that holds the row's own column tile.  The order of every sum depends on the sizes only, never on T.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace gogp {

typedef double cgm_f64x4 __attribute__((ext_vector_type(4)));
typedef float cgm_f32x2 __attribute__((ext_vector_type(2)));
typedef float cgm_f32x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr double CGM_LOG2E = 1.4426950408889634074;
constexpr float CGM_SQRT3 = 1.7320508075688772f, CGM_SQRT5 = 2.2360679774997900f;
constexpr float CGM_E_NORMAL = (float)(-0.5 * CGM_LOG2E);                     // exp(-s / 2) = exp2(E s)
constexpr float CGM_E_MATERN32 = (float)(-1.7320508075688772 * CGM_LOG2E);    // exp(-sqrt(3) r)
constexpr float CGM_E_MATERN52 = (float)(-2.2360679774997900 * CGM_LOG2E);    // exp(-sqrt(5) r)
constexpr float CGM_E_PERIODIC = (float)(-2.0 * CGM_LOG2E);                   // exp(-2 s)

// f(s), s = r^2, of a radial kind
__device__ __forceinline__ float cgm_radial(int kind, float s) {
  if (kind == GOGP_K_NORMAL) return __builtin_amdgcn_exp2f(CGM_E_NORMAL * s);
  const float r = __builtin_amdgcn_sqrtf(s);
  if (kind == GOGP_K_MATERN32) return (1.0f + CGM_SQRT3 * r) * __builtin_amdgcn_exp2f(CGM_E_MATERN32 * r);
  const float e = __builtin_amdgcn_exp2f(CGM_E_MATERN52 * r);
  if (kind == GOGP_K_MATERN52) return (1.0f + CGM_SQRT5 * r + s) * e;
  return (1.0f + CGM_SQRT5 * r + (5.0f / 3.0f) * s) * e;  // GOGP_K_MATERN52_TEXTBOOK
}

// what the generic instance keeps per workgroup behind the rows: float copies of the descriptor
struct CgmTerms {
  double c[GOGP_MAX_TERMS];
  float wrev[GOGP_MAX_TERMS];  // PERIODIC: w / (2 pi), the frequency in revolutions
  int kind[GOGP_MAX_TERMS];
};
}  // namespace

// Work item w = blockIdx.x + q gridDim.x: row tile w / nslab, slab w % nslab, as kmm_kernel.  Dynamic LDS:
//   Vs[64][VS] doubles (VS = 16 ng + 1), As[64][FS], Bs[64][FS] floats (fast: FS = DP; generic: FS = D | 1), and for the
//   generic instance CgmTerms and il[nterms][D] floats.
template <int KIND, int DP>
__global__ __launch_bounds__(256, 2) void kmm32_kernel(const DevParams *__restrict__ Pp, const double *__restrict__ A,
                                                       long rows, const double *__restrict__ B, long cols,
                                                       const double *__restrict__ centre, const double *__restrict__ V,
                                                       long ldv, int T, const double *__restrict__ diag, int nslab, int tps,
                                                       long nitems, long rpad, double *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr bool FAST = DP > 0;
  const DevParams &P = *Pp;
  const int D = P.ndim;
  const int FS = FAST ? DP : (D | 1);
  const int ng = (T + 15) >> 4;  // column groups of 16 right-hand sides (uniform)
  const int VS = 16 * ng + 1;
  double *Vs = sm;
  float *As = reinterpret_cast<float *>(Vs + 64 * VS), *Bs = As + 64 * FS;
  CgmTerms *tm = reinterpret_cast<CgmTerms *>(Bs + 64 * FS);  // (generic) behind the rows: 64 FS floats are whole doubles
  float *il = reinterpret_cast<float *>(tm + 1);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const long ctiles = (cols + 63) >> 6;
  const int nt = P.nterms;
  const double c0s = P.c[0];
  if constexpr (!FAST) {
    if (tid < nt) {
      tm->c[tid] = P.c[tid];
      tm->wrev[tid] = (float)(P.w[tid] * (0.5 / 3.14159265358979323846));
      tm->kind[tid] = P.kind[tid];
    }
    for (int idx = tid; idx < nt * D; idx += 256) {
      const int t = idx / D, d = idx - t * D;
      il[idx] = (float)P.inv_len[t][d];
    }
  }
  // one row of A or B, centred (and, fast, scaled) in fp64 and then rounded; zeros beyond the sizes
  auto stage = [&](float *dst, const double *__restrict__ X, long x0, long nx) {
    if constexpr (FAST) {
      for (int idx = tid; idx < 64 * DP; idx += 256) {
        const int r = idx / DP, d = idx - r * DP;
        float v = 0.0f;
        if (d < D && x0 + r < nx) v = (float)((X[(x0 + r) * D + d] - centre[d]) * P.inv_len[0][d]);
        dst[idx] = v;
      }
    } else {
      for (int idx = tid; idx < 64 * D; idx += 256) {
        const int r = idx / D, d = idx - r * D;
        dst[r * FS + d] = (x0 + r < nx) ? (float)(X[(x0 + r) * D + d] - centre[d]) : 0.0f;
      }
    }
  };
  for (long item = blockIdx.x; item < nitems; item += gridDim.x) {
    const long rt = item / nslab;
    const int slab = (int)(item - rt * nslab);
    const long r0 = rt * 64;
    __syncthreads();  // the previous item's reads of As are done
    stage(As, A, r0, rows);
    __syncthreads();
    const float *arow = As + (16 * w + fr) * FS;
    float ua[FAST ? DP : 1];
    if constexpr (FAST) {
#pragma unroll
      for (int q = 0; q < DP / 4; ++q) {
        const cgm_f32x4 v = *reinterpret_cast<const cgm_f32x4 *>(arow + 4 * q);
        ua[4 * q] = v.x, ua[4 * q + 1] = v.y, ua[4 * q + 2] = v.z, ua[4 * q + 3] = v.w;
      }
    }
    // k(a_fr, b_{jj + fk}) of the staged tile, times its scale, in fp64
    auto eval = [&](int jj) -> double {
      const float *brow = Bs + (jj + fk) * FS;
      if constexpr (FAST) {
        cgm_f32x2 s2 = {0.0f, 0.0f};
#pragma unroll
        for (int q = 0; q < DP / 4; ++q) {
          const cgm_f32x4 b = *reinterpret_cast<const cgm_f32x4 *>(brow + 4 * q);
          const cgm_f32x2 d0 = cgm_f32x2{ua[4 * q], ua[4 * q + 1]} - cgm_f32x2{b.x, b.y};
          const cgm_f32x2 d1 = cgm_f32x2{ua[4 * q + 2], ua[4 * q + 3]} - cgm_f32x2{b.z, b.w};
          s2 = d0 * d0 + s2;
          s2 = d1 * d1 + s2;
        }
        return c0s * (double)cgm_radial(KIND, s2.x + s2.y);
      } else {
      double k = 0.0;
      for (int t = 0; t < nt; ++t) {
        const int kind = tm->kind[t];
        const float *l = il + t * D;
        float s = 0.0f, f;
        if (kind == GOGP_K_PERIODIC) {
          const float wr = tm->wrev[t];
          for (int d = 0; d < D; ++d) {
            const float rev = fabsf(arow[d] - brow[d]) * wr;
            const float dd = __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(rev)) * l[d];
            s = fmaf(dd, dd, s);
          }
          f = __builtin_amdgcn_exp2f(CGM_E_PERIODIC * s);
        } else {
          for (int d = 0; d < D; ++d) {
            const float u = (arow[d] - brow[d]) * l[d];
            s = fmaf(u, u, s);
          }
          f = cgm_radial(kind, s);
        }
        k += tm->c[t] * (double)f;
      }
      return k;
      }
    };
    cgm_f64x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = cgm_f64x4{0.0, 0.0, 0.0, 0.0};
    auto mma = [&](int jj, double k) {
      const double *vp = Vs + (jj + fk) * VS + fr;
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(k, vp[0], acc[0], 0, 0, 0);
      if (ng > 1) acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(k, vp[16], acc[1], 0, 0, 0);
      if (ng > 2) acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(k, vp[32], acc[2], 0, 0, 0);
      if (ng > 3) acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(k, vp[48], acc[3], 0, 0, 0);
    };
    const long t0 = (long)slab * tps, t1 = std::min<long>(ctiles, t0 + tps);
    for (long ct = t0; ct < t1; ++ct) {
      const long c0 = ct * 64;
      __syncthreads();  // the previous tile's reads of Bs and Vs are done
      stage(Bs, B, c0, cols);
      for (int idx = tid; idx < 64 * 16 * ng; idx += 256) {
        const int j = idx & 63, t = idx >> 6;
        Vs[j * VS + t] = (t < T && c0 + j < cols) ? V[(long)t * ldv + c0 + j] : 0.0;
      }
      __syncthreads();
      if constexpr (FAST) {
        // four column steps per group, the next group's evaluations issued ahead of this group's MFMAs
        double kq[4], kn[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) kq[u] = eval(4 * u);
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          if (g4 < 3) {
#pragma unroll
            for (int u = 0; u < 4; ++u) kn[u] = eval(16 * (g4 + 1) + 4 * u);
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) mma(16 * g4 + 4 * u, kq[u]);
#pragma unroll
          for (int u = 0; u < 4; ++u) kq[u] = kn[u];
        }
      } else {
        for (int jj = 0; jj < 64; jj += 8) {
          const double k0 = eval(jj), k1 = eval(jj + 4);
          mma(jj, k0);
          mma(jj + 4, k1);
        }
      }
    }
    // C fragment: column (right-hand side) = lane & 15, row = (lane >> 4) + 4 v.  The slab that holds the rows' own
    // column tile adds diag_i V[t][i]; rows beyond the sizes are stored as zeros.
    const bool dhere = diag != nullptr && rt >= t0 && rt < t1;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int t = 16 * g + fr;
      if (t < T) {
        const long row0 = r0 + 16 * w + fk;
        double *dst = part + ((long)slab * T + t) * rpad + row0;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const long row = row0 + 4 * v;
          double val = 0.0;
          if (row < rows) {
            val = acc[g][v];
            if (dhere) val += diag[row] * V[(long)t * ldv + row];
          }
          dst[4 * v] = val;
        }
      }
    }
  }
}

// The restart of a round (cg_api.hip): column t is done -- frozen for good -- once its true residual is within the
// tolerance or its right-hand side is zero; the others go live again from r = the true residual.  One wave.
__global__ __launch_bounds__(64) void cg_restart_kernel(int T, double tol, const double *__restrict__ dots,
                                                        double *__restrict__ sc, int *__restrict__ st) {
  const int t = threadIdx.x;
  if (t >= T) return;
  const double bn = sc[CG_SC_BNORM2 * CG_MAX_T + t];
  const bool done = bn == 0.0 || sqrt(dots[t]) <= tol * sqrt(bn);
  st[CG_ST_FROZEN * CG_MAX_T + t] = done ? 1 : 0;
  st[CG_ST_BAD * CG_MAX_T + t] = 0;
  if (!done) sc[CG_SC_RR * CG_MAX_T + t] = dots[t];
}

void launch_cg_restart(hipStream_t s, int T, double tol, const double *dots, CgState cs) {
  GOGP_KLAUNCH(cg_restart_kernel, dim3(1), dim3(64), 0, s, T, tol, dots, cs.sc, cs.st);
}

// ---- launcher --------------------------------------------------------------------------------------------------------------------
namespace {
// the dynamic LDS of an instance; D = GOGP_MAX_NDIM, T = CG_MAX_T gives the cap that is said to the runtime
size_t kmm32_lds(int dp, int ndim, int nterms, int T) {
  const int ng = (T + 15) / 16;
  const size_t vs = (size_t)64 * (16 * ng + 1) * sizeof(double);
  if (dp > 0) return vs + (size_t)2 * 64 * dp * sizeof(float);
  const size_t fs = ndim | 1;
  return vs + 2 * 64 * fs * sizeof(float) + sizeof(CgmTerms) + (size_t)nterms * ndim * sizeof(float);
}

template <int KIND, int DP>
void kmm32_launch(hipStream_t s, long grid, size_t lds, const DevParams *p, const double *A, long rows, const double *B,
                  long cols, const double *centre, const double *V, long ldv, int T, const double *diag, int nslab, int tps,
                  long nitems, long rpad, double *part) {
  // more than 64 KB (the generic instance at 64 dimensions with 64 right-hand sides) is said to the runtime before the launch
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&kmm32_kernel<KIND, DP>),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)kmm32_lds(DP, GOGP_MAX_NDIM, GOGP_MAX_TERMS, CG_MAX_T));
  GOGP_KLAUNCH((kmm32_kernel<KIND, DP>), dim3((unsigned)grid), dim3(256), lds, s, p, A, rows, B, cols, centre, V, ldv, T, diag,
               nslab, tps, nitems, rpad, part);
}

template <int KIND>
void kmm32_launch_dp(int dp, hipStream_t s, long grid, size_t lds, const DevParams *p, const double *A, long rows,
                     const double *B, long cols, const double *centre, const double *V, long ldv, int T, const double *diag,
                     int nslab, int tps, long nitems, long rpad, double *part) {
  if (dp == 4)
    kmm32_launch<KIND, 4>(s, grid, lds, p, A, rows, B, cols, centre, V, ldv, T, diag, nslab, tps, nitems, rpad, part);
  else if (dp == 8)
    kmm32_launch<KIND, 8>(s, grid, lds, p, A, rows, B, cols, centre, V, ldv, T, diag, nslab, tps, nitems, rpad, part);
  else
    kmm32_launch<KIND, 16>(s, grid, lds, p, A, rows, B, cols, centre, V, ldv, T, diag, nslab, tps, nitems, rpad, part);
}
}  // namespace

// the padded dimension count of the fast instance, or 0 for the generic one: a function of the descriptor and D alone
int kmm32_fast_dims(int ndim, int nterms, int kind0) {
  if (nterms != 1 || kind0 == GOGP_K_PERIODIC || ndim > 16) return 0;
  return ndim <= 4 ? 4 : ndim <= 8 ? 8 : 16;
}

void launch_kmm32(hipStream_t s, const DevParams *p, int ndim, int nterms, int kind0, const double *A, int64_t rows,
                  const double *B, int64_t cols, const double *centre, const double *V, int64_t ldv, int T,
                  const double *diag, int nslab, int max_blocks, double *part, double *Out, int64_t ldo) {
  const long rt = (long)((rows + 63) / 64), ct = (long)((cols + 63) / 64);
  const long rpad = rt * 64;
  const int tps = (int)((ct + nslab - 1) / nslab);
  const long nitems = rt * nslab;
  long grid = std::min<long>(nitems, 1L << 20);
  if (max_blocks > 0) grid = std::min<long>(grid, max_blocks);
  const int dp = kmm32_fast_dims(ndim, nterms, kind0);
  const size_t lds = kmm32_lds(dp, ndim, nterms, T);
#define GOGP_KMM32_ARGS s, grid, lds, p, A, (long)rows, B, (long)cols, centre, V, (long)ldv, T, diag, nslab, tps, nitems, rpad, part
  if (dp == 0)
    kmm32_launch<0, 0>(GOGP_KMM32_ARGS);
  else if (kind0 == GOGP_K_NORMAL)
    kmm32_launch_dp<GOGP_K_NORMAL>(dp, GOGP_KMM32_ARGS);
  else if (kind0 == GOGP_K_MATERN32)
    kmm32_launch_dp<GOGP_K_MATERN32>(dp, GOGP_KMM32_ARGS);
  else if (kind0 == GOGP_K_MATERN52)
    kmm32_launch_dp<GOGP_K_MATERN52>(dp, GOGP_KMM32_ARGS);
  else
    kmm32_launch_dp<GOGP_K_MATERN52_TEXTBOOK>(dp, GOGP_KMM32_ARGS);
#undef GOGP_KMM32_ARGS
  launch_kmm_finish(s, part, nslab, T, rpad, rows, Out, ldo);
}

}  // namespace gogp
