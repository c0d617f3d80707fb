// grad.hip -- fused hyperparameter-gradient reduction (HBM-read-bound).
//
// Reference: gp.GP.Gradient (gp/gp.go:418-499) forms, PER PARAMETER p, the dense
// products r0 = (alpha alpha^T) dK_p and r1 = K^-1 dK_p and takes
// 1/2 tr(r0 - r1) (gp/gp.go:476-485), with dK_p = theta_p dK/dtheta_p built per
// pair by the AD tape during absorb (gp/gp.go:113-117,137-142).  Since
// tr(M dK) = sum_ij M_ij dK_ij for symmetric matrices this equals
//     grad_p = 1/2 sum_ij W_ij dK_p,ij ,   W = alpha alpha^T - K^-1,
// which is what this kernel evaluates in ONE pass over the lower triangle of
// K^-1, recomputing k(x_i,x_j) and its log-parameter derivatives on the fly
// (no dK matrix is ever stored).  Off-diagonal elements count twice.
//
// Output: NACC slot sums (see common.h); the host maps slots to theta indices.
#ifndef GOGP_EV  // first pass: the whole file, the kernels without event discounts
#include "kern_eval.h"

#define GOGP_EV 0
#define GOGP_EVN(name) name
namespace gogp {

constexpr int GR_BLOCKS_MAX = 2048;
#endif

// LOCAL: the tiles are the local ones of a 2-D block-cyclic K^-1 (rectangular nt x ntc tile
// grid, global row / column indices through `map`, tiles of the global upper triangle skipped).
// KT: element type of K^-1 (float on the fp32 path; all sums are fp64 either way).
// RADIAL1: the similarity kernel is ONE radial term (every BASELINE configuration; the host checks):
// that instance carries only the restructured loops below, the other only the generic accumulation.
// GOGP_EV = 1: the handle has event discounts (kern_eval.h: event_mask): the pair's weight is multiplied by its discount,
// so every slot of the similarity (scale, length, period) is; the noise slot (trace of W) is not.  This kernel and
// xgrad_kernel are compiled twice -- as before, and with GOGP_EV = 1 as grad_reduce_kernel_ev / xgrad_kernel_ev (the file
// includes itself once, below); the events instances are launched without ARD only (gogp_set_events refuses it).
template <int ARD_D, bool LOCAL, class KT, bool RADIAL1>
__global__ __launch_bounds__(256) void GOGP_EVN(grad_reduce_kernel)(
    const DevParams *__restrict__ Pp, const double *__restrict__ X,
    const double *__restrict__ alpha, const KT *__restrict__ Kinv, long ld, long n, int nt,
    int ntiles, double *__restrict__ partials, int ntc, BlockMap map, int ard0, long bstride) {
  extern __shared__ double sm[];
  const DevParams &P = *cand(Pp, bstride);  // candidate batching (common.h: Batch); X is shared
  alpha = cand(alpha, bstride);
  Kinv = cand(Kinv, bstride);
  partials = cand(partials, bstride);
  const int D = P.ndim;
  double *Ri = sm;              // [64][D]
  double *CjT = sm + 64 * D;    // [D + ARD_D][64]: ARD_D zero rows behind the D real ones (see the ARD pass below)
  double *ai = CjT + 64 * (D + (ARD_D > 0 ? ARD_D : 0));  // [64]
  double *aj = ai + 64;         // [64]
  double *red = aj + 64;        // [4][NACC]
  unsigned long long *Mr = reinterpret_cast<unsigned long long *>(red + 4 * NACC), *Mc = Mr + 64;  // GOGP_EV: [64] each
  const int tid = threadIdx.x;
  const int tx = tid & 63, ty = tid >> 6;

  double acc[ACC_TRACE + 1];
#pragma unroll
  for (int q = 0; q <= ACC_TRACE; ++q) acc[q] = 0.0;
  double ard[ARD_D > 0 ? ARD_D : 1];
#pragma unroll
  for (int q = 0; q < (ARD_D > 0 ? ARD_D : 1); ++q) ard[q] = 0.0;

  // zero rows D .. D + ARD_D - 1 of CjT, written once: a pass's slots beyond the last dimension read them (and X a
  // few doubles past its row: the X buffer carries zeroed slack) and multiply by inv_len = 0 -- exact zeros, never
  // 0 * (whatever LDS held)
  for (int idx = threadIdx.x; idx < 64 * (ARD_D > 0 ? ARD_D : 0); idx += 256) CjT[64 * D + idx] = 0.0;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    int ti, tj;
    long r0, c0, lr0, lc0;
    if (LOCAL) {
      ti = t / ntc;
      tj = t - ti * ntc;
      lr0 = (long)ti * 64;
      lc0 = (long)tj * 64;
      r0 = map.grow(lr0);
      c0 = map.gcol(lc0);
      if (c0 > r0) continue;  // workgroup-uniform: tile of the global upper triangle
    } else {
      ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
      while (ti * (ti + 1) / 2 > t) --ti;
      while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
      tj = t - ti * (ti + 1) / 2;
      lr0 = r0 = (long)ti * 64;
      lc0 = c0 = (long)tj * 64;
    }
    __syncthreads();  // previous tile's readers are done
    for (int idx = tid; idx < 64 * D; idx += 256) {
      const int r = idx / D, d = idx - r * D;
      Ri[idx] = (r0 + r < n) ? X[(r0 + r) * D + d] : 0.0;
    }
    // lanes along a row of CjT: conflict-free stores (with the lanes along d a wave's stores were 512 B apart, one
    // bank: 34 % of this kernel's LDS cycles were conflict cycles in the round-3 PMC pass)
    for (int idx = tid; idx < 64 * D; idx += 256) {
      const int d = idx >> 6, r = idx & 63;
      CjT[idx] = (c0 + r < n) ? X[(c0 + r) * D + d] : 0.0;
    }
    if (tid < 64) ai[tid] = (r0 + tid < n) ? alpha[r0 + tid] : 0.0;
    else if (tid < 128) aj[tid - 64] = (c0 + tid - 64 < n) ? alpha[c0 + tid - 64] : 0.0;
    else if (GOGP_EV && tid < 192) Mr[tid - 128] = event_mask(P, (r0 + tid - 128 < n) ? X[(r0 + tid - 128) * D + P.ev_axis] : 0.0);
    else if (GOGP_EV) Mc[tid - 192] = event_mask(P, (c0 + tid - 192 < n) ? X[(c0 + tid - 192) * D + P.ev_axis] : 0.0);
    __syncthreads();
    const long gj = c0 + tx;
    const double *cj = CjT + tx;
    const double ajv = aj[tx];
    if (RADIAL1) {
      // One radial term: dimension loops outside, the thread's 16 rows
      // inside (gram.hip has the same structure).  The column coordinate is read from LDS once per
      // dimension, the rows' coordinates are wave-uniform and come from X through scalar loads (X is
      // padded to npad rows).  Per accumulator the same additions in the same order as
      // simil_grad_accum(): bit-identical sums.
      const int rbase = __builtin_amdgcn_readfirstlane(ty) * 16;
      const double *xr = X + (r0 + rbase) * D;
      double s[16];
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) s[rr] = 0.0;
      for (int d = 0; d < D; ++d) {
        const double il = P.inv_len[0][d];
        const double c = cj[d * 64];
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
          const double u = (xr[rr * D + d] - c) * il;
          s[rr] += u * u;
        }
      }
      const int kind = P.kind[0];
      const double cc = P.c[0];
      const bool isard = P.ard[0] != 0;
      double gg[16];
      unsigned live = 0;
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) {
        const int r = rbase + rr;
        const long gi = r0 + r;
        gg[rr] = 0.0;
        if (gi < n && gj <= gi) {
          const double w = ai[r] * ajv - (double)Kinv[(lr0 + r) * ld + lc0 + tx];
          double wgt = (gj < gi) ? 2.0 * w : w;
          if (GOGP_EV) wgt *= event_discount(P, Mr[r], Mc[tx]);
          double f, dfdr2;
          radial_eval(kind, s[rr], f, dfdr2);
          acc[0] += wgt * cc * f;
          const double g = wgt * cc * dfdr2 * (-2.0);
          if (!isard) acc[1] += g * s[rr];
          if (gi == gj) acc[ACC_TRACE] += w;
          gg[rr] = g;
          live |= 1u << rr;
        }
      }
      if (ARD_D > 0 && isard) {
        // Everything that depends on the pass (ard0) sits in three base pointers; inside the unrolled
        // loop q is a compile-time constant, i.e. an immediate offset of the LDS read, of the scalar
        // loads and of the parameter load.  (With `d = ard0 + q` written out per q, hipcc hoisted 32
        // LDS offsets, 32 `d < D` masks and 32 parameter addresses out of the tile loop and parked them
        // in spill lanes: 190 SGPR spills in this instance.)
        // No test of `ard0 + q < D` either (32 more hoisted masks): a slot beyond the last dimension
        // multiplies by inv_len = 0 (fill_params zero-fills the table up to GOGP_MAX_NDIM), reads the zero
        // rows behind the column block in LDS and X past the row (the X buffer is allocated with
        // GOGP_MAX_NDIM zeroed doubles of slack): it adds exact zeros.  The launcher
        // picks the instance of each pass by the dimensions that are left, so at most half of a pass is
        // such padding.
        const double *cja = cj + ard0 * 64;
        const double *xra = xr + ard0;
        const double *ila = &P.inv_len[0][ard0];
#pragma unroll
        for (int q = 0; q < (ARD_D > 0 ? ARD_D : 1); ++q) {  // unrolled: ard[] stays in registers
          const double il = ila[q];
          const double c = cja[q * 64];
          double a = ard[q];
#pragma unroll
          for (int rr = 0; rr < 16; ++rr)
            if (live & (1u << rr)) {
              const double g = gg[rr];
              const double u = (xra[rr * D + q] - c) * il;
              a += g * u * u;
            }
          ard[q] = a;
        }
      }
      continue;
    }
    for (int rr = 0; RADIAL1 ? false : rr < 16; ++rr) {
      const int r = ty * 16 + rr;
      const long gi = r0 + r;
      if (gi < n && gj <= gi) {
        const double w = ai[r] * ajv - (double)Kinv[(lr0 + r) * ld + lc0 + tx];
        double wgt = (gj < gi) ? 2.0 * w : w;
        if (GOGP_EV) wgt *= event_discount(P, Mr[r], Mc[tx]);
        const double *ri = Ri + r * D;
        simil_grad_accum<ARD_D>(
            P, [&](int d) { return ri[d]; }, [&](int d) { return cj[d * 64]; }, wgt, acc, ard, ard0);
        if (gi == gj) acc[ACC_TRACE] += w;
      }
    }
  }

  // ---- block reduction: wave shuffles, then 4 waves through LDS -------------
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
  // the pass over the first ARD dimensions (ard0 == 0) writes every slot (zeros in the dead ones),
  // a later pass only the slots of its own dimensions
  if (tid < NACC) {
    const bool base = tid <= ACC_TRACE, mine = tid >= ACC_ARD0 && tid < ACC_ARD0 + ARD_D;
    double v = 0.0;
    if (base || mine) v = red[tid] + red[NACC + tid] + red[2 * NACC + tid] + red[3 * NACC + tid];
    if (ard0 == 0) partials[(long)blockIdx.x * NACC + tid] = v;
    else if (mine && tid + ard0 < NACC) partials[(long)blockIdx.x * NACC + tid + ard0] = v;
  }
}

#if !GOGP_EV  // second pass: the kernels of this file again, with event discounts, as *_ev
#undef GOGP_EV
#undef GOGP_EVN
#define GOGP_EV 1
#define GOGP_EVN(name) name##_ev
#include "grad.hip"
#undef GOGP_EV
#undef GOGP_EVN
#define GOGP_EV 0
#define GOGP_EVN(name) name
#endif

#ifndef GOGP_GRAD_KERNEL_ONLY  // (the hook library includes this file for the reduction kernel template alone)
#if !GOGP_EV
// out[q] = sum over blocks of partials[b][q]; one workgroup per slot q, fixed
// summation tree (bitwise reproducible)
__global__ __launch_bounds__(256) void grad_final_kernel(const double *__restrict__ partials,
                                                         int nblocks, double *__restrict__ out,
                                                         long bstride) {
  partials = cand(partials, bstride);  // candidate batching (common.h: Batch)
  out = cand(out, bstride);
  __shared__ double red[4];
  const int q = blockIdx.x;
  double v = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 256) v += partials[(long)b * NACC + q];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) out[q] = red[0] + red[1] + red[2] + red[3];
}

// dynamic LDS of one instance: Ri [64][D], CjT [D + AD][64], ai, aj, red [4][NACC] -- sized per instance (an isotropic
// kernel at D = 8 asks for 11.8 KB, not for the 32-slot instance's 28 KB: the LDS occupancy ceiling of the hot path)
static inline size_t gr_lds_bytes(int ndim, int ad, bool ev = false) {
  return (size_t)(128 * ndim + 64 * ad + 128 + 4 * NACC + (ev ? 128 : 0)) * sizeof(double);  // (the masks: 8 bytes each)
}
// launch one instance; above 64 KB of dynamic LDS (ndim >= 45 with 32 slots) the limit is raised explicitly, as
// launch_xgrad and grad_mfma.hip do, instead of relying on what the runtime tolerates
template <int AD, bool LOCAL, class KT, bool R1, bool EV = false, class... Args>
static void gr_launch(dim3 grid, hipStream_t s, int ndim, Args... args) {
  const size_t lds = gr_lds_bytes(ndim, AD, EV);
  if (lds > 64 * 1024) {
    // per launch, not once per process: the attribute belongs to the function ON THE CURRENT DEVICE, and a process may
    // launch the same instance on several (cheap next to the kernel; grad_mfma.hip and launch_xgrad do the same)
    const void *fn;
    if constexpr (EV) fn = reinterpret_cast<const void *>(&grad_reduce_kernel_ev<AD, LOCAL, KT, R1>);
    else fn = reinterpret_cast<const void *>(&grad_reduce_kernel<AD, LOCAL, KT, R1>);
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gr_lds_bytes(GOGP_MAX_NDIM, AD, EV));
  }
  if constexpr (EV)
    GOGP_KLAUNCH((grad_reduce_kernel_ev<AD, LOCAL, KT, R1>), grid, dim3(256), lds, s, args...);
  else
    GOGP_KLAUNCH((grad_reduce_kernel<AD, LOCAL, KT, R1>), grid, dim3(256), lds, s, args...);
}

// max_blocks > 0 caps the grid (tests: a small problem whose workgroups walk several tiles); 0: GR_BLOCKS_MAX alone
static inline int gr_cap_blocks(int blocks, int max_blocks) {
  return max_blocks > 0 && max_blocks < blocks ? max_blocks : blocks;
}

int grad_reduce_blocks(int64_t npad) {
  const int nt = (int)(npad / 64);
  const long ntiles = (long)nt * (nt + 1) / 2;
  return (int)(ntiles < GR_BLOCKS_MAX ? ntiles : GR_BLOCKS_MAX);
}

template <class KT>
static void grad_reduce_t(hipStream_t s, const DevParams *p, int ndim, int ard_dims,
                          const double *X, const double *alpha, const KT *Kinv, int64_t ld,
                          int64_t n, int64_t npad, double *partials, double *out, bool radial1, int mfma_min,
                          bool ev, int max_blocks) {
  const int nt = (int)(npad / 64);
  const int ntiles = nt * (nt + 1) / 2;
  const int blocks = gr_cap_blocks(grad_reduce_blocks(npad), max_blocks);
  const unsigned nz = (unsigned)tl_batch.k;
// More than 16 ARD dimensions: passes of 16 per-dimension accumulators each.  (Instances with 32 / 64
// accumulators need more than 256 VGPRs; the code hipcc (ROCm 7.2) generates for them -- VGPRs that carry
// SGPR spill lanes copied through AGPRs -- returned wrong, run-to-run varying sums on the sharded
// path at N >= 4096: tools/grad_probe.py.)
#define GOGP_LAUNCH_GR(AD, A0)                                                                    \
  do {                                                                                            \
    if (radial1)                                                                                  \
      gr_launch<AD, false, KT, true>(dim3(blocks, 1, nz), s, ndim, p, X, alpha, Kinv, (long)ld, (long)n, nt, ntiles, \
                                     partials, 0, BlockMap(), (int)(A0), (long)tl_batch.stride);   \
    else                                                                                          \
      gr_launch<AD, false, KT, false>(dim3(blocks, 1, nz), s, ndim, p, X, alpha, Kinv, (long)ld, (long)n, nt, ntiles, \
                                      partials, 0, BlockMap(), (int)(A0), (long)tl_batch.stride);  \
  } while (0)
  if (ev) {  // event discounts (never with ARD: gogp_set_events)
    if (radial1)
      gr_launch<0, false, KT, true, true>(dim3(blocks, 1, nz), s, ndim, p, X, alpha, Kinv, (long)ld, (long)n, nt, ntiles,
                                          partials, 0, BlockMap(), 0, (long)tl_batch.stride);
    else
      gr_launch<0, false, KT, false, true>(dim3(blocks, 1, nz), s, ndim, p, X, alpha, Kinv, (long)ld, (long)n, nt, ntiles,
                                           partials, 0, BlockMap(), 0, (long)tl_batch.stride);
  } else if (radial1 && ard_dims > 0 && ard_dims >= mfma_min)
    // one radial term, many ARD length scales: distances and per-dimension sums on the matrix cores
    launch_grad_ard_mfma(s, p, ndim, X, alpha, Kinv, ld, n, nt, 0, ntiles, blocks, BlockMap(), partials);
  else if (ard_dims <= 0) GOGP_LAUNCH_GR(0, 0);
  else if (ard_dims <= 8) GOGP_LAUNCH_GR(8, 0);
  else if (radial1 && ard_dims > 16) {
    // the restructured instance is lean enough for 32 accumulators (188 VGPRs, no AGPRs, no scratch): half the
    // passes, i.e. half the distance / exp work, for 17..64 ARD dimensions; the last pass takes the
    // smallest instance that holds what is left (the kernel does not test d < D per slot)
    for (int a0 = 0; a0 < ard_dims; a0 += 32) {
      const int left = ard_dims - a0;
      if (left <= 8)
        gr_launch<8, false, KT, true>(dim3(blocks, 1, nz), s, ndim, p, X, alpha, Kinv, (long)ld, (long)n, nt, ntiles, partials,
                                      0, BlockMap(), a0, (long)tl_batch.stride);
      else if (left <= 16)
        gr_launch<16, false, KT, true>(dim3(blocks, 1, nz), s, ndim, p, X, alpha, Kinv, (long)ld, (long)n, nt, ntiles, partials,
                                      0, BlockMap(), a0, (long)tl_batch.stride);
      else
        gr_launch<32, false, KT, true>(dim3(blocks, 1, nz), s, ndim, p, X, alpha, Kinv, (long)ld, (long)n, nt, ntiles, partials,
                                      0, BlockMap(), a0, (long)tl_batch.stride);
    }
  } else
    for (int a0 = 0; a0 < ard_dims; a0 += 16) GOGP_LAUNCH_GR(16, a0);
#undef GOGP_LAUNCH_GR
  GOGP_KLAUNCH(grad_final_kernel, dim3(NACC, 1, nz), dim3(256), 0, s, partials, blocks, out, tl_batch.stride);
}
void launch_grad_reduce(hipStream_t s, const DevParams *p, int ndim, int ard_dims,
                        const double *X, const double *alpha, const double *Kinv, int64_t ld,
                        int64_t n, int64_t npad, double *partials, double *out, bool radial1, int mfma_min, bool ev,
                        int max_blocks) {
  grad_reduce_t(s, p, ndim, ard_dims, X, alpha, Kinv, ld, n, npad, partials, out, radial1, mfma_min, ev, max_blocks);
}
void launch_grad_reduce(hipStream_t s, const DevParams *p, int ndim, int ard_dims,
                        const double *X, const double *alpha, const float *Kinv, int64_t ld,
                        int64_t n, int64_t npad, double *partials, double *out, bool radial1, int mfma_min, bool ev,
                        int max_blocks) {
  grad_reduce_t(s, p, ndim, ard_dims, X, alpha, Kinv, ld, n, npad, partials, out, radial1, mfma_min, ev, max_blocks);
}

int grad_reduce_blocks_local(int64_t mrows, int64_t ncols) {
  const long ntiles = (long)(mrows / 64) * (long)(ncols / 64);
  return (int)(ntiles < GR_BLOCKS_MAX ? (ntiles > 0 ? ntiles : 1) : GR_BLOCKS_MAX);
}

template <class KT>
static void grad_reduce_local_t(hipStream_t s, const DevParams *p, int ndim, int ard_dims,
                                const double *X, const double *alpha, const KT *Kinv, int64_t ld,
                                int64_t n, int64_t mrows, int64_t ncols, BlockMap map, double *partials,
                                double *out, bool radial1, int mfma_min, bool ev, int max_blocks) {
  const int nt = (int)(mrows / 64), ntc = (int)(ncols / 64);
  const int ntiles = nt * ntc;
  const int blocks = gr_cap_blocks(grad_reduce_blocks_local(mrows, ncols), max_blocks);
#define GOGP_LAUNCH_GRL(AD, A0)                                                                   \
  do {                                                                                            \
    if (radial1)                                                                                  \
      gr_launch<AD, true, KT, true>(dim3(blocks), s, ndim, p, X, alpha, Kinv, (long)ld, (long)n, nt, ntiles, partials, \
                                    ntc, map, (int)(A0), 0L);                                      \
    else                                                                                          \
      gr_launch<AD, true, KT, false>(dim3(blocks), s, ndim, p, X, alpha, Kinv, (long)ld, (long)n, nt, ntiles, partials, \
                                     ntc, map, (int)(A0), 0L);                                     \
  } while (0)
  if (ev) {  // event discounts (never with ARD: gogp_set_events)
    if (radial1)
      gr_launch<0, true, KT, true, true>(dim3(blocks), s, ndim, p, X, alpha, Kinv, (long)ld, (long)n, nt, ntiles, partials,
                                         ntc, map, 0, 0L);
    else
      gr_launch<0, true, KT, false, true>(dim3(blocks), s, ndim, p, X, alpha, Kinv, (long)ld, (long)n, nt, ntiles, partials,
                                          ntc, map, 0, 0L);
  } else if (radial1 && ard_dims > 0 && ard_dims >= mfma_min)
    launch_grad_ard_mfma(s, p, ndim, X, alpha, Kinv, ld, n, nt, ntc, ntiles, blocks, map, partials);
  else if (ard_dims <= 0) GOGP_LAUNCH_GRL(0, 0);
  else if (ard_dims <= 8) GOGP_LAUNCH_GRL(8, 0);
  else if (radial1 && ard_dims > 16) {
    for (int a0 = 0; a0 < ard_dims; a0 += 32) {
      const int left = ard_dims - a0;
      if (left <= 8)
        gr_launch<8, true, KT, true>(dim3(blocks), s, ndim, p, X, alpha, Kinv, (long)ld, (long)n, nt, ntiles, partials, ntc, map,
                                     a0, 0L);
      else if (left <= 16)
        gr_launch<16, true, KT, true>(dim3(blocks), s, ndim, p, X, alpha, Kinv, (long)ld, (long)n, nt, ntiles, partials, ntc, map,
                                     a0, 0L);
      else
        gr_launch<32, true, KT, true>(dim3(blocks), s, ndim, p, X, alpha, Kinv, (long)ld, (long)n, nt, ntiles, partials, ntc, map,
                                     a0, 0L);
    }
  } else
    for (int a0 = 0; a0 < ard_dims; a0 += 16) GOGP_LAUNCH_GRL(16, a0);
#undef GOGP_LAUNCH_GRL
  GOGP_KLAUNCH(grad_final_kernel, dim3(NACC), dim3(256), 0, s, partials, blocks, out, 0L);
}
void launch_grad_reduce_local(hipStream_t s, const DevParams *p, int ndim, int ard_dims,
                              const double *X, const double *alpha, const double *Kinv, int64_t ld,
                              int64_t n, int64_t mrows, int64_t ncols, BlockMap map, double *partials,
                              double *out, bool radial1, int mfma_min, bool ev, int max_blocks) {
  grad_reduce_local_t(s, p, ndim, ard_dims, X, alpha, Kinv, ld, n, mrows, ncols, map, partials, out, radial1, mfma_min,
                      ev, max_blocks);
}
void launch_grad_reduce_local(hipStream_t s, const DevParams *p, int ndim, int ard_dims,
                              const double *X, const double *alpha, const float *Kinv, int64_t ld,
                              int64_t n, int64_t mrows, int64_t ncols, BlockMap map, double *partials,
                              double *out, bool radial1, int mfma_min, bool ev, int max_blocks) {
  grad_reduce_local_t(s, p, ndim, ard_dims, X, alpha, Kinv, ld, n, mrows, ncols, map, partials, out, radial1, mfma_min,
                      ev, max_blocks);
}

// ---- gradient w.r.t. the inputs (full Observe form) ------------------------------
// gp/gp.go:118-129 builds one dense dK per input coordinate (N*D matrices of N x N);
// since dK^{(i,d)} has only row/column i non-zero,
//     dLML/dx_{i,d} = 1/2 tr(W dK^{(i,d)}) = sum_j W_ij dk(x_i,x_j)/dx_{i,d},
// one pass over the FULL symmetric W = alpha alpha^T - K^-1 (the lower triangle of
// K^-1 is mirrored first).  One workgroup per 64 rows; 4 threads share a row and
// split each 64-column tile; fixed-order reductions.

// upper 32x32 tiles <- transpose of the lower ones (diagonal 128-blocks are
// already full from the LAUUM tile kernel)
__global__ __launch_bounds__(256) void mirror_lower_kernel(double *__restrict__ A, long ld, int nt32) {
  __shared__ double tile[32][33];
  const int t = blockIdx.x;
  int ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (ti * (ti + 1) / 2 > t) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  const int tj = t - ti * (ti + 1) / 2;
  if (ti == tj || ti >= nt32) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int r = 0; r < 32; r += 8) tile[ty + r][tx] = A[(long)(ti * 32 + ty + r) * ld + tj * 32 + tx];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 32; r += 8) A[(long)(tj * 32 + ty + r) * ld + ti * 32 + tx] = tile[tx][ty + r];
}

#endif  // !GOGP_EV

// GOGP_EV = 1 (xgrad_kernel_ev): event discounts (kern_eval.h: event_mask), W_ij is multiplied by the pair's discount
template <int DMAX>
__global__ __launch_bounds__(256) void GOGP_EVN(xgrad_kernel)(const DevParams *__restrict__ Pp,
                                                    const double *__restrict__ X,
                                                    const double *__restrict__ alpha,
                                                    const double *__restrict__ Kinv, long ld,
                                                    long n, long npad, double *__restrict__ gx, int d0) {
  extern __shared__ double sm[];
  const DevParams &P = *Pp;
  const int D = P.ndim;
  double *Xi = sm;               // [64][D]
  double *Xj = Xi + 64 * D;      // [64][D]
  double *T = Xj + 64 * D;       // [64][65]  W tile
  double *aj = T + 64 * 65;      // [64]
  unsigned long long *Mj = reinterpret_cast<unsigned long long *>(aj + 64);  // GOGP_EV: [64] column masks
  const int tid = threadIdx.x;
  const long r0 = (long)blockIdx.x * 64;
  const int r = tid >> 2, q = tid & 3;
  for (int idx = tid; idx < 64 * D; idx += 256) {
    const int rr = idx / D, d = idx - rr * D;
    Xi[idx] = (r0 + rr < n) ? X[(r0 + rr) * D + d] : 0.0;
  }
  const double ai = (r0 + r < n) ? alpha[r0 + r] : 0.0;
  const unsigned long long mi = GOGP_EV ? event_mask(P, (r0 + r < n) ? X[(r0 + r) * D + P.ev_axis] : 0.0) : 0ull;
  double acc[DMAX];
#pragma unroll
  for (int d = 0; d < DMAX; ++d) acc[d] = 0.0;
  const double *xi = Xi + r * D;
  for (long c0 = 0; c0 < npad; c0 += 64) {
    __syncthreads();
    for (int idx = tid; idx < 64 * D; idx += 256) {
      const int rr = idx / D, d = idx - rr * D;
      Xj[idx] = (c0 + rr < n) ? X[(c0 + rr) * D + d] : 0.0;
    }
    if (tid < 64) aj[tid] = (c0 + tid < n) ? alpha[c0 + tid] : 0.0;
    else if (GOGP_EV && tid < 128) Mj[tid - 64] = event_mask(P, (c0 + tid - 64 < n) ? X[(c0 + tid - 64) * D + P.ev_axis] : 0.0);
    for (int idx = tid; idx < 64 * 64; idx += 256) {
      const int rr = idx >> 6, cc = idx & 63;
      T[rr * 65 + cc] = Kinv[(r0 + rr) * ld + c0 + cc];
    }
    __syncthreads();
    if (r0 + r < n) {
      for (int jj = 0; jj < 16; ++jj) {
        const int j = q * 16 + jj;
        if (c0 + j < n && c0 + j != r0 + r) {
          double W = ai * aj[j] - T[r * 65 + j];
          if (GOGP_EV) W *= event_discount(P, mi, Mj[j]);
          const double *xj = Xj + j * D;
          simil_xgrad_accum<DMAX>(
              P, [&](int d) { return xi[d]; }, [&](int d) { return xj[d]; }, W, acc, d0);
        }
      }
    }
  }
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    double v = acc[d];
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    if (q == 0 && d0 + d < D && r0 + r < n) gx[(r0 + r) * D + d0 + d] = v;
  }
}

#if !GOGP_EV
void launch_xgrad(hipStream_t s, const DevParams *p, int ndim, const double *X,
                  const double *alpha, double *Kinv, int64_t ld, int64_t n, int64_t npad,
                  double *gx, bool ev) {
  const int nt32 = (int)(npad / 32);
  GOGP_KLAUNCH(mirror_lower_kernel, dim3(nt32 * (nt32 + 1) / 2), dim3(256), 0, s, Kinv,
                     (long)ld, nt32);
  const size_t lds = (size_t)(128 * ndim + 64 * 65 + 64) * sizeof(double);
  const dim3 grid((unsigned)(npad / 64));
  // above 64 KB of dynamic LDS (D > 32) the limit has to be raised explicitly
#define GOGP_LAUNCH_XG(DM, D0)                                                                 \
  do {                                                                                         \
    if (lds > 64 * 1024)                                                                       \
      (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&xgrad_kernel<DM>),             \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);         \
    GOGP_KLAUNCH(xgrad_kernel<DM>, grid, dim3(256), lds, s, p, X, alpha, Kinv, (long)ld, \
                       (long)n, (long)npad, gx, D0);                                           \
  } while (0)
  // more than 32 dimensions: passes of 32 (a 64-accumulator instance needs 326 VGPRs, AGPRs included,
  // and 128 SGPR spills -- the register footprint that produced wrong sums in the parameter-gradient
  // reduction; see launch_grad_reduce)
  if (ev) {
    // event discounts: instances of up to 16 accumulators, passes of 16 beyond (inside the SGPR spill limit without an
    // allow-list entry)
    const size_t ldse = lds + 64 * sizeof(unsigned long long);
#define GOGP_LAUNCH_XGE(DM, D0)                                                                 \
  do {                                                                                          \
    if (ldse > 64 * 1024)                                                                       \
      (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&xgrad_kernel_ev<DM>),        \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldse);         \
    GOGP_KLAUNCH((xgrad_kernel_ev<DM>), grid, dim3(256), ldse, s, p, X, alpha, Kinv, (long)ld, \
                 (long)n, (long)npad, gx, D0);                                                  \
  } while (0)
    if (ndim <= 4) GOGP_LAUNCH_XGE(4, 0);
    else if (ndim <= 8) GOGP_LAUNCH_XGE(8, 0);
    else
      for (int d0 = 0; d0 < ndim; d0 += 16) GOGP_LAUNCH_XGE(16, d0);
#undef GOGP_LAUNCH_XGE
  } else if (ndim <= 4) GOGP_LAUNCH_XG(4, 0);
  else if (ndim <= 8) GOGP_LAUNCH_XG(8, 0);
  else if (ndim <= 16) GOGP_LAUNCH_XG(16, 0);
  else
    for (int d0 = 0; d0 < ndim; d0 += 32) GOGP_LAUNCH_XG(32, d0);
#undef GOGP_LAUNCH_XG
}

#endif  // !GOGP_EV
#endif  // GOGP_GRAD_KERNEL_ONLY

#if !GOGP_EV
}  // namespace gogp
#undef GOGP_EV
#undef GOGP_EVN
#endif
