// vecchia_blocks.hip -- Vecchia's approximation on BLOCKS of targets that share a conditioning set (gogp_vecchia_blocks_*;
// vecchia_api.hip orchestrates): the block NNGP of Quiroz et al. 2019, the "grouping" of Guinness 2018.
//
//     log p(y) ~ sum_k log p(y_T(k) | y_C(k)),     T(k) the nt_k targets of block k, C(k) its nc_k conditioning rows,
// every conditioning row a target of an EARLIER block, nc_k + nt_k <= 128.  Block b = [C..., T...] in the table's order,
// c = |C|, t = |T|, n = c + t:
//     K_b = k(X_b, X_b) + diag(noise_var + v_b),   L = chol(K_b),   X = L^-1,   z = X y_b.
// Target row q >= c (the conditional on C and on the block's earlier targets; their sum is the block's joint density):
//     mu_q = y_q - L_qq z_q,   s_q = L_qq,   log p_q = -1/2 log 2 pi - log L_qq - 1/2 z_q^2.
// With X_T the last t rows of X and z_T the last t entries of z, alpha = X^T z:
//     K_b^-1 - pad(K_C^-1) = X_T^T X_T,     d = alpha - pad(alpha_C) = X_T^T z_T,
//     d log p(y_T | y_C) / d log theta_p = 1/2 sum_ab W_ab dK_b,ab / d log theta_p,
//     W = alpha d^T + d alpha^T - d d^T - X_T^T X_T:
// one SYRK over the k range [c, n) -- K = t, not 128 -- on v_mfma_f64_16x16x4_f64 plus rank-one terms.  ACC_TRACE takes
// sum W_aa, so api.hip's assemble_gradient applies as it stands (the convention of batch_eval_kernel).  With t == 1 this
// is the model of vecchia.hip; with one block and c == 0 it is the dense LML.
// Produce: a group of test points shares one conditioning set C of at most 128 rows.  K_C is factored once; per point
// k* = k(X_C, z), v = X k*, mu = k*^T alpha, sigma = sqrt(k(z, z) - v^T v), latent and unclamped.
//
// One workgroup of 512 threads owns one block at a time; workgroup g of G = vblocks_grid(nb) takes the blocks g, g + G,
// ...: a function of the block count alone.  The walk over a workgroup's blocks is the HOST's: round r is one launch of
// the blocks r G .. r G + G - 1, and the workgroup's value, failure word and partial row live in global memory between
// the rounds, read, added to and written by that workgroup alone (launches of one stream: block order).  With the loop
// inside the kernel hipcc hoists the factorisation's addresses and scalars out of it and keeps them across the pivot
// pass: 31 VGPR and 135 SGPR spills and a private segment, against none and 26 for the body on its own.  A round costs
// one launch (N = 1048576, c = t = 64: 16 rounds).  The factorisation and the inverse are diag256.hip's in-LDS helpers
// (potrf128_lds, invert128_lds: 16-blocked, on the matrix cores), compiled into this translation unit's own namespace as
// blockcv.hip does.  LDS (158 KB of the 160): S[128][130] the Gram matrix, then L, then X, then W; G the helpers' scratch,
// then k* of Produce; the block's row indices, y, noise_var + v (then L_ii), z, alpha and d.
// The gathered rows of X are NOT staged: what is left of the 160 KB holds 128 rows of no more than 5 dimensions, so the Gram
// fill and the pair walk read them from L2 through the LDS index list (a block's rows are read by its own workgroup only,
// n (n + 1) / 2 pairs of them twice).
// Stages per block: gather (indices, y, diagonal); Gram (lower triangle, identity beyond n, as batch_eval_kernel pads);
// factor; X = L^-1; z, alpha, d by four threads per row, each a quarter of the sum in index order, added in a fixed order;
// the terms through the targets' row indices; X_T^T X_T (lower 16-tiles, the k range rounded up to the 4-wide step with
// zeros, kept in registers until every wave has read X), W in place in S; batch_eval_kernel's pair walk through
// simil_grad_accum.  A pivot that is not positive and finite ends that block only: NaN terms, nothing added, and the
// workgroup remembers its lowest such block.  The waves' slot sums of a block are added in wave order onto the
// workgroup's row; launch_sparse_grad_final adds the
// workgroups' rows, vblock_final_kernel (the order of vecchia_final_kernel) the values, and takes the lowest failing
// block.  No atomics, no spin-waits: identical calls give identical bits, and a block has the same bits alone as inside
// a launch.  ARD: launches per pass of 8 dimensions, as vecchia.hip; a later pass repeats the factorisation.
#define GOGP_NS gogp_vb
#define GOGP_DIAG256_DEVICE_ONLY
#include "diag256.hip"

namespace gogp_vb {

constexpr int VB_SLOTS = ACC_TRACE + 1 + 8;  // a wave's running row: the base slots, then the pass's ARD accumulators

// tile t of the lower triangle of 16-tiles in row-major order: (ti, tj), tj <= ti
__device__ __forceinline__ void vb_tile(int t, int &ti, int &tj) {
  ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  tj = t - ti * (ti + 1) / 2;
}

// Block k = k0 + blockIdx.x of the nb (the launch holds no workgroup beyond them); vpart, fpart and the rows of partials
// are ADDED to (fpart: set if still 0): zeroed before the first round.  Three roles (the head of the file):
// value (PRODUCE, GRAD false): out0 = terms (N x 3: mu, s, log p; may be nullptr), vpart / fpart the workgroup's sum of
//   log p and its lowest failing block + 1.
// gradient (GRAD): only `partials` is written (one row of NACC per workgroup; the pass with ard0 == 0 adds to the base
//   slots and its own ARD slots, a later one to its own only); a failing block is skipped.
// produce (PRODUCE): block k is group k: its nc[k] conditioning rows in row k of tbl, its test points goff[k] .. goff[k + 1]
//   - 1 of Z; out0 = mu, out1 = sigma (may be nullptr), fpart as above (the lowest failing group + 1).
template <int ARD_D, bool PRODUCE, bool GRAD>
__global__ __launch_bounds__(NT) void vblock_kernel(const DevParams *__restrict__ Pp, const double *__restrict__ X,
                                                    const double *__restrict__ y, const double *__restrict__ v,
                                                    const int *__restrict__ tbl, const int *__restrict__ nc,
                                                    const int *__restrict__ nt, int nb, int w,
                                                    const double *__restrict__ Z, const long long *__restrict__ goff,
                                                    double *__restrict__ out0, double *__restrict__ out1,
                                                    double *__restrict__ partials, double *__restrict__ vpart,
                                                    long long *__restrict__ fpart, int ard0, int k0) {
  __shared__ __attribute__((aligned(16))) double S[128 * SLD];
  __shared__ __attribute__((aligned(16))) double G[GSIZE];
  __shared__ double rinv_s[8 * 16];
  __shared__ double ys[128], zs[128], as[128], ds[128], dl[128];  // y; z; alpha; d; noise_var + v, then L_ii
  __shared__ double redv[2];
  __shared__ int rows[128];
  __shared__ long long info_s;
  const int D = Pp->ndim;
  const int k = k0 + blockIdx.x;
  {
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int fr = lane & 15, fk = lane >> 4;
    const int c = nc[k], n = PRODUCE ? c : c + nt[k];
    // the parameters are read again per stage (scalar loads): kept across the factorisation they cost more scalar
    // registers than the audit allows (as vecchia.hip)
    const DevParams *Pq = Pp;
    asm volatile("" : "+s"(Pq));
    const DevParams &P = *Pq;
    // ---- gather: the row list, y and the diagonal's addition -------------------------------------------------------------
    if (tid < 128) {
      const int r = tid < n ? tbl[(long)k * w + tid] : -1;
      rows[tid] = r;
      ys[tid] = r >= 0 ? y[r] : 0.0;
      dl[tid] = r >= 0 ? (v ? P.noise_var + v[r] : P.noise_var) : 0.0;
    }
    if (tid == 0) info_s = 0;
    __syncthreads();
    // ---- the Gram matrix, lower triangle (rows / columns >= n: identity) ------------------------------------------------
    for (int idx = tid; idx < 128 * 128; idx += NT) {
      const int i = idx >> 7, j = idx & 127;
      double kk = 0.0;
      if (j <= i) {
        if (i < n) {
          const double *xi = X + (long)rows[i] * D, *xj = X + (long)rows[j] * D;
          kk = simil_value(P, [&](int d) { return xi[d]; }, [&](int d) { return xj[d]; });
          if (i == j) kk += dl[i];
        } else {
          kk = (i == j) ? 1.0 : 0.0;
        }
      }
      S[i * SLD + j] = kk;
    }
    __syncthreads();
    potrf128_lds(S, G, rinv_s, tid, 0, n, &info_s);  // (ends with a barrier)
    // a pivot that is not positive is in info_s; one that is not finite shows on the factor's diagonal
    int bad = info_s != 0;
    if (tid < 128) {
      const double l = S[tid * SLD + tid];
      if (tid < n && !(l > 0.0 && l < INFINITY)) bad = 1;
      dl[tid] = l;
    }
    bad = __syncthreads_or(bad);  // (the inverse starts by overwriting the diagonal blocks)
    if (bad) {                    // workgroup-uniform: this block stops here
      if (tid == 0 && fpart && fpart[blockIdx.x] == 0) fpart[blockIdx.x] = (long long)k + 1;  // (a workgroup's blocks ascend)
      if (PRODUCE) {
        for (long long j = goff[k] + tid; j < goff[k + 1]; j += NT) {
          out0[j] = NAN;
          if (out1) out1[j] = NAN;
        }
      } else if (!GRAD && out0 && tid >= c && tid < n) {
        double *o = out0 + 3L * rows[tid];
        o[0] = NAN, o[1] = NAN, o[2] = NAN;
      }
      return;
    }
    invert128_lds(S, G, tid);  // S = X = L^-1 (lower; the upper triangle holds exact zeros); ends with a barrier
    // ---- z = X y: row tid / 4, a quarter of the sum each, added in a fixed order --------------------------------------------
    {
      const int i = tid >> 2, p = tid & 3;
      double a = 0.0;
      for (int q = p; q <= i; q += 4) a += S[i * SLD + q] * ys[q];
      a += __shfl_xor(a, 1);
      a += __shfl_xor(a, 2);
      if (p == 0) zs[i] = a;
    }
    __syncthreads();
    if (!PRODUCE && !GRAD) {
      // ---- the terms of the t target rows, through their row indices; the block's value -----------------------------------
      if (tid < 128) {
        double lp = 0.0;
        if (tid >= c && tid < n) {
          const double l = dl[tid], zq = zs[tid];
          lp = -0.5 * log(2.0 * GOGP_PI) - log(l) - 0.5 * zq * zq;
          if (out0) {
            double *o = out0 + 3L * rows[tid];
            o[0] = ys[tid] - l * zq;
            o[1] = l;
            o[2] = lp;
          }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) lp += __shfl_xor(lp, o);
        if (lane == 0) redv[wv] = lp;
      }
      __syncthreads();
      if (tid == 0) vpart[blockIdx.x] += redv[0] + redv[1];
      return;
    }
    // ---- alpha = X^T z and d = X_T^T z_T: column tid / 4 --------------------------------------------------------------------
    {
      const int j = tid >> 2, p = tid & 3;
      double a = 0.0, dd = 0.0;
      for (int q = j + p; q < n; q += 4) {
        const double xz = S[q * SLD + j] * zs[q];
        a += xz;
        if (q >= c) dd += xz;
      }
      a += __shfl_xor(a, 1);
      a += __shfl_xor(a, 2);
      dd += __shfl_xor(dd, 1);
      dd += __shfl_xor(dd, 2);
      if (p == 0) {
        as[j] = a;
        ds[j] = dd;
      }
    }
    __syncthreads();
    if (PRODUCE) {
      // ---- the group's test points, one after the other: k* into G, v = X k* (row tid / 4, as z above) -------------------
      double *ks = G, *red = G + 128;  // red: [8][2]
      const DevParams *Pq = Pp;
      asm volatile("" : "+s"(Pq));
      const DevParams &P = *Pq;
      const long long j1 = goff[k + 1];
      for (long long j = goff[k]; j < j1; ++j) {
        const double *zj = Z + j * D;
        if (tid < 128) {
          double kk = 0.0;
          if (tid < n) {
            const double *xi = X + (long)rows[tid] * D;
            kk = simil_value(P, [&](int d) { return xi[d]; }, [&](int d) { return zj[d]; });
          }
          ks[tid] = kk;
        }
        __syncthreads();
        const int i = tid >> 2, p = tid & 3;
        double a = 0.0;
        for (int q = p; q <= i; q += 4) a += S[i * SLD + q] * ks[q];
        a += __shfl_xor(a, 1);
        a += __shfl_xor(a, 2);
        double qq = (p == 0) ? a * a : 0.0, mm = (p == 0) ? ks[i] * as[i] : 0.0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          qq += __shfl_xor(qq, o);
          mm += __shfl_xor(mm, o);
        }
        if (lane == 0) {
          red[2 * wv] = qq;
          red[2 * wv + 1] = mm;
        }
        __syncthreads();
        if (tid == 0) {
          double qs = 0.0, ms = 0.0;
          for (int u = 0; u < NW; ++u) {
            qs += red[2 * u];
            ms += red[2 * u + 1];
          }
          const double prior = simil_value(P, [&](int d) { return zj[d]; }, [&](int d) { return zj[d]; });
          out0[j] = ms;
          if (out1) out1[j] = sqrt(prior - qs);
        }
        __syncthreads();  // ks and red are overwritten by the next point
      }
      return;
    }
    if (GRAD) {
      // ---- X_T^T X_T: the lower 16-tiles of the n rows in use, dealt to the waves; k = c .. n - 1 in steps of 4, a step's
      // rows >= n counted as zeros (they are the padding's identity rows, or past S: the address is clamped).  Tile row ti
      // needs k >= 16 ti only: X is lower triangular.
      const int nblk = (n + 15) >> 4, ntile = nblk * (nblk + 1) / 2, ksteps = (n - c + 3) >> 2;
      f64x4 m[5];
#pragma unroll
      for (int u = 0; u < 5; ++u) {
        m[u] = (f64x4){0.0, 0.0, 0.0, 0.0};
        const int tile = wv + u * NW;
        if (tile < ntile) {
          int ti, tj;
          vb_tile(tile, ti, tj);
          for (int ksi = ti * 16 > c ? (ti * 16 - c) >> 2 : 0; ksi < ksteps; ++ksi) {
            const int q = c + 4 * ksi + fk;
            const bool ok = q < n;
            const double *xr = S + (ok ? q : n - 1) * SLD;
            const double av = xr[ti * 16 + fr], bv = xr[tj * 16 + fr];
            m[u] = mfma(ok ? av : 0.0, ok ? bv : 0.0, m[u]);
          }
        }
      }
      __syncthreads();  // every wave has read X: S takes W
#pragma unroll
      for (int u = 0; u < 5; ++u) {
        const int tile = wv + u * NW;
        if (tile < ntile) {
          int ti, tj;
          vb_tile(tile, ti, tj);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int i = ti * 16 + fk + 4 * e, j = tj * 16 + fr;
            S[i * SLD + j] = as[i] * ds[j] + ds[i] * as[j] - ds[i] * ds[j] - m[u][e];
          }
        }
      }
      __syncthreads();
      // ---- the pair walk over the lower triangle (grad.hip's terms), thread tid: elements tid, tid + 512, ... of n rows ---------
      const DevParams *Pq = Pp;
      asm volatile("" : "+s"(Pq));
      const DevParams &P = *Pq;
      double acc[ACC_TRACE + 1];
#pragma unroll
      for (int q = 0; q <= ACC_TRACE; ++q) acc[q] = 0.0;
      double ard[ARD_D > 0 ? ARD_D : 1];
#pragma unroll
      for (int q = 0; q < (ARD_D > 0 ? ARD_D : 1); ++q) ard[q] = 0.0;
      for (int idx = tid; idx < n * 128; idx += NT) {
        const int i = idx >> 7, j = idx & 127;
        if (j <= i) {
          const double wv2 = S[i * SLD + j];
          const double wgt = (j < i) ? 2.0 * wv2 : wv2;
          const double *xi = X + (long)rows[i] * D, *xj = X + (long)rows[j] * D;
          simil_grad_accum<ARD_D>(
              P, [&](int d) { return xi[d]; }, [&](int d) { return xj[d]; }, wgt, acc, ard, ard0);
          if (i == j) acc[ACC_TRACE] += wv2;
        }
      }
      // the waves' sums of this block, added in wave order onto the workgroup's row
      double *red = G;  // [8][VB_SLOTS]; every wave is past its reads of G (the barriers above)
#pragma unroll
      for (int q = 0; q <= ACC_TRACE; ++q) {
        double t = acc[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
        if (lane == 0) red[wv * VB_SLOTS + q] = t;
      }
      if (ARD_D > 0) {
#pragma unroll
        for (int q = 0; q < (ARD_D > 0 ? ARD_D : 1); ++q) {
          double t = ard[q];
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
          if (lane == 0) red[wv * VB_SLOTS + ACC_TRACE + 1 + q] = t;
        }
      }
      __syncthreads();
      if (tid < NACC) {
        const bool base = tid <= ACC_TRACE, mine = ARD_D > 0 && tid >= ACC_ARD0 && tid < ACC_ARD0 + ARD_D;
        if ((base && ard0 == 0) || (mine && tid + ard0 < NACC)) {
          const int q = base ? tid : ACC_TRACE + 1 + (tid - ACC_ARD0);
          double t = 0.0;
          for (int u = 0; u < NW; ++u) t += red[u * VB_SLOTS + q];
          partials[(long)blockIdx.x * NACC + (base ? tid : tid + ard0)] += t;
        }
      }
    }
  }
}

// vecchia_final_kernel's sums in its order: value = sum_b vpart[b] (block order per thread, then a fixed tree) into out[0];
// info[0] = the lowest failing block + 1 of fpart, or 0.  One workgroup.
__global__ __launch_bounds__(256) void vblock_final_kernel(const double *__restrict__ vpart,
                                                           const long long *__restrict__ fpart, int nblocks,
                                                           double *__restrict__ out, long long *__restrict__ info) {
  __shared__ double red[4];
  __shared__ long long fred[4];
  double t = 0.0;
  long long f = 0;
  for (int b = threadIdx.x; b < nblocks; b += 256) {
    if (vpart) t += vpart[b];
    const long long fb = fpart[b];
    if (fb != 0 && (f == 0 || fb < f)) f = fb;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    t += __shfl_xor(t, o);
    const long long fo = __shfl_xor(f, o);
    if (fo != 0 && (f == 0 || fo < f)) f = fo;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t, fred[threadIdx.x >> 6] = f;
  __syncthreads();
  if (threadIdx.x == 0) {
    if (out) out[0] = red[0] + red[1] + red[2] + red[3];
    long long fm = 0;
    for (int u = 0; u < 4; ++u)
      if (fred[u] != 0 && (fm == 0 || fred[u] < fm)) fm = fred[u];
    info[0] = fm;
  }
}

}  // namespace gogp_vb

namespace gogp {

int vblocks_grid(int64_t nb, int max_grid) {
  const int64_t cap = max_grid > 0 && max_grid < VBLOCKS_GRID_MAX ? max_grid : VBLOCKS_GRID_MAX;
  return (int)(nb < cap ? (nb > 0 ? nb : 1) : cap);
}

// the rounds of one pass: round r takes the blocks r * grid .. (r + 1) * grid - 1
template <int AD, bool PR, bool GR>
static void vb_rounds(hipStream_t s, int grid, const DevParams *p, const double *X, const double *y, const double *v,
                      const int *tbl, const int *nc, const int *nt, int nb, int w, const double *Z, const long long *goff,
                      double *out0, double *out1, double *partials, double *vpart, long long *fpart, int ard0) {
  for (int k0 = 0; k0 < nb; k0 += grid)
    GOGP_KLAUNCH((gogp_vb::vblock_kernel<AD, PR, GR>), dim3(std::min(grid, nb - k0)), dim3(gogp_vb::NT), 0, s, p, X, y, v, tbl, nc,
                 nt, nb, w, Z, goff, out0, out1, partials, vpart, fpart, ard0, k0);
}

void launch_vblocks_observe(hipStream_t s, const DevParams *p, int ard_dims, const double *X, const double *y, const double *v,
                            const int *tbl, const int *nc, const int *nt, int nb, int w, double *terms, double *partials,
                            double *vpart, long long *fpart, double *gout, double *value, long long *info, int max_grid) {
  if (nb <= 0) return;
  const int grid = vblocks_grid(nb, max_grid);
  if (value) {
    (void)hipMemsetAsync(vpart, 0, (size_t)grid * sizeof(double), s);
    (void)hipMemsetAsync(fpart, 0, (size_t)grid * sizeof(long long), s);
    vb_rounds<0, false, false>(s, grid, p, X, y, v, tbl, nc, nt, nb, w, nullptr, nullptr, terms, nullptr, nullptr, vpart, fpart, 0);
    GOGP_KLAUNCH(gogp_vb::vblock_final_kernel, dim3(1), dim3(256), 0, s, (const double *)vpart, (const long long *)fpart, grid,
                 value, info);
  }
  if (!partials) return;
  (void)hipMemsetAsync(partials, 0, (size_t)grid * NACC * sizeof(double), s);
  if (ard_dims <= 0)
    vb_rounds<0, false, true>(s, grid, p, X, y, v, tbl, nc, nt, nb, w, nullptr, nullptr, nullptr, nullptr, partials, nullptr,
                              nullptr, 0);
  else  // ARD dimensions in passes of 8 accumulators, as launch_vecchia_observe
    for (int a0 = 0; a0 < ard_dims; a0 += 8)
      vb_rounds<8, false, true>(s, grid, p, X, y, v, tbl, nc, nt, nb, w, nullptr, nullptr, nullptr, nullptr, partials, nullptr,
                                nullptr, a0);
  launch_sparse_grad_final(s, partials, grid, gout, false);
}

void launch_vblocks_produce(hipStream_t s, const DevParams *p, const double *X, const double *y, const double *v,
                            const double *Z, const long long *goff, int ng, const int *tblz, int wz, const int *ncz, double *mu,
                            double *sigma, long long *fpart, long long *info, int max_grid) {
  if (ng <= 0) return;
  const int grid = vblocks_grid(ng, max_grid);
  (void)hipMemsetAsync(fpart, 0, (size_t)grid * sizeof(long long), s);
  vb_rounds<0, true, false>(s, grid, p, X, y, v, tblz, ncz, nullptr, ng, wz, Z, goff, mu, sigma, nullptr, nullptr, fpart, 0);
  GOGP_KLAUNCH(gogp_vb::vblock_final_kernel, dim3(1), dim3(256), 0, s, (const double *)nullptr, (const long long *)fpart, grid,
               (double *)nullptr, info);
}

}  // namespace gogp
