// vecchia.hip -- the kernel of Vecchia's approximation (gogp_vecchia_*; vecchia_api.hip orchestrates).
//
//     log p(y) ~ sum_i log p(y_i | y_c(i)),     c(i) a set of at most m <= 63 EARLIER rows (Vecchia 1988; Datta et al. 2016).
// Target i with conditioning rows c = c(i) in the table's order, q = |c|, block b = [c..., i] (the target LAST):
//     K_b = k(X_b, X_b) + diag(noise_var + v_b),   L = chol(K_b),   z = L^-1 y_b,
//     mu_i = y_i - L_qq z_q,   s_i = L_qq,   log p_i = -1/2 log 2 pi - log L_qq - 1/2 z_q^2.
// With alpha = L^-T z and r = L^-T e_q:  K_b^-1 - pad(K_c^-1) = r r^T  and  alpha - pad(alpha_c) = z_q r,  so
//     d log p_i / d log theta_p = 1/2 sum_ab W_ab dK_b,ab / d log theta_p,   W = e r^T + r e^T,   e = z_q alpha - 1/2 (1 + z_q^2) r:
// one factorisation, one forward and one two-column backward substitution per target, no inverse.  Produce: the target
// row is the test point with k(z, z) on its diagonal and no y: mu = sum_{t<q} L_qt z_t, sigma = L_qq.
//
// One wave owns one target at a time; a workgroup is ONE wave, so the barriers between the stages below are wave
// barriers and no two targets ever wait for each other.  Workgroup g of G = vecchia_blocks(targets) takes the targets
// g, g + G, ...: a function of the target count alone.  Everything of a block lives in LDS:
//     Ks  the lower triangle of K_b, then of L, row stride BS + 1 doubles (33 / 65: odd, so that the column walk -- lane i
//         reads element (i, k) -- and the row walk -- lane i reads (j, i) -- both touch every bank pair once per half wave
//         of a ds_read_b64);
//     Xs  the block's rows, stride ndim | 1 as kmm_kernel stages its rows;   es, rs  the vectors e and r;   rows  the indices.
// Stages per target: gather; Gram (pairs of the lower triangle over the lanes, simil_value); left-looking Cholesky with
// lane i owning row i (the sum over k runs in index order, so a target's bits depend on its block alone -- not on BS, not on
// what else is in the launch); column-oriented substitutions with lane i owning element i; the pair walk of the gradient
// through simil_grad_accum into grad.hip's slot layout (off-diagonal pairs twice, ACC_TRACE takes sum W_aa: the
// convention of batch_eval_kernel, so api.hip's assemble_gradient applies).  A pivot that is not positive and finite
// ends that target only: its terms are NaN, it adds nothing to the sums, and the workgroup remembers its lowest one.
// A wave keeps its slot sums and its sum of log p in registers across its targets and writes one row per workgroup;
// launch_sparse_grad_final adds the rows in block order, vecchia_final_kernel the values (block order per thread, then a
// fixed tree) and takes the lowest failing target.  No atomics, no spin-waits: identical calls give identical bits.
// The value and the gradient are separate passes (instances) over the same stages: fused, they exceed the register
// limits of tools/codeobj_audit.py.
// The matrix cores are not used: a block of at most 64 rows gives the trailing update too few 16 x 16 x 4 tiles to pay
// for moving the operands between LDS and the fragment layout ("Vecchia").
#include <algorithm>
#include <type_traits>

#include "kern_eval.h"

namespace gogp {

// the value of lane `src` (wave-uniform) in every lane, as a scalar
__device__ __forceinline__ double vc_bcast(double x, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(x), src);
  return __hiloint2double(hi, lo);
}

// pair p of the lower triangle in row-major order: (a, b), b <= a
__device__ __forceinline__ void vc_pair(int p, int &a, int &b) {
  a = (int)((sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);
  while (a * (a + 1) / 2 > p) --a;
  while ((a + 1) * (a + 2) / 2 <= p) ++a;
  b = p - a * (a + 1) / 2;
}

// BS: the largest block (rows) of the instance.  Three roles:
// value (PRODUCE, GRAD false): targets are the rows of X, the table is causal; out0 = terms (N x 3: mu, s, log p; may be
//   nullptr), vpart / fpart the workgroup's sum of log p and its lowest failing target + 1.
// gradient (GRAD): the same targets through the backward substitution and the pair walk; only `partials` is written, a
//   failing target is skipped.  ARD_D: ARD accumulators of a pass (dimensions ard0 .. ard0 + ARD_D - 1; the pass with
//   ard0 == 0 writes every slot, a later one only its own).
// produce (PRODUCE): targets are the rows of Z, out0 = mu, out1 = sigma (may be nullptr), fpart as above.
// Only Pp is read with scalar loads; the data pointers are moved to vector registers at entry (they are only ever used
// with per-lane addresses), which keeps the scalar registers under the audit's spill limit.
template <int BS, int ARD_D, bool PRODUCE, bool GRAD>
__global__ __launch_bounds__(64) void vecchia_kernel(const DevParams *__restrict__ Pp, const double *__restrict__ X,
                                                     const double *__restrict__ y, const double *__restrict__ v,
                                                     const double *__restrict__ Z, long ntargets,
                                                     const int *__restrict__ nbr, int m, double *__restrict__ out0,
                                                     double *__restrict__ out1, double *__restrict__ partials,
                                                     double *__restrict__ vpart, long long *__restrict__ fpart, int ard0) {
  extern __shared__ double sm[];
  asm volatile("" : "+v"(X), "+v"(y), "+v"(v), "+v"(nbr));
  if (PRODUCE) asm volatile("" : "+v"(Z), "+v"(out0), "+v"(out1), "+v"(fpart));
  else if (GRAD) asm volatile("" : "+v"(partials));
  else asm volatile("" : "+v"(out0), "+v"(vpart), "+v"(fpart));
  constexpr int KS = BS + 1;
  const DevParams &P = *Pp;
  const int D = P.ndim;
  const int xs = D | 1;
  double *Ks = sm;                 // [BS][KS]
  double *es = Ks + BS * KS;       // [BS]
  double *rs = es + BS;            // [BS]
  double *Xs = rs + BS;            // [BS][xs]
  int *rows = reinterpret_cast<int *>(Xs + BS * xs);  // [BS]
  const int lane = threadIdx.x;

  double acc[ACC_TRACE + 1];
#pragma unroll
  for (int s = 0; s <= ACC_TRACE; ++s) acc[s] = 0.0;
  double ard[ARD_D > 0 ? ARD_D : 1];
#pragma unroll
  for (int s = 0; s < (ARD_D > 0 ? ARD_D : 1); ++s) ard[s] = 0.0;
  double vsum = 0.0;
  long long fail = 0;  // lowest failing target + 1

  for (long i = blockIdx.x; i < ntargets; i += gridDim.x) {
    __syncthreads();  // the previous target's readers are done
    int mine = -1;
    if (lane < m) mine = nbr[i * m + lane];
    const int q = __builtin_popcountll(__ballot(mine >= 0));  // the padding is trailing (gogp_vecchia_check)
    const int n = q + 1;
    if (lane < q) rows[lane] = mine;
    __syncthreads();
    const double *trow = PRODUCE ? Z + i * D : X + i * D;
    for (int idx = lane; idx < n * D; idx += 64) {
      const int r = idx / D, d = idx - r * D;
      const double *src = r < q ? X + (long)rows[r] * D : trow;
      Xs[r * xs + d] = src[d];
    }
    // lane a < n: the right-hand side and the diagonal's addition of row a of the block
    double w = 0.0, dg = 0.0;
    if (lane < n && !(PRODUCE && lane == q)) {
      const long g = lane < q ? (long)mine : i;
      w = y[g];
      dg = v ? P.noise_var + v[g] : P.noise_var;
    }
    __syncthreads();
    // ---- Gram: the lower triangle ---------------------------------------------------------------------------------------
    const int npairs = n * (n + 1) / 2;
    for (int p = lane; p < npairs; p += 64) {
      int a, b;
      vc_pair(p, a, b);
      const double *xa = Xs + a * xs, *xb = Xs + b * xs;
      Ks[a * KS + b] = simil_value(
          P, [&](int d) { return xa[d]; }, [&](int d) { return xb[d]; });
    }
    __syncthreads();
    if (lane < n) Ks[lane * KS + lane] += dg;
    __syncthreads();
    // ---- Cholesky, left-looking: lane i forms column j of its row ------------------------------------------------------------
    double dj = 1.0;  // L_ii of this lane's row
    bool bad = false;
    for (int j = 0; j < n; ++j) {
      double s = 0.0;
      if (lane >= j && lane < n) {
        const double *li = Ks + lane * KS, *lj = Ks + j * KS;
        s = li[j];
        for (int k = 0; k < j; ++k) s -= li[k] * lj[k];
      }
      const double d = vc_bcast(s, j);
      if (!(d > 0.0) || !(d < INFINITY)) {
        bad = true;
        break;
      }
      const double l = sqrt(d);
      if (lane == j) {
        dj = l;
        Ks[lane * KS + j] = l;
      } else if (lane > j && lane < n) {
        Ks[lane * KS + j] = s / l;
      }
      __syncthreads();
    }
    if (bad) {
      if (fail == 0) fail = i + 1;
      if (!GRAD && lane == 0) {
        if (PRODUCE) {
          out0[i] = NAN;
          if (out1) out1[i] = NAN;
        } else if (out0) {
          out0[3 * i + 0] = NAN, out0[3 * i + 1] = NAN, out0[3 * i + 2] = NAN;
        }
      }
      continue;
    }
    // ---- forward substitution: lane j ends with z_j -------------------------------------------------------------------
    double zme = 0.0;
    for (int j = 0; j < n; ++j) {
      const double zj = vc_bcast(w / dj, j);
      if (lane == j) zme = zj;
      if (lane > j && lane < n) w -= Ks[lane * KS + j] * zj;
    }
    const double lqq = vc_bcast(dj, q);
    if (PRODUCE) {
      // y = 0 on the target row: what the loop left in lane q before its division is -sum_{t<q} L_qt z_t
      const double mu = -vc_bcast(w, q);
      if (lane == 0) {
        out0[i] = mu;
        if (out1) out1[i] = lqq;
      }
      continue;
    }
    const double zq = vc_bcast(zme, q);
    if (!GRAD) {  // the value alone
      const double logp = -0.5 * log(2.0 * GOGP_PI) - log(lqq) - 0.5 * zq * zq;
      vsum += logp;
      if (out0 && lane == 0) {
        out0[3 * i + 0] = y[i] - lqq * zq;
        out0[3 * i + 1] = lqq;
        out0[3 * i + 2] = logp;
      }
      continue;
    }
    // ---- backward substitution on two columns: alpha = L^-T z, r = L^-T e_q ------------------------------------------------
    double a = zme, b = lane == q ? 1.0 : 0.0, al = 0.0, rr = 0.0;
    for (int j = n - 1; j >= 0; --j) {
      const double aj = vc_bcast(a / dj, j), rj = vc_bcast(b / dj, j);
      if (lane == j) al = aj, rr = rj;
      if (lane < j) {
        const double l = Ks[j * KS + lane];
        a -= l * aj;
        b -= l * rj;
      }
    }
    if (lane < n) {
      es[lane] = zq * al - 0.5 * (1.0 + zq * zq) * rr;
      rs[lane] = rr;
    }
    __syncthreads();
    // ---- the pair walk: W_ab = e_a r_b + r_a e_b, off-diagonal pairs twice ---------------------------------------------------
    for (int p = lane; p < npairs; p += 64) {
      // the parameters are read again per pair (scalar loads): hoisted out of the target loop they cost more SGPRs than
      // the audit's spill limit allows
      const DevParams *Pq = Pp;
      asm volatile("" : "+s"(Pq));
      const DevParams &P = *Pq;
      int pa, pb;
      vc_pair(p, pa, pb);
      const double wv = es[pa] * rs[pb] + rs[pa] * es[pb];
      const double wgt = pb < pa ? 2.0 * wv : wv;
      const double *xa = Xs + pa * xs, *xb = Xs + pb * xs;
      simil_grad_accum<ARD_D>(
          P, [&](int d) { return xa[d]; }, [&](int d) { return xb[d]; }, wgt, acc, ard, ard0);
      if (pa == pb) acc[ACC_TRACE] += wv;
    }
  }

  if (PRODUCE) {
    if (lane == 0) fpart[blockIdx.x] = fail;
    return;
  }
  if (!GRAD) {
    if (lane == 0) {
      vpart[blockIdx.x] = vsum;
      fpart[blockIdx.x] = fail;
    }
    return;
  }
  // ---- the wave's slot sums: a fixed butterfly, one row per workgroup -----------------------------------------------------------
  double *row = partials + (long)blockIdx.x * NACC;
#pragma unroll
  for (int s = 0; s <= ACC_TRACE; ++s) {
    double t = acc[s];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
    if (ard0 == 0 && lane == 0) row[s] = t;
  }
  if (ard0 == 0)  // the first pass writes every slot: zeros in the ones no pass of this launch owns
    for (int s = ACC_TRACE + 1 + lane; s < NACC; s += 64)
      if (!(ARD_D > 0 && s >= ACC_ARD0 && s < ACC_ARD0 + ARD_D)) row[s] = 0.0;
  if (ARD_D > 0) {
#pragma unroll
    for (int s = 0; s < (ARD_D > 0 ? ARD_D : 1); ++s) {
      double t = ard[s];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
      if (lane == 0 && ACC_ARD0 + ard0 + s < NACC) row[ACC_ARD0 + ard0 + s] = t;
    }
  }
}

// value = sum_b vpart[b] (block order per thread, then a fixed tree) into out[0]; info[0] = the lowest failing target + 1 of
// fpart, or 0.  One workgroup.
__global__ __launch_bounds__(256) void vecchia_final_kernel(const double *__restrict__ vpart,
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

int vecchia_blocks(int64_t targets, int max_blocks) {
  const int64_t cap = max_blocks > 0 && max_blocks < VECCHIA_BLOCKS_MAX ? max_blocks : VECCHIA_BLOCKS_MAX;
  return (int)(targets < cap ? (targets > 0 ? targets : 1) : cap);
}

static size_t vecchia_lds_bytes(int bs, int ndim) {
  return ((size_t)bs * (bs + 1) + 2 * (size_t)bs + (size_t)bs * (ndim | 1)) * sizeof(double) + (size_t)bs * sizeof(int);
}

template <int BS, int AD, bool PR, bool GR>
static void vc_launch(hipStream_t s, int blocks, const DevParams *p, int ndim, const double *X, const double *y,
                      const double *v, const double *Z, long nt, const int *nbr, int m, double *out0, double *out1,
                      double *partials, double *vpart, long long *fpart, int ard0) {
  const size_t lds = vecchia_lds_bytes(BS, ndim);
  if (lds > 64 * 1024)  // BS = 64 beyond ndim = 61: raised per launch (the attribute belongs to the function on the current device)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&vecchia_kernel<BS, AD, PR, GR>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)vecchia_lds_bytes(BS, GOGP_MAX_NDIM));
  GOGP_KLAUNCH((vecchia_kernel<BS, AD, PR, GR>), dim3(blocks), dim3(64), lds, s, p, X, y, v, Z, nt, nbr, m, out0, out1, partials,
               vpart, fpart, ard0);
}

void launch_vecchia_observe(hipStream_t s, const DevParams *p, int ndim, int ard_dims, const double *X, const double *y,
                            const double *v, int64_t N, const int *nbr, int m, double *terms, double *partials,
                            double *vpart, long long *fpart, double *gout, double *value, long long *info, int max_blocks) {
  if (N <= 0) return;
  const int blocks = vecchia_blocks(N, max_blocks);
  auto pass = [&](auto bs, auto ad, auto gr, int a0) {
    vc_launch<decltype(bs)::value, decltype(ad)::value, false, decltype(gr)::value>(
        s, blocks, p, ndim, X, y, v, nullptr, (long)N, nbr, m, terms, nullptr, partials, vpart, fpart, a0);
  };
  using I32 = std::integral_constant<int, 32>;
  using I64 = std::integral_constant<int, 64>;
  using A0 = std::integral_constant<int, 0>;
  using A8 = std::integral_constant<int, 8>;
  const bool small = m + 1 <= 32;
  if (value) {
    if (small) pass(I32(), A0(), std::false_type(), 0);
    else pass(I64(), A0(), std::false_type(), 0);
    GOGP_KLAUNCH(vecchia_final_kernel, dim3(1), dim3(256), 0, s, (const double *)vpart, (const long long *)fpart, blocks,
                 value, info);
  }
  if (!partials) return;
  if (ard_dims <= 0) {
    if (small) pass(I32(), A0(), std::true_type(), 0);
    else pass(I64(), A0(), std::true_type(), 0);
  } else {
    // ARD dimensions in passes of 8 accumulators, as launch_sparse_grad; a later pass repeats the block's factorisation
    for (int a0 = 0; a0 < ard_dims; a0 += 8) {
      if (small) pass(I32(), A8(), std::true_type(), a0);
      else pass(I64(), A8(), std::true_type(), a0);
    }
  }
  if (partials) launch_sparse_grad_final(s, partials, blocks, gout, false);
}

void launch_vecchia_produce(hipStream_t s, const DevParams *p, int ndim, const double *X, const double *y, const double *v,
                            const double *Z, int64_t mz,
                            const int *nbrz, int m, double *mu, double *sigma, long long *fpart, long long *info,
                            int max_blocks) {
  if (mz <= 0) return;
  const int blocks = vecchia_blocks(mz, max_blocks);
  if (m + 1 <= 32)
    vc_launch<32, 0, true, false>(s, blocks, p, ndim, X, y, v, Z, (long)mz, nbrz, m, mu, sigma, nullptr, nullptr, fpart, 0);
  else
    vc_launch<64, 0, true, false>(s, blocks, p, ndim, X, y, v, Z, (long)mz, nbrz, m, mu, sigma, nullptr, nullptr, fpart, 0);
  GOGP_KLAUNCH(vecchia_final_kernel, dim3(1), dim3(256), 0, s, (const double *)nullptr, (const long long *)fpart, blocks,
               (double *)nullptr, info);
}

}  // namespace gogp
