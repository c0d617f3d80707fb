// common.h -- shared declarations of libgogp_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/gogp_hip.h"
#include "graphrec.h"

namespace gogp {

// Blocking constants.  TILE is the GEMM workgroup tile and the diagonal-block
// size; PANEL is the rank of one trailing update (2 diagonal blocks).
constexpr int TILE = 128;
constexpr int PANEL = 256;
constexpr int GEMM_BK = 16;

// Device-side copy of the kernel description + current hyperparameters.
// Lives in device memory; every field is read with wave-uniform (scalar) loads.
struct DevParams {
  int ndim, nterms, ns, nn;
  int kind[GOGP_MAX_TERMS];
  int ard[GOGP_MAX_TERMS];
  double c[GOGP_MAX_TERMS];  // output scale of the term (1 if it has none)
  double w[GOGP_MAX_TERMS];  // PERIODIC: pi / (period_mult * theta_p)
  double inv_len[GOGP_MAX_TERMS][GOGP_MAX_NDIM];  // 1/l_d (all equal unless ard)
  double noise_var;  // value added on the diagonal
  double dnoise;     // d noise_var / d log(std)  (0 for ConstantNoise)
  // event discounts (gogp_set_events; kern_eval.h: event_mask).  Appended: the fields above keep their offsets,
  // and only the kernel instances compiled with events (template flag EV) read these.
  int nevents, ev_axis;
  double ev_from[GOGP_MAX_EVENTS], ev_to[GOGP_MAX_EVENTS], ev_disc[GOGP_MAX_EVENTS];
};

// Accumulator slots of the fused gradient reduction (see grad.hip):
//   slot 3*t+0: d/dlog scale of term t, 3*t+1: d/dlog len (non-ARD),
//   3*t+2: d/dlog period; slot 12: trace(W) (noise); 16+d: ARD length d.
constexpr int ACC_TRACE = 3 * GOGP_MAX_TERMS;
constexpr int ACC_ARD0 = 16;
constexpr int NACC = ACC_ARD0 + GOGP_MAX_NDIM;

// Candidate batching (gogp_observe_gradient_candidates): one launch sequence evaluates k hyper-
// parameter candidates on the same data.  Every per-candidate buffer of candidate c lies
// c * stride BYTES after candidate 0's (one arena slot per candidate, api.hip); the launchers
// below that are on the Observe + Gradient path put the candidate index on gridDim.z and the
// kernels shift their per-candidate pointers by blockIdx.z * stride.  Inputs (X, y) are shared.
// The orchestrating thread sets tl_batch for the duration of the call; {1, 0} otherwise.
struct Batch {
  int k = 1;
  long stride = 0;
};
inline thread_local Batch tl_batch;
template <class P>
__device__ __forceinline__ P *cand(P *p, long bstride) {
  return (P *)((const char *)p + (long)blockIdx.z * bstride);
}

struct GemmProfile {
  bool on = false;
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  double flops = 0;
  int64_t launches = 0;
  // per launch, in launch order (the events are pool[2i], pool[2i+1]): flops and a tag
  // mode * 1e8 + (K / 16) * 1e5 + min(tiles, 99999) (gemm_plan.h) -- see gogp_profile_read_launches
  std::vector<double> lflops;
  std::vector<int64_t> ltag;
};

// Tile filter of the tile kernel in a sharded (2-D block-cyclic) evaluation (GemmArgs in
// gemm_tile.h): the launch covers LOCAL 128-tiles starting at local row / column block
// rblk0 / cblk0 (a distribution block = 2^tpb_shift tiles); this rank sits at (pr, pc) of
// the Pr x Pc process grid.  rule 1: keep the tiles of the GLOBAL lower triangle; rule 2:
// the same, and tiles of global row block beta0 overwrite C (beta = 0) while the others
// accumulate (beta = 1): the rank-k updates of K^-1 = Y Y^T.
// GEMM_LOWER only: new_row0 >= 0 -- tile rows ti >= new_row0 (128-tiles) overwrite C (beta = 0), the
// rows above them accumulate with the launch's beta: the rank-k updates K^-1 (+)= Y_P Y_P^T of the
// fused sweep (api.hip), whose newest block rows have no earlier contribution.
struct GemmGrid {
  int rule = 0, tpb_shift = 0, rblk0 = 0, cblk0 = 0, pr = 0, Pr = 1, pc = 0, Pc = 1, beta0 = -1;
  int new_row0 = -1;
  // GEMM_RECT: B (nt*128 x K) is lower triangular (a block inverse: the panel solves L21 = A21 inv(L11)^T):
  // tile column tj only sums k < (tj + 1) * tile -- the rest of its rows of B is zero
  int ktri = 0;
  // the launch sits on a dependency chain (panel solves, look-ahead updates): its waves raise their issue
  // priority (s_setprio 3), so that on a CU they share with bulk workgroups their MFMAs go first
  int prio = 0;
  // GEMM_RECT / GEMM_LOWER: the rows of A from tile row krag0 (128-tiles) on are upper triangular against the K
  // range (a super-panel of Y = L^-T with its triangular diagonal part: api.hip, trtri_superstep), so a workgroup
  // tile row starts at k = (its first row - krag0 * 128).  The launches on 64 x 64 tiles count that in 64-row
  // steps: row krag0 * 128 + r of A must be zero for k < 64 * floor(r / 64) -- zero per 128-row block (k < 128 i
  // in block krag0 + i) is NOT enough there (rows 64..127 of the block skip [128 i, 128 i + 64) too).  Y is zero
  // left of its diagonal element by element, which covers both.  -1: none.
  int krag0 = -1;
  // launches with fewer 128-tiles than this use 64 x 64 tiles (default 384).  Alone on the GPU the 64-tile shape wins
  // up to ~3000 tiles (820 tiles at K = 768: 61 against 51 TFLOP/s); inside an evaluation, beside other streams'
  // launches, it loses -- so only Produce, which runs alone, raises it.
  int small_below = 384;
  // GEMM_LAUUM in two launches (api.hip: option "kinv_split"): tile (ti, tj) sums k >= max(ti * 128, kbeg0) and the
  // tile rows above kbeg0 ACCUMULATE into C (the first launch, K = kbeg0, left their sums over k < kbeg0 there)
  int kbeg0 = 0;
};

// Local <-> global index map of the 2-D block-cyclic layout: distribution blocks of
// nb = 2^nb_shift rows / columns; local row block bi of the rank at grid row pr is global block
// bi * Pr + pr (columns: pc, Pc).
struct BlockMap {
  int nb_shift = 9, pr = 0, Pr = 1, pc = 0, Pc = 1;
  __host__ __device__ long grow(long lrow) const {
    const long nbm = (1L << nb_shift) - 1;
    return ((((lrow >> nb_shift) * Pr + pr)) << nb_shift) + (lrow & nbm);
  }
  __host__ __device__ long gcol(long lcol) const {
    const long nbm = (1L << nb_shift) - 1;
    return ((((lcol >> nb_shift) * Pc + pc)) << nb_shift) + (lcol & nbm);
  }
};

// ---- per-workgroup time stamps (probe build only: make stamp -> tools/exp/lib_stamp.so, -DGOGP_WGSTAMP) -----------------
// where INSIDE a launch of the chain's tile kernel / the diagonal-block kernel the time goes
// when it runs beside the bulk updates.  Every workgroup of those kernels writes s_memrealtime (100 MHz, one clock for the
// whole chip) at entry / operands of the first k-step in LDS / last k-step done / stores drained, plus HW_ID and XCC_ID,
// into a buffer the probe (tools/wg_stamps.py) hands in through these globals; one record per launch says which slice of
// the buffer is whose.  The product library is built without the macro and contains none of this.
#ifdef GOGP_WGSTAMP
struct StampRec {
  long long base, nwg, tag, stream;
};
constexpr int STAMP_SLOTS = 8;
extern unsigned long long *g_stamp_buf;  // device buffer, STAMP_SLOTS x g_stamp_cap entries
extern long long g_stamp_cap, g_stamp_used, g_stamp_nrec;
extern StampRec g_stamp_rec[1 << 16];
// reserve nwg workgroup slots for a launch; nullptr when the probe is not armed or the buffer is full
unsigned long long *stamp_reserve(long long nwg, long long tag, hipStream_t s);
#endif

// ---- launchers implemented in the .hip files ------------------------------
enum GemmMode { GEMM_RECT = 0, GEMM_LOWER = 1, GEMM_LAUUM = 2,
                // GEMM_RECT whose tiles in strictly upper 256x256 blocks (block column > block row,
                // counted from the C origin) are skipped: several adjacent block columns updated
                // "each from its own diagonal block down" in ONE launch
                GEMM_TRAP = 3 };

// C(mt*128 x nt*128) = beta*C + alpha * A * B^T, row-major, K multiple of 16.
// GEMM_LOWER: square tile grid mt x mt, only tiles ti >= tj.
// GEMM_LAUUM: lower tiles; tile (ti,tj) sums k over [ti*128, K).
void launch_dgemm_nt(hipStream_t s, GemmMode mode, int mt, int nt, int64_t K,
                     double alpha, const double *A, int64_t lda, const double *B,
                     int64_t ldb, double beta, double *C, int64_t ldc,
                     GemmProfile *prof, const GemmGrid *grid = nullptr);

// fp32 path (BASELINE config 5): the same launchers overloaded on the MATRIX element type.
// Inputs, vectors (y, z, alpha) and every reduction stay fp64; only the N x N matrices
// (K / L / Y / K^-1, the block inverses, the Produce workspaces) are float.
void launch_gemm_nt(hipStream_t s, GemmMode mode, int mt, int nt, int64_t K, double alpha, const double *A,
                    int64_t lda, const double *B, int64_t ldb, double beta, double *C, int64_t ldc,
                    GemmProfile *prof, const GemmGrid *grid = nullptr);  // = launch_dgemm_nt
void launch_gemm_nt(hipStream_t s, GemmMode mode, int mt, int nt, int64_t K, double alpha, const float *A,
                    int64_t lda, const float *B, int64_t ldb, double beta, float *C, int64_t ldc,
                    GemmProfile *prof, const GemmGrid *grid = nullptr);  // sgemm.hip; both: gemm_tile.h, launch_tile_gemm
void launch_gram_lower_split(hipStream_t s_first, hipStream_t s_rest, const DevParams *p, int ndim,
                             const double *X, int64_t n, int64_t npad, float *K, int64_t ld,
                             int64_t wcols, bool ev = false);
void launch_cross(hipStream_t s, const DevParams *p, int ndim, const double *X, int64_t n,
                  int64_t npad, const double *Z, int64_t m, int64_t mpad, float *KsT, int64_t ld, bool ev = false);
void launch_trsv_fwd_step(hipStream_t s, const float *L, int64_t ld, const float *Dinv, int b, int nblk,
                          double *y, double *z);
void launch_trsv_bwd_step(hipStream_t s, const float *L, int64_t ld, const float *Dinv, int b, int nblk,
                          double *zwork, double *alpha);
void launch_lml_scalars(hipStream_t s, const float *L, int64_t ld, const double *z, const double *y,
                        const double *alpha, int64_t n, double *scalars);
void launch_alpha_from_y(hipStream_t s, const float *Y, int64_t ld, const double *z, int64_t npad,
                         double *alpha);
void launch_rownorm_dot(hipStream_t s, const float *V, int64_t ld, const double *vec, int64_t ncols,
                        int64_t m, double *dot, double *sq);
void launch_zero_upper_blocks(hipStream_t s, float *R, int64_t ld, int64_t npad);
void launch_zero_block(hipStream_t s, float *B, int64_t ld, int64_t rows, int64_t cols);
void launch_ydiag(hipStream_t s, const float *Dinv, float *Ydiag, int64_t ld);
void launch_extract_lower(hipStream_t s, const float *L, int64_t ld, int64_t n, double *out);
void launch_pack_lower(hipStream_t s, const double *in, int64_t n, int64_t npad, float *L, int64_t ld);
void launch_convert_block(hipStream_t s, const float *src, int64_t lds_, double *dst, int64_t ldd, int rows,
                          int cols);
void launch_convert_block(hipStream_t s, const double *src, int64_t lds_, float *dst, int64_t ldd, int rows,
                          int cols);
void launch_grad_reduce(hipStream_t s, const DevParams *p, int ndim, int ard_dims, const double *X,
                        const double *alpha, const float *Kinv, int64_t ld, int64_t n, int64_t npad,
                        double *partials, double *out, bool radial1 = false, int mfma_min_dims = 1, bool ev = false,
                        int max_blocks = 0);

// gram.hip.  What every launcher of it below relies on (the test hooks of include/gogp_testhooks.h refuse the rest):
//  - npad, mpad, mrows, ncols are positive multiples of 64 and ld covers the padded width; the kernels write WHOLE
//    64 x 64 tiles, so the output holds all npad (cross: mpad; local: mrows) rows.
//  - X holds npad rows of ndim doubles that may be READ, whatever they hold: with one radial term (nterms == 1, not
//    periodic) gram_kernel<false>, gram_local_kernel and kmatvec_kernel<true> read rows n .. npad - 1 unguarded, through
//    scalar loads, and keep them out of every result.  Z (launch_cross, launch_prior) and v are read guarded: rows < m / n.
//  - radial1 (launch_residual, launch_kmatvec_share) may be set only with one radial term; false there selects the
//    generic instance, which returns the same.
//  - ev is never combined with an ARD term (gogp_set_events refuses it).
//  - launch_gram_lower_split: wcols is a multiple of 64 and at least 64 (0 would launch an empty grid); beyond npad it is
//    clipped, and the second launch is skipped.  Tiles above the diagonal are not written.
// Local tiles (mrows x ncols) of a 2-D block-cyclic Gram matrix: tiles of the global lower
// triangle get kernel values (identity padding for rows >= n), distribution blocks strictly
// above the diagonal are zero-filled (the work area R of the triangular inverse); the 64-tiles above the diagonal
// inside a diagonal distribution block (nb >= 128) are not written.
void launch_gram_local(hipStream_t s, const DevParams *p, int ndim, const double *X, int64_t n,
                       int64_t mrows, int64_t ncols, BlockMap map, double *K, int64_t ld, bool ev = false);
void launch_gram_local(hipStream_t s, const DevParams *p, int ndim, const double *X, int64_t n,
                       int64_t mrows, int64_t ncols, BlockMap map, float *K, int64_t ld, bool ev = false);
void launch_gram_lower_split(hipStream_t s_first, hipStream_t s_rest, const DevParams *p, int ndim,
                             const double *X, int64_t n, int64_t npad, double *K, int64_t ld,
                             int64_t wcols, bool ev = false);
// KsT (mpad x npad): KsT[j][i] = k(x_i, z_j); zero for i >= n or j >= m.
void launch_cross(hipStream_t s, const DevParams *p, int ndim, const double *X, int64_t n,
                  int64_t npad, const double *Z, int64_t m, int64_t mpad, double *KsT,
                  int64_t ld, bool ev = false);
// r = y - K v with K recomputed in fp64 on the fly (iterative refinement of alpha on the fp32 path);
// part: nslab * npad doubles of scratch
void launch_residual(hipStream_t s, const DevParams *p, int ndim, const double *X, int64_t n, int64_t npad,
                     const double *v, const double *y, double *part, int nslab, double *r, bool radial1 = false,
                     bool ev = false);
void launch_kmatvec_share(hipStream_t s, const DevParams *p, int ndim, const double *X, int64_t n, int64_t npad,
                          const double *v, int part_idx, int nparts, double *part, int nslab, double *out,
                          bool radial1 = false, bool ev = false);
void launch_prior(hipStream_t s, const DevParams *p, const double *Z, int64_t m,
                  double *prior);

// forward / backward substitution steps with the stored 256x256 block inverses
// (b, nb count 256-blocks)
void launch_trsv_fwd_step(hipStream_t s, const double *L, int64_t ld, const double *Dinv,
                          int b, int nblk, double *y, double *z);
void launch_trsv_bwd_step(hipStream_t s, const double *L, int64_t ld, const double *Dinv,
                          int b, int nblk, double *zwork, double *alpha);

// scalars[0] = sum_i 2 log L_ii, scalars[1] = sum z_i^2, scalars[2] = sum y_i alpha_i
// (i < n; the last only when alpha != nullptr: exactly 0 otherwise), scalars[3], [4] = min, max L_ii; scalars[5 ..] are left
// alone.  Reads the diagonal of L and z, y, alpha on i < n only; one workgroup, any n >= 0.  Batched: L, z, alpha and
// scalars lie tl_batch.stride bytes apart per candidate, y is shared.
void launch_lml_scalars(hipStream_t s, const double *L, int64_t ld, const double *z,
                        const double *y, const double *alpha, int64_t n, double *scalars);
// potrf + dense inverse of one 256x256 diagonal block (diag256.hip); Dinv has
// leading dimension 256.  A (ld): in: lower triangle of the block; Lout (ldl): out: lower
// factor (upper zeroed); Dinv: out: dense inverse of the factor (upper zero).  info: device
// int64, set to (row0+j+1) at the first non-positive pivot with row0+j < nvalid (first
// failure wins).
void launch_diag256(hipStream_t s, const double *A, int64_t ld, double *Lout, int64_t ldl,
                    double *Dinv, int64_t row0, int64_t nvalid, long long *info);
// the same with Dinv written into a 256x256 sub-block of a matrix of leading dimension 512
void launch_diag256_ld512(hipStream_t s, const double *A, int64_t ld, double *Lout, int64_t ldl,
                          double *Dinv, int64_t row0, int64_t nvalid, long long *info);
void launch_diag256_inv_only(hipStream_t s, const double *L, int64_t ld, double *Dinv);
// diagsyrk.hip (fp32 path, option "diag_fp64"): D64 block b (256 x 256 doubles, b < nblocks) -= R_b R_b^T with R_b the
// 256 x K float rows at Lrows + b * 256 * ld, summed in fp64; and the strip's start: the float diagonal blocks widened
void launch_diag_syrk_f64(hipStream_t s, const float *Lrows, int64_t ld, int64_t K, double *D64, int nblocks);
void launch_widen_diag_blocks(hipStream_t s, const float *A, int64_t ld, double *D64, int nblocks);
// the same for blocks of bs x bs (256 or 512) whose rows start row_stride floats apart (the diagonal tiles of a shard)
void launch_diag_syrk_f64_tiles(hipStream_t s, const float *Lrows, int64_t ld, int64_t K, double *D64, int nblocks,
                                int64_t row_stride, int bs);
// panel128.hip (option "chain_split" = 2): one 128-column step of the Cholesky chain in one launch -- the diagonal 128-block of
// half 0 / 1 of the 256-block at A is factored and the rows_below (multiple of 64) rows under it are solved against it
void launch_panel128(hipStream_t s, const double *A, int64_t ld, double *Lout, int64_t ldl, int half, int64_t rows_below,
                     int64_t row0, int64_t nvalid, long long *info);
// the same with the number of 64-row slabs per workgroup forced (0: by size); the result does not depend on it
void launch_panel128_slabs(hipStream_t s, const double *A, int64_t ld, double *Lout, int64_t ldl, int half,
                           int64_t rows_below, int64_t row0, int64_t nvalid, long long *info, int slabs);
// diag256.hip: a whole evaluation of n <= 128 observations in one launch (npad = 256): Gram matrix, factor, block inverse, z,
// alpha and (want_kinv) K^-1, left where the general path leaves them (A: K^-1 lower, L, Dinv: leading dimension 256)
void launch_tiny_eval(hipStream_t s, const DevParams *P, const double *X, const double *y, int64_t n, double *A, double *L,
                      double *Dinv, double *z, double *alpha, long long *info, bool want_kinv, bool ev = false);
// diag256.hip: batches of small GPs (gogp_batch_*), one workgroup per (member, theta) pair.  Pair b evaluates rows
// off .. off + n - 1 (n <= 128) of the batch data at P and writes row b of `rows` (BATCH_ROW doubles: the scalars of
// judge_scalars in [0..15], the NACC gradient slot sums from [16] on) or, produce, mu / sigma of Z's rows zoff .. zoff + m - 1
// Full Observe form (gogp_batch_*_full): the pair's observations ride in its own parameter vector.  X is the upload of
// the k vectors; the pair's inputs (n x D) start at double `off` of it and its outputs follow them; its results go to
// the block at double `roff` of `rows`: the BATCH_ROW doubles above, then (Observe) the n * D input gradients and the
// n output gradients -alpha.
struct BatchItem {
  DevParams P;
  long off, n;
  long zoff, m;
  long roff;  // full form only
};
constexpr int BATCH_ROW = NACC + 16;
void launch_batch_eval(hipStream_t s, const BatchItem *items, int k, const double *X, const double *y, const double *Z,
                       double *rows, double *mu, double *sigma, int ard_dims, bool produce, bool ev);
void launch_batch_eval_full(hipStream_t s, const BatchItem *items, int k, const double *x, const double *Z, double *rows,
                            double *mu, double *sigma, int ard_dims, bool produce, bool ev);
// dense inverses of nblk consecutive 256 x 256 diagonal blocks of a finished factor (block b at L + b * 256 * (ld + 1))
void launch_dinv256_blocks(hipStream_t s, const double *L, int64_t ld, double *Dinv, int nblk);
void launch_diag256_inv_only_ld512(hipStream_t s, const double *L, int64_t ld, double *Dinv);  // Dinv: ld 512
void launch_convert_block(hipStream_t s, const double *src, int64_t lds_, double *dst, int64_t ldd, int rows,
                          int cols);
void launch_pack_lower(hipStream_t s, const double *in, int64_t n, int64_t npad, double *L,
                       int64_t ld);
void launch_sigma(hipStream_t s, const double *prior, const double *q, int64_t m,
                  double *sigma);
// pgrad.hip (gogp_produce_gradient).  launch_bwd_panel: C (16 rows16 x ncols, ncols a multiple of 64) = A B (sub: C - A B)
// with A 16 rows16 x K and B K x ncols row-major, K a multiple of 32; tri: B[k][j] == 0 for k < j.  The rows are taken
// in groups of 64: beyond 32 rows, A and C must hold a multiple of 64.
void launch_bwd_panel(hipStream_t s, int64_t rows16, const double *A, int64_t lda, const double *B, int64_t ldb,
                      double *C, int64_t ldc, int64_t ncols, int K, bool tri, bool sub);
// dmu[j][d] = sum_i alpha_i dk(z_j, x_i)/dz_jd, dsigma[j][d] = -2 sum_i Wt[j][i] dk(z_j, x_i)/dz_jd / (2 sigma_j);
// part: 2 * pgrad_slabs(npad, m) * m * ndim doubles of scratch
int pgrad_slabs(int64_t npad, int64_t m, int *tiles_per_slab);
void launch_pgrad(hipStream_t s, const DevParams *p, int ndim, const double *X, int64_t n, int64_t npad,
                  const double *Z, int64_t m, const double *alpha, const double *Wt, int64_t ld, const double *sigma,
                  double *part, double *dmu, double *dsigma, bool ev);
// pcov.hip (gogp_produce_covariance, gogp_produce_samples).  launch_pcov: out (mo x mo, ldo; mo >= m) = k(Z, Z) - Vt Vt^T
// on its leading m x m (+ diag_add on the diagonal), both triangles from the same value, identity on the rest; Vt: m rows
// (one test point each) of npad columns, nullptr = no observations.  part: pcov_slabs(...) * pairs * 4096 doubles of
// scratch, pairs = t (t + 1) / 2 with t = ceil(m / 64).  pcov_slabs: the split of the npad columns over workgroups for
// `ncu` compute units (a slab is a whole number of 256-column panels).
int pcov_slabs(int64_t npad, int64_t m, int ncu, int *cols_per_slab);
void launch_pcov(hipStream_t s, const DevParams *p, const double *Z, int64_t m, const double *Vt, int64_t ld,
                 int64_t npad, int ncu, double *part, double diag_add, double *out, int64_t mo, int64_t ldo, bool ev);
// out (ns x m, compact) = mu (broadcast over the rows) + G (ns rows of ldg doubles)
void launch_pcov_add_mu(hipStream_t s, const double *G, int64_t ldg, const double *mu, int64_t ns, int64_t m, double *out);
int grad_reduce_blocks(int64_t npad);

// fused gradient reduction over lower tiles of Kinv; out: NACC doubles
// Contract on the operands: X holds npad rows of ndim doubles and GOGP_MAX_NDIM ZEROED doubles of slack behind them, and
// its rows n .. npad - 1 are FINITE (the product zero-fills them); p->inv_len[t][d] is 0 for d >= ndim.  The last ARD pass
// of the one-radial-term instances does not test d < ndim per slot: it multiplies the coordinates that follow a live
// row's own -- the next row's, or the slack -- by inv_len = 0 (grad.hip).  Of alpha and Kinv only the elements i < n,
// j <= i are used (alpha's first n; the whole 64 x 64 tile of Kinv may be LOADED: npad rows of ld >= npad).
// max_blocks > 0 caps the grid below the GR_BLOCKS_MAX rule (tests: workgroups that walk several tiles at a small size).
void launch_grad_reduce(hipStream_t s, const DevParams *p, int ndim, int ard_dims,
                        const double *X, const double *alpha, const double *Kinv, int64_t ld, int64_t n,
                        int64_t npad, double *partials, double *out, bool radial1 = false, int mfma_min_dims = 1,
                        bool ev = false, int max_blocks = 0);
// the same over the LOCAL tiles (mrows x ncols, leading dimension ld) of a 2-D block-cyclic
// K^-1: tiles of the global lower triangle only; `partials` needs grad_reduce_blocks_local
int grad_reduce_blocks_local(int64_t mrows, int64_t ncols);
void launch_grad_reduce_local(hipStream_t s, const DevParams *p, int ndim, int ard_dims,
                              const double *X, const double *alpha, const double *Kinv, int64_t ld,
                              int64_t n, int64_t mrows, int64_t ncols, BlockMap map, double *partials,
                              double *out, bool radial1 = false, int mfma_min_dims = 1, bool ev = false,
                              int max_blocks = 0);
void launch_grad_reduce_local(hipStream_t s, const DevParams *p, int ndim, int ard_dims,
                              const double *X, const double *alpha, const float *Kinv, int64_t ld,
                              int64_t n, int64_t mrows, int64_t ncols, BlockMap map, double *partials,
                              double *out, bool radial1 = false, int mfma_min_dims = 1, bool ev = false,
                              int max_blocks = 0);

// grad_mfma.hip: the reduction pass for ONE radial term with ARD length scales, distances and per-dimension sums
// on the matrix cores; ntc == 0: lower triangle of an unsharded K^-1 (nt x nt tiles of 64, candidate batching
// honoured), ntc > 0: the local nt x ntc tiles of a 2-D block-cyclic one.  Writes `blocks` x NACC partials.
void launch_grad_ard_mfma(hipStream_t s, const DevParams *p, int ndim, const double *X, const double *alpha,
                          const double *Kinv, int64_t ld, int64_t n, int nt, int ntc, int ntiles, int blocks,
                          BlockMap map, double *partials);
void launch_grad_ard_mfma(hipStream_t s, const DevParams *p, int ndim, const double *X, const double *alpha,
                          const float *Kinv, int64_t ld, int64_t n, int nt, int ntc, int ntiles, int blocks,
                          BlockMap map, double *partials);
// (ARD kernels with at least `mfma_min_dims` dimensions take it -- option "ard_mfma_min_dims", default 1: measured at
// N = 16384 it beats the scalar-row kernel of grad.hip at every D: 8: 1.16 -> 0.76 ms, 16: 1.91 -> 0.76, 32: 3.63 -> 1.01,
// 64: 10.85 -> 2.50; 65 = never)

// gradient w.r.t. the inputs: mirrors K^-1 to the upper triangle, then
// gx[i][d] = sum_j (alpha_i alpha_j - Kinv_ij) dk(x_i,x_j)/dx_{i,d}
void launch_xgrad(hipStream_t s, const DevParams *p, int ndim, const double *X,
                  const double *alpha, double *Kinv, int64_t ld, int64_t n, int64_t npad,
                  double *gx, bool ev = false);

// dot_j = sum_i V[j][i] vec_i ; sq_j = sum_i V[j][i]^2  (either output may be null)
void launch_rownorm_dot(hipStream_t s, const double *V, int64_t ld, const double *vec,
                        int64_t ncols, int64_t m, double *dot, double *sq);

// +0.0 on the strictly upper 256-blocks of npad x npad; nothing else is touched (npad <= 256: no launch).  Pairs of
// columns are stored: npad and ld even, R 8-B (float) / 16-B aligned.
void launch_zero_upper_blocks(hipStream_t s, double *R, int64_t ld, int64_t npad);
// npad and ld even (pairs of columns, 16-B loads of z).  Of every row i < npad the columns q0(i) .. npad - 1 are read (q0:
// first column of the row's 256-block), padding included; what lies left of q0(i) is never read.
void launch_alpha_from_y(hipStream_t s, const double *Y, int64_t ld, const double *z,
                         int64_t npad, double *alpha);
// +0.0 on rows x cols.  Pairs of columns are stored: cols and ld even (an odd cols would write one column too many), B
// 8-B (float) / 16-B aligned.
void launch_zero_block(hipStream_t s, double *B, int64_t ld, int64_t rows, int64_t cols);
// Ydiag (256 x 256, ld) = Dinv^T; Dinv contiguous 256 x 256.
void launch_ydiag(hipStream_t s, const double *Dinv, double *Ydiag, int64_t ld);
// T^-1 of a super-panel's diagonal block (api.hip: assemble_tinv): diagonal / zero blocks, and nprod (<= 6) products
// C_b (256 x 256) = alpha A_b (256 x K_b) B_b (K_b x 256), row-major, in one launch (solve.hip)
void launch_tinv_init(hipStream_t s, const double *Dinv, double *X, double *XT, int nsub, int64_t tld);
void launch_tinv_init(hipStream_t s, const float *Dinv, float *X, float *XT, int nsub, int64_t tld);
void launch_blockmm(hipStream_t s, int nprod, const double *const *A, const int64_t *lda, const double *const *B,
                    const int64_t *ldb, double *const *C, const int64_t *ldc, const int *K, double alpha);
void launch_blockmm(hipStream_t s, int nprod, const float *const *A, const int64_t *lda, const float *const *B,
                    const int64_t *ldb, float *const *C, const int64_t *ldc, const int *K, double alpha);
// fp32 path: out[0] = sum_{i<n} alpha_i^2 - |Y|_F^2 (= tr(alpha alpha^T - K^-1)) in fp64 from Y = L^-T; part: n doubles.
// Of the rows i < n the columns q0(i) .. npad - 1 are READ -- the padding columns n .. npad - 1 too, which must hold zeros
// for the trace to be that of the n x n block; what lies left of q0(i) (the row's 256-block start) is never read.
void launch_trace_from_y(hipStream_t s, const float *Y, int64_t ld, int64_t n, int64_t npad, const double *alpha,
                         double *part, double *out);
// trsm_small.hip: V = L^-1 Kstar for the right-hand sides j0 .. j0 + cnt - 1 (rows of KsT, cnt <= 32) in ONE persistent
// launch that reads the factor once; dq[j] = |V_j|^2.  ws: trsm_small_workspace_bytes(npad) bytes of this launch's own;
// *tmo_dev: device word that is non-zero afterwards if a workgroup gave up waiting (the caller copies it back and
// reports GOGP_EHIP)
size_t trsm_small_workspace_bytes(int64_t npad);
void launch_trsm_small(hipStream_t s, const double *L, int64_t ld, const double *Dinv, const double *KsT, int64_t ldk,
                       int64_t npad, int j0, int cnt, void *ws, double *dq, unsigned **tmo_dev);
void launch_trsm_small(hipStream_t s, const float *L, int64_t ld, const float *Dinv, const float *KsT, int64_t ldk,
                       int64_t npad, int j0, int cnt, void *ws, double *dq, unsigned **tmo_dev);  // fp32 path
// ... and where that launch leaves V: TS_SOL_PAIRED element (row k, rhs j) at ((k >> 1) * width + j) * 2 + (k & 1) doubles,
// TS_SOL_COMPACT at k * width + j doubles, TS_SOL_GRANULE (one right-hand side) 16 bytes per row: {tag, low word, tag, high word}
// (TS_SOL_ROWS, never that kernel's: at j * width + k doubles -- one solution per row, as the substitution steps of solve.hip leave it)
enum { TS_SOL_PAIRED = 0, TS_SOL_COMPACT = 1, TS_SOL_GRANULE = 2, TS_SOL_ROWS = 3 };
struct TsSolution {
  const void *p = nullptr;
  int kind = TS_SOL_PAIRED, width = 32;
};
// (f32: the launch was the float overload's, which has no granule form: one right-hand side is TS_SOL_COMPACT of width 1)
TsSolution trsm_small_solution(int64_t npad, int j0, int cnt, void *ws, bool f32 = false);
// append.hip: the kernels of gogp_append (api.hip) -- rows n .. n + m - 1 (m <= 64) join a factor of n rows.
// V = L11^-1 B^T (npc rows, the columns j < m0 in v0 and the rest in v1, as launch_trsm_small left them).
// launch_append_gram: one workgroup per 256 rows of V writes its part of G = V^T V (lower 16 x 16 tiles) and of V^T z to
// part[slab] (APPEND_PART doubles each) and its columns k < n of the new rows L21 = V^T to Lnew (row j at Lnew + j * ld).
// launch_append_commit: one workgroup sums the parts in slab order, forms S = C - G (C from X2, the m new inputs, with the
// noise on the diagonal), factors it, and -- positive definite -- writes L22 behind L21, z2 = L22^-1 (y2 - V^T z) to
// z2out; else *info = n + pivot + 1 (first failure wins) and nothing else is written.
constexpr int APPEND_PART = 64 * 64 + 64;
void launch_append_gram(hipStream_t s, TsSolution v0, TsSolution v1, int m0, int m, int64_t npc, int64_t n,
                        const double *z, double *part, double *Lnew, int64_t ld);
void launch_append_commit(hipStream_t s, const DevParams *p, const double *X2, const double *y2, int m, int64_t n,
                          const double *part, int nslab, double *Lnew, int64_t ld, double *z2out, long long *info,
                          bool ev);
// rows r0 .. r1 - 1 of L (columns < ncols) := rows of the identity
void launch_append_identity_rows(hipStream_t s, double *L, int64_t ld, int64_t r0, int64_t r1, int64_t ncols);
// dst (npad1 rows, ld1) := src (npad0 rows, ld0) on the 256-blocks of the lower triangle, identity on the new ones
void launch_append_restride(hipStream_t s, const double *src, int64_t ld0, int64_t npad0, double *dst, int64_t ld1,
                            int64_t npad1);
// remove.hip: the kernels of gogp_remove (api.hip) -- n - n1 rows leave a factor; map[i] (i < n1) is the old index of new
// row i, rem[j] the old index of removed row j.
// launch_remove_gather: dst (npad1 rows, ld npad1) := src[map, map] on the lower triangle, zero above it inside the
// diagonal 256-blocks, identity on the padding.  launch_remove_rows: dst[i] := src[map[i]] for rows of `width` doubles.
// launch_remove_w: W (mw columns of npad1 doubles each, column-major) := src[map, rem[0 .. mc)] for the rows r0 <= i < npad1,
// zero above the diagonal of src, on the padding and in the columns mc <= j < mw.
// launch_remove_snap: snap[b] := the diagonal 128-block b of L, b0 <= b < b0 + nb.
// launch_remove_block: the rank-mw update of columns kb .. kb + 127 (kb a multiple of 128) of L by W, whose rows < kb
// are not read; the rows kb .. of W are consumed, the ones below the block updated.  mw: REMOVE_W_SMALL or REMOVE_W.
constexpr int REMOVE_W = 32, REMOVE_W_SMALL = 4;
void launch_remove_gather(hipStream_t s, const double *src, int64_t ld0, const int *map, int64_t n1, double *dst,
                          int64_t npad1);
void launch_remove_rows(hipStream_t s, const double *src, const int *map, int64_t n1, int width, double *dst);
void launch_remove_w(hipStream_t s, const double *src, int64_t ld0, const int *map, const int *rem, int mc, int mw, int64_t r0,
                     int64_t n1, int64_t npad1, double *W);
void launch_remove_snap(hipStream_t s, const double *L, int64_t ld, int b0, int nb, double *snap);
void launch_remove_block(hipStream_t s, double *L, int64_t ld, const double *snap, double *W, int mw, int64_t kb, int64_t n1);
// loo.hip (gogp_loo, gogp_loo_gradient): the passes over K^-1 (lower triangle, ld) behind leave-one-out cross-validation.
// launch_loo_stats: mu, sigma, log p of the rows i < n, v_i = alpha_i / kappa_i and s_i (zero from row n on; npad doubles
// each) and the npad / 256 block sums of log p in `part`.  launch_loo_scale_symv: B (npad x npad, ldb) = K^-1 diag(s) in
// full and u = K^-1 v, both exactly zero from row / column n on; upart: npad / 64 * npad doubles of scratch.
// launch_loo_rank2: G_ij -= u_i alpha_j + alpha_i u_j on the lower 64-tiles.
// PRECONDITIONS (tests/test_finish_kernels.py holds the kernels to them): launch_loo_scale_symv reads sc and v, and
// launch_loo_rank2 reads u, over all npad rows -- they must be finite and zero from row n on, as launch_loo_stats and
// launch_loo_scale_symv leave them; G must be finite on the lower 64-tiles, whose elements with i >= n or j >= n then
// keep their bits.  Of Kinv the stats read the diagonal elements i < n alone, of alpha and y the rows i < n.
void launch_loo_stats(hipStream_t s, const double *Kinv, int64_t ld, const double *alpha, const double *y, int64_t n,
                      int64_t npad, double *mu, double *sigma, double *logp, double *v, double *sc, double *part);
void launch_loo_scale_symv(hipStream_t s, const double *Kinv, int64_t ld, int64_t n, int64_t npad, const double *sc,
                           const double *v, double *B, int64_t ldb, double *upart, double *u);
void launch_loo_rank2(hipStream_t s, double *G, int64_t ld, int64_t n, int64_t npad, const double *u, const double *alpha);
// blockcv.hip (gogp_blockcv, gogp_blockcv_gradient): leave-block-out cross-validation.  bstart (F + 1 block starts) and
// gfirst (ngroups + 1 first blocks of the groups, from blockcv_pack) are device arrays.  blockcv_pack: the greedy packing
// of consecutive blocks into groups of at most 128 columns; first needs F + 1 entries, returns the number of groups.
// launch_blockcv_groups, one workgroup per group: of Kinv (ld) only the elements j <= i < n inside the blocks are read;
// writes mu, sigma, v and ones (= 1.0) at the rows < n, logp[f] per block, the groups' 128 x 128 S_g (ngroups * 16384
// doubles; exact zeros off the blocks) and info[g] = first failing pivot's row + 1, or 0 (a failing group writes nothing
// else).  launch_blockcv_apply: Q (at least ceil(n / 64) * 64 rows of ld doubles) <- Q blockdiag(S_g) in place on the rows
// r0 < n of the 64-row slices and the columns < n; nothing else of Q is read or written.
int blockcv_pack(const int64_t *start, int64_t F, int64_t *first);
void launch_blockcv_groups(hipStream_t s, const double *Kinv, int64_t ld, const double *alpha, const double *y,
                           const int64_t *bstart, const int64_t *gfirst, int ngroups, double *mu, double *sigma, double *v,
                           double *ones, double *logp, double *Sg, long long *info);
void launch_blockcv_apply(hipStream_t s, double *Q, int64_t ld, int64_t n, const int64_t *bstart, const int64_t *gfirst,
                          int ngroups, const double *Sg);
// multi.hip (gogp_multi_*): T output columns on one factorisation.  At / Yt: one output per row of ld >= npad doubles.
// launch_multi_weight: G (ldk, as Kinv) = scale Kinv - A A^T (gogp_multi_*: scale = T) on the elements j <= i < n of the lower 64-tiles of npad, exact
// zeros on the rest of those tiles, nothing outside them; At must hold T rounded up to a multiple of 4 rows, the rows
// from T on zero; of Kinv only j <= i < n is read.  launch_multi_dots: dots[t] = sum_{i < n} Yt[t][i] At[t][i], t < T.
void launch_multi_weight(hipStream_t s, const double *At, int64_t ld, int T, const double *Kinv, int64_t ldk, int64_t n,
                         int64_t npad, double scale, double *G);
void launch_multi_dots(hipStream_t s, const double *Yt, const double *At, int64_t ld, int64_t n, int T, double *dots);
// basis.hip (gogp_basis_*): explicit basis functions.  Ht / Wt: one basis column per row of ld >= npad doubles, p <= 64.
// launch_basis_symm: Wt (p rounded up to a multiple of 4 rows) = (Kinv H)^T from the symmetric Kinv (ldk) of which only
// the elements j <= i < n are read; columns >= n and rows >= p of Wt exact zeros; of Ht the rows < p and the columns < n
// are read; part: basis_symm_slabs(n) * p4 * ld doubles of scratch.  launch_basis_gram: Ag (p x (p + 1)) = Ht [Wt^T |
// alpha] over the observations < n; part: basis_gram_slabs(n) * p (p + 1) doubles.  launch_basis_finish: from Ag the
// factor LA (p x p), Ainv (p x p), beta (p), scal = {log|A|, g^T beta} and info = 0 or the first bad pivot + 1 (nothing
// else is written then).  launch_basis_cols: Ct ((p + 1) rounded up to a multiple of 4 rows of ld doubles) = [W LA^-T |
// alpha - W beta]^T, zero rows behind and zero columns >= n.  launch_basis_predict: mu = mu0 + R beta and sigma (unless
// NULL) = sqrt(prior - q + diag(R Ainv R^T)), R = Hz (m x p) - KW (ldkw doubles per row).
constexpr int BASIS_SYMM_SLABS_MAX = 16, BASIS_GRAM_SLABS_MAX = 64;
int basis_symm_slabs(int64_t n);
int basis_gram_slabs(int64_t n);
void launch_basis_symm(hipStream_t s, const double *Kinv, int64_t ldk, int64_t n, int64_t npad, const double *Ht, int64_t ld,
                       int p, double *part, double *Wt);
void launch_basis_gram(hipStream_t s, const double *Ht, const double *Wt, int64_t ld, const double *alpha, int64_t n, int p,
                       double *part, double *Ag);
void launch_basis_finish(hipStream_t s, const double *Ag, int p, double *LA, double *Ainv, double *beta, double *scal,
                         long long *info);
void launch_basis_cols(hipStream_t s, const double *Wt, int64_t ld, int64_t n, int p, const double *LA, const double *beta,
                       const double *alpha, double *Ct);
void launch_basis_predict(hipStream_t s, const double *Hz, const double *KW, int64_t ldkw, int64_t m, int p,
                          const double *beta, const double *Ainv, const double *mu0, const double *prior, const double *q,
                          double *mu, double *sigma);
// sparse.hip (gogp_sparse_*): the inducing-point approximation.  Vt: `rows` rows (one observation of the chunk each) of
// ld >= Mp doubles, as Produce's forward substitution leaves V^T; Mp a multiple of 64.
// launch_sparse_syrk: Bacc (ldb) += Vt^T Vt on the whole lower 64-tiles of Mp x Mp and r += Vt^T y (rows doubles); rows
// >= `rows` of Vt are not read and its columns >= M count as exact zeros.  launch_sparse_grad: out (NACC slot sums,
// `accumulate`: added to what out holds) = sum_{f < rows, u < M} (Wt[f][u] + y_f mvec_u s4) dk(x_f, u_u)/dlog theta;
// partials: sparse_grad_blocks(rows, M) * NACC doubles of scratch.  The element-wise passes: B (full) = I + Bacc / s2 from
// the lower tiles; T = I - Binv - g g^T s4 and S = 2 I - B - Binv - g g^T s4; the five scalars of the bound (sparse.hip);
// sum y^2; mu = dot / s2 and sigma = sqrt(prior - q + rowdot(A, V)) of Produce.
void launch_sparse_syrk(hipStream_t s, const double *Vt, int64_t ld, int64_t rows, int64_t M, int64_t Mp, const double *y,
                        double *Bacc, int64_t ldb, double *r);
constexpr int SPARSE_GRAD_BLOCKS_MAX = 2048;  // workgroups (rows of `partials`) of launch_sparse_grad at most
int sparse_grad_blocks(int64_t rows, int64_t M);
// out[q] (+)= sum_b partials[b][q] for the NACC slots, in block order per thread and then a fixed tree
void launch_sparse_grad_final(hipStream_t s, const double *partials, int blocks, double *out, bool accumulate);
void launch_sparse_grad(hipStream_t s, const DevParams *p, int ndim, int ard_dims, const double *X, int64_t rows,
                        const double *U, int64_t M, const double *Wt, int64_t ldw, const double *y, const double *mvec,
                        double s4, double *partials, double *out, bool accumulate);
// launch_sparse_ugrad: dU (M x ndim; `accumulate`: added to what it holds) = sum_{f < rows} (Wt[f][u] + y_f mvec_u s4)
// dk(u_u, x_f)/du_u, the arguments of launch_sparse_grad; part: sparse_ugrad_slabs(rows, M) * M * ndim doubles of scratch
// (shared by launches of up to `rows` rows: sparse_ugrad_slabs_bound(rows, M) * M * ndim).
int sparse_ugrad_slabs(int64_t rows, int64_t M, int *tps_out);  // slabs of row tiles and the 64-row tiles of one
int sparse_ugrad_slabs_bound(int64_t rows, int64_t M);  // >= sparse_ugrad_slabs(r, M) for every r <= rows (it is not monotone)
void launch_sparse_ugrad(hipStream_t s, const DevParams *p, int ndim, const double *X, int64_t rows, const double *U,
                         int64_t M, const double *Wt, int64_t ldw, const double *y, const double *mvec, double s4,
                         double *part, double *dU, bool accumulate);
void launch_sparse_finish_b(hipStream_t s, const double *Bacc, int64_t Mp, double inv_s2, double *B);
void launch_sparse_copy_upper(hipStream_t s, const double *src, int64_t Mp, double *dst);  // zeros below the diagonal
void launch_sparse_weights(hipStream_t s, const double *B, const double *Binv, const double *g, int64_t Mp, double s4,
                           double *T, double *S);
void launch_sparse_scalars(hipStream_t s, const double *C, const double *B, const double *Binv, const double *r,
                           const double *g, int64_t M, int64_t Mp, double *out);
void launch_sparse_sumsq(hipStream_t s, const double *y, int64_t n, double *out);
void launch_sparse_predict(hipStream_t s, const double *A, const double *V, int64_t ld, int64_t ncols, int64_t m,
                           const double *prior, const double *q, const double *dot, double inv_s2, double *mu,
                           double *sigma);
// Multi-output (gogp_sparse_multi_*).  launch_sparse_xty: Rt (T rounded up to 64 rows of ldr doubles; the columns below
// M rounded up to 64) += Yc^T Vt, Yc: rows x T of ldy doubles per row; rows >= `rows` are not read, columns >= M of Vt and
// >= T of Yc count as exact zeros.  One workgroup per (inducing tile, output tile, slab of rows); the slabs' sums are
// added in index order.  part: sparse_xty_part_doubles(rows, M, T) doubles of scratch, which covers every launch of up
// to `rows` rows (sparse_xty_slabs_bound >= sparse_xty_slabs(r, M, T) for every r <= rows).
int sparse_xty_slabs(int64_t rows, int64_t M, int64_t T, int64_t *rows_per_slab);
int sparse_xty_slabs_bound(int64_t rows, int64_t M, int64_t T);
size_t sparse_xty_part_doubles(int64_t rows, int64_t M, int64_t T);
void launch_sparse_xty(hipStream_t s, const double *Vt, int64_t ld, int64_t rows, int64_t M, const double *Y, int64_t ldy,
                       int64_t T, double *part, double *Rt, int64_t ldr);
// Tm = T (I - Binv) - GG s4 and S = T (2 I - B - Binv) - GG s4; out[t] = r_t . gamma_t and out[tstride + t] = gamma_t .
// gamma_t from the rows of Rt / Gt; out[t] = sum_i Y[i][t]^2; Yp (rpad x kp, ldp) = the rows of Y padded with exact
// zeros (rpad a multiple of 128, kp of 16: rpad * kp must be a multiple of 256 -- the launcher starts whole workgroups and
// launches NOTHING otherwise; its one caller asserts it); sigma of launch_sparse_predict alone.  The four Mp x Mp
// element-wise launchers take Mp a multiple of 256 (Mp / 256 workgroups per row).
void launch_sparse_multi_weights(hipStream_t s, const double *B, const double *Binv, const double *GG, int64_t Mp, int T,
                                 double s4, double *Tm, double *S);
void launch_sparse_multi_dots(hipStream_t s, const double *Rt, const double *Gt, int64_t ld, int64_t M, int T, int tstride,
                              double *out);
void launch_sparse_multi_sumsq(hipStream_t s, const double *Y, int64_t ldy, int64_t n, int T, double *out);
void launch_sparse_multi_pad(hipStream_t s, const double *Y, int64_t ldy, int64_t rows, int64_t T, int64_t kp, int64_t rpad,
                             double *Yp, int64_t ldp);
void launch_sparse_multi_sigma(hipStream_t s, const double *A, const double *V, int64_t ld, int64_t ncols, int64_t m,
                               const double *prior, const double *q, double *sigma);
// select.hip (gogp_sparse_select_inducing): greedy pivoted Cholesky of k(X, X), one launch per step (the algorithm is at
// the head of select.hip).  SelectBufs: the factor Lt (column t at Lt + t * ldn, ldn = N rounded up to 256; min(M, N)
// columns) and the small buffers select_layout places at `base` (nullptr: the bytes alone, its return value): d (ldn),
// the double-buffered partial maxima, piv / pv (M), the step count, the trace, U (M x ndim) and the selection mask.
// launch_select_init: d_i = k(x_i, x_i) (d0 given: d0_i), the mask cleared, the first partials.  launch_select_step: step
// j on `blocks` workgroups (the same for every launch of a run: the partials are one per workgroup); it writes nothing
// once piv[j - 1] < 0 or the best residual is not > tol.  launch_select_final: trace and (gather) U = X[piv[0 .. m)].
// select_run: the whole loop on stream s -- piv cleared to -1, init, up to min(M, N) steps with a look at the step count
// every SELECT_SYNC_STEPS launches, final -- synchronised; *m_out = the steps taken.  max_blocks > 0 caps the grid below
// select_blocks' rule (tests: workgroups that stride over several row blocks at a small N).
struct SelPair {
  double v;
  long long i;
};
struct SelectBufs {
  double *Lt = nullptr;
  int64_t ldn = 0;
  double *d = nullptr, *pv = nullptr, *trace = nullptr, *U = nullptr;
  SelPair *part = nullptr;
  long long *piv = nullptr, *state = nullptr;
  unsigned char *sel = nullptr;
};
constexpr int SELECT_BLOCKS_MAX = 1024;  // workgroups of a step at most: the pairs every workgroup of the next one reduces
constexpr int SELECT_SYNC_STEPS = 256;
int select_blocks(int64_t N, int max_blocks);
size_t select_layout(char *base, int64_t N, int64_t M, int ndim, SelectBufs *b);
void launch_select_init(hipStream_t s, const DevParams *p, const double *X, int64_t N, int blocks, const double *d0,
                        const SelectBufs &b);
void launch_select_step(hipStream_t s, const DevParams *p, int ndim, const double *X, int64_t N, int blocks, int j,
                        double tol, const SelectBufs &b);
void launch_select_final(hipStream_t s, const double *X, int64_t N, int ndim, const SelectBufs &b, bool gather);
hipError_t select_run(hipStream_t s, const DevParams *p, int ndim, const double *X, int64_t N, int64_t M, double tol,
                      int max_blocks, const double *d0, const SelectBufs &b, int64_t *m_out);
// cg.hip (gogp_cg_*): matrix-free preconditioned conjugate gradients on up to CG_MAX_T systems in lock-step.  A block of
// T vectors lies as T rows of ld doubles (ld >= n); the launchers read and write the elements i < n of the rows t < T and
// nothing else, unless stated.
// launch_kmm: Out[t][i] = sum_{j < cols} k(a_i, b_j) V[t][j] (+ diag[i] V[t][i]: diag != nullptr, which needs A == B and
// rows == cols) for i < rows, t < T <= CG_MAX_T, on v_mfma_f64_16x16x4_f64; Out[t][i] = 0 for rows <= i < ldo.  A: rows x
// ndim, B: cols x ndim, read on their first rows / cols rows only; V is read on t < T, j < cols only; noise_var of *p is
// NOT added.  The column tiles (64 columns each) are split into nslab slabs (1 <= nslab <= KMM_SLABS_MAX; kmm_slabs gives
// the product's choice, which depends on rows and cols alone); part: nslab * T * rpad doubles, rpad = rows rounded up
// to 64, every one of which is written: part[(slab * T + t) * rpad + i]; the finish kernel adds them in slab order.
// max_blocks > 0 caps the grid (tests: a workgroup that walks several row tiles and slabs).
// launch_cg_dots: out-of-place partial sums (part: T * cg_dot_blocks(n) doubles) and a final kernel per column that adds
// them in a fixed order and, by `mode`, updates the per-column state of the iteration (CgState; cg.hip states the modes).
// launch_cg_update_xr: x += a p, r -= a q; launch_cg_update_p: p = z + beta p; both leave a frozen column untouched.
// launch_cg_scale: out = in o w - sub (w == nullptr: in; sub == nullptr: nothing subtracted); w has n entries.
// launch_cg_status: st.status[0] = columns t < T not frozen, st.status[1] = first column + 1 with a bad p^T q, or 0.
constexpr int CG_MAX_T = GOGP_CG_MAX_RHS;
constexpr int KMM_SLABS_MAX = 64;
enum CgDotMode { CG_DOT_PLAIN = 0, CG_DOT_BNORM = 1, CG_DOT_RHO0 = 2, CG_DOT_PQ = 3, CG_DOT_RR = 4, CG_DOT_BETA = 5 };
// per-column state on the device: CG_SC_* rows of CG_MAX_T doubles in sc, CG_ST_* rows of CG_MAX_T ints in st
enum { CG_SC_RHO = 0, CG_SC_A = 1, CG_SC_BETA = 2, CG_SC_BNORM2 = 3, CG_SC_RR = 4, CG_SC_PQ = 5, CG_SC_ROWS = 6 };
enum { CG_ST_FROZEN = 0, CG_ST_ITERS = 1, CG_ST_BAD = 2, CG_ST_STATUS = 3, CG_ST_ROWS = 4 };
struct CgState {
  double *sc = nullptr;  // CG_SC_ROWS * CG_MAX_T
  int *st = nullptr;     // CG_ST_ROWS * CG_MAX_T
};
int kmm_slabs(int64_t rows, int64_t cols);
void launch_kmm(hipStream_t s, const DevParams *p, int ndim, const double *A, int64_t rows, const double *B, int64_t cols,
                const double *V, int64_t ldv, int T, const double *diag, int nslab, int max_blocks, double *part,
                double *Out, int64_t ldo);
int cg_dot_blocks(int64_t n);
void launch_cg_dots(hipStream_t s, const double *A, const double *B, int64_t ld, int64_t n, int T, int mode, int it,
                    double tol, double *part, double *out, CgState cs, double *hist = nullptr);
void launch_cg_update_xr(hipStream_t s, double *x, double *r, const double *p, const double *q, int64_t ld, int64_t n, int T,
                         CgState cs);
void launch_cg_update_p(hipStream_t s, double *p, const double *z, int64_t ld, int64_t n, int T, CgState cs);
void launch_cg_scale(hipStream_t s, const double *in, const double *w, const double *sub, int64_t ld, int64_t n, int T,
                     double *out);
void launch_cg_status(hipStream_t s, int T, CgState cs);
// The preconditioner P = L L^T + D (cg.hip).  launch_cg_diag: d_i = noise_var + v_i (v == nullptr: 0), dis_i = d_i^-1/2
// for i < n and 0 for n <= i < npad.  launch_cg_scale_factor: Ls = D^-1/2 L in place on the r columns of the column-major
// factor (column k at Lt + k * ldn; rows >= n are neither read nor written).  launch_cg_capacitance: C (rp x rp, rp = r
// rounded up to 16) = I + Ls^T Ls, both triangles.  launch_cg_lst: W[t][k] = sum_i Ls[i][k] dis_i R[t][i] (W: T rows of rp
// doubles; part: cg_lst_slabs(n) * T16 * rp doubles, T16 = T rounded up to 16).  launch_cg_small_mm: Y[t][k] = sum_k'
// Cinv[k][k'] W[t][k'].  launch_cg_precond: Z[t][i] = dis_i (dis_i R[t][i] - sum_k Ls[i][k] Y[t][k]); r == 0: Jacobi.
int cg_lst_slabs(int64_t n);
void launch_cg_diag(hipStream_t s, const DevParams *p, const double *v, int64_t n, int64_t npad, double *d, double *dis);
void launch_cg_scale_factor(hipStream_t s, double *Lt, int64_t ldn, int64_t n, int r, const double *dis);
void launch_cg_capacitance(hipStream_t s, const double *Ls, int64_t ldn, int64_t n, int r, int rp, double *C);
void launch_cg_lst(hipStream_t s, const double *Ls, int64_t ldn, int64_t n, int r, int rp, const double *dis,
                   const double *R, int64_t ld, int T, double *part, double *W);
void launch_cg_small_mm(hipStream_t s, const double *Cinv, int r, int rp, const double *W, int T, double *Y);
void launch_cg_precond(hipStream_t s, const double *Ls, int64_t ldn, int64_t n, int r, int rp, const double *dis,
                       const double *R, const double *Y, int64_t ld, int T, double *Z);
// The LML and its gradient (gogp_cg_lml_gradient).  launch_cg_dots with hist != nullptr records the iteration's
// coefficients of every column t < T: a at hist[(2 (it - 1)) CG_MAX_T + t] in mode CG_DOT_PQ, beta at
// hist[(2 (it - 1) + 1) CG_MAX_T + t] in mode CG_DOT_BETA (0 for a frozen column); other modes leave it alone.
// launch_cg_probes: Z[t][i] = sqrt(d_i) (sum_{k < r} Ls[i][k] Xi[t][n + k] + Xi[t][i]) for i < n, t < T; Xi: T rows of ldxi
// >= n + r doubles.  launch_cg_grad: out[slot] (+)= sum_{i, j < n} (scale sum_{s < S} A[s][i] B[s][j]) theta_p
// dk(x_i, x_j)/dtheta_p in the slot layout of grad.hip (ACC_*), the trace slot taking the weights of the pairs i == j;
// A, B: S >= 1 rows of ld >= n doubles, taken in passes of CG_MAX_T rows, read on s < S, i < n only; noise_var of *p is
// not used; n < 2^21 (tiles are counted in 32 bits; a larger n launches nothing).  partials: cg_grad_blocks(n) * NACC
// doubles of scratch.  cg_lanczos_quadrature (host): rho0 e_1^T log(T) e_1
// of the m x m Lanczos tridiagonal T that the coefficients a[k stride], beta[k stride] (k < m) of one column define.
int cg_grad_blocks(int64_t n);
void launch_cg_probes(hipStream_t s, const double *Ls, int64_t ldn, int64_t n, int r, const double *d, const double *Xi,
                      int64_t ldxi, int64_t ld, int T, double *Z);
void launch_cg_grad(hipStream_t s, const DevParams *p, int ndim, int ard_dims, const double *X, int64_t n, const double *A,
                    const double *B, int64_t ld, int S, double scale, double *partials, double *out, bool accumulate);
double cg_lanczos_quadrature(const double *a, const double *beta, int64_t stride, int m, double rho0);
// vecchia.hip (gogp_vecchia_*): Vecchia's approximation, one wave per target (the head of vecchia.hip states the kernel).
// nbr: `targets` rows of m <= 63 int32 indices into X's rows, -1 padding trailing, as gogp_vecchia_check accepts them --
// the kernel indexes X, y and v with them unchecked.  launch_vecchia_observe, value != nullptr: the value's pass -- terms (N
// x 3: mu, s, log p; nullptr: not written), value[0] = sum_i log p_i, info[0] = the lowest target with a bad pivot + 1, or
// 0; partials != nullptr (vecchia_blocks(N) * NACC doubles): the gradient's pass(es), which leave the NACC slot sums in
// gout and skip a target with a bad pivot.  vpart / fpart: vecchia_blocks(targets) entries each.  launch_vecchia_produce: mu, sigma (nullptr: not written) of the mz rows
// of Z, each conditioned on the rows nbrz names; info as above.  Both instances (blocks of at most 32 / 64 rows) give a
// target the same bits.  max_blocks > 0 caps the grid below VECCHIA_BLOCKS_MAX (tests: waves that walk several targets at
// a small size).
constexpr int VECCHIA_BLOCKS_MAX = 2048;  // workgroups (one wave each; rows of `partials`) at most
int vecchia_blocks(int64_t targets, int max_blocks = 0);
void launch_vecchia_observe(hipStream_t s, const DevParams *p, int ndim, int ard_dims, const double *X, const double *y,
                            const double *v, int64_t N, const int *nbr, int m, double *terms, double *partials,
                            double *vpart, long long *fpart, double *gout, double *value, long long *info,
                            int max_blocks = 0);
void launch_vecchia_produce(hipStream_t s, const DevParams *p, int ndim, const double *X, const double *y, const double *v,
                            const double *Z, int64_t mz, const int *nbrz, int m, double *mu, double *sigma,
                            long long *fpart, long long *info, int max_blocks = 0);
// vecchia_knn.hip (gogp_vecchia_neighbours, ..._set_data_nearest, ..._reneighbour, ..._produce_nearest): the exact
// nearest-neighbour tables of gogp_amd/vecchia.py, integer for integer (the head of vecchia_knn.hip states the definition
// and the kernel).  launch_vknn_scale: xs = x / lengths per dimension (lengths: ndim doubles on the device, or nullptr: a
// copy).  launch_vknn: Xs the n scaled rows; Zs == nullptr: the causal table of Xs (targets == n), else row z of the table
// holds the m nearest rows of Xs to row z of Zs; nbr: targets x m, d2out (nullptr: not written): the squared distance of
// every entry, 0.0 under the padding; ws: vknn_plan(targets, n, m, slabs).ws_bytes bytes of scratch.  slabs > 0 forces the
// candidate split, tile_cap > 0 caps the grid (tests); the table does not depend on either.  n < 2^31, 0 <= m <= 63.
constexpr int VKNN_TILE = 64;  // targets of a work unit: one lane each
// the workspace at most: 12 bytes per (target, slab, entry), and tiles * slabs < 768 wherever a search is split
constexpr size_t VKNN_WS_MAX = (size_t)768 * VKNN_TILE * 12 * 63;
struct VknnPlan {
  int tile, slabs;
  int64_t slab_len;  // slab s holds the candidates [s * slab_len, min(n, (s + 1) * slab_len))
  size_t ws_bytes;
};
VknnPlan vknn_plan(int64_t targets, int64_t n, int m, int slabs = 0);
void launch_vknn_scale(hipStream_t s, const double *x, int64_t rows, int ndim, const double *lengths, double *xs);
void launch_vknn(hipStream_t s, const double *Xs, int64_t n, const double *Zs, int64_t targets, int ndim, int m, int slabs,
                 int tile_cap, void *ws, int *nbr, double *d2out);
// laplace.hip (gogp_laplace_*): the passes around the factorisation of B = I + diag(sw) K diag(sw).  Vectors hold npad
// doubles (npad a multiple of 256) and leave every launcher zero from row n on.
// launch_lap_site: g, W, sw = sqrt(W), b = W f + g, rho of the rows i < n; part: 5 * npad / 256 doubles of block results;
// out[0 .. 4] = sum log p, sum a f, max |a - g|, max |a|, the first row whose y the likelihood refuses or -1.
// launch_lap_scale_gram: A := diag(sw) A diag(sw) + I on the elements i, j < n of the lower 64-tiles, right behind
// launch_gram_lower_split with the same streams and column split.  launch_lap_vec: out = q o r (p == nullptr) or
// p - q o r.  launch_lap_interp: at = a + t (a1 - a), ft = f + t (f1 - f).  launch_lap_weight_vectors: sv_i = 1/2 (1 -
// Binv_ii) rho_i.  launch_lap_symv_u: u = sv - sw o (Binv v) from the elements j <= i < n of Binv; upart: npad / 64 * npad
// doubles of scratch.  launch_lap_weight: in place, G = diag(sw) Binv diag(sw) - u a^T - a u^T on j <= i < n, exact zeros
// on the rest of the lower 64-tiles.  launch_lap_colscale: KsT (rows x ld) := KsT diag(sw).  launch_lap_mean: the
// response-scale prediction from the latent mu and sigma.
void launch_lap_site(hipStream_t s, int lik, const double *f, const double *y, const double *a, int64_t n, int64_t npad,
                     double *g, double *W, double *sw, double *b, double *rho, double *part, double *out);
void launch_lap_scale_gram(hipStream_t s_first, hipStream_t s_rest, double *A, int64_t ld, int64_t n, int64_t npad,
                           const double *sw, int64_t wcols);
void launch_lap_vec(hipStream_t s, const double *p, const double *q, const double *r, int64_t n, int64_t npad, double *out);
void launch_lap_interp(hipStream_t s, const double *a, const double *a1, const double *f, const double *f1, double t,
                       int64_t n, int64_t npad, double *at, double *ft);
void launch_lap_weight_vectors(hipStream_t s, const double *Binv, int64_t ld, const double *rho, int64_t n, int64_t npad,
                               double *sv);
void launch_lap_symv_u(hipStream_t s, const double *Binv, int64_t ld, int64_t n, int64_t npad, const double *v,
                       const double *sv, const double *sw, double *upart, double *u);
void launch_lap_weight(hipStream_t s, double *G, int64_t ld, int64_t n, int64_t npad, const double *sw, const double *u,
                       const double *a);
void launch_lap_colscale(hipStream_t s, double *KsT, int64_t ld, int64_t rows, int64_t npad, const double *sw);
void launch_lap_mean(hipStream_t s, int lik, const double *mu, const double *sigma, int64_t m, double *mean);
// noisevar.hip (gogp_set_noise_variances): per-observation noise variances v on the diagonal of K.
// launch_nv_diag_add: A_ii += v_i for i < n, right behind launch_gram_lower_split with the same streams and column
// split: the rows i < wcols on s_first, the rest on s_rest; nothing else of A is read or written.
// launch_nv_gradient: dv_i = 1/2 (alpha_i^2 - Kinv_ii) for i < n, one fused multiply-add per row; reads the diagonal of
// Kinv only.  launch_nv_append_fold: part[i * 64 + i] -= v2_i for i < m <= 64 on the first slab's partial sums of
// append_gram_kernel, so that append_commit_kernel's S = C - sum carries v2 on its diagonal.
void launch_nv_diag_add(hipStream_t s_first, hipStream_t s_rest, double *A, int64_t ld, int64_t n, const double *v,
                        int64_t wcols);
void launch_nv_gradient(hipStream_t s, const double *Kinv, int64_t ld, const double *alpha, int64_t n, double *dv);
void launch_nv_append_fold(hipStream_t s, double *part, const double *v2, int m);
void launch_fill(hipStream_t s, double *p, int64_t count, double v);  // grid-stride loop, grid capped at 4096 workgroups
void launch_axpy(hipStream_t s, double *a, const double *b, int64_t count);  // a += b
void launch_dot(hipStream_t s, const double *a, const double *b, int64_t n, double *out);  // out[0] = a.b; one workgroup
// helpers of the sharded evaluation (solve.hip); tests/test_shard_kernels.py holds the kernels to what is stated here
// dst (n x n, ldd) = src^T; n a multiple of 32: whole 32 x 32 tiles are moved (n < 32 launches nothing)
void launch_transpose_sq(hipStream_t s, const double *src, int64_t lds_, double *dst, int64_t ldd,
                         int n);
void launch_transpose_sq(hipStream_t s, const float *src, int64_t lds_, float *dst, int64_t ldd, int n);
// dst block d (blk doubles) = src block first + d stride, d < nblk; blk even and both pointers 16-B aligned (pairs of
// doubles are moved: an odd blk drops its last one); only the selected source blocks are read
void launch_pack_blocks(hipStream_t s, double *dst, const double *src, int nblk, int64_t blk,
                        int first, int stride);
// out[c] = sum_{r < rows} chunk[r][c] v[r], c < nb.  nb a multiple of 64 (the grid is nb / 64 column groups: other
// columns would never be written), rows >= 1; chunk and v are read on the rows < `rows` only; of part the first
// ceil(rows / 256) slabs of nb doubles are written
int64_t chunk_tdot_scratch(int64_t max_rows, int nb);  // doubles of `part` scratch
void launch_chunk_tdot(hipStream_t s, const double *chunk, int64_t rows, int nb, const double *v,
                       double *part, double *out);
void launch_chunk_tdot(hipStream_t s, const float *chunk, int64_t rows, int nb, const double *v,
                       double *part, double *out);
// out[global row] = sum over this rank's chunks with global block column gP >= the row's global block row gI of
// Ych[bj][bi][r][.] . z[gP nb ..], for EVERY local row, padding rows included; the rest of out is left alone and the
// chunks with gP < gI are never read.  nb even, the chunks 8-B (float) / 16-B aligned, z 16-B aligned
void launch_chunk_alpha(hipStream_t s, const double *Ych, int mloc, int nloc, int nb, BlockMap map,
                        const double *z, double *out);
void launch_chunk_alpha(hipStream_t s, const float *Ych, int mloc, int nloc, int nb, BlockMap map,
                        const double *z, double *out);
// out[0] = |Y_local|_F^2 over this rank's chunks of Y (rows < n), fp64; part: mloc * nb doubles.  The local rows with
// global index >= n are not read at all (their part[] is exactly 0), nor the chunks with gP < gI; alignment as chunk_alpha
void launch_chunk_sumsq(hipStream_t s, const double *Ych, int mloc, int nloc, int nb, BlockMap map, int64_t n, double *part,
                        double *out);
void launch_chunk_sumsq(hipStream_t s, const float *Ych, int mloc, int nloc, int nb, BlockMap map, int64_t n, double *part,
                        double *out);
// acc[0] += sum_{i < nb, row0 + i < n} 2 log L_ii: ACCUMULATES; the other L_ii are not read
void launch_logdet_block(hipStream_t s, const double *L, int64_t ld, int64_t row0, int64_t n, int nb,
                         double *acc);
// out[0] = sum_{i < n} z_i^2 and, info given, out[1] = (double)*info (out[1] left alone otherwise); one workgroup
void launch_sumsq_info(hipStream_t s, const double *z, int64_t n, const long long *info, double *out);
void launch_info_to_double(hipStream_t s, const long long *info, double *out);
void launch_extract_lower(hipStream_t s, const double *L, int64_t ld, int64_t n,
                          double *out);
// dist2d.hip: the kernels of the sharded evaluation that work on one rank's buffers.  Nothing below reads or writes
// beyond what is stated; "global row" is BlockMap::grow of the local one.
// launch_gather_rows: yloc[i] = y[global row of i], i < rows -- y must hold every global row a local one maps to (the
// padded length), there is no n here.  launch_gather_x: Xloc (rows x D), aloc = X, a at the global rows < n, exact zeros
// for the others; X and a are not read from row n on.
void launch_gather_rows(hipStream_t s, const double *y, double *yloc, int64_t rows, BlockMap map);
void launch_gather_x(hipStream_t s, const double *X, const double *a, int D, int64_t n, int64_t rows, BlockMap map,
                     double *Xloc, double *aloc);
// launch_scatter_tile: dst[r * n + c] = src tile (nb x nb, contiguous) for the global rows row0 <= r < min(row0 + nb, n)
// and columns col0 <= c < min(col0 + nb, n), diag: c <= r only; dst has n columns and may be offset by a band start (the
// caller passes dst - r0 * n).  Rows / columns of src at or beyond n are not read.
void launch_scatter_tile(hipStream_t s, const double *src, int nb, double *dst, int64_t n, int64_t row0, int64_t col0,
                         int diag);
void launch_scatter_tile(hipStream_t s, const float *src, int nb, double *dst, int64_t n, int64_t row0, int64_t col0,
                         int diag);
// launch_gather_rows_of_l: diag_only 0: out (nrows x n) row k = row rows[k] of L on the columns this rank's tiles hold
// (<= rows[k]), rows[k] in [0, n) -- the kernel indexes the chunks with them unchecked; diag_only 1 (rows unused): out[r] =
// L_rr for the r < n whose diagonal tile is this rank's.  Everything else of out is left alone (the caller zeroes it).
void launch_gather_rows_of_l(hipStream_t s, const double *Lch, int mloc, int nloc, int nb, BlockMap map,
                             const int64_t *rows, int64_t nrows, int64_t n, int diag_only, double *out);
void launch_gather_rows_of_l(hipStream_t s, const float *Lch, int mloc, int nloc, int nb, BlockMap map, const int64_t *rows,
                             int64_t nrows, int64_t n, int diag_only, double *out);
// launch_scatter_stage: stage (nb rows of lds_ >= nloc * nb doubles: one local tile row, this rank's tile columns side by
// side) into the tiles (bj, bi), bj < nloc, of the chunks Lch[bj][bi][r][c]; bi < mloc; rounds once to T.
void launch_scatter_stage(hipStream_t s, const double *stage, int64_t lds_, double *Lch, int nloc, int mloc, int bi, int nb);
void launch_scatter_stage(hipStream_t s, const double *stage, int64_t lds_, float *Lch, int nloc, int mloc, int bi, int nb);
// launch_transpose_rect: dst (cols x rows, ldd) = src (rows x cols, lds_)^T; rows and cols multiples of 32 (whole tiles; a
// remainder is neither read nor written).
void launch_transpose_rect(hipStream_t s, const double *src, int64_t lds_, double *dst, int64_t ldd, int64_t rows, int cols);
void launch_transpose_rect(hipStream_t s, const float *src, int64_t lds_, float *dst, int64_t ldd, int64_t rows, int cols);
// launch_copy_block: dst (rows x nb, contiguous) = the rows x nb block at src (ld).  launch_residual_block: W (rows x nb,
// contiguous) = Ks block - (U block + recv[0] + .. + recv[nrecv - 1]) with Ks, U of leading dimension ld and the nrecv
// received blocks rows x nb contiguous, one behind the other; summed in fp64 in that order, rounded to T once.
void launch_copy_block(hipStream_t s, double *dst, const double *src, int64_t ld, int nb, int64_t rows);
void launch_residual_block(hipStream_t s, double *W, const double *Ks, const double *U, int64_t ld, const double *recv,
                           int nrecv, int nb, int64_t rows);
void launch_residual_block(hipStream_t s, float *W, const float *Ks, const double *U, int64_t ld, const double *recv,
                           int nrecv, int nb, int64_t rows);
void launch_residual_from(hipStream_t s, double *kv, const double *y, int64_t count);  // kv := y - kv
void launch_add_inplace(hipStream_t s, double *a, const double *b, int64_t count);    // a += b; grid-stride, 1024 workgroups
void launch_add_inplace(hipStream_t s, float *a, const float *b, int64_t count);
void launch_scale(hipStream_t s, double *a, double f, int64_t count);                 // a *= f
void launch_add_vec(hipStream_t s, double *a, const double *b, int64_t count);        // a += b

}  // namespace gogp
