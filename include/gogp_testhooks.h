/*
 * gogp_testhooks.h -- measurement and diagnostic entry points of
 * gogp_amd/libgogp_testhooks.so (tests/, tools/ and bench.py's roofline calibration).
 *
 * NOT part of the drop-in boundary: the product library libgogp_hip.so
 * (include/gogp_hip.h) does not export these.  The hook library links the product
 * library and drives its internal launchers.
 */
#ifndef GOGP_TESTHOOKS_H
#define GOGP_TESTHOOKS_H

#include <stdint.h>

#include "gogp_hip.h" /* GOGP_MAX_TERMS, GOGP_MAX_NDIM, GOGP_MAX_EVENTS */

#ifdef __cplusplus
extern "C" {
#endif

/* Micro-benchmark used to calibrate the fp64 MFMA roofline: every SIMD issues
 * `iters` x 8 back-to-back v_mfma_f64_16x16x4_f64 from two waves; returns the
 * achieved TFLOP/s and (optionally) the shader cycles per MFMA on one SIMD and
 * the shader clock in MHz observed by one wave during the run. */
int gogp_mfma_f64_peak(int device, int iters, double *tflops, double *cyc_per_mfma,
                       double *clock_mhz);
/* The same for the fp32 path's instruction, v_mfma_f32_32x32x2_f32 (157.3 TFLOP/s spec). */
int gogp_mfma_f32_peak(int device, int iters, double *tflops, double *cyc_per_mfma,
                       double *clock_mhz);

/* Stand-alone fp64 GEMM test hook: C(MxN,row-major) = beta*C + alpha*A(MxK)*B(NxK)^T
 * on host buffers (copied to the device and back); M,N multiples of 128,
 * K multiple of 16.  Exists so the tile kernel can be parity-tested in
 * isolation against a host reference. */
int gogp_test_dgemm_nt(int device, int64_t M, int64_t N, int64_t K, double alpha,
                       const double *A, const double *B, double beta, double *C);

/* Every GemmGrid field of the tile kernel's launcher (gogp_amd/csrc/common.h) and the candidate batch: k launches
 * side by side on gridDim.z, candidate c's A, B and C lying c * bstride ELEMENTS after candidate 0's. */
typedef struct gogp_test_gemm_opts {
  int32_t ktri, krag0, new_row0, kbeg0, small_below, prio;
  int32_t rule, tpb_shift, rblk0, cblk0, pr, Pr, pc, Pc, beta0;
  int32_t k;
  int64_t bstride;
} gogp_test_gemm_opts;

/* The product launcher of the tile kernel on host buffers: C = beta C + alpha A B^T over mt x nt tiles of 128 in `mode`
 * (0 RECT, 1 LOWER, 2 LAUUM, 3 TRAP), precision 64 (double) or 32 (float).  A, B, C hold a_len, b_len, c_len elements;
 * the launch sees them at element offsets a_off, b_off, c_off with leading dimensions lda, ldb, ldc.  Each array is
 * copied whole to the device and C whole back.  opt == NULL: the launcher's defaults.  Returns GOGP_EARG, before the
 * device is touched, for K not a multiple of the K-step (16 / 32), leading dimensions or offsets that are not 16-byte
 * aligned, arrays that do not cover the region the launch addresses, mt != nt for LOWER / LAUUM, alpha == 0, options
 * the mode does not have, and fp32 with k > 1 or kbeg0 != 0 (the fp32 kernel has neither). */
int gogp_test_gemm_nt(int device, int precision, int mode, int mt, int nt, int64_t K, double alpha, double beta,
                      const void *A, int64_t a_len, int64_t a_off, int64_t lda, const void *B, int64_t b_len,
                      int64_t b_off, int64_t ldb, void *C, int64_t c_len, int64_t c_off, int64_t ldc,
                      const gogp_test_gemm_opts *opt);

/* What the launcher of the tile kernel would launch for these arguments (gemm_plan, gogp_amd/csrc/gemm_plan.h): the
 * instance (tile 64 or 128, 4 or 8 waves), the grid, the flops it books on the profile (all opt->k candidates) and its
 * launch tag.  Never touches the device.  GOGP_EARG for the arguments gogp_test_gemm_nt refuses (buffers aside). */
typedef struct gogp_test_gemm_plan_out {
  int32_t tile, waves;
  int64_t grid_x, grid_z;
  double flops;
  int64_t tag;
} gogp_test_gemm_plan_out;
int gogp_test_gemm_plan(int precision, int mode, int mt, int nt, int64_t K, const gogp_test_gemm_opts *opt,
                        gogp_test_gemm_plan_out *out);

/* The fp32 path's fp64 update of the diagonal blocks (diagsyrk.hip): D64 block b (bs x bs, bs = 256 or 512) -= R_b R_b^T
 * with R_b the bs x K floats at L + l_off + b * row_stride (leading dimension ld), for b < nblocks.  bs = 256 drives
 * launch_diag_syrk_f64 (row_stride must be 256 ld), bs = 512 launch_diag_syrk_f64_tiles.  GOGP_EARG for K not a
 * multiple of 16 or below 16 and for buffers that do not cover the launch. */
int gogp_test_diag_syrk(int device, int bs, const float *L, int64_t l_len, int64_t l_off, int64_t ld, int64_t K,
                        int64_t row_stride, double *D64, int64_t d_len, int nblocks);

/* The product build of the diagonal-block kernel (diag256.hip) on one 256 x 256 block: variant 0 factor + inverse,
 * 1 the same with Dinv of leading dimension 512, 2 inverse only (A holds the factor), 3 inverse only at 512.  A: 256 x ld,
 * L: 256 x ldl (in / out; variants 0, 1 write the factor), Dinv: 256 x (256 | 512) (in / out), info: in / out. */
int gogp_test_diag256_product(int device, int variant, const double *A, int64_t ld, double *L, int64_t ldl,
                              double *Dinv, int64_t row0, int64_t nvalid, long long *info);

/* ---- the kernels that consume the factor, through their product launchers (tests/test_substitution_kernels.py).
 * As gogp_test_gemm_nt: precision 64 (double) or 32 (float) is the element type of the MATRICES (vectors, sums of squares
 * and solutions are doubles either way); lengths count elements; every array is copied to the device whole and every
 * in / out array whole back; GOGP_EARG, before the device is touched, for anything a launch cannot honour or that the
 * arrays do not cover. */

/* Bytes of the workspace of one launch of the one-pass substitution (trsm_small_workspace_bytes); -1: bad npad. */
int64_t gogp_test_trsm_small_workspace(int64_t npad);

/* One launch_trsm_small (trsm_small.hip): V = L^-1 Kstar for the right-hand sides j0 .. j0 + cnt - 1 (rows of KsT, leading
 * dimension ldk; cnt <= 32) by the blocked substitution with the GIVEN block inverses Dinv (npad / 256 blocks of 256 x 256,
 * npad * 256 elements).  L: npad rows of ld.  dq (in / out): dq[j] = |V_j|^2 for those j.  sol (in / out, sol_len bytes =
 * gogp_test_trsm_small_workspace(npad)): the launch's workspace -- its initial contents go to the device, so a test can
 * hand in what an earlier launch left there.  kind, width, sol_off: what trsm_small_solution says for this launch --
 * the layout (common.h: TS_SOL_*) and the byte offset of V in the workspace.  tmo: the time-out word (0: fine).  The
 * instances on 16-column tiles read the rows j0 .. j0 + 15 (cnt <= 16) or .. j0 + 31 of KsT: k_len must cover them. */
int gogp_test_trsm_small(int device, int precision, int64_t npad, const void *L, int64_t l_len, int64_t ld,
                         const void *Dinv, const void *KsT, int64_t k_len, int64_t ldk, int j0, int cnt, double *dq,
                         int64_t dq_len, void *sol, int64_t sol_len, int *kind, int *width, int64_t *sol_off,
                         unsigned *tmo);

/* The substitution steps of solve.hip as the product runs them: dir 0 launch_trsv_fwd_step for b = b0 .. b1 ascending
 * (out = z), dir 1 launch_trsv_bwd_step for b = b1 .. b0 descending (out = alpha); w in / out.  k > 1 (fp64 forward
 * only, as in the product): k candidates, candidate c's L, Dinv, w and out lying c * bstride ELEMENTS after candidate
 * 0's.  Dinv holds (k - 1) * bstride + npad * 256 elements. */
int gogp_test_trsv_steps(int device, int precision, int dir, int64_t npad, const void *L, int64_t l_len, int64_t ld,
                         const void *Dinv, int b0, int b1, int k, int64_t bstride, double *w, int64_t w_len, double *out,
                         int64_t out_len);

/* launch_alpha_from_y: alpha_i = sum_{q >= q0(i)} Y[i][q] z[q], q0 the first column of row i's 256-block. */
int gogp_test_alpha_from_y(int device, int precision, int64_t npad, const void *Y, int64_t y_len, int64_t ld,
                           const double *z, int64_t z_len, double *alpha, int64_t alpha_len);

/* launch_rownorm_dot over the m rows of V (ncols columns, ld): dot_j = V_j . vec, sq_j = |V_j|^2; vec, dot and sq may
 * each be NULL, as for the launcher. */
int gogp_test_rownorm_dot(int device, int precision, const void *V, int64_t v_len, int64_t ld, int64_t ncols, int64_t m,
                          const double *vec, int64_t vec_len, double *dot, int64_t dot_len, double *sq, int64_t sq_len);

/* launch_tinv_init: the diagonal 256-blocks of X (256 nsub rows of tld; in / out) := Dinv_i (nsub blocks), zeros above
 * them; with_xt: XT (x_len elements too; in / out) the same for the transpose. */
int gogp_test_tinv(int device, int precision, int nsub, const void *Dinv, void *X, int64_t x_len, int64_t tld, int with_xt,
                   void *XT);

/* launch_blockmm: nprod (<= 6) products C_b (256 x 256, ldc) = alpha A_b (256 x K_b, lda) B_b (K_b x 256, ldb), plain
 * A B, all operands at element offsets into ONE arena (in / out), K_b multiples of 32; k > 1 (fp64 only): candidates
 * bstride elements apart. */
int gogp_test_blockmm(int device, int precision, int nprod, void *arena, int64_t arena_len, const int64_t *a_off,
                      const int64_t *lda, const int64_t *b_off, const int64_t *ldb, const int64_t *c_off,
                      const int64_t *ldc, const int *K, double alpha, int k, int64_t bstride);

/* ---- the kernels that turn K^-1 into the gradient, through their product launchers (tests/test_grad_kernels.py):
 * grad_reduce_kernel and grad_final_kernel (grad.hip), grad_ard_mfma_kernel (grad_mfma.hip), mirror_lower_kernel and
 * xgrad_kernel (grad.hip).  The rules of the hooks above: lengths count elements, every array goes to the device whole and
 * every in / out array whole back, GOGP_EARG before the device is touched for anything a launch cannot honour or the
 * arrays do not cover. */

/* Every field of the kernels' DevParams (gogp_amd/csrc/common.h) that they read, stated directly -- not derived from a
 * descriptor and natural parameters as the product does: inv_len[t][d] = 1 / l_d of term t (0 for d >= ndim), w[t] =
 * pi / period of a periodic term, c[t] its output scale. */
typedef struct gogp_test_kparams {
  int32_t ndim, nterms;
  int32_t kind[GOGP_MAX_TERMS], ard[GOGP_MAX_TERMS];
  double c[GOGP_MAX_TERMS], w[GOGP_MAX_TERMS], inv_len[GOGP_MAX_TERMS][GOGP_MAX_NDIM];
  double noise_var, dnoise;
  int32_t nevents, ev_axis;
  double ev_from[GOGP_MAX_EVENTS], ev_to[GOGP_MAX_EVENTS], ev_disc[GOGP_MAX_EVENTS];
} gogp_test_kparams;

#define GOGP_TEST_NACC (16 + GOGP_MAX_NDIM) /* slot sums of the reduction (common.h: NACC) */

/* Workgroups launch_grad_reduce (mrows == 0: npad x npad, lower tiles) or launch_grad_reduce_local (mrows x ncols local
 * tiles) starts for max_blocks: `partials` holds that many rows of GOGP_TEST_NACC.  -1: bad arguments.  No device. */
int gogp_test_grad_blocks(int64_t npad, int64_t mrows, int64_t ncols, int max_blocks);

/* launch_grad_reduce.  precision: element type of Kinv (64 / 32; npad rows of ld >= npad).  kparams: k structs.  X:
 * npad * ndim + GOGP_MAX_NDIM doubles (the slack the product allocates zeroed).  ard_dims: 0 or ndim (exactly when one
 * term has ard set); radial1: one term, not periodic; ev: the instances with event discounts (never with ard_dims).
 * max_blocks: 0 or a cap on the grid.  k > 1 (precision 64 only): candidates -- X is shared; candidate c's alpha, Kinv and
 * partials lie c * bstride ELEMENTS after candidate 0's in their host arrays (on the device every per-candidate buffer,
 * the parameters included, c * bstride * 8 bytes after candidate 0's: bstride must cover each of them).  partials (in /
 * out): gogp_test_grad_blocks rows; out (in / out): k x GOGP_TEST_NACC, compact. */
int gogp_test_grad_reduce(int device, int precision, const gogp_test_kparams *kparams, int ard_dims, int radial1,
                          int mfma_min, int ev, const double *X, int64_t x_len, const double *alpha, int64_t alpha_len,
                          const void *Kinv, int64_t kinv_len, int64_t ld, int64_t n, int64_t npad, int max_blocks, int k,
                          int64_t bstride, double *partials, int64_t partials_len, double *out);

/* launch_grad_reduce_local: the same over the mrows x ncols local tiles (ld >= ncols) of a 2-D block-cyclic K^-1 of npad
 * rows, distribution blocks of 2^nb_shift, this rank at (pr, pc) of the Pr x Pc grid (common.h: BlockMap).  X and alpha
 * are the global ones.  The launcher has no candidates: k must be 1. */
int gogp_test_grad_reduce_local(int device, int precision, const gogp_test_kparams *kparams, int ard_dims, int radial1,
                                int mfma_min, int ev, const double *X, int64_t x_len, const double *alpha,
                                int64_t alpha_len, const void *Kinv, int64_t kinv_len, int64_t ld, int64_t n, int64_t npad,
                                int64_t mrows, int64_t ncols, int nb_shift, int pr, int Pr, int pc, int Pc, int max_blocks,
                                int k, int64_t bstride, double *partials, int64_t partials_len, double *out);

/* launch_xgrad: mirrors the lower triangle of Kinv (npad rows of ld; in / out) to the upper one outside the diagonal
 * 32 x 32 blocks, then gx (npad x ndim; in / out) rows < n := sum_j (alpha_i alpha_j - Kinv_ij) dk(x_i, x_j) / dx_i. */
int gogp_test_xgrad(int device, const gogp_test_kparams *kparams, int ev, const double *X, int64_t x_len,
                    const double *alpha, int64_t alpha_len, double *Kinv, int64_t kinv_len, int64_t ld, int64_t n,
                    int64_t npad, double *gx, int64_t gx_len);

/* ---- the kernels that update a factor or consume Produce's V^T, through their product launchers
 * (tests/test_update_kernels.py): append_gram_kernel and append_commit_kernel (append.hip), the kernels of remove.hip,
 * bwd_panel_kernel (pgrad.hip) and the two kernels of launch_pcov (pcov.hip).  The rules of the hooks above: lengths count
 * elements (BYTES for the raw solution buffers, as sol_len of gogp_test_trsm_small), every array goes to the device whole
 * and every in / out array whole back, GOGP_EARG before the device is touched. */

/* launch_append_gram: V (npc rows, a multiple of 256; m <= 64 right-hand sides) is read from two raw buffers -- the columns
 * j < m0 from sol0, the others (as column j - m0) from sol1 --, each in the layout `kind` (common.h: TS_SOL_*; 3 = ROWS, one
 * solution per row of `width` doubles) of `width`, beginning `off` bytes into the buffer.  A buffer no column is read from
 * may be NULL.  z: npc doubles.  part (in / out): npc / 256 slots of 64 * 64 + 64 doubles.  Lnew (in / out): m rows of ld,
 * columns k < n <= npc are written. */
int gogp_test_append_gram(int device, const void *sol0, int64_t sol0_len, int kind0, int width0, int64_t off0,
                          const void *sol1, int64_t sol1_len, int kind1, int width1, int64_t off1, int m0, int m,
                          int64_t npc, int64_t n, const double *z, int64_t z_len, double *part, int64_t part_len,
                          double *Lnew, int64_t lnew_len, int64_t ld);

/* launch_append_commit: S = k(X2, X2) + noise - sum of the nslab parts, its factor to Lnew (in / out; m rows of ld) columns
 * n .. n + m - 1, z2 (in / out) = L22^-1 (y2 - sum of the parts' V^T z); not positive definite: *info (in / out) = n + pivot
 * + 1 unless it was non-zero already, nothing else written. */
int gogp_test_append_commit(int device, const gogp_test_kparams *kparams, int ev, const double *X2, int64_t x2_len,
                            const double *y2, int64_t y2_len, int m, int64_t n, const double *part, int64_t part_len,
                            int nslab, double *Lnew, int64_t lnew_len, int64_t ld, double *z2, int64_t z2_len,
                            long long *info);

/* gogp_test_append_commit behind launch_nv_append_fold (noisevar.hip), as gogp_append_noisy launches them: the first
 * part's diagonal takes -v2 (m values), so that S = k(X2, X2) + noise + diag(v2) - sum of the parts.  v2 == NULL with
 * v2_len == 0: launch_append_commit alone.  part is in / out here: it comes back whole. */
int gogp_test_nv_append_commit(int device, const gogp_test_kparams *kparams, int ev, const double *X2, int64_t x2_len,
                               const double *y2, int64_t y2_len, const double *v2, int64_t v2_len, int m, int64_t n,
                               double *part, int64_t part_len, int nslab, double *Lnew, int64_t lnew_len, int64_t ld,
                               double *z2, int64_t z2_len, long long *info);

/* launch_remove_gather: dst (in / out; npad1 x npad1) from src (leading dimension ld0) through map (n1 old row indices,
 * every one a row src holds whole). */
int gogp_test_remove_gather(int device, const double *src, int64_t src_len, int64_t ld0, const int *map, int64_t map_len,
                            int64_t n1, double *dst, int64_t dst_len, int64_t npad1);

/* launch_remove_w: W (in / out; mw <= 32 columns of npad1 doubles) rows r0 .. npad1 - 1 from src[map, rem[0 .. mc)]. */
int gogp_test_remove_w(int device, const double *src, int64_t src_len, int64_t ld0, const int *map, int64_t map_len,
                       const int *rem, int64_t rem_len, int mc, int mw, int64_t r0, int64_t n1, int64_t npad1, double *W,
                       int64_t w_len);

/* launch_remove_snap for the 128-blocks snap_b0 .. snap_b0 + snap_nb - 1 (none with snap_nb == 0: the snapshot is what the
 * caller hands in), then launch_remove_block for kb = kb0, kb0 + 128, .. kb1 (kb1 == kb0: one step; the product loops to the
 * last kb < n1).  L (in / out): ld x ld, ld a multiple of 256; W (in / out): mw (4 or 32) columns of ld doubles; snap
 * (in / out): 128 x 128 doubles per block, block b at b * 16384. */
int gogp_test_remove_block(int device, double *L, int64_t l_len, int64_t ld, int snap_b0, int snap_nb, double *snap,
                           int64_t snap_len, double *W, int64_t w_len, int mw, int64_t kb0, int64_t kb1, int64_t n1);

/* launch_bwd_panel: C (in / out) = A B, or C - A B with sub; A 16 rows16 x K, B K x ncols, C 16 rows16 x ncols at element
 * offsets into their arrays; ncols a multiple of 64, K of 32.  Beyond 32 rows the kernel works on groups of 64 rows: A and
 * C must hold 64 ceil(rows16 / 4) rows then (GOGP_EARG otherwise). */
int gogp_test_bwd_panel(int device, int64_t rows16, const double *A, int64_t a_len, int64_t a_off, int64_t lda,
                        const double *B, int64_t b_len, int64_t b_off, int64_t ldb, double *C, int64_t c_len, int64_t c_off,
                        int64_t ldc, int64_t ncols, int64_t K, int tri, int sub);

/* pcov_slabs: the number of slabs launch_pcov splits npad columns into for m test points on ncu compute units, and the
 * columns per slab.  -1: bad arguments.  No device. */
int gogp_test_pcov_slabs(int64_t npad, int64_t m, int ncu, int *cols_per_slab);

/* launch_pcov with the number of compute units GIVEN: out (in / out; mo rows of ldo) = k(Z, Z) - Vt Vt^T (+ diag_add on the
 * diagonal) on the leading m x m, identity up to mo.  Vt: m rows of ld (even) doubles, npad columns read; NULL: the prior
 * Gram matrix (part may be NULL then).  part (in / out): gogp_test_pcov_slabs x pairs x 4096 doubles, pairs = t (t + 1) / 2,
 * t = ceil(m / 64). */
int gogp_test_pcov(int device, const gogp_test_kparams *kparams, int ev, const double *Z, int64_t z_len, int64_t m,
                   const double *Vt, int64_t vt_len, int64_t ld, int64_t npad, int ncu, double *part, int64_t part_len,
                   double diag_add, double *out, int64_t out_len, int64_t mo, int64_t ldo);

/* launch_multi_weight (multi.hip): G (in / out; npad rows of ldk, as Kinv) = T Kinv - A A^T on the elements j <= i < n of the
 * lower 64 x 64 tiles of npad, exact zeros on the rest of those tiles, nothing outside them.  At: T (1 .. GOGP_MULTI_MAX_T)
 * rows of ld doubles, npad columns read, row t = column t of A; the hook appends the zero rows up to a multiple of 4 that the
 * product keeps.  Of Kinv only j <= i < n is read.  npad a multiple of 256, 1 <= n <= npad. */
int gogp_test_multi_weight(int device, const double *At, int64_t at_len, int64_t ld, int T, const double *Kinv,
                           int64_t kinv_len, int64_t ldk, int64_t n, int64_t npad, double *G, int64_t g_len);

/* ---- the kernels of basis.hip through their product launchers (tests/test_basis_kernels.py).  The rules of the hooks
 * above: lengths count elements, every array goes to the device whole and every in / out array whole back, GOGP_EARG before
 * the device is touched.  npad a multiple of 256, 1 <= n <= npad, 1 <= p <= GOGP_BASIS_MAX_P, p4 = p rounded up to 4.
 * gogp_test_basis_symm_slabs / gram_slabs: the slabs the launchers split n observations into (no device is touched).
 * basis_symm: Wt (in / out; at least p4 rows of ld >= npad) = (Kinv H)^T, of the symmetric Kinv (npad rows of ldk) only
 * j <= i < n read; Ht: p rows of ld; part (in / out): slabs * p4 * ld.  Rows < p4 of Wt are written whole (ld columns).
 * basis_gram: Ag (in / out; p (p + 1)) = Ht [Wt^T | alpha]; part: slabs * p (p + 1).  basis_finish: LA, Ainv (p p),
 * beta (p), scal (2), info (1: 0 or the first bad pivot + 1, as a double; the others are then left as they were).
 * basis_cols: Ct (in / out; (p + 1 rounded up to 4) rows of ld).  basis_predict: mu, sigma (m; sigma_len == 0 with
 * sigma NULL: not computed); Hz m x p, KW m rows of ldkw >= p. */
int gogp_test_basis_symm_slabs(int64_t n);
int gogp_test_basis_gram_slabs(int64_t n);
int gogp_test_basis_symm(int device, const double *Kinv, int64_t kinv_len, int64_t ldk, int64_t n, int64_t npad,
                         const double *Ht, int64_t ht_len, int64_t ld, int p, double *part, int64_t part_len, double *Wt,
                         int64_t wt_len);
int gogp_test_basis_gram(int device, const double *Ht, int64_t ht_len, const double *Wt, int64_t wt_len, int64_t ld,
                         const double *alpha, int64_t alpha_len, int64_t n, int p, double *part, int64_t part_len, double *Ag,
                         int64_t ag_len);
int gogp_test_basis_finish(int device, const double *Ag, int64_t ag_len, int p, double *LA, int64_t la_len, double *Ainv,
                           int64_t ainv_len, double *beta, int64_t beta_len, double *scal, int64_t scal_len, double *info,
                           int64_t info_len);
int gogp_test_basis_cols(int device, const double *Wt, int64_t wt_len, int64_t ld, int64_t n, int p, const double *LA,
                         int64_t la_len, const double *beta, int64_t beta_len, const double *alpha, int64_t alpha_len,
                         double *Ct, int64_t ct_len);
int gogp_test_basis_predict(int device, const double *Hz, int64_t hz_len, const double *KW, int64_t kw_len, int64_t ldkw,
                            int64_t m, int p, const double *beta, int64_t beta_len, const double *Ainv, int64_t ainv_len,
                            const double *mu0, int64_t mu0_len, const double *prior, int64_t prior_len, const double *q,
                            int64_t q_len, double *mu, int64_t mu_len, double *sigma, int64_t sigma_len);

/* launch_sparse_syrk (sparse.hip): Bacc (in / out; Mp rows of ldb) += Vt^T Vt on the whole lower 64 x 64 tiles of Mp x Mp and
 * r (in / out; Mp doubles) += Vt^T y.  Vt: `rows` (1 .. 65536) rows of ld doubles, Mp columns read, of which the columns
 * >= M count as exact zeros; Mp a multiple of 64 up to GOGP_SPARSE_MAX_M, 1 <= M <= Mp. */
int gogp_test_sparse_syrk(int device, const double *Vt, int64_t vt_len, int64_t ld, int64_t rows, int64_t M, int64_t Mp,
                          const double *y, int64_t y_len, double *Bacc, int64_t b_len, int64_t ldb, double *r, int64_t r_len);
/* launch_sparse_grad (sparse.hip): out (in / out; GOGP_TEST_NACC slot sums; `accumulate`: added to what it holds) =
 * sum_{f < rows, u < M} (Wt[f][u] + y_f mvec_u s4) dk(x_f, u_u) / dlog theta.  X: rows x ndim, U: M x ndim, Wt: rows rows of
 * ldw >= M doubles; no event discounts. */
int gogp_test_sparse_grad(int device, const gogp_test_kparams *kparams, const double *X, int64_t x_len, int64_t rows,
                          const double *U, int64_t u_len, int64_t M, const double *Wt, int64_t wt_len, int64_t ldw,
                          const double *y, int64_t y_len, const double *mvec, int64_t m_len, double s4, int accumulate,
                          double *out /* GOGP_TEST_NACC */);
/* launch_sparse_ugrad (sparse.hip): dU (in / out; M x ndim of du_len doubles; `accumulate`: added to what it holds, what lies
 * beyond M x ndim is left alone) = sum_{f < rows} (Wt[f][u] + y_f mvec_u s4) dk(u_u, x_f) / du_u: the arguments of
 * gogp_test_sparse_grad. */
int gogp_test_sparse_ugrad(int device, const gogp_test_kparams *kparams, const double *X, int64_t x_len, int64_t rows,
                           const double *U, int64_t u_len, int64_t M, const double *Wt, int64_t wt_len, int64_t ldw,
                           const double *y, int64_t y_len, const double *mvec, int64_t m_len, double s4, int accumulate,
                           double *dU /* in / out, M x ndim */, int64_t du_len);
/* sparse_ugrad_slabs: the slabs of row tiles launch_sparse_ugrad splits `rows` rows into for M inducing points and the
 * 64-row tiles of one (the last may hold fewer); no device is touched.  0 for rows or M out of range. */
int gogp_test_sparse_ugrad_slabs(int64_t rows, int64_t M, int *tiles_per_slab);
/* sparse_ugrad_slabs_bound: the slabs gogp_sparse_gradient_inducing sizes its partials by for chunks of up to `rows` rows: at
 * least gogp_test_sparse_ugrad_slabs(r, M) for every r <= rows (the slab count is not monotone in the rows).  0 out of range. */
int gogp_test_sparse_ugrad_slabs_bound(int64_t rows, int64_t M);
/* launch_sparse_xty (sparse.hip): R (in / out; T rounded up to 64 rows of ldr doubles, row t = output t, of which the columns
 * below M rounded up to 64 are touched) += Y^T Vt.  Vt: `rows` (1 .. 65536) rows of ld doubles, of which the columns >= M count
 * as exact zeros and are never multiplied; Y: `rows` rows of ldy >= T doubles, 1 <= T <= GOGP_SPARSE_MULTI_MAX_T, the columns
 * >= T likewise.  Mp a multiple of 64 up to GOGP_SPARSE_MAX_M, 1 <= M <= Mp <= ldr. */
int gogp_test_sparse_xty(int device, const double *Vt, int64_t vt_len, int64_t ld, int64_t rows, int64_t M, int64_t Mp,
                         const double *Y, int64_t y_len, int64_t ldy, int64_t T, double *R, int64_t r_len, int64_t ldr);
/* sparse_xty_slabs: the slabs of rows launch_sparse_xty splits `rows` rows into for M inducing points and T outputs, and the
 * rows of one (the last may hold fewer); sparse_xty_slabs_bound: the slabs gogp_sparse_multi_observe sizes its partials by for
 * chunks of up to `rows` rows, at least gogp_test_sparse_xty_slabs(r, M, T) for every r <= rows.  No device is touched; 0 for
 * an argument out of range. */
int gogp_test_sparse_xty_slabs(int64_t rows, int64_t M, int64_t T, int64_t *rows_per_slab);
int gogp_test_sparse_xty_slabs_bound(int64_t rows, int64_t M, int64_t T);

/* Greedy selection of inducing points (select.hip; the algorithm: include/gogp_hip.h, gogp_sparse_select_inducing).
 * gogp_test_select_step: ONE step j (0 <= j < GOGP_SPARSE_MAX_M) of launch_select_step on host arrays.  X: N rows (1 <= N <=
 * 2^22) of kparams->ndim; Lt (in / out): j + 1 columns of ldn doubles (ldn >= N, a multiple of 256), column t at Lt + t ldn --
 * the columns < j are read on the rows < N, column j receives the new column on the rows < N, nothing else is touched; d
 * (in / out, N), sel (in / out, N: 1 = selected earlier); part_v / part_i: the previous launch's partial maxima, one (value,
 * row) pair per workgroup, part_len == the workgroups of the launch = min(ceil(N / 256), 1024), or max_blocks where that is
 * positive and smaller (workgroup b owns the rows i with (i / 256) mod workgroups == b), every part_i in [0, N).  out_v /
 * out_i (out_len >= workgroups): the new partials; *p, *dp: the pivot and its residual, *p = -1 (and nothing else written)
 * where the step stops: not (dp > tol).  tol finite, >= 0.  No event discounts.
 * gogp_test_select_run: the whole loop (select_run) with max_blocks forced and, d0 != NULL, d0 (N) in the place of the
 * initial diagonal k(x_i, x_i).  idx, pivots: M entries, the first *m_out written; optional (NULL or with their lengths) U
 * (M x ndim), Lt (min(M, N) columns of N rounded up to 256; NaN where no step wrote) and d (N, the final residuals). */
int gogp_test_select_step(int device, const gogp_test_kparams *kparams, const double *X, int64_t x_len, int64_t N,
                          double *Lt, int64_t lt_len, int64_t ldn, int64_t j, double tol, double *d, int64_t d_len,
                          unsigned char *sel, int64_t sel_len, const double *part_v, const int64_t *part_i,
                          int64_t part_len, int max_blocks, double *out_v, int64_t *out_i, int64_t out_len, int64_t *p,
                          double *dp);
int gogp_test_select_run(int device, const gogp_test_kparams *kparams, const double *X, int64_t x_len, int64_t N, int64_t M,
                         double tol, int max_blocks, const double *d0, int64_t d0_len, int64_t *idx, double *pivots,
                         double *U, int64_t u_len, double *Lt, int64_t lt_len, double *d, int64_t d_len, int64_t *m_out,
                         double *trace);

/* ---- the small kernels that finish a leave-one-out, multi-output or sparse evaluation, through their product launchers
 * (tests/test_finish_kernels.py): the four kernels of loo.hip, multi_dots_kernel (multi.hip) and the element-wise, scalar and
 * Produce kernels of sparse.hip.  The rules of the hooks above: lengths count elements, every array goes to the device whole
 * and every in / out array whole back, GOGP_EARG before the device is touched for anything a launch cannot honour or the
 * arrays do not cover.  npad: a multiple of 256, 1 <= n <= npad. */

/* launch_loo_stats: Kinv npad rows of ld >= npad, of which only the diagonal elements i < n are read; alpha, y: n doubles
 * read.  mu, sigma, logp (in / out): the rows i < n written.  v, sc (in / out, npad doubles): written in full, exact zeros
 * from row n on.  part (in / out): npad / 256 block sums of log p, a block without a live row exactly 0. */
int gogp_test_loo_stats(int device, const double *Kinv, int64_t kinv_len, int64_t ld, const double *alpha, int64_t alpha_len,
                        const double *y, int64_t y_len, int64_t n, int64_t npad, double *mu, int64_t mu_len, double *sigma,
                        int64_t sigma_len, double *logp, int64_t logp_len, double *v, int64_t v_len, double *sc, int64_t sc_len,
                        double *part, int64_t part_len);
/* launch_loo_scale_symv (loo_scale_symv_kernel, then loo_u_final_kernel): B (in / out; npad rows of ldb >= npad) = K^-1
 * diag(sc) on npad x npad, u (in / out; npad doubles) = K^-1 v, both exactly zero from row / column n on; upart (in / out):
 * npad / 64 slots of npad doubles, every one written.  Of Kinv (npad rows of ld) only j <= i < n is read.  PRECONDITION of the
 * launcher: sc and v (npad doubles each) are finite and zero from row n on -- the kernel multiplies the masked zeros of the
 * rows and columns >= n by them. */
int gogp_test_loo_scale_symv(int device, const double *Kinv, int64_t kinv_len, int64_t ld, int64_t n, int64_t npad,
                             const double *sc, int64_t sc_len, const double *v, int64_t v_len, double *B, int64_t b_len,
                             int64_t ldb, double *upart, int64_t upart_len, double *u, int64_t u_len);
/* launch_loo_rank2: G (in / out; npad rows of ld) -= u alpha^T + alpha u^T on the whole lower 64 x 64 tiles.  alpha: n doubles
 * read (zero beyond).  PRECONDITION of the launcher: u (npad doubles) is finite and zero from row n on, and G is finite on
 * those tiles: the elements with i >= n or j >= n then keep their bits. */
int gogp_test_loo_rank2(int device, double *G, int64_t g_len, int64_t ld, int64_t n, int64_t npad, const double *u,
                        int64_t u_len, const double *alpha, int64_t alpha_len);
/* The two kernels of leave-block-out cross-validation (blockcv.hip; tests/test_blockcv_kernels.py) on caller-supplied
 * matrices.  start, F: as gogp_blockcv_check accepts them for n (else GOGP_EARG); the packing into groups is
 * gogp_blockcv_groups'.
 * launch_blockcv_groups: Kinv n rows of ld >= n, of which only the elements j <= i inside a block are read; alpha, y: n
 * doubles read.  In / out: mu, sigma, v, ones (n doubles: every row written, ones with 1.0), logp (F doubles), Sg
 * (ngroups x 128 x 128 doubles: S_B on the diagonal blocks of each group, exact zeros elsewhere) and info (ngroups
 * entries: the first failing pivot's row + 1, or 0; a failing group writes nothing else). */
int gogp_test_blockcv_groups(int device, const double *Kinv, int64_t kinv_len, int64_t ld, const double *alpha,
                             int64_t alpha_len, const double *y, int64_t y_len, int64_t n, const int64_t *start, int64_t F,
                             double *mu, int64_t mu_len, double *sigma, int64_t sigma_len, double *v, int64_t v_len,
                             double *ones, int64_t ones_len, double *logp, int64_t logp_len, double *Sg, int64_t sg_len,
                             int64_t *info, int64_t info_len);
/* launch_blockcv_apply: the matrix at Q + q_off (in / out; `rows` rows of ld >= n, rows a multiple of 64 and >= n)
 * <- itself times blockdiag(S_g), in place, on the 64-row slices that hold a row < n and the columns < n; nothing else of
 * Q is read or written.  Sg: ngroups x 128 x 128 doubles, read. */
int gogp_test_blockcv_apply(int device, double *Q, int64_t q_len, int64_t q_off, int64_t ld, int64_t rows, int64_t n,
                            const int64_t *start, int64_t F, const double *Sg, int64_t sg_len);
/* launch_multi_dots: dots[t] (in / out) = sum_{i < n} Yt[t][i] At[t][i], t < T <= GOGP_MULTI_MAX_T; Yt, At: T rows of
 * ld >= n. */
int gogp_test_multi_dots(int device, const double *Yt, int64_t yt_len, const double *At, int64_t at_len, int64_t ld, int64_t n,
                         int T, double *dots, int64_t dots_len);
/* The four Mp x Mp element-wise launchers of sparse.hip (leading dimension Mp): Mp a multiple of 256 -- their grid is Mp / 256
 * workgroups per row -- up to GOGP_SPARSE_MAX_M; every matrix holds Mp * Mp elements at least, g holds Mp.
 * finish_b: B (in / out) = I + Bacc inv_s2 in both triangles from the elements a >= b of Bacc.  copy_upper: dst (in / out) =
 * src on j >= i, +0.0 below.  weights: T = I - Binv - g g^T s4, S = 2 I - B - Binv - g g^T s4.  multi_weights: Tm =
 * T (I - Binv) - GG s4, S = T (2 I - B - Binv) - GG s4 with T (1 .. GOGP_SPARSE_MULTI_MAX_T) the number of outputs. */
int gogp_test_sparse_finish_b(int device, const double *Bacc, int64_t bacc_len, int64_t Mp, double inv_s2, double *B,
                              int64_t b_len);
int gogp_test_sparse_copy_upper(int device, const double *src, int64_t src_len, int64_t Mp, double *dst, int64_t dst_len);
int gogp_test_sparse_weights(int device, const double *B, int64_t b_len, const double *Binv, int64_t binv_len, const double *g,
                             int64_t g_len, int64_t Mp, double s4, double *T, int64_t t_len, double *S, int64_t s_len);
int gogp_test_sparse_multi_weights(int device, const double *B, int64_t b_len, const double *Binv, int64_t binv_len,
                                   const double *GG, int64_t gg_len, int64_t Mp, int T, double s4, double *Tm, int64_t tm_len,
                                   double *S, int64_t s_len);
/* launch_sparse_scalars: out[0 .. 4] (in / out) = sum_{i < M} of 2 log C_ii, B_ii - 1, Binv_ii, r_i g_i, g_i^2; of the
 * matrices (leading dimension Mp, 1 <= M <= Mp <= GOGP_SPARSE_MAX_M) only the diagonal elements i < M are read, of r and g the
 * first M. */
int gogp_test_sparse_scalars(int device, const double *C, int64_t c_len, const double *B, int64_t b_len, const double *Binv,
                             int64_t binv_len, const double *r, int64_t r_len, const double *g, int64_t g_len, int64_t M,
                             int64_t Mp, double *out, int64_t out_len);
/* launch_sparse_sumsq: out[0] (in / out) = sum_{i < n} y_i^2. */
int gogp_test_sparse_sumsq(int device, const double *y, int64_t y_len, int64_t n, double *out, int64_t out_len);
/* launch_sparse_predict: mu_j (in / out) = dot_j inv_s2, sigma_j (in / out) = sqrt(prior_j - q_j + sum_{i < ncols} A[j][i]
 * V[j][i]) for j < m <= 4 * 65535, unclamped; A, V: m rows of ld >= ncols.  launch_sparse_multi_sigma: the sigma alone. */
int gogp_test_sparse_predict(int device, const double *A, int64_t a_len, const double *V, int64_t v_len, int64_t ld,
                             int64_t ncols, int64_t m, const double *prior, int64_t prior_len, const double *q, int64_t q_len,
                             const double *dot, int64_t dot_len, double inv_s2, double *mu, int64_t mu_len, double *sigma,
                             int64_t sigma_len);
int gogp_test_sparse_multi_sigma(int device, const double *A, int64_t a_len, const double *V, int64_t v_len, int64_t ld,
                                 int64_t ncols, int64_t m, const double *prior, int64_t prior_len, const double *q,
                                 int64_t q_len, double *sigma, int64_t sigma_len);
/* launch_sparse_multi_dots: out[t] (in / out) = sum_{i < M} Rt[t][i] Gt[t][i] and out[tstride + t] = sum_{i < M} Gt[t][i]^2,
 * t < T <= tstride; Rt, Gt: T rows of ld >= M.  launch_sparse_multi_sumsq: out[t] = sum_{i < n} Y[i][t]^2, Y: n rows of
 * ldy >= T. */
int gogp_test_sparse_multi_dots(int device, const double *Rt, int64_t rt_len, const double *Gt, int64_t gt_len, int64_t ld,
                                int64_t M, int T, int tstride, double *out, int64_t out_len);
int gogp_test_sparse_multi_sumsq(int device, const double *Y, int64_t y_len, int64_t ldy, int64_t n, int T, double *out,
                                 int64_t out_len);
/* launch_sparse_multi_pad: Yp (in / out; rpad rows of ldp >= kp) = the `rows` <= rpad rows of Y (ldy >= T, T <= kp) on
 * rpad x kp, +0.0 outside rows x T.  rpad * kp must be a multiple of 256: the launcher starts whole workgroups, and would
 * return without a launch otherwise (the hook refuses instead). */
int gogp_test_sparse_multi_pad(int device, const double *Y, int64_t y_len, int64_t ldy, int64_t rows, int64_t T, int64_t kp,
                               int64_t rpad, double *Yp, int64_t yp_len, int64_t ldp);

/* Benchmark hook for the tile kernel: `reps` launches of one shape (mode 0 RECT
 * mt x nt tiles, 1 LOWER mt x mt, 2 LAUUM mt x mt with K = mt*128) on device
 * buffers; returns ms per launch and TFLOP/s on the flops launched. */
int gogp_bench_gemm(int device, int mode, int mt, int nt, int64_t K, int reps,
                    double *ms_per_launch, double *tflops);

/* Benchmark hook for sparse_syrk_kernel (sparse.hip): `reps` launches on device buffers, Vt rows x Mp with Mp = M rounded up to
 * 256; returns ms per launch and TFLOP/s on the flops of the lower 64-tiles. */
int gogp_bench_sparse_syrk(int device, int64_t rows, int64_t M, int reps, double *ms_per_launch, double *tflops);

/* Benchmark hook for launch_sparse_xty (sparse.hip; the kernel and its ordered final sum): `reps` launches on device buffers,
 * Vt rows x Mp with Mp = M rounded up to 256, Y rows x T; returns ms per launch and TFLOP/s on 2 rows M T flops. */
int gogp_bench_sparse_xty(int device, int64_t rows, int64_t M, int64_t T, int reps, double *ms_per_launch, double *tflops);

/* Diagnostic hook for the diagonal-block kernel: factor + invert one 256x256 SPD
 * block given on the host (row-major, lower triangle used); returns the factor,
 * its dense inverse, 24 in-kernel s_memtime stamps of a diagnostic build and the
 * HIP-event time (us) of the product build. */
int gogp_test_diag256(int device, const double *A, double *Lout, double *Dinv,
                      unsigned long long *stamps, double *elapsed_us);

/* Cycles per instruction (s_memtime) of one wave alone on its SIMD, the operations of the pivot chain (pivot16.h):
 * out8[0..7] = dependent v_fma_f64, independent v_fma_f64, dependent v_mov_b64_dpp row_newbcast, independent v_mov_b64_dpp,
 * dependent v_rsq_f64, independent v_rsq_f64, dependent v_mul_f64, one dependent (dpp, fma) pair. */
int gogp_test_valu_cost(int device, double *out8);

/* Diagnostic hook for one 128-column step of the Cholesky chain (panel128.hip): a (128 + rows_below) x 128 panel given on
 * the host (row-major, ld 128, lower triangle of the diagonal block used; rows_below a multiple of 64); returns the factor
 * of the diagonal block with the solved rows under it (same layout), 72 in-kernel s_memtime stamps of a diagnostic build
 * and the HIP-event time (us per launch over `reps` launches) of the product build. */
int gogp_test_panel128(int device, const double *A, double *Lout, int64_t rows_below, int reps,
                       unsigned long long *stamps, double *elapsed_us);

/* The product build of that step with the number of 64-row slabs per workgroup forced (0: by size): the factor and the
 * solved rows (same layout) and the HIP-event time per launch.  The result must not depend on `slabs`. */
int gogp_test_panel128_slabs(int device, const double *A, double *Lout, int64_t rows_below, int slabs, int reps,
                             double *elapsed_us);

/* Per-rank replay of a sharded evaluation (tools/sharded_replay.py): makes handle `h` (a
 * gogp_handle of the product library) rank `rank` of a prow x pcol grid ALONE on its GPU -- nothing is sent, a receive
 * zero-fills its buffer, an all-reduce is the identity.  Every launch of that rank's share of the sweep runs with its
 * real shape, so the wall time of Observe + Gradient is the rank's compute time; the values returned mean nothing. */
int gogp_test_dist_init_replay(void *h, int rank, int nranks, int prow, int pcol);

/* The kernels of the Laplace approximation in isolation (laplace.hip; tests/test_laplace_kernels.py), under the rules
 * of the finishing hooks above: arguments are checked before the device is touched (GOGP_EARG), every array goes up
 * whole and every in / out array comes back whole.  npad: a multiple of 256, 1 <= n <= npad; vectors written by a
 * kernel hold npad doubles and are zero from row n on.  lik: enum gogp_lik_kind.
 * lap_site: g, W, sw, b = W f + g, rho of (f, y); part: 5 rows of npad / 256 block results; out[0 .. 4] = sum log p,
 * sum a f, max |a - g|, max |a|, the first row whose y is refused or -1.  lap_scale_gram: A := diag(sw) A diag(sw) + I on
 * i, j < n of the lower 64-tiles, the block columns below wcols and the remaining triangle in two launches.  lap_step:
 * rhs = sw o beta and a1 = b - sw o beta.  lap_interp: at = a + t (a1 - a), ft = f + t (f1 - f).  lap_weight_vectors:
 * sv_i = 1/2 (1 - Binv_ii) rho_i.  lap_symv_u: u = sv - sw o (Binv v) from the elements j <= i < n of Binv (v zero from
 * row n on; upart: npad / 64 * npad doubles).  lap_weight: in place, G = diag(sw) G diag(sw) - u a^T - a u^T on j <= i < n,
 * exact zeros on the rest of the lower 64-tiles.  lap_colscale: KsT (rows x ld) := KsT diag(sw) on npad columns.
 * lap_mean: the response-scale prediction from the latent mu and sigma. */
int gogp_test_lap_site(int device, int lik, const double *f, int64_t f_len, const double *y, int64_t y_len, const double *a,
                       int64_t a_len, int64_t n, int64_t npad, double *g, int64_t g_len, double *W, int64_t w_len, double *sw,
                       int64_t sw_len, double *b, int64_t b_len, double *rho, int64_t rho_len, double *part, int64_t part_len,
                       double *out, int64_t out_len);
int gogp_test_lap_scale_gram(int device, double *A, int64_t a_len, int64_t ld, int64_t n, int64_t npad, const double *sw,
                             int64_t sw_len, int64_t wcols);
int gogp_test_lap_step(int device, const double *b, int64_t b_len, const double *sw, int64_t sw_len, const double *beta,
                       int64_t beta_len, int64_t n, int64_t npad, double *rhs, int64_t rhs_len, double *a1, int64_t a1_len);
int gogp_test_lap_interp(int device, const double *a, int64_t a_len, const double *a1, int64_t a1_len, const double *f,
                         int64_t f_len, const double *f1, int64_t f1_len, double t, int64_t n, int64_t npad, double *at,
                         int64_t at_len, double *ft, int64_t ft_len);
int gogp_test_lap_weight_vectors(int device, const double *Binv, int64_t binv_len, int64_t ld, const double *rho,
                                 int64_t rho_len, int64_t n, int64_t npad, double *sv, int64_t sv_len);
int gogp_test_lap_symv_u(int device, const double *Binv, int64_t binv_len, int64_t ld, int64_t n, int64_t npad, const double *v,
                         int64_t v_len, const double *sv, int64_t sv_len, const double *sw, int64_t sw_len, double *upart,
                         int64_t upart_len, double *u, int64_t u_len);
int gogp_test_lap_weight(int device, double *G, int64_t g_len, int64_t ld, int64_t n, int64_t npad, const double *sw,
                         int64_t sw_len, const double *u, int64_t u_len, const double *a, int64_t a_len);
int gogp_test_lap_colscale(int device, double *KsT, int64_t k_len, int64_t ld, int64_t rows, int64_t npad, const double *sw,
                           int64_t sw_len);
int gogp_test_lap_mean(int device, int lik, const double *mu, int64_t mu_len, const double *sigma, int64_t sigma_len, int64_t m,
                       double *mean, int64_t mean_len);

/* The kernels of the per-observation noise variances in isolation (noisevar.hip; tests/test_noise_variances_kernels.py),
 * under the same rules.  nv_diag_add: A_ii += v_i for i < n in two launches, the rows below wcols and the rest; nothing
 * else of A (in / out; npad rows of ld) is read or written.  nv_gradient: dv_i = 1/2 (alpha_i^2 - Kinv_ii) for i < n, one
 * fused multiply-add per row; only the diagonal of Kinv is read.  (The append fold: gogp_test_nv_append_commit above.) */
int gogp_test_nv_diag_add(int device, double *A, int64_t a_len, int64_t ld, int64_t n, int64_t npad, const double *v,
                          int64_t v_len, int64_t wcols);
int gogp_test_nv_gradient(int device, const double *Kinv, int64_t kinv_len, int64_t ld, const double *alpha,
                          int64_t alpha_len, int64_t n, int64_t npad, double *dv, int64_t dv_len);

/* The kernels of the sharded path -- dist2d.hip and the "helpers of the sharded evaluation" of solve.hip -- and the rest of
 * solve.hip (the LML scalars, the fp64 trace, the layout kernels around the factor, the one-line vector kernels) in
 * isolation, through their product launchers (tests/test_shard_kernels.py), under the rules of the hooks above: arguments
 * are checked before the device is touched (GOGP_EARG), every array goes up whole and every in / out array comes back
 * whole.  `void *` arrays hold doubles (precision 64) or floats (32); lengths count elements.  The preconditions of the
 * launchers stand in csrc/common.h; the hooks refuse what breaks them.
 * Block map: this rank sits at (pr, pc) of a Pr x Pc grid (1 .. 8 each) with tiles of nb = 2^nb_shift (5 .. 10); local tile
 * counts must satisfy mloc Pr = nloc Pc, as the product pads.  Chunk buffers: nloc chunks of (mloc nb) x nb.
 * Batched launchers (lml_scalars, alpha_from_y_batched, zero_upper_blocks, ydiag, zero_block): k candidates `bstride`
 * ELEMENTS apart (even; precision 64 only when k > 1), set in tl_batch around the launch and restored to {1, 0}.
 * scatter_tile: dst is the band of the rows from r0 on (the launcher gets dst - r0 n).  gather_rows_of_l: rows NULL and
 * rows_len 0 with diag_only 1.  residual_block: recv NULL with nrecv 0.  convert_block: src has `precision`, dst
 * `precision2` (not both 32).  chunk_tdot: part holds gogp_test_chunk_tdot_scratch(rows, nb) doubles (-1: bad arguments).
 * lml_scalars, sigma: alpha / q may be NULL (length 0).  sumsq_info: info NULL or one int64.
 * vector_op: 0 fill (a := f), 1 axpy, 2 add_vec (a += b), 3 scale (a *= f), 4 residual_from (a := b - a), 5 add_inplace
 * (a += b; precision 32 allowed), 6 info_to_double (a[0] := (double) the int64 in b[0]; count 1); fill and scale take
 * b NULL with length 0. */
int64_t gogp_test_chunk_tdot_scratch(int64_t rows, int nb);
int gogp_test_gather_rows(int device, const double *y, int64_t y_len, int64_t rows, int nb_shift, int Pr, int Pc, int pr, int
    pc, double *yloc, int64_t yloc_len);
int gogp_test_gather_x(int device, const double *X, int64_t x_len, const double *a, int64_t a_len, int D, int64_t n, int64_t
    rows, int nb_shift, int Pr, int Pc, int pr, int pc, double *Xloc, int64_t xloc_len, double *aloc, int64_t aloc_len);
int gogp_test_scatter_tile(int device, int precision, const void *src, int64_t src_len, int nb, int64_t n, int64_t row0,
    int64_t col0, int diag, int64_t r0, double *dst, int64_t dst_len);
int gogp_test_gather_rows_of_l(int device, int precision, const void *Lch, int64_t lch_len, int mloc, int nloc, int nb_shift,
    int Pr, int Pc, int pr, int pc, const int64_t *rows, int64_t rows_len, int64_t n, int diag_only, double *out, int64_t
    out_len);
int gogp_test_scatter_stage(int device, int precision, const double *stage, int64_t stage_len, int64_t lds, void *Lch, int64_t
    lch_len, int nloc, int mloc, int bi, int nb);
int gogp_test_transpose_rect(int device, int precision, const void *src, int64_t src_len, int64_t lds, void *dst, int64_t
    dst_len, int64_t ldd, int64_t rows, int cols);
int gogp_test_transpose_sq(int device, int precision, const void *src, int64_t src_len, int64_t lds, void *dst, int64_t
    dst_len, int64_t ldd, int n);
int gogp_test_copy_block(int device, double *dst, int64_t dst_len, const double *src, int64_t src_len, int64_t ld, int nb,
    int64_t rows);
int gogp_test_residual_block(int device, int precision, void *W, int64_t w_len, const void *Ks, int64_t ks_len, const double
    *U, int64_t u_len, int64_t ld, const double *recv, int64_t recv_len, int nrecv, int nb, int64_t rows);
int gogp_test_pack_blocks(int device, double *dst, int64_t dst_len, const double *src, int64_t src_len, int nblk, int64_t blk,
    int first, int stride);
int gogp_test_convert_block(int device, int precision, int precision2, const void *src, int64_t src_len, int64_t lds, void
    *dst, int64_t dst_len, int64_t ldd, int rows, int cols);
int gogp_test_chunk_tdot(int device, int precision, const void *chunk, int64_t chunk_len, int64_t rows, int nb, const double
    *v, int64_t v_len, double *part, int64_t part_len, double *out, int64_t out_len);
int gogp_test_chunk_alpha(int device, int precision, const void *Ych, int64_t ych_len, int mloc, int nloc, int nb_shift, int
    Pr, int Pc, int pr, int pc, const double *z, int64_t z_len, double *out, int64_t out_len);
int gogp_test_chunk_sumsq(int device, int precision, const void *Ych, int64_t ych_len, int mloc, int nloc, int nb_shift, int
    Pr, int Pc, int pr, int pc, int64_t n, double *part, int64_t part_len, double *out, int64_t out_len);
int gogp_test_lml_scalars(int device, int precision, const void *L, int64_t l_len, int64_t ld, const double *z, int64_t z_len,
    const double *y, int64_t y_len, const double *alpha, int64_t alpha_len, int64_t n, int k, int64_t bstride, double
    *scalars, int64_t scalars_len);
int gogp_test_alpha_from_y_batched(int device, const double *Y, int64_t y_len, int64_t ld, const double *z, int64_t z_len,
    int64_t npad, int k, int64_t bstride, double *alpha, int64_t alpha_len);
int gogp_test_trace_from_y(int device, const float *Y, int64_t y_len, int64_t ld, int64_t n, int64_t npad, const double
    *alpha, int64_t alpha_len, double *part, int64_t part_len, double *out, int64_t out_len);
int gogp_test_zero_upper_blocks(int device, int precision, void *R, int64_t r_len, int64_t ld, int64_t npad, int k, int64_t
    bstride);
int gogp_test_ydiag(int device, int precision, const void *Dinv, int64_t dinv_len, void *Y, int64_t y_len, int64_t ld, int k,
    int64_t bstride);
int gogp_test_zero_block(int device, int precision, void *B, int64_t b_len, int64_t ld, int64_t rows, int64_t cols, int k,
    int64_t bstride);
int gogp_test_extract_lower(int device, int precision, const void *L, int64_t l_len, int64_t ld, int64_t n, double *out,
    int64_t out_len);
int gogp_test_pack_lower(int device, int precision, const double *src, int64_t src_len, int64_t n, int64_t npad, void *L,
    int64_t l_len, int64_t ld);
int gogp_test_sigma(int device, const double *prior, int64_t prior_len, const double *q, int64_t q_len, int64_t m, double
    *sigma, int64_t sigma_len);
int gogp_test_logdet_block(int device, const double *L, int64_t l_len, int64_t ld, int64_t row0, int64_t n, int nb, double
    *acc, int64_t acc_len);
int gogp_test_dot(int device, const double *a, int64_t a_len, const double *b, int64_t b_len, int64_t n, double *out, int64_t
    out_len);
int gogp_test_sumsq_info(int device, const double *z, int64_t z_len, int64_t n, const int64_t *info, int64_t info_len, double
    *out, int64_t out_len);
int gogp_test_vector_op(int device, int op, int precision, void *a, int64_t a_len, const void *b, int64_t b_len, int64_t
    count, double f);

/* ---- the kernels of gram.hip and the forecast-derivative kernels of pgrad.hip through their product launchers
 * (tests/test_gram_kernels.py).  The rules of the hooks above.  Refused with GOGP_EARG besides short arrays: npad, mpad,
 * mrows, ncols that are not positive multiples of 64 (whole 64 x 64 tiles are written: the output holds all of their
 * rows, ld covers the padded width); X shorter than npad * ndim + GOGP_MAX_NDIM doubles (with one radial term the kernels
 * read rows n .. npad - 1 of X unguarded; the slack is gogp_test_grad_reduce's convention); wcols that is not a multiple of
 * 64 or below 64; radial1 without exactly one radial (non-periodic) term -- radial1 = 0 on such a kernel is legal and
 * selects the generic instance; ev with an ARD term.  Z, v, alpha and Wt are read on their first m / n rows only. */

/* launch_gram_lower_split (both launches on stream 0): K (in / out; npad rows of ld; float with precision 32) = the lower
 * 64-tiles of the Gram matrix, identity on the padding.  k candidates (fp64 only beyond 1): kparams holds k structs, X is
 * shared, candidate c's matrix AND parameters lie c * bstride elements (of 8 bytes) on. */
int gogp_test_gram_split(int device, int precision, const gogp_test_kparams *kparams, int ev, const double *X, int64_t x_len,
                         int64_t n, int64_t npad, int64_t wcols, int k, int64_t bstride, void *K, int64_t k_len, int64_t ld);

/* launch_gram_local: the mrows x ncols local tiles (K: in / out, ld >= ncols) of rank (pr, pc) of a Pr x Pc grid with
 * distribution blocks of 2^nb_shift; the last local row and column must be global ones below npad. */
int gogp_test_gram_local(int device, int precision, const gogp_test_kparams *kparams, int ev, const double *X, int64_t x_len,
                         int64_t n, int64_t npad, int64_t mrows, int64_t ncols, int nb_shift, int pr, int Pr, int pc, int Pc,
                         void *K, int64_t k_len, int64_t ld);

/* launch_cross: KsT (in / out; mpad rows of ld >= npad) [j][i] = k(x_i, z_j), zero for i >= n or j >= m.  Z: mpad rows. */
int gogp_test_cross(int device, int precision, const gogp_test_kparams *kparams, int ev, const double *X, int64_t x_len,
                    int64_t n, int64_t npad, const double *Z, int64_t z_len, int64_t m, int64_t mpad, void *KsT, int64_t k_len,
                    int64_t ld);

/* launch_prior: prior (in / out) [j] = k(z_j, z_j), j < m. */
int gogp_test_prior(int device, const gogp_test_kparams *kparams, const double *Z, int64_t z_len, int64_t m, double *prior,
                    int64_t prior_len);

/* y given: launch_residual, out = y - K v (nparts must be 1); y NULL (length 0): launch_kmatvec_share(part_idx, nparts),
 * out = the share's columns of K v.  Rows >= n of out are zero.  part (in / out): nslab x npad; out (in / out): npad. */
int gogp_test_kmatvec(int device, const gogp_test_kparams *kparams, int radial1, int ev, const double *X, int64_t x_len,
                      int64_t n, int64_t npad, const double *v, int64_t v_len, const double *y, int64_t y_len, int part_idx,
                      int nparts, int nslab, double *part, int64_t part_len, double *out, int64_t out_len);

/* pgrad_slabs itself: the slabs launch_pgrad splits npad rows into for m test points, and the 64-row tiles per slab.
 * -1: bad arguments.  No device. */
int gogp_test_pgrad_slabs(int64_t npad, int64_t m, int *tiles_per_slab);

/* launch_pgrad: dmu, dsigma (in / out; m x ndim) and part (in / out; 2 x gogp_test_pgrad_slabs x m x ndim).  Wt: m rows of
 * ld >= npad; alpha: npad; sigma: m. */
int gogp_test_pgrad(int device, const gogp_test_kparams *kparams, int ev, const double *X, int64_t x_len, int64_t n,
                    int64_t npad, const double *Z, int64_t z_len, int64_t m, const double *alpha, int64_t alpha_len,
                    const double *Wt, int64_t wt_len, int64_t ld, const double *sigma, int64_t sigma_len, double *part,
                    int64_t part_len, double *dmu, int64_t dmu_len, double *dsigma, int64_t dsigma_len);

/* ---- the kernels of cg.hip (the iterative exact GP; tests/test_cg_kernels.py), through their product launchers
 * (common.h states what each reads and writes).  A block of T <= 64 vectors: T rows of ld >= n doubles, (T - 1) * ld + n
 * elements at least.  The per-column state: sc, 6 rows of 64 doubles (rho, a, beta, |b|^2, |r|^2, p^T q); st, 4 rows of 64
 * 32-bit integers (frozen, iterations, bad, status).  Every argument is refused before the device is touched. */
/* kmm_slabs / cg_dot_blocks themselves; -1: bad arguments.  No device. */
int gogp_test_kmm_slabs(int64_t rows, int64_t cols);
int gogp_test_cg_dot_blocks(int64_t n);
/* launch_kmm: Out (in / out; T rows of ldo >= rows) [t][i] = sum_j k(a_i, b_j) V[t][j] (+ diag[i] V[t][i]), zero for
 * rows <= i < ldo; part (in / out): nslab x T x rpad, rpad = rows rounded up to 64.  B NULL (length 0): the square
 * product on the rows of A, the only form that takes diag (rows entries; NULL with length 0: none).  1 <= nslab <= 64;
 * max_blocks 0: no cap on the grid. */
int gogp_test_kmm(int device, const gogp_test_kparams *kparams, const double *A, int64_t a_len, int64_t rows,
                  const double *B, int64_t b_len, int64_t cols, const double *V, int64_t v_len, int64_t ldv, int T,
                  const double *diag, int64_t diag_len, int nslab, int max_blocks, double *part, int64_t part_len,
                  double *Out, int64_t out_len, int64_t ldo);
/* launch_cg_dots: the T dot products A[t] . B[t] and, by mode (0 plain, 1 |b|^2, 2 rho0, 3 p^T q, 4 |r|^2 and the freeze
 * test, 5 beta), the update of sc / st (in / out).  part (in / out): T x gogp_test_cg_dot_blocks(n); out (in / out, T;
 * NULL with length 0 except in mode 0) receives the dot products. */
int gogp_test_cg_dots(int device, const double *A, int64_t a_len, const double *B, int64_t b_len, int64_t ld, int64_t n,
                      int T, int mode, int it, double tol, double *part, int64_t part_len, double *out, int64_t out_len,
                      double *sc, int64_t sc_len, int32_t *st, int64_t st_len);
/* launch_cg_update_xr: x += a p, r -= a q (x, r in / out); launch_cg_update_p: p = z + beta p (p in / out); a frozen
 * column keeps its bits. */
int gogp_test_cg_update_xr(int device, double *x, int64_t x_len, double *r, int64_t r_len, const double *p, int64_t p_len,
                           const double *q, int64_t q_len, int64_t ld, int64_t n, int T, const double *sc, int64_t sc_len,
                           const int32_t *st, int64_t st_len);
int gogp_test_cg_update_p(int device, double *p, int64_t p_len, const double *z, int64_t z_len, int64_t ld, int64_t n, int T,
                          const double *sc, int64_t sc_len, const int32_t *st, int64_t st_len);
/* launch_cg_scale: out (in / out) = in o w - sub; w (n entries) and sub (a block) may be NULL with length 0. */
int gogp_test_cg_scale(int device, const double *in, int64_t in_len, const double *w, int64_t w_len, const double *sub,
                       int64_t sub_len, int64_t ld, int64_t n, int T, double *out, int64_t out_len);
/* launch_cg_status: st (in / out) row 3: [0] = columns t < T not frozen, [1] = first bad column + 1 or 0. */
int gogp_test_cg_status(int device, int T, int32_t *st, int64_t st_len);
/* The preconditioner on a given scaled factor: Z (in / out) = D^-1/2 (R' - Ls Cinv Ls^T R'), R' = D^-1/2 R, through
 * launch_cg_lst, launch_cg_small_mm and launch_cg_precond.  Ls: r columns of ldn >= n doubles, column-major; dis: n;
 * Cinv: rp x rp, rp = r rounded up to 16; r == 0: Jacobi, Ls and Cinv NULL with length 0.  C (in / out, rp x rp; NULL
 * with length 0: not asked for) receives launch_cg_capacitance's I + Ls^T Ls. */
int gogp_test_cg_precond(int device, const double *Ls, int64_t ls_len, int64_t ldn, int64_t n, int r, const double *dis,
                         int64_t dis_len, const double *Cinv, int64_t cinv_len, const double *R, int64_t r_len, int64_t ld,
                         int T, double *Z, int64_t z_len, double *C, int64_t c_len);
/* The kernels of gogp_cg_lml_gradient (tests/test_cg_grad_kernel.py, test_cg_lml_cpu.py).
 * launch_cg_grad: out (in / out; GOGP_TEST_NACC slot sums; `accumulate`: added to what it holds) [slot] = sum over i, j < n
 * of (scale sum_{s < S} A[s][i] B[s][j]) theta_p dk(x_i, x_j)/dtheta_p, the trace slot taking the weights of i == j.  A, B:
 * S >= 1 rows of ld >= n doubles ((S - 1) * ld + n elements at least), rows in passes of 64; X: n x ndim. */
int gogp_test_cg_grad(int device, const gogp_test_kparams *kparams, const double *X, int64_t x_len, int64_t n,
                      const double *A, int64_t a_len, const double *B, int64_t b_len, int64_t ld, int S, double scale,
                      int accumulate, double *out /* GOGP_TEST_NACC */);
/* launch_cg_probes: Z (in / out; T <= 64 rows of ld >= n) [t][i] = sqrt(d_i) (sum_{k < r} Ls[i][k] Xi[t][n + k] + Xi[t][i]).
 * Ls: r columns of ldn >= n doubles, column-major (r == 0: NULL with length 0); d: n; Xi: T rows of ldxi >= n + r. */
int gogp_test_cg_probes(int device, const double *Ls, int64_t ls_len, int64_t ldn, int64_t n, int r, const double *d,
                        int64_t d_len, const double *Xi, int64_t xi_len, int64_t ldxi, int64_t ld, int T, double *Z,
                        int64_t z_len);
/* The host's quadrature: *out = rho0 e_1^T log(T) e_1 of the m x m Lanczos tridiagonal of the coefficients a[0 .. m),
 * beta[0 .. m) (beta[m - 1] is not used); m == 0: 0.  No device. */
int gogp_test_cg_quadrature(const double *a, const double *beta, int64_t m, double rho0, double *out);

/* ---- the kernel of vecchia.hip (Vecchia's approximation; tests/test_vecchia_kernel.py), through its product launchers.
 * The table nbr (`targets` rows of m int32; NULL with length 0 when m == 0) must pass gogp_vecchia_check -- causal for
 * observe (targets == n), indices in [0, n) for produce -- and every length is checked before the device is touched.
 * Observe (produce == 0, Z NULL with length 0): terms (in / out; n x 3: mu, s, log p; NULL with length 0: not asked for),
 * value[0] = sum log p, info[0] = the lowest target with a bad pivot + 1 or 0, vpart (in / out) the workgroups' values;
 * grad != 0 also fills partials (in / out; gogp_test_vecchia_blocks(n) rows of GOGP_TEST_NACC slot sums).  Produce: terms is
 * targets x 2 (mu, sigma), partials and vpart NULL with length 0.  X: n x ndim, y: n, v: n or NULL with length 0.
 * max_blocks > 0 caps the grid (a wave then walks several targets at a small size); gogp_test_vecchia_blocks: the rows
 * of partials and vpart (-1: bad arguments; no device). */
int gogp_test_vecchia_blocks(int64_t targets, int max_blocks);
int gogp_test_vecchia(int device, const gogp_test_kparams *kparams, int produce, int grad, const double *X, int64_t x_len,
                      const double *y, int64_t y_len, const double *v, int64_t v_len, int64_t n, const double *Z,
                      int64_t z_len, int64_t targets, const int32_t *nbr, int64_t nbr_len, int m, double *terms,
                      int64_t terms_len, double *partials, int64_t partials_len, double *vpart, int64_t vpart_len,
                      double *value /* 1 */, int64_t *info /* 1 */, int max_blocks);

/* ---- the search of vecchia_knn.hip (tests/test_vecchia_knn_kernel.py), through its product launchers on caller-supplied
 * rows.  X: n x ndim (x_len >= n ndim; what lies behind row n - 1 travels to the device too).  Z NULL with length 0: the
 * causal table of X (targets == n); else `targets` rows of Z against all of X.  lengths: ndim values > 0 or NULL.
 * 0 <= m <= 63, n and targets in 1 .. 2^20, 0 <= slabs <= 256 (> 0 forces the candidate split), tile_cap >= 0 (> 0 caps
 * the grid).  In / out: nbr (nbr_len >= targets m) the table, d2 (same length) the squared distance of every entry taken
 * (0.0 under the padding), xs (xs_len >= n ndim) the scaled copy of X; with m == 0 nbr and d2 may be NULL with length 0.
 * Every length is checked before the device is touched.
 * gogp_test_vecchia_knn_plan: out = {targets of a tile, slabs, bytes of workspace} of a search of `targets` targets over n
 * candidates: tile t holds the targets [t tile, min(targets, (t + 1) tile)), slab s the candidates [s L, min(n, (s + 1) L))
 * with L = ceil(n / slabs); the workspace stays under 768 * 64 * 12 * m bytes.  No device. */
int gogp_test_vecchia_knn(int device, const double *X, int64_t x_len, int64_t n, int ndim, const double *Z, int64_t z_len,
                          int64_t targets, const double *lengths, int m, int slabs, int tile_cap, int32_t *nbr,
                          int64_t nbr_len, double *d2, int64_t d2_len, double *xs, int64_t xs_len);
int gogp_test_vecchia_knn_plan(int64_t targets, int64_t n, int m, int64_t out[3]);

#ifdef __cplusplus
}
#endif
#endif /* GOGP_TESTHOOKS_H */
