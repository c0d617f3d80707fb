// handle.h -- the handle behind the C ABI, shared by api.hip (single-GPU orchestration), cg_api.hip and vecchia_api.hip
// (two call families of their own) and dist2d.hip (2-D block-cyclic sharded evaluation).  Private to libgogp_hip.so.
#pragma once
#include <algorithm>
#include <array>
#include <string>
#include <vector>

#include "common.h"

namespace gogp {
struct Dist2D;  // dist2d.hip
}
using gogp::DevParams;
using gogp::GemmProfile;

constexpr int REFINE_SLABS = 8;  // column slabs of the residual kernel (gram.hip: launch_residual)

// One evaluation's row of pinned staging (hscal; a candidate's row of cand_hscal; a batch pair's row of common.h: BATCH_ROW
// doubles): the factorisation's scalars in [0 .. 7] (api.hip: judge_scalars), then these
constexpr int HS_INFO = 8;    // first failing pivot + 1 (a long long; 0: positive definite)
constexpr int HS_TRACE = 9;   // fp32 K^-1: tr(alpha alpha^T - K^-1) summed in fp64 from Y (NaN: not computed)
constexpr int HS_TMO = 10;    // the two time-out words (unsigned) of the persistent substitution kernel's launches (trsm_small.hip)
constexpr int HS_PIVOT = 12;  // gogp_produce_samples: first failing pivot + 1 of the test points' covariance (HS_INFO keeps K's)
constexpr int HS_GRAD = 16;   // the gradient's NACC slot sums
static_assert(HS_INFO < HS_TMO && HS_TMO < HS_PIVOT && HS_PIVOT < HS_GRAD, "the staging words lie below the gradient's sums");
static_assert(HS_GRAD + gogp::NACC == gogp::BATCH_ROW, "the pinned row is a batch row");

// The device buffers of one evaluation: the handle's own, or an arena slot of a candidates call (api.hip: cand_layout)
struct EvalBufs {
  DevParams *devP = nullptr;
  long long *info = nullptr;
  double *scalars = nullptr;  // 8 doubles
  double *gout = nullptr;
  double *bufA = nullptr, *bufL = nullptr, *bufY = nullptr, *Dinv = nullptr;
  double *z = nullptr, *w = nullptr, *alpha = nullptr;
  double *gpart = nullptr;
};

// The buffers sized by the number of observations that gogp_set_data allocates and gogp_append replaces as one set
// (bufY and the fp32 path's scratch have capacities of their own).  nbufs_alloc holds their sizes.
struct NBufs {
  double *dX = nullptr, *dy = nullptr, *bufA = nullptr, *bufL = nullptr, *Dinv = nullptr;
  double *z = nullptr, *w = nullptr, *alpha = nullptr, *gpart = nullptr;
};

// Device bytes grown on demand and never shrunk: the scratch of one family of calls, whose contents no call expects to
// find again.  Not a general allocator: buffers tied to a validity flag or a typed capacity keep their own code.
struct gogp_handle;
struct Workspace {
  void *p = nullptr;
  size_t bytes = 0;  // capacity
  // at least `need` bytes; on failure the old block is gone, the capacity is 0 and h->err says why (GOGP_ENOMEM / GOGP_EHIP)
  inline int reserve(gogp_handle *h, size_t need);
  void release() {
    (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <class T>
  T *as() const { return static_cast<T *>(p); }
};

// The state of the iterative calls (cg_api.hip: gogp_cg_*): a data set and a copy of the parameters of its own, resident, so
// that devP keeps what the last evaluation uploaded.  (common.h's CgState is a lock-step block's per-column state.)
struct CgHandleState {
  double *X = nullptr, *y = nullptr, *v = nullptr;  // N x D (+ slack, npad rows), npad, npad (nullptr: no variances)
  double *d = nullptr, *dis = nullptr, *alpha = nullptr;  // D, D^-1/2, alpha: npad doubles each
  DevParams *P = nullptr;
  int64_t N = 0, npad = 0;
  bool have = false, solved = false;
  int rank = 0, rp = 0;         // columns of the factor in use and their count rounded up to 16
  int64_t ldn = 0;
  int check = 8;                // option "cg_check": iterations between two looks at the status word
  int products = 0, blocks = 0;  // counters of the call in progress (gogp_cg_last_info)
  double yta = 0.0;
  double vmin = 0.0;            // the smallest noise variance given (0 without variances)
  Workspace L;                  // Ls = D^-1/2 L, column-major, `rank` columns of ldn doubles
  Workspace small;              // C^-1 (rp x rp), W and Y (CG_MAX_T x rp each), the per-column state
  Workspace vec;                // a block's six vectors, the dots' partials and results
  Workspace part;               // the slab partials of the product and of the skinny transposed product
  Workspace ks;                 // gogp_cg_produce: 64 rows of k*, the test points, prior, q, mu
  double logdet_c = 0.0;        // log |C| of the last solve's capacitance matrix (0 at rank 0)
  double dnoise = 0.0;          // d noise_var / d log(noise parameter) at the last solve's theta
  Workspace lml;                // gogp_cg_lml_gradient: a block's rows of Xi, the a / beta history, rho0, slot sums and partials
  void release() {  // the option stays, and so do the last solve's counters and scalars (gogp_cg_last_info reports them)
    for (double *q : {X, y, v, d, dis, alpha}) (void)hipFree(q);
    (void)hipFree(P);
    X = y = v = d = dis = alpha = nullptr;
    P = nullptr;
    for (Workspace *w : {&L, &small, &vec, &part, &ks, &lml}) w->release();
    N = npad = 0;
    have = solved = false;
    rank = rp = 0;
  }
};

// The state of the Vecchia calls (vecchia_api.hip: gogp_vecchia_*).  Device memory: X, y and v (N (D + 2) doubles), 4 N m
// bytes of table, the terms (3 N doubles, from the first observe that asks for them) and at most VECCHIA_BLOCKS_MAX partial
// rows with the workgroups' values and failure words.
struct VecchiaState {
  double *X = nullptr, *y = nullptr, *v = nullptr;  // N x D, N, N (nullptr: no variances)
  int *nbr = nullptr;                               // N x m, row-major
  DevParams *P = nullptr;                           // the parameters of the last observe
  int64_t N = 0;
  int m = 0;
  bool have = false, observed = false;
  double dnoise = 0.0;  // d noise_var / d log(noise parameter) at the last observe's theta
  Workspace small;      // value, info word, NACC slot sums, the workgroups' values, failure words and partial rows
  Workspace terms;      // N x 3
  Workspace prod;       // gogp_vecchia_produce: Z, the table, mu, sigma, the failure words
  // the table's origin (gogp_vecchia_set_data_nearest, gogp_vecchia_reneighbour): built on the device from the resident X
  // under these length scales (scaled false: the unscaled distance); false for a caller's table
  bool built_here = false, scaled = false;
  double lengths[GOGP_MAX_NDIM] = {};
  Workspace knn;        // a search's scratch: the lengths, the scaled copies of X and Z, the partial lists (vknn_plan)
  void release() {  // leaves the state of a new handle
    for (double *q : {X, y, v}) (void)hipFree(q);
    (void)hipFree(nbr);
    (void)hipFree(P);
    for (Workspace *w : {&small, &terms, &prod, &knn}) w->release();
    *this = VecchiaState();
  }
};

// What an evaluation leaves in the handle; a candidates call saves it and puts it back
struct EvalState {
  bool factored = false, have_alpha = false, have_kinv = false;
  bool observed = false, with_obs = false;
  bool grad_valid = false;
  bool trtri_done = false;  // Y = L^-T of the current factor is (being) computed
  double lml = 0.0;
  double logdet2 = 0.0;     // 2 sum_i log L_ii of the factor `lml` belongs to (fp64 handles; gogp_multi_lml)
  double cond_lb = 1.0;    // (max L_ii / min L_ii)^2 of the last factorisation
  int64_t notpd = -1;
};

// What a captured candidates graph was recorded for: its size and the raw pointers it holds.  No option is part of it:
// gogp_set_option and gogp_set_events drop the graph (api.hip: drop_cand_graph) before they change what is launched.
struct CandGraphKey {
  int k = 0;
  int64_t n = 0, cap_npad = 0;
  size_t stride = 0;
  const void *arena = nullptr, *dX = nullptr, *dy = nullptr, *hostP = nullptr, *hscal = nullptr;
  bool operator==(const CandGraphKey &o) const {
    return k == o.k && n == o.n && cap_npad == o.cap_npad && stride == o.stride && arena == o.arena && dX == o.dX &&
           dy == o.dy && hostP == o.hostP && hscal == o.hscal;
  }
};

struct gogp_handle : EvalBufs, EvalState {
  gogp_desc desc;
  int device = 0;
  int ns = 0, nn = 0, P = 0, D = 0;
  int ard_dims = 0;
  bool radial1 = false;  // the similarity kernel is one radial (non-periodic) term: restructured O(N^2) kernels
  // event discounts (gogp_set_events): nevents x {from, to, discount} on input dimension ev_axis; > 0 selects the
  // *_ev_kernel instances of every kernel that evaluates the similarity
  int nevents = 0, ev_axis = 0;
  double events[GOGP_MAX_EVENTS][3] = {};
  bool ev() const { return nevents > 0; }
  int64_t n = 0, npad = 0;
  int nblk = 0;  // 128-blocks
  // device buffers (and those of EvalBufs)
  double *dX = nullptr, *dy = nullptr;
  double *dscr = nullptr;     // fp32 path: fp64 scratch of the diagonal-block kernel (3 x 256 x 256)
  double *D64 = nullptr;      // fp32 path: the diagonal blocks accumulated in fp64 (diagsyrk.hip), npad / 256 blocks of 256 x 256
  int64_t cap_d64 = 0;        // ... allocated for this npad
  int diag_fp64 = 1;          // option "diag_fp64": 1 (default) the fp32 path's pivots come from that strip, 0 from the float matrix
  bool d64_active = false;    // set by the factorisation in progress
  int prec = 64;              // 64: fp64 throughout; 32: N x N matrices and O(N^3) products in fp32
  size_t esz() const { return prec == 32 ? sizeof(float) : sizeof(double); }
  int refine_steps = 1;       // fp32 path: iterative-refinement steps of alpha against the fp64 K
  double *rw = nullptr, *rz = nullptr, *rd = nullptr, *rpart = nullptr;  // its scratch
  DevParams *hostP = nullptr;  // pinned
  double *hscal = nullptr;     // pinned staging, one row (HS_*)
  int64_t cap_npad = 0;        // allocation size of the N-dependent buffers
  int64_t cap_y = 0;           // npad bufY was allocated for (it is allocated lazily)
  // produce workspace
  double *dZ = nullptr, *KsT = nullptr, *Vt = nullptr, *pvec = nullptr;
  int64_t cap_m = 0, cap_mp_npad = 0;
  // released with the M buffers (api.hip: free_m_buffers)
  Workspace pg_ws;             // gogp_produce_gradient: partial sums of pgrad_kernel + the two derivative arrays
  Workspace pc_ws;             // gogp_produce_covariance / gogp_produce_samples: the SYRK's partial tiles, the covariance,
                               // and for samples its factor, a block inverse, xi, the product and the pivot word (pcov.hip)
  int ncu = 0;                 // compute units of the device (0: not asked yet): the slab policy of pcov.hip
  hipStream_t s = nullptr;   // main stream: Gram, big trailing updates, reductions
  hipStream_t sp = nullptr;  // panel stream (high priority): diagonal blocks, TRSM-as-GEMM,
                             // skinny updates, substitution steps -- overlaps the big updates
  // candidate batching (gogp_observe_gradient_candidates): k arena slots, each with its own copy of
  // every per-candidate buffer at the same offset (common.h: Batch); the handle's own buffers are
  // not touched by a batched evaluation
  char *cand_arena = nullptr;
  size_t cand_stride = 0;       // bytes per slot
  int cand_cap_k = 0;
  int64_t cand_cap_npad = 0;
  DevParams *cand_hostP = nullptr;  // pinned, cand_host_k entries
  double *cand_hscal = nullptr;     // pinned, cand_host_k rows (HS_*)
  int cand_host_k = 0;
  int batch_k = 1;              // > 1 only while a batched evaluation is being enqueued
  bool batch_mode = false;      // a batched evaluation is being enqueued (also with k = 1)
  // option "graph": the launch sequence of a batched evaluation captured once into a hipGraph and
  // replayed (the parameters change in pinned host memory only)
  int use_graph = 1;            // 1: linear graph from stream capture (N <= 1024; the default), 2: explicitly built DAG (graphrec.h), 3: the same recorder as one chain in enqueue order (diagnostics), 0: none
  bool graph_failed = false;    // the runtime refused the explicit graph once: stream path from then on
  int graph_nodes = 0;          // nodes of the graph in use (diagnostics)
  std::string graph_note;
  hipGraphExec_t cand_graph = nullptr;
  hipStream_t sg = nullptr;     // capture / replay stream of that graph (created on first use)
  CandGraphKey cand_graph_key, cand_seen_key;  // what the graph was captured for / what the last call asked for
  // batches of small GPs (gogp_batch_*): the members' data (row ranges of one uploaded X / y) and the staging of one
  // call -- the pairs' BatchItems + test points in (pinned -> device: one copy), result rows + mu + sigma out
  double *bt_X = nullptr, *bt_y = nullptr;  // bt_cap_rows x D (+ GOGP_MAX_NDIM slack), bt_cap_rows
  int64_t bt_rows = 0, bt_cap_rows = 0;
  std::vector<int64_t> bt_off, bt_n;
  bool bt_have = false;
  char *bt_din = nullptr, *bt_hin = nullptr;
  size_t bt_in_cap = 0;
  double *bt_dout = nullptr, *bt_hout = nullptr;
  size_t bt_out_cap = 0;
  // sharded evaluation (gogp_dist_init_*): 2-D block-cyclic state, nullptr on a single GPU
  gogp::Dist2D *dist = nullptr;
  hipStream_t sl = nullptr;  // forward substitution steps (low priority, off the chain)
  hipStream_t s2 = nullptr;  // big updates of the triangular inverse (fused sweep)
  hipStream_t st = nullptr;  // its chain: column panels of Y = L^-T
  hipStream_t sk = nullptr;  // rank-k updates K^-1 (+)= Y_P Y_P^T behind the inverse (low priority)
  void *stream_set = nullptr;  // the pooled StreamSet the five streams belong to
  std::vector<hipEvent_t> evs;  // cross-stream ordering events (timing disabled)
  int lookahead = 1;
  int superpanel = 2;          // 256-wide panels per trailing update (K = 256*superpanel)
  int eager = 1;               // Observe also runs the triangular inverse (gradient
                               // preparation), interleaved with the Cholesky sweep
  int superpanel_head = -1;    // > 0: super-panel width while more than head_remaining panels are to come; -1: 3 (fp64) / 4 (fp32)
  int head_remaining = 16;     // (measured, N = 16384: 3 / 16 72.7 ms, 3 / 24 72.8, 4 / 32 74.2, off 73.0-73.4)
  int chain_prio = -1;         // tile-kernel launches on the two chains raise their waves' issue priority (-1: by size)
  int tiny = 1;                // N <= 128 observations: one launch for the whole factorisation (api.hip: tiny_factorize)
  int chain_slabs = 0;         // chain_split = 2: slabs of 64 panel rows per workgroup (panel128.hip); 0: by the launch's size
  int chain_split = -1;        // 0: the 256-block kernel + a panel solve; 2: panel128.hip (api.hip: chain_split_of; -1: by size)
  int ktri = 1;                // panel solves skip the zero half of the block inverse (common.h: GemmGrid)
  // T^-1 (lower, row-major) of the diagonal block of every super-panel of the factor: rows C0.. of an npad x tinv_ld
  // matrix, assembled by the first Produce on a factor (api.hip: assemble_tinv, produce_solve_t).  Produce then solves
  // a super-panel of columns with ONE product instead of a solve + update per 256 columns.
  double *TX = nullptr, *Tmt = nullptr;  // Tmt: 256 x 256 scratch blocks of the assembly
  int64_t tinv_ld = 0;
  size_t cap_tinv = 0;                   // elements allocated for TX
  // option "gradient_precision" = 32 on an fp64 handle: the factorisation, LML, alpha and Produce stay fp64; only what
  // the GRADIENT needs beyond them -- Y = L^-T and K^-1 = Y Y^T, 2/3 of an evaluation's flops -- runs on the fp32 tile
  // kernel (157 TFLOP/s) from a float copy of L, in float buffers of their own (api.hip: "mixed gradient")
  int grad_prec = 64;
  float *g32A = nullptr, *g32L = nullptr, *g32Y = nullptr, *g32D = nullptr;  // R / K^-1, copy of L, Y, copy of Dinv
  int64_t g32_cap = 0;
  int produce_panels = 4;                // 256-panels per super-panel of Produce's substitution
  int produce_small_below = 1024;        // Produce runs alone on the GPU: 64 x 64 tiles below this many 128-tiles (common.h: GemmGrid)
  int produce_tinv = 1;                  // option: 0 = Produce substitutes panel by panel (round 3)
  bool tinv_valid = false, tinv_pending = false;  // assembled for the current factor
  int64_t tinv_sig = 0;                  // super-panel layout it was assembled for
  // Produce for few test points (M <= produce_small_max, fp64, one GPU): ONE persistent launch that reads the factor
  // once (trsm_small.hip) instead of the tile-kernel chain; 0: off
  int produce_small_max = 64;
  Workspace small_ws;          // its workspace (solution / w blocks, counters, partial sums); released with the N buffers
  int produce_groups = 2;      // Produce: independent substitution chains (streams) over the test points' tile rows
  int krag = 1;                // the inverse's updates skip the zero triangle of a super-panel of Y (common.h: GemmGrid::krag0)
  int ard_mfma_min = 1;        // ARD kernels (one radial term) with at least this many dimensions reduce the
                               // gradient on the matrix cores (grad_mfma.hip); 65: never
  int kinv_split = 60;         // percent of the columns whose part of K^-1 = Y Y^T is launched DURING the sweep (api.hip; 0: off)
  int64_t kinv_c1 = 0;         // ... columns that launch covered in the current factorisation (0: none)
  int kinv_fused = -1;          // ... and accumulates K^-1 = sum_P Y_P Y_P^T behind it, one rank-k update
                               // per super-panel of Y (0: one LAUUM launch over the finished Y in Gradient; -1: by size)
  bool kinv_pending = false;   // K^-1 is being accumulated on sk (wait for EV_KINV)
  bool trtri_pending = false;  // Y = L^-T (trtri_done) is still running on st/s2 (wait for EV_TRTRI)
  bool ydone_valid = false;    // EV_YDONE was recorded by the factorisation trtri_pending refers to
  bool alpha_pending = false;   // alpha was enqueued on sp; consumers on s wait for ev_alpha
  // state (and that of EvalState)
  std::vector<double> theta_s, theta_n;
  bool have_data = false;
  bool have_theta = false;  // theta_s / theta_n were given by an Absorb, Observe or set_factor
  bool z_valid = false;     // z = L^-1 y of the current factor is in `z` (not after gogp_set_factor, which stores none)
  // released with the N buffers (api.hip: free_n_buffers)
  Workspace app_ws;         // gogp_append: the saved block inverse + the partial sums of its Gram kernel (append.hip)
  Workspace rm_ws;          // gogp_remove: index maps, a pass's columns of W, the diagonal-block snapshot, compacted X / y (remove.hip)
  Workspace loo_vec;        // gogp_loo / gogp_loo_gradient: mu, sigma, log p, v, s, u, a zero vector and the block sums (loo.hip)
  Workspace loo_mat;        // gogp_loo_gradient: B = K^-1 diag(s) and G = B B^T - u alpha^T - alpha u^T, npad x npad each
  Workspace bcv_vec;        // gogp_blockcv / gogp_blockcv_gradient: the vectors, the block and group tables, the pivots (blockcv.hip)
  Workspace bcv_s;          // ... and the groups' 128 x 128 S_g; the gradient's two matrices are loo_mat
  // T output columns on the handle's factorisation (gogp_multi_*, multi.hip); all released with the N buffers
  int multi_T = 0;             // outputs set (gogp_multi_set_outputs) for the current data; 0: none
  bool multi_solved = false;   // A = K^-1 Y of the current factor is in multi_vec: cleared with every new factor of the handle's own
                               // (not by a batched evaluation in the candidates arena: begin_evaluation) and restored by Append's rollback
  Workspace multi_vec;      // Y^T, then A^T: GOGP_MULTI_MAX_T rows of npad doubles each, zero from column n and from row T on
  Workspace multi_mean;     // gogp_multi_produce: Kstar^T A, mpad x GOGP_MULTI_MAX_T; gogp_multi_lml: the T dots
  Workspace multi_mat;      // gogp_multi_gradient: G = T K^-1 - A A^T and a zero vector, (npad + 1) x npad
  // explicit basis functions on the handle's factorisation (gogp_basis_*, basis.hip); all released with the N buffers
  int basis_p = 0;             // basis columns set (gogp_basis_set) for the current data; 0: none
  bool basis_solved = false;   // W, A's factor, beta and [Q | alpha~] of the current factor are in basis_vec: cleared and kept exactly where multi_solved is
  int basis_symm = -1;         // option "basis_symm": W from the explicit K^-1 (1), from the factor (0), -1: from K^-1 where it is there
  Workspace basis_vec;      // H^T, W^T, [Q | alpha~]^T and the p x p results (api.hip: BasisBufs)
  Workspace basis_part;     // the slabs' partial sums of basis_symm_kernel
  Workspace basis_mean;     // gogp_basis_produce: Kstar^T W (mpad x 128), H_z, mu
  double basis_logdet = 0.0, basis_gtb = 0.0;  // log|A| and g^T beta of the solved state
  std::vector<double> basis_beta, basis_cov;   // ... and beta (p) and A^-1 (p x p)
  // the inducing-point approximation (gogp_sparse_*, sparse.hip): a data set of its own and a private dense handle for
  // the process on the inducing points; nothing of the handle's own data, factor or workspaces is touched
  gogp_handle *sp_ind = nullptr;   // the inducing process: same similarity terms, constant noise sqrt(jitter), data U, y = 0
  double *sp_X = nullptr, *sp_y = nullptr;  // N x D (+ GOGP_MAX_NDIM slack) and N doubles, resident
  int64_t sp_N = 0, sp_M = 0;
  bool sp_have = false, sp_observed = false;
  int sp_jitter_log10 = -8;        // option "sparse_jitter_log10"
  int64_t sp_chunk = 8192;         // option "sparse_chunk": rows of X per pass
  Workspace sp_ws;                 // the Mp x Mp matrices, block inverses, vectors and slot sums (api.hip: sparse_layout)
  Workspace sp_vec;                // gogp_sparse_produce: one dot product per test point
  Workspace sp_ug;                 // gogp_sparse_gradient_inducing: the slab partials of launch_sparse_ugrad and two M x D arrays
  double sp_yty = 0.0;             // y^T y of the sparse data
  double sp_s2 = 0.0, sp_dnoise = 0.0, sp_csum = 0.0;  // of the last gogp_sparse_observe: noise variance, its derivative, sum of the output scales
  double sp_scal[5] = {};          // ... and its scalars (sparse.hip: sparse_scalars_kernel)
  std::vector<double> sp_cterm;    // ... and every term's output scale
  // gogp_sparse_multi_*: T output columns on the sparse data (api.hip).  sp_observed / sp_mobserved: whose observe the
  // shared Mp x Mp workspace holds -- the last observe of either flavour clears the other's flag.
  double *sp_Y = nullptr;          // N x T row-major as given, resident
  int sp_T = 0;
  bool sp_mobserved = false;
  std::vector<double> sp_myty;     // y_t^T y_t, from gogp_sparse_multi_set_outputs
  std::vector<double> sp_mdots;    // of the last gogp_sparse_multi_observe: r_t^T gamma_t (T), then gamma_t^T gamma_t (T)
  Workspace sp_mws;                // state of the multi observe, sized by gogp_sparse_multi_set_outputs (api.hip: SparseMultiBufs)
  Workspace sp_mscr;               // scratch sized by the chunk: the partials of launch_sparse_xty, the padded chunk of Y
  Workspace sp_mmu;                // gogp_sparse_multi_produce: mpad x 128 means
  // the iterative exact GP (cg_api.hip: gogp_cg_*) and Vecchia's approximation (vecchia_api.hip: gogp_vecchia_*): each a
  // data set of its own, resident; nothing of the handle's other state is touched
  CgHandleState cg;
  VecchiaState vc;
  // the Laplace approximation (gogp_laplace_*, laplace.hip; api.hip: LapVecs).  B's factor lies in bufL / Dinv, B^-1 and
  // then the gradient's weight matrix in bufA; only vectors are its own (released with the N buffers).
  Workspace lap_ws;
  bool lap_observed = false;     // a Laplace observe's factor, mode and site vectors are in place (also with n == 0)
  bool lap_grad_valid = false;   // lap_grad belongs to them (bufA then holds the weight matrix, not B^-1)
  std::vector<double> lap_grad;
  int lap_lik = 0, lap_iters = 0;
  int lap_max_iter = 50, lap_tol_log10 = -10, lap_warm = 0;  // options "laplace_max_iter", "laplace_tol_log10", "laplace_warm"
  bool lap_warm_valid = false;   // the workspace holds a converged a^ of lap_warm_lik for the current data (lap_warm_n rows)
  int lap_warm_lik = 0;
  int64_t lap_warm_n = 0;
  // set only while a Laplace observe factors (api.hip: Sweep::build_gram, factorize_t): the Gram stage scales K into
  // B = I + diag(lap_sw) K diag(lap_sw) and the forward substitution's working copy comes from lap_rhs instead of dy
  const double *lap_sw = nullptr, *lap_rhs = nullptr;
  // per-observation noise variances (gogp_set_noise_variances, noisevar.hip): K = k(X, X) + s2 I + diag(nv).  nv_cap
  // doubles, zero from row n on; released with the N buffers, grown with them by gogp_append.  nv_set: they apply to
  // the current data -- the sweep adds them behind the Gram build, gogp_append / gogp_remove carry them.
  double *nv = nullptr;
  int64_t nv_cap = 0;
  bool nv_set = false;
  Workspace nv_ws;          // gogp_noise_variances_gradient: dv (npad doubles)
  double yta = 0.0;     // y^T alpha of the last factorisation (fp32 path: of the refined alpha)
  int trace_fp64 = 1;    // fp32 path: tr(alpha alpha^T - K^-1) summed in fp64 from Y, scale component by its identity
  double cond_limit = 1e16;  // gonum's mat.ConditionTolerance
  std::vector<double> grad_cache;
  std::string err;
  GemmProfile prof;
  // HIP-event timing of the O(N^2) kernels (gogp_profile_read_aux): class -> event pairs
  std::vector<hipEvent_t> aux_ev[GOGP_PROF_NCLASS];
  size_t aux_used[GOGP_PROF_NCLASS] = {0, 0, 0, 0};
};

// Bracket the launches of one O(N^2) kernel class with events on their stream (only while
// profiling is enabled).
struct AuxTimer {
  gogp_handle *h;
  int cls;
  hipStream_t s;
  hipEvent_t e1 = nullptr;
  AuxTimer(gogp_handle *h_, int cls_, hipStream_t s_) : h(h_), cls(cls_), s(s_) {
    if (!h->prof.on || cls < 0 || cls >= GOGP_PROF_NCLASS) return;
    auto &pool = h->aux_ev[cls];
    size_t &used = h->aux_used[cls];
    while (pool.size() < used + 2) {
      hipEvent_t e = nullptr;
      (void)hipEventCreate(&e);
      pool.push_back(e);
    }
    (void)hipEventRecord(pool[used], s);
    e1 = pool[used + 1];
    used += 2;
  }
  ~AuxTimer() {
    if (e1) (void)hipEventRecord(e1, s);
  }
};

#define HIPCHK(h, call)                                                                \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) {                                                            \
      char buf_[512];                                                                  \
      snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
               __FILE__, __LINE__);                                                    \
      (h)->err = buf_;                                                                 \
      (void)hipGetLastError(); /* reset the sticky error: later calls must not see it */ \
      return (e_ == hipErrorOutOfMemory) ? GOGP_ENOMEM : GOGP_EHIP;                     \
    }                                                                                  \
  } while (0)

inline int Workspace::reserve(gogp_handle *h, size_t need) {
  if (p && bytes >= need) return GOGP_OK;
  release();
  HIPCHK(h, hipMalloc(&p, need));
  bytes = need;
  return GOGP_OK;
}

// the two time-out words of the pinned staging row (HS_TMO)
static inline unsigned *hs_tmo(const gogp_handle *h) { return reinterpret_cast<unsigned *>(h->hscal + HS_TMO); }

// ---- the set of N-sized buffers ----------------------------------------------------------------
static inline void nbufs_free(const NBufs &b) {
  for (double *q : {b.dX, b.dy, b.bufA, b.bufL, b.Dinv, b.z, b.w, b.alpha, b.gpart}) (void)hipFree(q);
}
// A whole set for `cap` (a multiple of PANEL) observations into *b, or nothing.  Matrices are float on the fp32 path.
static inline hipError_t nbufs_alloc(const gogp_handle *h, int64_t cap, NBufs *b) {
  const size_t nn = (size_t)cap * (size_t)cap * h->esz(), vec = (size_t)cap * sizeof(double);
  // (+ GOGP_MAX_NDIM doubles of slack: grad.hip reads a few coordinates past the last row)
  hipError_t e = hipMalloc(&b->dX, ((size_t)cap * h->D + GOGP_MAX_NDIM) * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&b->dy, vec);
  if (e == hipSuccess) e = hipMalloc(&b->bufA, nn);
  if (e == hipSuccess) e = hipMalloc(&b->bufL, nn);
  if (e == hipSuccess) e = hipMalloc(&b->Dinv, (size_t)(cap / gogp::PANEL) * gogp::PANEL * gogp::PANEL * h->esz());
  if (e == hipSuccess) e = hipMalloc(&b->z, vec);
  if (e == hipSuccess) e = hipMalloc(&b->w, vec);
  if (e == hipSuccess) e = hipMalloc(&b->alpha, vec);
  if (e == hipSuccess) e = hipMalloc(&b->gpart, (size_t)gogp::grad_reduce_blocks(cap) * gogp::NACC * sizeof(double));
  if (e != hipSuccess) {
    nbufs_free(*b);
    *b = NBufs();
  }
  return e;
}
static inline NBufs nbufs_of(const gogp_handle *h) {
  NBufs b;
  b.dX = h->dX, b.dy = h->dy, b.bufA = h->bufA, b.bufL = h->bufL, b.Dinv = h->Dinv;
  b.z = h->z, b.w = h->w, b.alpha = h->alpha, b.gpart = h->gpart;
  return b;
}
static inline void nbufs_put(gogp_handle *h, const NBufs &b) {
  h->dX = b.dX, h->dy = b.dy, h->bufA = b.bufA, h->bufL = b.bufL, h->Dinv = b.Dinv;
  h->z = b.z, h->w = b.w, h->alpha = b.alpha, h->gpart = b.gpart;
}

// every work stream of the handle (the communication stream of a sharded handle is dist2d's)
static inline std::array<hipStream_t, 6> work_streams(const gogp_handle *h) {
  return {h->s, h->sp, h->s2, h->st, h->sl, h->sk};
}

static inline int fail(gogp_handle *h, int code, const char *msg) {
  if (h) h->err = msg;
  return code;
}

// ---- cross-stream events -----------------------------------------------------------------
enum { EV_GRAM = 0, EV_FWD = 1, EV_ALPHA = 2, EV_INIT = 3, EV_TRTRI = 4, EV_W = 5, EV_ENTRY = 6, EV_KINV = 7,
       EV_YDONE = 8,  // Y is final (EV_TRTRI: everything on the inverse's chain stream is done, alpha = Y z included)
       EV_TINV = 9,   // T^-1 of every super-panel assembled (stream sk)
       EV_BASE = 10 };
// per panel p: EV_BASE + 4p + {0: panel p of L final, 1: next block column of A final,
//                              2: column panel p of Y final, 3: next column panel of R final}
static inline hipEvent_t ev(gogp_handle *h, size_t i) {
  while (h->evs.size() <= i) {
    hipEvent_t e = nullptr;
    (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
    h->evs.push_back(e);
  }
  return h->evs[i];
}
// "a then b": work enqueued on `to` after this call waits for everything
// enqueued on `from` before it
static inline void order(gogp_handle *h, size_t i, hipStream_t from, hipStream_t to) {
  hipEvent_t e = ev(h, i);
  (void)gogp::rec_event_record(e, from);  // an explicit graph under construction takes these as dependencies (graphrec.h)
  (void)gogp::rec_stream_wait(to, e);
}


// ---- sharded evaluation (dist2d.hip) -----------------------------------------------------------
int gogp_upload_params(gogp_handle *h);            // api.hip: theta -> DevParams on h->s
void gogp_dist_destroy(gogp_handle *h);
int gogp_dist_sync(gogp_handle *h);                // drain the communication stream
int gogp_dist_ensure_n(gogp_handle *h, int64_t n);  // sizes + buffers of this rank's shard
int gogp_dist_factorize(gogp_handle *h, bool want_kinv);
int gogp_dist_gradient_sums(gogp_handle *h, double *hacc /* NACC, pinned host */);
int gogp_dist_produce(gogp_handle *h, const double *Z, int64_t m, double *mu, double *sigma);
int gogp_dist_get_factor(gogp_handle *h, double *Lout /* n*n, every rank */);
// rows != nullptr: nrows selected rows of L (nrows x n); rows == nullptr: the diagonal (n); collective
int gogp_dist_get_factor_part(gogp_handle *h, const int64_t *rows, int64_t nrows, double *out);
int gogp_dist_set_factor(gogp_handle *h, const double *Lin /* n*n, every rank */, const double *alpha /* n */);
