// api.hip -- C ABI (include/gogp_hip.h) and orchestration of the hot path.
//
// Data layout in HBM (all fp64, row-major, leading dimension npad):
//   npad = N rounded up to a multiple of 256; rows/cols >= N are identity
//          padding, so every kernel works on whole 128x128 tiles.
//   bufA : Gram matrix K (lower triangle) -> destroyed in place by the
//          trailing updates of the blocked Cholesky; during Gradient it is
//          re-used for R (right-hand side of the triangular inverse) and
//          finally holds K^-1 (lower triangle).
//   bufL : the lower Cholesky factor L (gp.GP.L, gp/gp.go:35).
//   bufY : Y = L^-T (upper triangular), allocated on the first Gradient.
//   Dinv : dense inverse of every 256x256 diagonal block of L (npad/256 blocks).
//   X (npad x D), y, z = L^-1 y, alpha = K^-1 y (gp.GP.Alpha, gp/gp.go:36).
//
// Step list of one Observe + Gradient (reference call stack: SURVEY.md 3.1):
//   gram_lower -> per 256-panel { diag256 (factor + inverse of the diagonal block),
//   panel solve as ONE GEMM with the inverse, forward-substitution step | next
//   block column update, SYRK K=256 of the rest } -> LML scalars
//   -> [Gradient] identity fill, per panel { Y = R*Dinv^T | R updates } ->
//   LAUUM (K^-1 = Y Y^T) -> fused gradient reduce.   ("|" = two streams)
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <mutex>
#include <new>
#include <thread>
#include <type_traits>
#include <utility>

#include "api_internal.h"

using namespace gogp;

static thread_local std::string g_create_error;

// ---- descriptor helpers -------------------------------------------------------
extern "C" int gogp_desc_ntheta_noise(const gogp_desc *d) {
  return (d && (d->noise_kind == GOGP_NOISE_UNIFORM || d->noise_kind == GOGP_NOISE_CONSTANT_PARAM)) ? 1 : 0;
}

extern "C" int gogp_desc_check(const gogp_desc *d) {
  if (!d) return GOGP_EARG;
  if (d->ndim < 1 || d->ndim > GOGP_MAX_NDIM) return GOGP_EARG;
  if (d->nterms < 1 || d->nterms > GOGP_MAX_TERMS) return GOGP_EARG;
  if (d->ntheta_simil < 1 || d->ntheta_simil > GOGP_MAX_NDIM + 8) return GOGP_EARG;
  if (d->noise_kind != GOGP_NOISE_CONSTANT && d->noise_kind != GOGP_NOISE_UNIFORM &&
      d->noise_kind != GOGP_NOISE_CONSTANT_PARAM)
    return GOGP_EARG;
  int nard = 0;
  for (int t = 0; t < d->nterms; ++t) {
    const gogp_term &T = d->terms[t];
    if (T.kind < GOGP_K_NORMAL || T.kind > GOGP_K_PERIODIC) return GOGP_EARG;
    if (T.scale_idx >= d->ntheta_simil || T.scale_idx < -1) return GOGP_EARG;
    const int nlen = T.ard ? d->ndim : 1;
    if (T.len_idx < 0 || T.len_idx + nlen > d->ntheta_simil) return GOGP_EARG;
    if (T.kind == GOGP_K_PERIODIC) {
      if (T.period_idx < 0 || T.period_idx >= d->ntheta_simil) return GOGP_EARG;
      if (!(T.period_mult > 0)) return GOGP_EARG;
    }
    if (T.ard) ++nard;
  }
  if (nard > 1) return GOGP_EARG;  // one ARD term per kernel (grad.hip accumulators)
  return GOGP_OK;
}

extern "C" int gogp_events_check(const double *events, int nevents, int axis, int ndim) {
  if (nevents < 0 || nevents > GOGP_MAX_EVENTS) return GOGP_EARG;
  if (ndim < 1 || ndim > GOGP_MAX_NDIM || axis < 0 || axis >= ndim) return GOGP_EARG;
  if (nevents > 0 && !events) return GOGP_EARG;
  for (int i = 0; i < 3 * nevents; ++i)
    if (!isfinite(events[i])) return GOGP_EARG;
  return GOGP_OK;
}

extern "C" const char *gogp_version(void) {
#ifndef GOGP_BUILD_ID
#define GOGP_BUILD_ID "unknown"
#endif
  return "gogp_hip 0.3 gfx950 fp64-mfma(v_mfma_f64_16x16x4_f64) tile128 panel256 build " GOGP_BUILD_ID;
}

extern "C" const char *gogp_last_error(const gogp_handle *h) {
  if (!h) return g_create_error.c_str();
  return h->err.c_str();
}

extern "C" int64_t gogp_notpd_index(const gogp_handle *h) { return h ? h->notpd : -1; }
extern "C" int64_t gogp_n(const gogp_handle *h) { return h ? h->n : 0; }

// ---- lifecycle ---------------------------------------------------------------------
static void free_n_buffers(gogp_handle *h) {
  nbufs_free(nbufs_of(h));
  nbufs_put(h, NBufs());
  (void)hipFree(h->bufY);
  h->bufY = nullptr;
  (void)hipFree(h->rw);
  (void)hipFree(h->rz);
  (void)hipFree(h->rd);
  (void)hipFree(h->rpart);
  h->small_ws.release();
  h->app_ws.release();
  h->rm_ws.release();
  h->loo_vec.release();
  h->loo_mat.release();
  h->lap_ws.release();
  h->lap_observed = h->lap_grad_valid = h->lap_warm_valid = false;
  (void)hipFree(h->nv);
  h->nv = nullptr;
  h->nv_cap = 0;
  h->nv_set = false;
  h->nv_ws.release();
  h->bcv_vec.release();
  h->bcv_s.release();
  h->multi_vec.release();
  h->multi_mean.release();
  h->multi_mat.release();
  h->multi_T = 0;
  h->multi_solved = false;
  h->basis_vec.release();
  h->basis_part.release();
  h->basis_mean.release();
  h->basis_p = 0;
  h->basis_solved = false;
  (void)hipFree(h->TX);
  (void)hipFree(h->Tmt);
  h->TX = h->Tmt = nullptr;
  h->cap_tinv = 0;
  h->tinv_valid = h->tinv_pending = false;
  (void)hipFree(h->g32A);
  (void)hipFree(h->g32L);
  (void)hipFree(h->g32Y);
  (void)hipFree(h->g32D);
  h->g32A = h->g32L = h->g32Y = h->g32D = nullptr;
  h->g32_cap = 0;
  h->rw = h->rz = h->rd = h->rpart = nullptr;
  h->cap_npad = 0;
  h->cap_y = 0;
}

static void drop_cand_graph(gogp_handle *h) {
  if (h->cand_graph) (void)hipGraphExecDestroy(h->cand_graph);
  h->cand_graph = nullptr;
  // "captured on its second identical use" starts over: what was seen was seen under the old options / buffers
  h->cand_seen_key = CandGraphKey();
}
// the capture / replay stream belongs to the handle's pooled stream set (streams are never destroyed,
// see "stream sets" below): created on first use, handed on with the set
static hipError_t graph_stream(gogp_handle *h);

static void free_cand_buffers(gogp_handle *h) {
  drop_cand_graph(h);
  (void)hipFree(h->cand_arena);
  (void)hipHostFree(h->cand_hostP);
  (void)hipHostFree(h->cand_hscal);
  h->cand_arena = nullptr;
  h->cand_hostP = nullptr;
  h->cand_hscal = nullptr;
  h->cand_stride = 0;
  h->cand_cap_k = h->cand_host_k = 0;
  h->cand_cap_npad = 0;
}

static void free_m_buffers(gogp_handle *h) {
  (void)hipFree(h->dZ);
  (void)hipFree(h->KsT);
  (void)hipFree(h->Vt);
  (void)hipFree(h->pvec);
  h->pg_ws.release();
  h->pc_ws.release();
  h->dZ = h->KsT = h->Vt = h->pvec = nullptr;
  h->cap_m = h->cap_mp_npad = 0;
}

// ---- stream sets ------------------------------------------------------------------------
// A handle works on five streams.  They come from a per-device pool and go back to it when
// the handle is destroyed; a stream is never destroyed.  Measured reason (tools/
// handle_probe.py): after hipStreamDestroy, newly created streams get a poor mapping onto
// the few hardware queues ROCm multiplexes streams on, and every later handle of the
// process ran 55 % slower at N = 4096 (7.2 ms per evaluation instead of 4.55).  Handles
// that are alive at the same time get distinct sets.
struct StreamSet {
  int device = -1;
  bool in_use = false;
  hipStream_t s = nullptr, s2 = nullptr, sp = nullptr, st = nullptr, sl = nullptr, sk = nullptr;
  hipStream_t sg = nullptr;  // capture / replay stream of the candidates' hipGraph, created on first use
};
static std::mutex g_pool_mutex;
static std::vector<StreamSet *> g_stream_pool;

static hipError_t create_stream_set(StreamSet *ss, int device) {
  ss->device = device;
  hipError_t e = hipSuccess;
  e = hipStreamCreateWithFlags(&ss->s, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&ss->s2, hipStreamNonBlocking);
  if (e == hipSuccess) {
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    // Only the Cholesky chain is high priority.  Measured (tools/batch_probe.py): with the
    // inverse's chain high as well, the chain kernels of concurrently evaluated candidates
    // serialise behind each other's event waits (k = 4 handles at N = 4096: 282 evals/s; with
    // this layout 350) and one evaluation at N = 16384 is 1 % slower.
    const int normal = (least + greatest) / 2;
    e = hipStreamCreateWithPriority(&ss->sp, hipStreamNonBlocking, greatest);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&ss->st, hipStreamNonBlocking, normal);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&ss->sl, hipStreamNonBlocking, normal);
    // K^-1 accumulates behind everything else: whatever the chains leave idle
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&ss->sk, hipStreamNonBlocking, least);
  }
  return e;
}

static hipError_t acquire_streams(gogp_handle *h, int device) {
  std::lock_guard<std::mutex> lock(g_pool_mutex);
  StreamSet *ss = nullptr;
  for (StreamSet *c : g_stream_pool)
    if (!c->in_use && c->device == device) {
      ss = c;
      break;
    }
  if (!ss) {
    ss = new StreamSet();
    const hipError_t e = create_stream_set(ss, device);
    if (e != hipSuccess) {  // partial sets are not pooled
      for (hipStream_t q : {ss->s, ss->s2, ss->sp, ss->st, ss->sl, ss->sk})
        if (q) (void)hipStreamDestroy(q);
      delete ss;
      return e;
    }
    g_stream_pool.push_back(ss);
  }
  ss->in_use = true;
  h->stream_set = ss;
  h->s = ss->s;
  h->s2 = ss->s2;
  h->sp = ss->sp;
  h->st = ss->st;
  h->sl = ss->sl;
  h->sk = ss->sk;
  return hipSuccess;
}

static hipError_t graph_stream(gogp_handle *h) {
  StreamSet *ss = static_cast<StreamSet *>(h->stream_set);
  if (!ss->sg) {
    const hipError_t e = hipStreamCreateWithFlags(&ss->sg, hipStreamNonBlocking);
    if (e != hipSuccess) return e;
  }
  h->sg = ss->sg;
  return hipSuccess;
}

static void sparse_free(gogp_handle *h);  // the inducing-point state (gogp_sparse_*), below

static void release_streams(gogp_handle *h) {
  std::lock_guard<std::mutex> lock(g_pool_mutex);
  if (h->stream_set) static_cast<StreamSet *>(h->stream_set)->in_use = false;
  h->stream_set = nullptr;
  h->sg = nullptr;
  h->s = h->s2 = h->sp = h->st = h->sl = h->sk = nullptr;
}

extern "C" void gogp_destroy(gogp_handle *h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->s) (void)hipStreamSynchronize(h->s);
  gogp_dist_destroy(h);
  sparse_free(h);
  h->cg.release();
  h->vc.release();
  free_n_buffers(h);
  free_m_buffers(h);
  free_cand_buffers(h);
  (void)hipFree(h->bt_X);
  (void)hipFree(h->bt_y);
  (void)hipFree(h->bt_din);
  (void)hipFree(h->bt_dout);
  if (h->bt_hin) (void)hipHostFree(h->bt_hin);
  if (h->bt_hout) (void)hipHostFree(h->bt_hout);
  (void)hipFree(h->scalars);
  (void)hipFree(h->dscr);
  (void)hipFree(h->D64);
  (void)hipFree(h->info);
  (void)hipFree(h->gout);
  (void)hipFree(h->devP);
  if (h->hostP) (void)hipHostFree(h->hostP);
  if (h->hscal) (void)hipHostFree(h->hscal);
  for (auto e : h->prof.pool) (void)hipEventDestroy(e);
  for (auto &pool : h->aux_ev)
    for (auto e : pool) (void)hipEventDestroy(e);
  for (auto e : h->evs) (void)hipEventDestroy(e);
  for (hipStream_t q : work_streams(h))
    if (q) (void)hipStreamSynchronize(q);
  release_streams(h);
  delete h;
}

extern "C" int gogp_create(const gogp_desc *desc, int device, gogp_handle **out) {
  if (!out) return GOGP_EARG;
  *out = nullptr;
  if (gogp_desc_check(desc) != GOGP_OK) {
    g_create_error = "invalid kernel descriptor";
    return GOGP_EARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_create_error = "no HIP device available (libgogp_hip has no CPU fallback)";
    return GOGP_EHIP;
  }
  if (device < 0) {
    if (hipGetDevice(&device) != hipSuccess) device = 0;
  }
  if (device >= ndev) {
    g_create_error = "device index out of range";
    return GOGP_EARG;
  }
  gogp_handle *h = new (std::nothrow) gogp_handle();
  if (!h) return GOGP_ENOMEM;
  h->desc = *desc;
  h->device = device;
  h->D = desc->ndim;
  h->ns = desc->ntheta_simil;
  h->nn = gogp_desc_ntheta_noise(desc);
  h->P = h->ns + h->nn;
  for (int t = 0; t < desc->nterms; ++t)
    if (desc->terms[t].ard) h->ard_dims = desc->ndim;
  h->radial1 = desc->nterms == 1 && desc->terms[0].kind != GOGP_K_PERIODIC;
  h->theta_s.assign(h->ns, 0.0);  // gp/gp.go:50-56
  h->theta_n.assign(h->nn > 0 ? h->nn : 1, 0.0);
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = acquire_streams(h, device);
  if (e == hipSuccess) e = hipMalloc(&h->scalars, 8 * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&h->dscr, (size_t)3 * PANEL * PANEL * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&h->info, sizeof(long long));
  if (e == hipSuccess) e = hipMalloc(&h->gout, NACC * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&h->devP, sizeof(DevParams));
  if (e == hipSuccess) e = hipHostMalloc((void **)&h->hostP, sizeof(DevParams), hipHostMallocDefault);
  if (e == hipSuccess)
    e = hipHostMalloc((void **)&h->hscal, BATCH_ROW * sizeof(double), hipHostMallocDefault);
  if (e != hipSuccess) {
    g_create_error = std::string("HIP initialisation failed: ") + hipGetErrorString(e);
    gogp_destroy(h);
    return GOGP_EHIP;
  }
  *out = h;
  return GOGP_OK;
}

// ---- data -------------------------------------------------------------------------------
static int ensure_n(gogp_handle *h, int64_t n) {
  const int64_t npad = n <= 0 ? 0 : ((n + PANEL - 1) / PANEL) * PANEL;
  h->n = n;
  h->npad = npad;
  h->nblk = (int)(npad / TILE);
  h->factored = h->have_alpha = h->have_kinv = h->observed = h->grad_valid = false;
  h->multi_solved = false;
  h->basis_solved = false;
  h->trtri_done = false;
  h->lap_observed = h->lap_grad_valid = h->lap_warm_valid = false;  // the Laplace fit and its warm start belonged to the old data
  if (npad > h->cap_npad) {
    free_n_buffers(h);
    NBufs nb;
    HIPCHK(h, nbufs_alloc(h, npad, &nb));
    nbufs_put(h, nb);
    if (h->prec == 32) {  // scratch of the iterative refinement of alpha
      HIPCHK(h, hipMalloc(&h->rw, (size_t)npad * sizeof(double)));
      HIPCHK(h, hipMalloc(&h->rz, (size_t)npad * sizeof(double)));
      HIPCHK(h, hipMalloc(&h->rd, (size_t)npad * sizeof(double)));
      HIPCHK(h, hipMalloc(&h->rpart, (size_t)REFINE_SLABS * npad * sizeof(double)));
    }
    h->cap_npad = npad;
    // invalidate the produce workspace that depends on npad
    free_m_buffers(h);
  }
  return GOGP_OK;
}

static int set_data_impl(gogp_handle *h, const double *X, const double *y, int64_t n,
                         hipMemcpyKind kind) {
  if (!h) return GOGP_EARG;
  if (n < 0 || (n > 0 && (!X || !y))) return fail(h, GOGP_EARG, "set_data: bad arguments");
  HIPCHK(h, hipSetDevice(h->device));
  // nothing of a previous evaluation may still be running when buffers are
  // replaced or re-filled
  for (hipStream_t q : work_streams(h)) HIPCHK(h, hipStreamSynchronize(q));
  h->trtri_pending = h->alpha_pending = h->kinv_pending = false;
  h->tinv_valid = h->tinv_pending = false;
  if (h->dist) {
    const int rcs = gogp_dist_sync(h);
    if (rcs != GOGP_OK) return rcs;
  }
  int rc = h->dist ? gogp_dist_ensure_n(h, n) : ensure_n(h, n);
  if (rc != GOGP_OK) return rc;
  h->have_data = true;
  h->multi_T = 0;  // the outputs of gogp_multi_set_outputs belonged to the data that was replaced
  h->basis_p = 0;  // ... and so did the basis of gogp_basis_set
  h->basis_solved = false;
  h->nv_set = false;  // ... and the variances of gogp_set_noise_variances
  if (n == 0) return GOGP_OK;
  // zero padding rows, then copy
  HIPCHK(h, hipMemsetAsync(h->dX, 0, ((size_t)h->npad * h->D + GOGP_MAX_NDIM) * sizeof(double), h->s));
  HIPCHK(h, hipMemsetAsync(h->dy, 0, (size_t)h->npad * sizeof(double), h->s));
  HIPCHK(h, hipMemcpyAsync(h->dX, X, (size_t)n * h->D * sizeof(double), kind, h->s));
  HIPCHK(h, hipMemcpyAsync(h->dy, y, (size_t)n * sizeof(double), kind, h->s));
  HIPCHK(h, hipStreamSynchronize(h->s));
  return GOGP_OK;
}

extern "C" int gogp_set_data(gogp_handle *h, const double *X, const double *y, int64_t n) {
  return set_data_impl(h, X, y, n, hipMemcpyHostToDevice);
}

extern "C" int gogp_set_data_device(gogp_handle *h, const double *dX, const double *dy,
                                    int64_t n) {
  return set_data_impl(h, dX, dy, n, hipMemcpyDeviceToDevice);
}

// ---- event discounts (tutorial/events/kernel/kernel.go:14-44) --------------------------------
// Host state only: fill_params copies the table into every DevParams, and h->ev() selects the kernels' *_ev_kernel
// instances at every launch that evaluates the similarity.
extern "C" int gogp_set_events(gogp_handle *h, const double *events, int nevents, int axis) {
  if (!h) return GOGP_EARG;
  if (nevents == 0 && !events) axis = 0;  // clearing: the axis does not matter
  if (gogp_events_check(events, nevents, axis, h->D) != GOGP_OK)
    return fail(h, GOGP_EARG, "set_events: need 0 <= nevents <= GOGP_MAX_EVENTS, 0 <= axis < ndim, finite values");
  if (nevents > 0 && h->ard_dims > 0)
    return fail(h, GOGP_EARG, "set_events: event discounts are not supported with an ARD term");
  HIPCHK(h, hipSetDevice(h->device));
  // nothing enqueued may still read the old kernel; stored results (factor, alpha, K^-1) no longer match it
  for (hipStream_t q : work_streams(h)) HIPCHK(h, hipStreamSynchronize(q));
  if (h->dist) {
    const int rcs = gogp_dist_sync(h);
    if (rcs != GOGP_OK) return rcs;
  }
  drop_cand_graph(h);  // a captured candidates sequence launched the other kernel instances
  h->nevents = nevents;
  h->ev_axis = axis;
  for (int e = 0; e < nevents; ++e)
    for (int f = 0; f < 3; ++f) h->events[e][f] = events[3 * e + f];
  h->factored = h->have_alpha = h->have_kinv = h->observed = h->grad_valid = false;
  h->multi_solved = false;
  h->basis_solved = false;
  h->lap_observed = h->lap_grad_valid = false;
  h->trtri_done = h->trtri_pending = h->alpha_pending = h->kinv_pending = false;
  h->tinv_valid = h->tinv_pending = false;
  return GOGP_OK;
}

// ---- parameters ---------------------------------------------------------------------------
// DevParams of the natural parameters ts (similarity), tn (noise)
void gogp::fill_params_theta(const gogp_handle *h, const double *ts, const double *tn, DevParams &p) {
  const gogp_desc &d = h->desc;
  memset(&p, 0, sizeof p);
  p.ndim = d.ndim;
  p.nterms = d.nterms;
  p.ns = h->ns;
  p.nn = h->nn;
  for (int t = 0; t < d.nterms; ++t) {
    const gogp_term &T = d.terms[t];
    p.kind[t] = T.kind;
    p.ard[t] = T.ard;
    p.c[t] = T.scale_idx >= 0 ? ts[T.scale_idx] : 1.0;
    p.w[t] = 0.0;
    if (T.kind == GOGP_K_PERIODIC)
      p.w[t] = M_PI / (T.period_mult * ts[T.period_idx]);
    for (int j = 0; j < d.ndim; ++j)
      p.inv_len[t][j] = 1.0 / ts[T.len_idx + (T.ard ? j : 0)];
  }
  if (d.noise_kind == GOGP_NOISE_CONSTANT || d.noise_kind == GOGP_NOISE_CONSTANT_PARAM) {
    // kernel/noise.go:27-30; tutorial/anynoise/kernel/kernel.go:31-33 (the parameter is unused)
    p.noise_var = d.noise_std * d.noise_std;
    p.dnoise = 0.0;
  } else {
    const double sd = tn[0];
    p.noise_var = d.noise_scale * sd * sd;  // kernel/noise.go:47-49
    p.dnoise = 2.0 * p.noise_var;
  }
  p.nevents = h->nevents;
  p.ev_axis = h->ev_axis;
  for (int e = 0; e < h->nevents; ++e) {
    p.ev_from[e] = h->events[e][0];
    p.ev_to[e] = h->events[e][1];
    p.ev_disc[e] = h->events[e][2];
  }
}

// ... of the handle's current natural parameters (theta_s, theta_n)
static void fill_params(const gogp_handle *h, DevParams &p) {
  fill_params_theta(h, h->theta_s.data(), h->theta_n.data(), p);
}

int gogp_upload_params(gogp_handle *h) {
  if (h->batch_mode) return GOGP_OK;  // a batched evaluation uploaded every candidate's parameters
  fill_params(h, *h->hostP);
  HIPCHK(h, hipMemcpyAsync(h->devP, h->hostP, sizeof(DevParams), hipMemcpyHostToDevice, h->s));
  return GOGP_OK;
}

// ---- per-candidate copies of a batched evaluation (batch_k slots, cand_stride bytes apart; one
// ---- plain call when no batch is active) ---------------------------------------------------------
static hipError_t cand_memset(gogp_handle *h, void *dst, size_t bytes, hipStream_t s) {
  hipError_t e = hipSuccess;
  for (int c = 0; c < h->batch_k && e == hipSuccess; ++c)
    e = gogp::rec_memset_async((char *)dst + (size_t)c * h->cand_stride, 0, bytes, s);
  return e;
}
// shared source (y) into every candidate's copy
static hipError_t cand_copy_in(gogp_handle *h, void *dst, const void *src, size_t bytes, hipStream_t s) {
  hipError_t e = hipSuccess;
  for (int c = 0; c < h->batch_k && e == hipSuccess; ++c)
    e = gogp::rec_memcpy_async((char *)dst + (size_t)c * h->cand_stride, src, bytes, hipMemcpyDeviceToDevice, s);
  return e;
}
// device results of every candidate into its row of the pinned staging block (rows of BATCH_ROW doubles, HS_*)
static hipError_t cand_d2h(gogp_handle *h, double *hdst, const void *dsrc, size_t bytes, hipStream_t s) {
  hipError_t e = hipSuccess;
  for (int c = 0; c < h->batch_k && e == hipSuccess; ++c)
    e = gogp::rec_memcpy_async(hdst + (size_t)c * BATCH_ROW, (const char *)dsrc + (size_t)c * h->cand_stride, bytes,
                               hipMemcpyDeviceToHost, s);
  return e;
}

// bufY (Y = L^-T) is allocated on first use and tracked by its own capacity: the other
// N-dependent buffers may have been sized by an Absorb that never needed it.
static int ensure_y(gogp_handle *h) {
  if (h->bufY && h->cap_y >= h->npad) return GOGP_OK;
  (void)hipFree(h->bufY);
  h->bufY = nullptr;
  h->cap_y = 0;
  const int64_t cap = std::max(h->npad, h->cap_npad);
  HIPCHK(h, hipMalloc(&h->bufY, (size_t)cap * (size_t)cap * h->esz()));
  h->cap_y = cap;
  return GOGP_OK;
}

// fp32 path: the strip of diagonal blocks accumulated in fp64 (diagsyrk.hip)
static int ensure_d64(gogp_handle *h) {
  if (h->D64 && h->cap_d64 >= h->npad) return GOGP_OK;
  (void)hipFree(h->D64);
  h->D64 = nullptr;
  h->cap_d64 = 0;
  const int64_t cap = std::max(h->npad, h->cap_npad);
  HIPCHK(h, hipMalloc(&h->D64, (size_t)cap * PANEL * sizeof(double)));
  h->cap_d64 = cap;
  return GOGP_OK;
}

// What the scalars of one factorisation say (row of the pinned staging block: [0] 2 sum log L_ii,
// [1] z^T z, [3], [4] min / max L_ii, [5] fp64 log-determinant of the fp32 path, [6] y^T alpha of the
// refined alpha, [HS_INFO] first failing pivot + 1).
struct FactorResult {
  int rc = GOGP_OK;
  double lml = 0.0, cond_lb = 1.0, yta = 0.0;
  int64_t notpd = -1;
  std::string msg;
};
// n: the number of observations the scalars belong to (-1: the handle's own; a batch pair: its member's)
static FactorResult judge_scalars(const gogp_handle *h, const double *hs, bool fp32, bool refine, int64_t n = -1) {
  FactorResult r;
  long long info = 0;
  memcpy(&info, hs + HS_INFO, sizeof info);
  char buf[160];
  if (info != 0) {
    r.rc = GOGP_ENOTPD;
    r.notpd = (int64_t)info - 1;
    snprintf(buf, sizeof buf, "Factorize: matrix is not positive definite (pivot %lld)", (long long)r.notpd);
    r.msg = buf;
    return r;
  }
  // fp32 path: the log-determinant summed from the fp64 diagonal-block factors
  const double logdet = fp32 ? hs[5] : hs[0];
  const double ztz = refine ? hs[6] : hs[1];  // y^T alpha (refined) / z^T z
  r.yta = ztz;
  // gp/gp.go:244-253
  r.lml = -0.5 * (double)(n < 0 ? h->n : n) * log(2 * M_PI) - 0.5 * logdet - 0.5 * ztz;
  // gonum's Cholesky solves return a Condition error when its condition estimate exceeds
  // 1e16 (mat.ConditionTolerance), which gp/gp.go:233-236 passes on (Absorb: error, Observe:
  // panic).  (max L_ii / min L_ii)^2 is a lower bound of cond_2(K); beyond 1e16 the matrix is
  // numerically singular whatever the estimator.  The factor, alpha and LML stay available.
  const double dmin = hs[3], dmax = hs[4];
  r.cond_lb = (dmin > 0.0) ? (dmax / dmin) * (dmax / dmin) : INFINITY;
  if (!(r.cond_lb <= h->cond_limit)) {
    snprintf(buf, sizeof buf, "Condition: matrix singular or near-singular with condition number >= %.4e",
             r.cond_lb);
    r.msg = buf;
    r.rc = GOGP_ECOND;
  }
  return r;
}

// The end of a factorisation whose scalars are on their way to h->hscal on the main stream: in a batched evaluation the
// caller synchronises and judges every candidate from its own row; otherwise wait, judge and keep the result.
// kinv: K^-1 came with the factor (tiny_factorize).
static int finish_factorize(gogp_handle *h, bool fp32, bool refine, bool kinv) {
  h->alpha_pending = true;
  if (h->batch_mode) {
    h->factored = h->have_alpha = true;
    if (kinv) h->have_kinv = true;
    return GOGP_OK;
  }
  HIPCHK(h, hipStreamSynchronize(h->s));
  HIPCHK(h, hipGetLastError());
  const FactorResult fr = judge_scalars(h, h->hscal, fp32, refine);
  if (fr.rc == GOGP_ENOTPD) {
    h->alpha_pending = h->kinv_pending = false;
    h->tinv_valid = h->tinv_pending = false;
    h->trtri_done = h->trtri_pending = false;
    h->notpd = fr.notpd;
    h->err = fr.msg;
    return GOGP_ENOTPD;
  }
  h->lml = fr.lml;
  h->logdet2 = h->hscal[0];
  h->yta = fr.yta;
  h->factored = h->have_alpha = true;
  h->z_valid = true;
  if (kinv) h->have_kinv = true;
  h->cond_lb = fr.cond_lb;
  if (fr.rc == GOGP_ECOND) h->err = fr.msg;
  return fr.rc;
}

// ---- factorisation: Gram + blocked right-looking Cholesky + forward solve ----------------
// One 256x256 diagonal block: factor + dense inverse (diag256.hip, always fp64 arithmetic).  On
// the fp32 path the block is widened into fp64 scratch, factored and inverted there, and the
// factor and the inverse are rounded to float once; the log-determinant is accumulated from
// the fp64 factor (scalars[5]).
static void diag_block(gogp_handle *h, hipStream_t sp, const double *A, int64_t ld, double *L, int64_t ldl,
                       double *Dp, int64_t c0) {
  launch_diag256(sp, A, ld, L, ldl, Dp, c0, h->n, h->info);
}
static void diag_block(gogp_handle *h, hipStream_t sp, const float *A, int64_t ld, float *L, int64_t ldl,
                       float *Dp, int64_t c0) {
  double *A64 = h->dscr, *L64 = h->dscr + PANEL * PANEL, *D64 = h->dscr + 2 * PANEL * PANEL;
  if (h->d64_active)  // option "diag_fp64": the block as the fp64 strip accumulated it (diagsyrk.hip), not the float one
    A64 = h->D64 + (size_t)(c0 / PANEL) * PANEL * PANEL;
  else
    launch_convert_block(sp, A, ld, A64, PANEL, PANEL, PANEL);
  launch_diag256(sp, A64, PANEL, L64, PANEL, D64, c0, h->n, h->info);
  launch_convert_block(sp, L64, PANEL, L, ldl, PANEL, PANEL);
  launch_convert_block(sp, D64, PANEL, Dp, PANEL, PANEL, PANEL);
  launch_logdet_block(sp, L64, PANEL, c0, h->n, PANEL, h->scalars + 5);
}
static void diag_inv_only(gogp_handle *h, hipStream_t s, const double *L, int64_t ld, double *Dp) {
  (void)h;
  launch_diag256_inv_only(s, L, ld, Dp);
}
static void diag_inv_only(gogp_handle *h, hipStream_t s, const float *L, int64_t ld, float *Dp) {
  double *L64 = h->dscr + PANEL * PANEL, *D64 = h->dscr + 2 * PANEL * PANEL;
  launch_convert_block(s, L, ld, L64, PANEL, PANEL, PANEL);
  launch_diag256_inv_only(s, L64, PANEL, D64);
  launch_convert_block(s, D64, PANEL, Dp, PANEL, PANEL, PANEL);
}

// Width (in 256-panels) of the super-panel that starts at panel P0: `superpanel`, or -- option
// "superpanel_head" -- a wider one while more than `head_remaining` panels are still to come: the bulk
// updates of the first part of the sweep then carry K = 256 * superpanel_head (fewer passes over the
// trailing matrix, longer tiles), and the chain, which has slack while the trailing matrix is large,
// pays for it with more work inside the super-panel; near the end the chain is the critical path and the
// super-panels are narrow again.
// option "chain_prio": tile-kernel launches on the two chains raise their waves' issue priority (s_setprio 3), so
// that on a CU they share with bulk workgroups their MFMAs go first.  Measured: the chain's skinny GEMMs get 25 %
// faster under load, and that helps where the evaluation is chain-bound (N = 4096: 4.08 -> 3.95 ms) but costs
// where it is throughput-bound (N = 8192: 12.97 -> 13.14 ms, 16384: 73.2 -> 74.0): a bulk launch ends with its
// slowest tile, and the tiles that shared a CU with a prioritised workgroup are late.  -1 (default): on up to
// npad = 6144; 0: off; 1: the chains' 64x64-tile launches; 2: all their launches.
static inline int chain_prio_of(const gogp_handle *h) {
  return h->chain_prio < 0 ? (h->npad <= 6144 ? 1 : 0) : h->chain_prio;
}
// the grid options of a tile-kernel launch on one of the two chains
static inline GemmGrid chain_grid(const gogp_handle *h) {
  GemmGrid g;
  g.prio = chain_prio_of(h);
  return g;
}

// superpanel_head = -1 (default): 3 panels in fp64, 4 on the fp32 path, whose bulk updates run twice as fast
// beside the same fp64 diagonal-block chain (N = 32768: 311.6 -> 309.4 ms, N = 65536: 2322 -> 2303 ms; 6: 312.5)
static inline int superpanel_width(const gogp_handle *h, int npanel, int P0) {
  const int head = h->superpanel_head < 0 ? (h->prec == 32 ? 4 : 3) : h->superpanel_head;
  const int sw = (head > 0 && npanel - P0 > h->head_remaining) ? head : h->superpanel;
  return (npanel - P0 < sw) ? npanel - P0 : sw;
}
// One super-panel of the sweep: 256-panels P0 .. P0 + nsub - 1, columns C0 .. CE; prevP0: the one before it (-1: none),
// next_nsub: the width of the one after it (0: none)
struct SuperPanel {
  int P0, nsub, prevP0, next_nsub;
  int64_t C0() const { return (int64_t)P0 * PANEL; }
  int64_t CE() const { return C0() + (int64_t)nsub * PANEL; }
};
// the super-panels of the handle's matrix in the order of the sweep: the Cholesky sweep and the triangular inverse,
// fused behind it or lazy, walk the same ones
static std::vector<SuperPanel> superpanels(const gogp_handle *h) {
  const int npanel = (int)(h->npad / PANEL);
  std::vector<SuperPanel> v;
  for (int P0 = 0; P0 < npanel; P0 += v.back().nsub) {
    const int nsub = superpanel_width(h, npanel, P0);
    if (!v.empty()) v.back().next_nsub = nsub;
    v.push_back({P0, nsub, v.empty() ? -1 : v.back().P0, 0});
  }
  return v;
}
// Updates inside a super-panel are grouped like a binary counter: after its panel q (columns up to c2) the next
// grp = lowbit(q + 1) block columns, c2 .. ce, receive the LAST grp panels, columns k0 .. c2, at once (K = 256 grp).
// Every block column has all earlier panels of the super-panel when its turn comes; for two panels per super-panel this
// is the single K = 256 update of the second column.
struct InnerGroup {
  int grp;
  int64_t k0, ce;
};
static inline InnerGroup inner_group(int q, int64_t c2, int64_t CE) {
  const int done = q + 1, grp = done & -done;
  return {grp, c2 - (int64_t)grp * PANEL, std::min(c2 + (int64_t)grp * PANEL, CE)};
}

// ---- T^-1 of the super-panels' diagonal blocks (for Produce) --------------------------------------------------------
// widest super-panel (in 256-panels) the options allow = leading dimension of the T^-1 store
constexpr int TMT_BLOCKS = 8;  // scratch blocks M of one block diagonal (super-panels are at most 8 panels wide)
// Produce blocks the substitution by its own super-panels of `produce_panels` 256-panels (T^-1 is assembled by Produce,
// so its blocking is independent of the factorisation's)
static inline int tinv_panels(const gogp_handle *h) { return h->produce_panels; }
static inline int64_t tinv_signature(const gogp_handle *h) {
  return (int64_t)h->produce_panels + (h->npad << 8) + ((int64_t)h->prec << 56);
}
static int ensure_tinv(gogp_handle *h) {
  const int64_t tld = (int64_t)tinv_panels(h) * PANEL;
  const size_t need = (size_t)std::max(h->npad, h->cap_npad) * (size_t)tld;
  if (!h->TX || h->cap_tinv < need) {
    (void)hipFree(h->TX);
    (void)hipFree(h->Tmt);
    h->TX = h->Tmt = nullptr;
    h->cap_tinv = 0;
    HIPCHK(h, hipMalloc(&h->TX, need * h->esz()));
    HIPCHK(h, hipMalloc(&h->Tmt, (size_t)TMT_BLOCKS * PANEL * PANEL * h->esz()));
    h->cap_tinv = need;
  }
  h->tinv_ld = tld;  // every block that is read is written by the same assembly: a new ld needs no clearing
  return GOGP_OK;
}

// X = T^-1 (lower, row-major, ld tinv_ld) of the super-panel starting at panel P0, from its 256-block inverses and the
// factor's blocks inside it:  X_ii = Dinv_i,  X_ij = -Dinv_i sum_{k=j}^{i-1} L_ik X_kj  (i > j), block diagonal by
// block diagonal: all blocks at distance d = i - j in two launches of the batched 256-block product (solve.hip:
// blockmm_kernel: M = L[i, j..i-1] X[j..i-1, j], then X_ij = -Dinv_i M) -- 1 + 2 (panels - 1) tiny launches.
template <class T>
static void assemble_tinv(gogp_handle *h, hipStream_t sp, int P0, int nsub) {
  const int64_t ld = h->npad, tld = h->tinv_ld, C0 = (int64_t)P0 * PANEL;
  T *X = reinterpret_cast<T *>(h->TX) + C0 * tld;
  T *MT = reinterpret_cast<T *>(h->Tmt);
  const T *L = reinterpret_cast<const T *>(h->bufL);
  const T *Dinv = reinterpret_cast<const T *>(h->Dinv) + (size_t)P0 * PANEL * PANEL;
  launch_tinv_init(sp, Dinv, X, (T *)nullptr, nsub, tld);
  for (int d = 1; d < nsub; ++d) {
    const int cnt = nsub - d;  // blocks (i, i - d), i = d .. nsub-1
    for (int b0 = 0; b0 < cnt; b0 += 6) {
      const int nb = std::min(6, cnt - b0);
      const T *A1[6], *B1[6], *A2[6], *B2[6];
      T *C1[6], *C2[6];
      int64_t lda1[6], ldb1[6], ldc1[6], lda2[6], ldb2[6], ldc2[6];
      int K1[6], K2[6];
      for (int b = 0; b < nb; ++b) {
        const int i = d + b0 + b, j = i - d;
        A1[b] = L + (C0 + (int64_t)i * PANEL) * ld + C0 + (int64_t)j * PANEL;
        lda1[b] = ld;
        B1[b] = X + (int64_t)j * PANEL * tld + (int64_t)j * PANEL;
        ldb1[b] = tld;
        C1[b] = MT + (size_t)(b0 + b) * PANEL * PANEL;
        ldc1[b] = PANEL;
        K1[b] = d * PANEL;
        A2[b] = Dinv + (size_t)i * PANEL * PANEL;
        lda2[b] = PANEL;
        B2[b] = C1[b];
        ldb2[b] = PANEL;
        C2[b] = X + (int64_t)i * PANEL * tld + (int64_t)j * PANEL;
        ldc2[b] = tld;
        K2[b] = PANEL;
      }
      launch_blockmm(sp, nb, A1, lda1, B1, ldb1, C1, ldc1, K1, 1.0);
      launch_blockmm(sp, nb, A2, lda2, B2, ldb2, C2, ldc2, K2, -1.0);
    }
  }
}

// the matrices one super-step of the inverse works on: R (strictly upper blocks of A), Y, the factor and its block
// inverses -- the handle's own, or the float copies of the mixed-precision gradient
template <class T>
struct InvBufs {
  T *A, *Y;
  const T *L, *Dinv;
};
// One super-step of the triangular inverse Y = L^-T (upper): column panels
// P0 .. P0+nsub-1 (256 wide each), then ONE rank-(nsub*256) update of everything
// to the right:
//   per sub-panel p:  Y[c0:c2, c0:c2] = inv(L_pp)^T ;  Y[0:c0, c0:c2] = R[0:c0, c0:c2] inv(L_pp)^T
//                     R[0:c2, c2:CE] -= Y[0:c2, c0:c2] L[c2:CE, c0:c2]^T      (inside the super-panel)
//   R[0:CE, CE:]   -= Y[0:CE, C0:CE] L[CE:, C0:CE]^T                          (updates, s2)
// R occupies the strictly upper 256-block triangle of bufA (zero-initialised),
// which the Cholesky sweep never touches: the step only needs the panels of L it
// names and their diagonal inverses, so it runs right behind their factorisation.
template <class T>
static void trtri_superstep(gogp_handle *h, const InvBufs<T> &B, const SuperPanel &P, hipStream_t st, hipStream_t s2) {
  const int64_t npad = h->npad, ld = npad;
  T *R = B.A, *Y = B.Y;
  const T *L = B.L;
  GemmProfile *pf = &h->prof;
  const int P0 = P.P0;
  const int64_t C0 = P.C0(), CE = P.CE();
  // R[0:C0, C0:CE] is final: its last update (the previous super-step's next-columns update)
  // ran on this chain stream, in order
  for (int q = 0; q < P.nsub; ++q) {
    const int p = P0 + q;
    const int64_t c0 = (int64_t)p * PANEL, c2 = c0 + PANEL;
    const T *Dp = B.Dinv + (size_t)p * PANEL * PANEL;
    launch_ydiag(st, Dp, Y + c0 * ld + c0, ld);
    if (c2 < CE)  // block below the diagonal inside the super-panel: part of the K range
      launch_zero_block(st, Y + c2 * ld + c0, ld, CE - c2, PANEL);
    if (c0 > 0) {
      GemmGrid gtri = chain_grid(h);  // Dp is lower triangular: the first tile column only needs k < 128
      gtri.ktri = h->ktri;
      launch_gemm_nt(st, GEMM_RECT, (int)(c0 / TILE), 2, PANEL, 1.0, R + c0, ld, Dp, PANEL, 0.0,
                      Y + c0, ld, pf, &gtri);
    }
    if (c2 < CE) {  // the Cholesky chain's grouping of the updates inside a super-panel
      const InnerGroup g = inner_group(q, c2, CE);
      GemmGrid gch = chain_grid(h);
      if (h->krag) gch.krag0 = (int)(g.k0 / TILE);  // rows >= k0 of Y[:, k0:c2] are zero left of their diagonal tile
      launch_gemm_nt(st, GEMM_RECT, (int)(c2 / TILE), (int)((g.ce - c2) / TILE), (int64_t)g.grp * PANEL,
                      -1.0, Y + g.k0, ld, L + c2 * ld + g.k0, ld, 1.0, R + c2, ld, pf, &gch);
    }
  }
  order(h, EV_BASE + 4 * P0 + 2, st, s2);  // column panels P0.. of Y are final
  const int nt = (int)((npad - CE) / TILE);
  if (nt > 0) {
    const int64_t Kw = CE - C0;
    const int mr = (int)(CE / TILE);
    const int ntn = nt < 2 * P.next_nsub ? nt : 2 * P.next_nsub;  // next super-panel's columns
    // The next super-step's columns stay on the CHAIN stream (as in the Cholesky sweep: no
    // event hop on the chain); they were last touched by the previous super-step's bulk update.
    if (P0 > 0 && st != s2)
      (void)gogp::rec_stream_wait(st, ev(h, EV_BASE + 4 * P.prevP0 + 3));
    // The super-panel of Y is upper triangular in its own block rows C0 .. CE: tile row C0/128 + i only sums
    // k >= i * 128 (krag0) -- half of the K range of those rows, 0.1 TFLOP of an N = 16384 evaluation that is
    // no longer launched (4.58 -> 4.50 TFLOP; the evaluation's time does not move: 71.43 -> 71.35 ms, the
    // inverse's bulk stream has that much slack behind its chain).
    GemmGrid gch = chain_grid(h), gbulk;
    if (h->krag) gch.krag0 = gbulk.krag0 = (int)(C0 / TILE);
    launch_gemm_nt(st, GEMM_RECT, mr, ntn, Kw, -1.0, Y + C0, ld, L + CE * ld + C0, ld, 1.0,
                    R + CE, ld, pf, &gch);
    if (nt > ntn) {
      const int64_t C3 = CE + (int64_t)ntn * TILE;
      launch_gemm_nt(s2, GEMM_RECT, mr, nt - ntn, Kw, -1.0, Y + C0, ld, L + C3 * ld + C0, ld, 1.0,
                      R + C3, ld, pf, &gbulk);
    }
    (void)gogp::rec_event_record(ev(h, EV_BASE + 4 * P0 + 3), s2);  // bulk R update of super-step P0 done
  }
}

// ---- mixed gradient (option "gradient_precision" = 32 on an fp64 handle) --------------------------------------------
// The factorisation, LML, alpha and Produce stay fp64.  What only the gradient needs -- Y = L^-T and K^-1 = Y Y^T,
// two thirds of an evaluation's flops -- runs on the fp32 tile kernel from a float copy of L, in float buffers of its
// own.  The reference checks its gradient to 1e-4 (gp_test.go:170,248); an optimiser that tolerates a gradient good to
// ~1e-5 gets evaluations beyond the native-fp64 roof (BASELINE.md section 3 names exactly this lever).  Never the
// default and never the bench's `value`.
static inline bool mixed_gradient(const gogp_handle *h) {
  return h->grad_prec == 32 && h->prec == 64 && !h->batch_mode && !h->dist;
}
static int ensure_g32(gogp_handle *h) {
  const int64_t cap = std::max(h->npad, h->cap_npad);
  if (h->g32A && h->g32_cap >= cap) return GOGP_OK;
  (void)hipFree(h->g32A);
  (void)hipFree(h->g32L);
  (void)hipFree(h->g32Y);
  (void)hipFree(h->g32D);
  h->g32A = h->g32L = h->g32Y = h->g32D = nullptr;
  h->g32_cap = 0;
  const size_t nn = (size_t)cap * (size_t)cap * sizeof(float);
  HIPCHK(h, hipMalloc(&h->g32A, nn));
  HIPCHK(h, hipMalloc(&h->g32L, nn));
  HIPCHK(h, hipMalloc(&h->g32Y, nn));
  HIPCHK(h, hipMalloc(&h->g32D, (size_t)(cap / PANEL) * PANEL * PANEL * sizeof(float)));
  h->g32_cap = cap;
  return GOGP_OK;
}
// one super-step of the inverse in float: float copies of the super-panel of L (rows C0.., its columns) and of its
// block inverses, then the same launches as the fp64 sweep on the fp32 tile kernel
static void mixed_superstep(gogp_handle *h, const SuperPanel &P, hipStream_t st, hipStream_t s2) {
  const int64_t npad = h->npad, ld = npad, C0 = P.C0(), W = P.CE() - C0;
  launch_convert_block(st, h->bufL + C0 * ld + C0, ld, h->g32L + C0 * ld + C0, ld, (int)(npad - C0), (int)W);
  launch_convert_block(st, h->Dinv + (size_t)P.P0 * PANEL * PANEL, PANEL, h->g32D + (size_t)P.P0 * PANEL * PANEL, PANEL,
                       (int)W, PANEL);
  const InvBufs<float> B{h->g32A, h->g32Y, h->g32L, h->g32D};
  trtri_superstep<float>(h, B, P, st, s2);
}

// K^-1 = Y Y^T = sum over the column panels of Y, right behind the super-step that made columns C0 .. CE of Y: the
// rank-(CE - C0) update K^-1[0:CE, 0:CE] (+)= Y[0:CE, C0:CE] Y[0:CE, C0:CE]^T on the lower tiles of A (block rows
// C0.. are new: overwritten).  That corner of A is dead (panels < CE of L are final) and
// disjoint from R.  The updates wait for nothing but their panel of Y and grow towards the
// end of the sweep, where the two chains leave most of the GPU idle: lowest priority.
template <class T>
static void kinv_accumulate(gogp_handle *h, const T *Y, T *A, int64_t C0, int64_t CE) {
  (void)gogp::rec_stream_wait(h->sk, ev(h, EV_BASE + 4 * (size_t)(C0 / PANEL) + 2));
  GemmGrid gk;
  gk.new_row0 = (int)(C0 / TILE);
  if (h->krag) gk.krag0 = (int)(C0 / TILE);
  launch_gemm_nt(h->sk, GEMM_LOWER, (int)(CE / TILE), (int)(CE / TILE), CE - C0, 1.0, Y + C0, h->npad, Y + C0, h->npad,
                 1.0, A, h->npad, &h->prof, &gk);
}

// R of the triangular inverse := 0: the strictly upper block triangle of bufA, or of the mixed gradient's float buffer
template <class T>
static void zero_inverse_rhs(gogp_handle *h, bool mixed, hipStream_t s) {
  if (mixed)
    launch_zero_upper_blocks(s, h->g32A, h->npad, h->npad);
  else
    launch_zero_upper_blocks(s, reinterpret_cast<T *>(h->bufA), h->npad, h->npad);
}
// one super-step of the inverse in the handle's own buffers or the mixed gradient's (chain on st, bulk updates on s2),
// with fuse_kinv its panel's share of K^-1 behind it
template <class T>
static void inverse_superstep(gogp_handle *h, bool mixed, const SuperPanel &P, hipStream_t st, hipStream_t s2,
                              bool fuse_kinv) {
  if (mixed) {
    mixed_superstep(h, P, st, s2);
    if (fuse_kinv) kinv_accumulate<float>(h, h->g32Y, h->g32A, P.C0(), P.CE());
  } else {
    const InvBufs<T> B{reinterpret_cast<T *>(h->bufA), reinterpret_cast<T *>(h->bufY), reinterpret_cast<const T *>(h->bufL),
                       reinterpret_cast<const T *>(h->Dinv)};
    trtri_superstep<T>(h, B, P, st, s2);
    if (fuse_kinv) kinv_accumulate<T>(h, B.Y, B.A, P.C0(), P.CE());
  }
}

// ---- option "chain_split" (fp64): the form of the Cholesky chain per 256-panel ----------------------------------------
// 0: the 256-block kernel factors and inverts the diagonal block on one compute unit, then a K = 256 panel solve on the
// tile kernel.  2: the chain per 128 columns is ONE launch (panel128.hip: every workgroup factors the diagonal 128-block
// redundantly and forward-substitutes its own 64 panel rows on the way: no block inverse and no solve launch on the
// chain); the 256 x 256 block inverses are formed off the chain from the finished factor (Sweep::panels_final).
// -1 (default): 2 where the evaluation is latency-bound (npad <= 8192) and wherever no inverse runs beside the
// factorisation (Absorb, eager = 0); 0 above that size beside the inverse, where the GPU is throughput-bound and the
// redundant factorisations of form 2 cost more than its shorter chain saves.  Measured (tools/split_probe.py, DESIGN.md
// "The chain step in one launch"): Observe + Gradient 0 -> 2 N = 1024 0.89 -> 0.66 ms, 4096 3.48 -> 3.07, 16384 70.4 ->
// 73.1; Observe only 4096 3.25 -> 2.46, 16384 32.9 -> 30.0.  (Not for the mixed gradient above that size: its LML is
// promised to be the native path's bit for bit.)
static inline int chain_split_of(const gogp_handle *h, bool eager) {
  if (h->dist || h->prec != 64) return 0;
  if (h->chain_split >= 0) return h->chain_split;
  return (h->npad <= 8192 || !eager) ? 2 : 0;
}
// chain_split = 2: panel128 (half 0) -> A[c1:, c1:c2] -= L[c1:, c0:c1] L[c1:c2, c0:c1]^T (tile kernel) -> panel128 (half 1)
static void fused_panel(gogp_handle *h, hipStream_t sp, double *A, double *L, int64_t ld, int64_t c0, int64_t npad,
                        GemmProfile *pf) {
  const int64_t c1 = c0 + TILE, c2 = c0 + PANEL;
  const int mt1 = (int)((npad - c1) / TILE);
  const GemmGrid gch = chain_grid(h);
  launch_panel128_slabs(sp, A + c0 * ld + c0, ld, L + c0 * ld + c0, ld, 0, npad - c1, c0, h->n, h->info, h->chain_slabs);
  launch_gemm_nt(sp, GEMM_RECT, mt1, 1, TILE, -1.0, L + c1 * ld + c0, ld, L + c1 * ld + c0, ld, 1.0, A + c1 * ld + c1, ld,
                 pf, &gch);
  launch_panel128_slabs(sp, A + c0 * ld + c0, ld, L + c0 * ld + c0, ld, 1, npad - c2, c0, h->n, h->info, h->chain_slabs);
}

// ---- what every evaluation starts and ends with -------------------------------------------------------------------------
// Entry of an evaluation that makes a new factor: `streams` -- the ones that write L, Dinv and bufA first -- wait for
// what a previous evaluation left running, and everything the handle says about the old factor is reset, here only.
static void begin_evaluation(gogp_handle *h, std::initializer_list<hipStream_t> streams) {
  auto wait = [&](int e) {
    for (hipStream_t q : streams) (void)gogp::rec_stream_wait(q, ev(h, e));
  };
  if (h->trtri_pending) wait(EV_TRTRI);  // a previous Observe left its triangular inverse running: it reads L / Dinv
  if (h->kinv_pending) wait(EV_KINV);    // ... and K^-1 accumulating in bufA
  // ... or the first of K^-1's two launches (option "kinv_split") that no Gradient picked up
  if (h->kinv_c1 > 0 && !h->have_kinv) wait(EV_KINV);
  h->trtri_pending = h->kinv_pending = false;
  h->factored = h->have_alpha = h->have_kinv = h->grad_valid = false;
  h->alpha_pending = h->trtri_done = h->ydone_valid = h->d64_active = false;
  h->notpd = -1;
  h->kinv_c1 = 0;
  // A batched evaluation factors in its arena and gets EvalState back afterwards: what was solved on the handle's own
  // factor, a Laplace fit in the handle's own buffers and Produce's T^-1 stay as they are (none is part of EvalState).
  if (h->batch_mode) return;
  h->multi_solved = false;
  h->basis_solved = false;
  h->lap_observed = h->lap_grad_valid = false;  // a new factor replaces a Laplace fit's (gogp_laplace_observe sets them behind its own)
  h->tinv_valid = false;  // Produce assembles T^-1 of the new factor on its first call
}
// the factorisation's scalars and its pivot word on their way to the pinned row(s) that judge_scalars reads
static hipError_t enqueue_result_scalars(gogp_handle *h, hipStream_t s) {
  const hipError_t e = cand_d2h(h, h->hscal, h->scalars, 7 * sizeof(double), s);
  return e != hipSuccess ? e : cand_d2h(h, h->hscal + HS_INFO, h->info, sizeof(long long), s);
}

// dst = L^-1 w (fwd) / L^-T src (bwd) on stream q, one step per 256-panel.  The steps use up w; bwd copies src there first.
template <class T>
static void substitute_fwd(gogp_handle *h, hipStream_t q, const T *L, const T *Dinv, double *w, double *dst) {
  const int npanel = (int)(h->npad / PANEL);
  for (int b = 0; b < npanel; ++b) launch_trsv_fwd_step(q, L, h->npad, Dinv, b, npanel, w, dst);
}
template <class T>
static hipError_t substitute_bwd(gogp_handle *h, hipStream_t q, const T *L, const T *Dinv, const double *src, double *w,
                                 double *dst) {
  const int npanel = (int)(h->npad / PANEL);
  const hipError_t e = hipMemcpyAsync(w, src, (size_t)h->npad * sizeof(double), hipMemcpyDeviceToDevice, q);
  for (int b = npanel - 1; b >= 0 && e == hipSuccess; --b) launch_trsv_bwd_step(q, L, h->npad, Dinv, b, npanel, w, dst);
  return e;
}

// ---- the sweep in stages ---------------------------------------------------------------------------------------------------
// What the stages of one factorize_t share: the matrices in the handle's element type, the streams, and what the options
// choose.  The stages stand in the order they enqueue; factorize_t below them is the algorithm.
template <class T>
struct Sweep {
  static constexpr bool fp32 = sizeof(T) == 4;
  gogp_handle *h;
  bool eager;  // the triangular inverse runs behind the sweep, on st and s2 (needs lookahead)
  T *A = reinterpret_cast<T *>(h->bufA), *L = reinterpret_cast<T *>(h->bufL), *Dinv = reinterpret_cast<T *>(h->Dinv);
  int64_t npad = h->npad, ld = npad;
  int npanel = (int)(npad / PANEL);
  GemmProfile *pf = &h->prof;
  hipStream_t s = h->s, st = h->st, s2 = h->s2;
  hipStream_t sp = h->lookahead ? h->sp : h->s;  // without lookahead everything runs in order on the main stream
  // The forward substitution z = L^-1 y needs each panel once it is final and nothing
  // needs z before the end: it runs on the low-priority stream, off the chain.
  hipStream_t sz = h->lookahead ? h->sl : sp;
  bool mixed = !fp32 && mixed_gradient(h);
  // option "kinv_fused": -1 (default) fuses up to npad = 10240 (measured: N = 1024 .. 8192 5-10 % faster,
  // N = 16384 1.7 % slower than one LAUUM launch over the finished Y, which runs at the longest K)
  // (the mixed gradient fuses at every size: its rank-k updates are fp32 and fill CUs the fp64 Cholesky chain leaves
  // idle -- N = 16384: 52.2 -> 51.1 ms)
  bool fuse_kinv = eager && (h->kinv_fused < 0 ? (npad <= 10240 || mixed) : h->kinv_fused != 0);
  int split = fp32 ? 0 : chain_split_of(h, eager);  // the form of the chain: 0 or 2

  // fp32 path, option "diag_fp64": blocks first .. first + nblk - 1 of the fp64 strip := those of the float matrix, widened
  void d64_init(hipStream_t q, int first, int nblk) const {
    if constexpr (fp32)
      launch_widen_diag_blocks(q, A + (int64_t)first * PANEL * (ld + 1), ld, h->D64 + (size_t)first * PANEL * PANEL, nblk);
  }
  // ... -= their rows of L[:, k0 : k0 + K] times themselves (float operands, fp64 sums); nothing without the option
  void d64_update(hipStream_t q, int64_t k0, int64_t K, int first, int nblk) const {
    if constexpr (fp32) {
      if (h->d64_active)
        launch_diag_syrk_f64(q, L + (int64_t)first * PANEL * ld + k0, ld, K, h->D64 + (size_t)first * PANEL * PANEL, nblk);
    }
  }

  // The Gram matrix into A, the fp64 strip of its diagonal blocks, and R := 0 for the inverse behind the sweep
  int build_gram() const {
    // the panel stream joins whatever the main stream still holds from the previous call
    // (bufA's last readers) and the parameter upload
    if (sp != s) order(h, EV_ENTRY, s, sp);
    HIPCHK(h, cand_memset(h, h->info, sizeof(long long), sp));
    const int w0 = superpanel_width(h, npanel, 0);
    // Gram matrix: the first super-panel's block columns on the panel stream -- the chain
    // starts ~30 us later instead of after the whole 0.5 ms build -- the rest on the main stream
    {
      AuxTimer tm(h, GOGP_PROF_GRAM, s);  // the main-stream part: all but the first block columns
      launch_gram_lower_split(sp, s, h->devP, h->D, h->dX, h->n, npad, A, ld, (int64_t)w0 * PANEL, h->ev());
      // a Laplace observe in progress: B = I + diag(sw) K diag(sw), right behind each part on its own stream
      if constexpr (!fp32) {
        if (h->lap_sw) launch_lap_scale_gram(sp, s, A, ld, h->n, npad, h->lap_sw, (int64_t)w0 * PANEL);
        // per-observation noise variances: A_ii += v_i, each part behind the Gram launch that wrote its columns
        if (h->nv_set) launch_nv_diag_add(sp, s, A, ld, h->n, h->nv, (int64_t)w0 * PANEL);
      }
    }
    // fp32 path, option "diag_fp64": the diagonal blocks leave the float matrix here -- widened once, every later
    // contribution summed in fp64 (diagsyrk.hip); the first super-panel's on the chain stream, the rest behind the build
    h->d64_active = fp32 && h->diag_fp64 != 0;
    if (h->d64_active) {
      const int rc = ensure_d64(h);
      if (rc != GOGP_OK) return rc;
      d64_init(sp, 0, w0);
      if (npanel > w0) d64_init(s, w0, npanel - w0);
    }
    (void)gogp::rec_event_record(ev(h, EV_GRAM), s);  // the whole lower triangle is written (s after sp's part
                                              // is NOT implied: consumers of columns < 512 are on sp)
    if (eager) {
      // R := 0 on the strictly upper block triangle (after whatever used bufA last)
      (void)gogp::rec_stream_wait(s2, ev(h, EV_GRAM));
      (void)gogp::rec_stream_wait(st, ev(h, EV_GRAM));
      zero_inverse_rhs<T>(h, mixed, s2);
      order(h, EV_INIT, s2, st);  // st also writes R (updates inside a super-panel)
    }
    return GOGP_OK;
  }

  // The dependency chain of one super-panel, in 256-wide steps: diagonal block, panel solve, updates inside it
  void chain_superpanel(const SuperPanel &P) const {
    const int64_t CE = P.CE();
    for (int q = 0; q < P.nsub; ++q) {
      const int p = P.P0 + q;
      const int64_t c0 = (int64_t)p * PANEL, c2 = c0 + PANEL;
      if constexpr (!fp32) {
        if (split) fused_panel(h, sp, A, L, ld, c0, npad, pf);
      }
      if (!split) {
        T *Dp = Dinv + (size_t)p * PANEL * PANEL;
        // 256x256 diagonal block: factor + dense inverse, one workgroup
        diag_block(h, sp, A + c0 * ld + c0, ld, L + c0 * ld + c0, ld, Dp, c0);
        // L[c2:, c0:c2] = A[c2:, c0:c2] * inv(L_pp)^T   (one K=256 GEMM)
        const int mt2 = (int)((npad - c2) / TILE);
        if (mt2 > 0) {
          GemmGrid gtri = chain_grid(h);  // Dp is lower triangular: the first tile column only needs k < 128
          gtri.ktri = h->ktri;
          launch_gemm_nt(sp, GEMM_RECT, mt2, 2, PANEL, 1.0, A + c2 * ld + c0, ld, Dp, PANEL, 0.0,
                          L + c2 * ld + c0, ld, pf, &gtri);
        }
      }
      if (c2 < CE) {
        // fp32 path: the rest of the super-panel's diagonal blocks take this panel's contribution in fp64
        d64_update(sp, c0, PANEL, p + 1, (int)((CE - c2) / PANEL));
        // The updates inside the super-panel (inner_group), each column from its own diagonal block down (the
        // blocks above belong to R of the fused triangular inverse) -- one trapezoid launch.
        const InnerGroup g = inner_group(q, c2, CE);
        const GemmGrid gch = chain_grid(h);
        launch_gemm_nt(sp, GEMM_TRAP, (int)((npad - c2) / TILE), (int)((g.ce - c2) / TILE),
                        (int64_t)g.grp * PANEL, -1.0, L + c2 * ld + g.k0, ld, L + c2 * ld + g.k0, ld, 1.0,
                        A + c2 * ld + c2, ld, pf, &gch);
      }
    }
  }

  // Panels P0 .. P0+nsub-1 of L are final: off the chain, chain form 2's block inverses and the substitution's steps
  void panels_final(const SuperPanel &P) const {
    order(h, EV_BASE + 4 * P.P0, sp, s);
    if (sz != sp) (void)gogp::rec_stream_wait(sz, ev(h, EV_BASE + 4 * P.P0));
    if constexpr (!fp32) {
      if (split) {
        // the inverses of the super-panel's diagonal blocks, off the chain: the substitution steps right below and the
        // triangular inverse (st) are their first readers
        launch_dinv256_blocks(sz, L + (int64_t)P.P0 * PANEL * (ld + 1), ld, Dinv + (size_t)P.P0 * PANEL * PANEL, P.nsub);
        if (eager) {
          (void)gogp::rec_event_record(ev(h, EV_BASE + 5 * (size_t)npanel + 32 + (size_t)P.P0), sz);
          (void)gogp::rec_stream_wait(st, ev(h, EV_BASE + 5 * (size_t)npanel + 32 + (size_t)P.P0));
        }
      }
    }
    for (int q = 0; q < P.nsub; ++q) launch_trsv_fwd_step(sz, L, ld, Dinv, P.P0 + q, npanel, h->w, h->z);
  }

  // The super-panel's rank-(nsub*256) update of the trailing matrix
  void trailing_update(const SuperPanel &P) const {
    const int64_t C0 = P.C0(), CE = P.CE();
    const int mtE = (int)((npad - CE) / TILE);
    if (mtE <= 0) return;
    const int64_t Kw = CE - C0;
    const int ntn = mtE < 2 * P.next_nsub ? mtE : 2 * P.next_nsub;
    // The next super-panel's block columns, each from its diagonal block down, stay on the
    // CHAIN stream: the critical path (diag -> panel solve -> these updates -> diag) then
    // never crosses streams (two event hops of ~15 us per super-panel otherwise).  They
    // only wait for the previous super-panel's bulk update of these columns, which in
    // steady state finished long ago.
    (void)gogp::rec_stream_wait(sp, ev(h, P.P0 > 0 ? EV_BASE + 4 * P.prevP0 + 1 : EV_GRAM));
    // ONE trapezoid launch for all of them (rows CE.., columns CE .. CE + ntn*128, the
    // strictly upper 256-blocks -- R of the triangular inverse -- skipped): separate
    // launches would run one after the other on this in-order stream
    const GemmGrid gch = chain_grid(h);
    launch_gemm_nt(sp, GEMM_TRAP, mtE, ntn, Kw, -1.0, L + CE * ld + C0, ld, L + CE * ld + C0, ld,
                    1.0, A + CE * ld + CE, ld, pf, &gch);
    // fp32 path: ... and so do the next super-panel's diagonal blocks, in fp64 (diagsyrk.hip)
    d64_update(sp, C0, Kw, (int)(CE / PANEL), ntn / 2);
    // the rest of the trailing matrix, lower tiles only (main stream)
    if (mtE > ntn) {
      const int64_t C3 = CE + (int64_t)ntn * TILE;
      launch_gemm_nt(s, GEMM_LOWER, mtE - ntn, mtE - ntn, Kw, -1.0, L + C3 * ld + C0, ld,
                      L + C3 * ld + C0, ld, 1.0, A + C3 * ld + C3, ld, pf);
      d64_update(s, C0, Kw, (int)(C3 / PANEL), (mtE - ntn) / 2);
    }
    (void)gogp::rec_event_record(ev(h, EV_BASE + 4 * P.P0 + 1), s);  // bulk update of super-panel P0 done
  }

  // The fused sweep: the same super-step of the triangular inverse right behind, and K^-1 behind that
  void inverse_behind(const SuperPanel &P) const {
    const int64_t CE = P.CE();
    (void)gogp::rec_stream_wait(st, ev(h, EV_BASE + 4 * P.P0));
    inverse_superstep<T>(h, mixed, P, st, s2, fuse_kinv);
    if (!fp32 && !fuse_kinv && !mixed && !h->batch_mode && h->kinv_split > 0 && h->kinv_c1 == 0 && CE < npad &&
        CE * 100 >= npad * (int64_t)h->kinv_split) {
      // ---- option "kinv_split" (sizes above the fused ones): the part of K^-1 = Y Y^T that the finished column
      // panels of Y determine -- K^-1[0:CE, 0:CE] = sum over k < CE -- as ONE ragged-K launch now, at the lowest
      // priority, into the dead corner of bufA (as the fused updates: kinv_accumulate); Gradient's launch then only
      // sums k >= CE on top of it, in the same order of k: bit-identical.  N = 16384, alternating runs on one box:
      // 71.98-72.19 ms without, 71.65-71.85 with 60 % (50 %: 71.8, 30-40 %: 72.0, 80 %: 71.75, 90 %: 72.2);
      // N = 32768: no difference (547.5 / 550.7 against 550.0 / 547.6).
      (void)gogp::rec_stream_wait(h->sk, ev(h, EV_BASE + 4 * P.P0 + 2));
      const T *Y0 = reinterpret_cast<const T *>(h->bufY);
      launch_gemm_nt(h->sk, GEMM_LAUUM, (int)(CE / TILE), (int)(CE / TILE), CE, 1.0, Y0, ld, Y0, ld, 0.0, A, ld, pf);
      (void)gogp::rec_event_record(ev(h, EV_KINV), h->sk);
      h->kinv_c1 = CE;
    }
  }

  // alpha = K^-1 y, one of three ways, around the result scalars' copies to the host: the refinement's scalar goes
  // with them, the other two ways are not needed for the LML and follow them
  int finish_alpha() const {
    if (fp32) {
      // fp32 path: alpha by substitution with the fp32 factor, then `refine_steps` steps of
      // iterative refinement against the EXACT Gram matrix (recomputed in fp64 on the fly, never
      // read back from its rounded copy): r = y - K alpha, alpha += K~^-1 r.  The quadratic term of
      // the LML is y^T alpha of the refined alpha (fp64).  All of it on the chain stream, which is
      // idle after the last panel; the triangular inverse keeps running on its own streams.
      if (sz != sp) (void)gogp::rec_stream_wait(sp, ev(h, EV_FWD));
      HIPCHK(h, substitute_bwd(h, sp, L, Dinv, h->z, h->w, h->alpha));
      for (int it = 0; it < h->refine_steps; ++it) {
        launch_residual(sp, h->devP, h->D, h->dX, h->n, npad, h->alpha, h->dy, h->rpart, REFINE_SLABS, h->rw,
                        h->radial1, h->ev());
        substitute_fwd(h, sp, L, Dinv, h->rw, h->rz);
        HIPCHK(h, substitute_bwd(h, sp, L, Dinv, h->rz, h->rw, h->rd));
        launch_axpy(sp, h->alpha, h->rd, npad);
      }
      launch_dot(sp, h->dy, h->alpha, h->n, h->scalars + 6);
      order(h, EV_ALPHA, sp, s);
    }
    HIPCHK(h, enqueue_result_scalars(h, s));
    if (fp32) {
      if (eager) (void)gogp::rec_event_record(ev(h, EV_TRTRI), st);
    } else if (eager && !mixed) {
      // alpha = K^-1 y = Y (L^-1 y) = Y z: one bandwidth-bound pass over Y once the
      // triangular inverse is complete (st), instead of 64 dependent substitution steps
      (void)gogp::rec_stream_wait(st, ev(h, EV_FWD));
      launch_alpha_from_y(st, reinterpret_cast<const T *>(h->bufY), ld, h->z, npad, h->alpha);
      (void)gogp::rec_event_record(ev(h, EV_ALPHA), st);
      (void)gogp::rec_event_record(ev(h, EV_TRTRI), st);
    } else {
      // backward substitution alpha = L^-T z on the panel stream: not needed for LML
      if (sz != sp) (void)gogp::rec_stream_wait(sp, ev(h, EV_FWD));
      HIPCHK(h, substitute_bwd(h, sp, L, Dinv, h->z, h->w, h->alpha));
      (void)gogp::rec_event_record(ev(h, EV_ALPHA), sp);
    }
    return GOGP_OK;
  }
};

// Right-looking blocked Cholesky in super-panels of SW 256-wide panels: the
// dependency chain (diagonal blocks, panel solves, updates inside the
// super-panel) runs on the panel stream with 256-wide steps; the trailing
// matrix gets ONE rank-(SW*256) update per super-panel on the main stream
// (next super-panel's block columns first: look-ahead).
template <class T>
static int factorize_t(gogp_handle *h, bool eager) {
  const Sweep<T> c{h, eager && h->lookahead != 0};
  begin_evaluation(h, {c.s, c.sp});
  int rc = gogp_upload_params(h);
  if (rc == GOGP_OK && (c.mixed || c.eager)) rc = c.mixed ? ensure_g32(h) : ensure_y(h);
  if (rc == GOGP_OK) rc = c.build_gram();
  if (rc != GOGP_OK) return rc;
  if (c.fp32) HIPCHK(h, hipMemsetAsync(h->scalars + 5, 0, sizeof(double), c.sp));  // fp64 logdet
  // working copy of y for the forward substitution, whose steps follow the chain on sz
  // (a Laplace observe: of its Newton step's right-hand side)
  HIPCHK(h, cand_copy_in(h, h->w, h->lap_rhs ? h->lap_rhs : h->dy, (size_t)c.npad * sizeof(double), c.sp));
  if (c.sz != c.sp) order(h, EV_W, c.sp, c.sz);
  for (const SuperPanel &P : superpanels(h)) {
    c.chain_superpanel(P);
    c.panels_final(P);
    c.trailing_update(P);
    if (c.eager) c.inverse_behind(P);
  }
  if (c.fuse_kinv) {
    (void)gogp::rec_event_record(ev(h, EV_KINV), h->sk);
    h->kinv_pending = true;
  }
  if (c.eager) {
    (void)gogp::rec_event_record(ev(h, EV_TRTRI), c.st);
    (void)gogp::rec_event_record(ev(h, EV_YDONE), c.st);  // K^-1 = Y Y^T may start here; alpha = Y z (finish_alpha) runs beside it
    h->ydone_valid = h->trtri_done = h->trtri_pending = true;
  }
  order(h, EV_FWD, c.sz, c.s);  // z complete
  launch_lml_scalars(c.s, c.L, c.ld, h->z, nullptr, nullptr, h->n, h->scalars);
  rc = c.finish_alpha();
  if (rc != GOGP_OK) return rc;
  const int rcf = finish_factorize(h, c.fp32, c.fp32, false);  // the fp32 path's alpha is the refined one
  if (rcf == GOGP_ENOTPD)  // nothing of the failed factorisation may still run on the other streams
    for (hipStream_t q : {c.sp, c.st, c.s2, h->sl, h->sk}) (void)hipStreamSynchronize(q);
  return rcf;
}

// ---- option "tiny" (default on): N <= 128 observations, the whole factorisation in ONE launch (diag256.hip: tiny_eval_kernel)
// The reference's own case studies have 20 .. 44 observations (tutorial/data/*.csv); the general sweep is then a chain of
// ~15 dependent launches (0.34 ms per Observe at N = 64, 30 us of it arithmetic).  Everything the later calls read is left
// where the general path leaves it -- L, the block inverse, z, alpha, K^-1 (Observe) -- so Gradient, Produce, the factor
// export and the lazy inverse after Absorb run unchanged; only Y = L^-T is not formed (nobody needs it once K^-1 exists).
static inline bool tiny_ok(const gogp_handle *h) {
  // (tiny_eval_kernel builds its own Gram matrix: a handle with noise variances takes the general sweep)
  return h->tiny && !h->dist && h->prec == 64 && h->npad == PANEL && h->n <= TILE && !mixed_gradient(h) && !h->nv_set;
}
static int tiny_factorize(gogp_handle *h, bool eager) {
  hipStream_t s = h->s;
  begin_evaluation(h, {s});
  int rc = gogp_upload_params(h);
  if (rc != GOGP_OK) return rc;
  // whatever the chain / substitution streams still hold from a previous general-path call (the backward substitution of
  // an Absorb reads L and Dinv) comes first
  // (not inside a candidates call: its previous call joined every stream into the main one, and a captured sequence may
  // not wait for work outside the capture)
  if (h->lookahead && !h->batch_mode) {
    order(h, EV_ENTRY, h->sp, s);
    order(h, EV_W, h->sl, s);
  }
  HIPCHK(h, cand_memset(h, h->info, sizeof(long long), s));
  launch_tiny_eval(s, h->devP, h->dX, h->dy, h->n, h->bufA, h->bufL, h->Dinv, h->z, h->alpha, h->info, eager, h->ev());
  launch_lml_scalars(s, h->bufL, h->npad, h->z, nullptr, nullptr, h->n, h->scalars);
  (void)gogp::rec_event_record(ev(h, EV_ALPHA), s);
  HIPCHK(h, enqueue_result_scalars(h, s));
  return finish_factorize(h, false, false, eager);
}

static int factorize(gogp_handle *h, bool eager) {
  if (tiny_ok(h)) return tiny_factorize(h, eager && h->lookahead);
  return h->prec == 32 ? factorize_t<float>(h, eager) : factorize_t<double>(h, eager);
}

// alpha is computed by factorize() on the panel stream; make the main stream
// wait for it before anything there reads it
static int ensure_alpha(gogp_handle *h) {
  if (!h->factored || !h->have_alpha) return fail(h, GOGP_ESTATE, "no factorisation");
  if (h->alpha_pending) {
    HIPCHK(h, gogp::rec_stream_wait(h->s, ev(h, EV_ALPHA)));
    h->alpha_pending = false;
  }
  return GOGP_OK;
}

// NULL, or what is wrong with the natural parameters ts / tn
const char *gogp::theta_refusal(const gogp_handle *h, const double *ts, const double *tn) {
  for (int i = 0; i < h->ns; ++i)
    if (!(ts[i] > 0.0) || !std::isfinite(ts[i])) return "similarity parameters must be positive and finite";
  for (int i = 0; i < h->nn; ++i)
    if (!std::isfinite(tn[i])) return "noise parameter must be finite";
  return nullptr;
}

static int set_theta_natural(gogp_handle *h, const double *ts, const double *tn) {
  // validate everything first: a refused vector leaves the handle's parameters as they were
  if (const char *why = theta_refusal(h, ts, tn)) return fail(h, GOGP_EARG, why);
  for (int i = 0; i < h->ns; ++i) h->theta_s[i] = ts[i];
  for (int i = 0; i < h->nn; ++i) h->theta_n[i] = tn[i];
  h->have_theta = true;
  return GOGP_OK;
}

extern "C" int gogp_absorb(gogp_handle *h, const double *theta_simil,
                           const double *theta_noise) {
  if (!h || !theta_simil || (h->nn > 0 && !theta_noise)) return fail(h, GOGP_EARG, "absorb: NULL");
  if (!h->have_data) return fail(h, GOGP_ESTATE, "absorb: no data (gogp_set_data)");
  HIPCHK(h, hipSetDevice(h->device));
  int rc = set_theta_natural(h, theta_simil, theta_noise);
  if (rc != GOGP_OK) return rc;
  h->observed = false;  // gp/gp.go:85-86: no gradient after Absorb
  h->with_obs = false;
  h->grad_valid = false;
  h->lap_observed = h->lap_grad_valid = false;
  if (h->n == 0) {  // gp/gp.go:101-104
    h->lml = 0.0;
    h->factored = false;
    return GOGP_OK;
  }
  rc = h->dist ? gogp_dist_factorize(h, false) : factorize(h, false);
  if (rc != GOGP_OK && rc != GOGP_ECOND) return rc;
  const int rcond = rc;
  rc = ensure_alpha(h);  // gp/gp.go:232-236
  if (rc != GOGP_OK) return rc;
  HIPCHK(h, hipStreamSynchronize(h->s));
  return rcond;
}

static int observe_theta(gogp_handle *h, const double *x, double *lml) {
  // gp/gp.go:378-385: theta = exp(x)
  std::vector<double> th(h->P > 0 ? h->P : 1);
  for (int i = 0; i < h->P; ++i) th[i] = exp(x[i]);
  int rc = set_theta_natural(h, th.data(), th.data() + h->ns);
  if (rc != GOGP_OK) return rc;
  h->grad_valid = false;
  h->lap_observed = h->lap_grad_valid = false;
  if (h->n == 0) {
    h->lml = 0.0;
    h->factored = false;
    h->observed = true;
    if (lml) *lml = 0.0;
    return GOGP_OK;
  }
  rc = h->dist ? gogp_dist_factorize(h, true)
               : factorize(h, h->eager != 0);  // gp/gp.go:402 (with gradient preparation)
  if (rc != GOGP_OK && rc != GOGP_ECOND) return rc;
  h->observed = true;
  if (lml) *lml = h->lml;  // gp/gp.go:412
  return rc;
}

extern "C" int gogp_observe(gogp_handle *h, const double *x, int64_t len, double *lml) {
  if (!h || !x) return fail(h, GOGP_EARG, "observe: NULL");
  if (len != h->P) return fail(h, GOGP_EARG, "len(x)");  // gp/gp.go:398-400
  if (!h->have_data) return fail(h, GOGP_ESTATE, "observe: no data (gogp_set_data)");
  HIPCHK(h, hipSetDevice(h->device));
  h->with_obs = false;
  return observe_theta(h, x, lml);
}

extern "C" int gogp_observe_full(gogp_handle *h, const double *x, int64_t len, double *lml) {
  if (!h || !x) return fail(h, GOGP_EARG, "observe: NULL");
  if (len < h->P) return fail(h, GOGP_EARG, "len(x)");
  const int64_t rest = len - h->P;
  if (rest == 0) return gogp_observe(h, x, len, lml);
  const int64_t n = rest / (h->D + 1);  // gp/gp.go:391
  if (n * (h->D + 1) != rest) return fail(h, GOGP_EARG, "len(x)");  // gp/gp.go:398-400
  int rc = gogp_set_data(h, x + h->P, x + h->P + n * h->D, n);
  if (rc != GOGP_OK) return rc;
  h->with_obs = true;
  return observe_theta(h, x, lml);
}

extern "C" int gogp_lml(gogp_handle *h, double *lml) {
  if (!h || !lml) return GOGP_EARG;
  if (h->n == 0) {
    *lml = 0.0;
    return GOGP_OK;
  }
  if (!h->factored) return fail(h, GOGP_ESTATE, "LML: nothing absorbed");
  *lml = h->lml;
  return GOGP_OK;
}

// ---- gradient --------------------------------------------------------------------------------
template <class T>
static int compute_kinv_t(gogp_handle *h) {
  if (h->have_kinv) return GOGP_OK;
  const int64_t npad = h->npad, ld = npad;
  hipStream_t s = h->s;
  GemmProfile *pf = &h->prof;
  if (h->kinv_pending) {
    // the fused sweep accumulated K^-1 behind the triangular inverse (factorize_t): nothing to launch
    (void)gogp::rec_stream_wait(s, ev(h, EV_KINV));
    if (h->trtri_pending) (void)gogp::rec_stream_wait(s, ev(h, EV_TRTRI));
    h->kinv_pending = h->trtri_pending = false;
    h->have_kinv = true;
    return GOGP_OK;
  }
  const bool mixed = std::is_same<T, double>::value && mixed_gradient(h);
  if (!h->trtri_done) {
    // lazy path: the triangular inverse was not fused into the factorisation
    hipStream_t sp = h->lookahead ? h->sp : h->s;
    const int rcy = mixed ? ensure_g32(h) : ensure_y(h);
    if (rcy != GOGP_OK) return rcy;
    zero_inverse_rhs<T>(h, mixed, s);
    order(h, EV_INIT, s, sp);
    for (const SuperPanel &P : superpanels(h)) inverse_superstep<T>(h, mixed, P, sp, s, false);
    order(h, EV_TRTRI, sp, s);
    h->trtri_done = true;
  } else if (h->trtri_pending) {
    // Y final is enough to start; what the inverse's chain stream still does behind it (alpha = Y z, a
    // bandwidth-bound 0.2 ms at N = 16384) reads Y and writes alpha only
    (void)gogp::rec_stream_wait(s, ev(h, h->ydone_valid ? EV_YDONE : EV_TRTRI));
  }
  // K^-1 (lower tiles) = Y Y^T, ragged K range; the Cholesky work area is dead, write over it
  if (mixed) {
    launch_gemm_nt(s, GEMM_LAUUM, h->nblk, h->nblk, npad, 1.0, h->g32Y, ld, h->g32Y, ld, 0.0, h->g32A, ld, pf);
  } else {
    GemmGrid gk;
    if (h->kinv_c1 > 0) {  // the sweep launched the sums over k < kinv_c1 (factorize_t)
      (void)gogp::rec_stream_wait(s, ev(h, EV_KINV));
      gk.kbeg0 = (int)h->kinv_c1;
    }
    launch_gemm_nt(s, GEMM_LAUUM, h->nblk, h->nblk, npad, 1.0, reinterpret_cast<const T *>(h->bufY), ld,
                   reinterpret_cast<const T *>(h->bufY), ld, 0.0, reinterpret_cast<T *>(h->bufA), ld, pf, &gk);
  }
  // whatever follows on s is ordered behind ALL of the inverse's chain stream
  if (h->trtri_pending && h->ydone_valid) (void)gogp::rec_stream_wait(s, ev(h, EV_TRTRI));
  h->trtri_pending = false;
  h->have_kinv = true;
  return GOGP_OK;
}
static int compute_kinv(gogp_handle *h) {
  return h->prec == 32 ? compute_kinv_t<float>(h) : compute_kinv_t<double>(h);
}

static int64_t grad_len(const gogp_handle *h) {
  return h->with_obs ? h->P + h->n * (h->D + 1) : h->P;  // gp/gp.go:420-425
}

// d LML / d log theta from the slot sums of the fused reduction (common.h: ACC_*); out: P zeros
void gogp::assemble_gradient(const gogp_handle *h, const double *a, double dnoise, double *out) {
  const gogp_desc &d = h->desc;
  for (int t = 0; t < d.nterms; ++t) {
    const gogp_term &T = d.terms[t];
    if (T.scale_idx >= 0) out[T.scale_idx] += 0.5 * a[3 * t + 0];
    if (T.ard) {
      for (int j = 0; j < d.ndim; ++j) out[T.len_idx + j] += 0.5 * a[ACC_ARD0 + j];
    } else {
      out[T.len_idx] += 0.5 * a[3 * t + 1];
    }
    if (T.kind == GOGP_K_PERIODIC) out[T.period_idx] += 0.5 * a[3 * t + 2];
  }
  if (h->nn > 0) out[h->ns] = 0.5 * a[ACC_TRACE] * dnoise;
}

// fp32 path: two slot sums of the gradient reduction cancel badly when K is ill-conditioned -- the entries of the fp32
// K^-1 are of the size 1 / noise and the sums over W = alpha alpha^T - K^-1 are what is left of them -- and both have
// closed forms that never touch the off-diagonal of K^-1:
//   trace slot     tr(W) = |alpha|^2 - |Y|_F^2                    (fp64 sums over Y = L^-T, launch_trace_from_y)
//   scale slot     sum_ij W_ij c k_ij = tr(W (K - v I)) = (y^T alpha - n) - v tr(W)     (K alpha = y holds for the
//                  refined alpha; v: the noise variance on the diagonal) -- one radial term with an output scale.
//                  It holds with event discounts too: the discounted similarity c f d is still homogeneous of
//                  degree 1 in c, so the scale slot c d f summed against W is still tr(W (K - v I)).
// Measured on the stress case of round 3 (Matern-3/2, N = 1721, D = 2, gradient error 3.6e-3 of its largest
// component, all of it in the scale slot): tests/test_gpu_parity.py::test_fp32_gradient_ill_conditioned_case.
static void fp32_gradient_identities(const gogp_handle *h, double *a, double trace_w, double yta, double noise_var) {
  const gogp_desc &d = h->desc;
  a[ACC_TRACE] = trace_w;
  if (d.nterms == 1 && d.terms[0].scale_idx >= 0) a[0] = (yta - (double)h->n) - noise_var * trace_w;
}

// Enqueue on the main stream: the gradient's slot sums over the current K^-1 into the pinned row(s) at HS_GRAD, and with
// `trace` tr(alpha alpha^T - K^-1) in fp64 from the float Y itself (solve.hip: launch_trace_from_y) into HS_TRACE, NaN
// without.  rw (fp32 path) / w (mixed gradient: the substitution's scratch, done with) and scalars[7] are free here.
static int enqueue_grad_sums(gogp_handle *h, bool trace) {
  hipStream_t s = h->s;
  auto reduce = [&](auto *kinv) {
    AuxTimer tm(h, GOGP_PROF_GRAD, s);
    launch_grad_reduce(s, h->devP, h->D, h->ard_dims, h->dX, h->alpha, kinv, h->npad, h->n, h->npad, h->gpart, h->gout,
                       h->radial1, h->ard_mfma_min, h->ev());
  };
  if (h->prec == 32)
    reduce(reinterpret_cast<const float *>(h->bufA));
  else if (mixed_gradient(h))
    reduce((const float *)h->g32A);
  else
    reduce((const double *)h->bufA);
  HIPCHK(h, cand_d2h(h, h->hscal + HS_GRAD, h->gout, NACC * sizeof(double), s));
  h->hscal[HS_TRACE] = NAN;
  if (trace) {
    launch_trace_from_y(s, h->prec == 32 ? reinterpret_cast<const float *>(h->bufY) : (const float *)h->g32Y, h->npad, h->n,
                        h->npad, h->alpha, h->prec == 32 ? h->rw : h->w, h->scalars + 7);
    HIPCHK(h, hipMemcpyAsync(h->hscal + HS_TRACE, h->scalars + 7, sizeof(double), hipMemcpyDeviceToHost, s));
  }
  return GOGP_OK;
}

extern "C" int gogp_gradient(gogp_handle *h, double *grad, int64_t len) {
  if (!h || !grad) return fail(h, GOGP_EARG, "gradient: NULL");
  if (!h->observed) return fail(h, GOGP_ESTATE, "Gradient before Observe");
  if (len != grad_len(h)) return fail(h, GOGP_EARG, "gradient: wrong length");
  for (int64_t i = 0; i < len; ++i) grad[i] = 0.0;
  if (h->n == 0) return GOGP_OK;  // gp/gp.go:427-430
  HIPCHK(h, hipSetDevice(h->device));
  if (h->dist && h->with_obs)
    return fail(h, GOGP_EARG, "sharded evaluation: the full Observe form is not supported");
  if (h->prec == 32 && h->with_obs)
    return fail(h, GOGP_EARG, "fp32 path: the full Observe form is not supported");
  if (mixed_gradient(h) && h->with_obs)
    return fail(h, GOGP_EARG, "gradient_precision = 32: the full Observe form is not supported");
  if (!h->grad_valid && h->dist) {
    // sharded: every rank reduces its own tiles of K^-1, one all-reduce of the slot sums
    int rc = gogp_dist_gradient_sums(h, h->hscal + HS_GRAD);
    if (rc != GOGP_OK) return rc;
    // float tiles: the output-scale component from its closed form (fp32_gradient_identities); the trace slot already
    // holds |alpha|^2 - |Y|_F^2 from fp64 sums over the shards' chunks of Y (dist2d.hip: gogp_dist_gradient_sums)
    if (h->prec == 32 && h->trace_fp64)
      fp32_gradient_identities(h, h->hscal + HS_GRAD, h->hscal[HS_GRAD + ACC_TRACE], h->yta, h->hostP->noise_var);
  } else if (!h->grad_valid) {
    int rc = compute_kinv(h);
    if (rc != GOGP_OK) return rc;
    rc = ensure_alpha(h);
    if (rc != GOGP_OK) return rc;
    const bool f32k = h->prec == 32 || mixed_gradient(h);  // K^-1 and Y are float
    rc = enqueue_grad_sums(h, f32k && h->trace_fp64 && (h->prec == 32 ? h->bufY : (double *)h->g32Y) && h->trtri_done);
    if (rc != GOGP_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(h->s));
    HIPCHK(h, hipGetLastError());
    if (f32k && std::isfinite(h->hscal[HS_TRACE]))
      fp32_gradient_identities(h, h->hscal + HS_GRAD, h->hscal[HS_TRACE], h->yta, h->hostP->noise_var);
  }
  if (!h->grad_valid) {
    h->grad_cache.assign(h->P, 0.0);
    assemble_gradient(h, h->hscal + HS_GRAD, h->hostP->dnoise, h->grad_cache.data());
    h->grad_valid = true;
  }
  for (int i = 0; i < h->P; ++i) grad[i] = h->grad_cache[i];
  if (h->with_obs) {
    // gp/gp.go:118-129 (inputs) and :488-493 (outputs: -alpha)
    hipStream_t s = h->s;
    const int64_t n = h->n;
    double *gx = nullptr;
    HIPCHK(h, hipMalloc(&gx, (size_t)h->npad * h->D * sizeof(double)));
    launch_xgrad(s, h->devP, h->D, h->dX, h->alpha, h->bufA, h->npad, n, h->npad, gx, h->ev());
    hipError_t e = hipMemcpyAsync(grad + h->P, gx, (size_t)n * h->D * sizeof(double),
                                  hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
      e = hipMemcpyAsync(grad + h->P + n * h->D, h->alpha, (size_t)n * sizeof(double),
                         hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(gx);
    HIPCHK(h, e);
    for (int64_t i = 0; i < n; ++i) grad[h->P + n * h->D + i] = -grad[h->P + n * h->D + i];
  }
  return GOGP_OK;
}

// ---- leave-one-out cross-validation (loo.hip) ----------------------------------------------------------------------
// No reference counterpart (its forecast harness refits per prefix).  Both calls read the explicit K^-1 the gradient
// leaves in bufA (lower tiles) and alpha, and write only workspaces of their own: the handle's state afterwards is
// what a gogp_gradient at this point would have left -- K^-1 formed -- and nothing a later call reads has changed.
struct LooVecs {
  double *mu, *sigma, *logp, *v, *sc, *u, *zero, *part;
};
// The refusals of both calls, then -- with observations -- K^-1 and alpha ordered on the main stream and the vectors in
// place.  *empty: n == 0, nothing to launch.
static int loo_prepare(gogp_handle *h, const char *who, LooVecs *lv, bool *empty) {
  char buf[160];
  const char *refuse = h->prec == 32        ? "precision = 32 handles"
                       : mixed_gradient(h) ? "gradient_precision = 32 (a float K^-1)"
                       : h->dist           ? "sharded handles"
                                           : nullptr;
  if (refuse) {
    snprintf(buf, sizeof buf, "%s: %s are not supported", who, refuse);
    return fail(h, GOGP_EARG, buf);
  }
  *empty = h->n == 0;
  if (*empty) return GOGP_OK;
  if (!h->factored) {
    snprintf(buf, sizeof buf, "%s: nothing absorbed", who);
    return fail(h, GOGP_ESTATE, buf);
  }
  HIPCHK(h, hipSetDevice(h->device));
  int rc = compute_kinv(h);
  if (rc == GOGP_OK) rc = ensure_alpha(h);
  const size_t np = (size_t)h->npad;
  if (rc == GOGP_OK) rc = h->loo_vec.reserve(h, (7 * np + np / PANEL) * sizeof(double));
  if (rc != GOGP_OK) return rc;
  double *q = h->loo_vec.as<double>();
  *lv = LooVecs{q, q + np, q + 2 * np, q + 3 * np, q + 4 * np, q + 5 * np, q + 6 * np, q + 7 * np};
  launch_loo_stats(h->s, h->bufA, h->npad, h->alpha, h->dy, h->n, h->npad, lv->mu, lv->sigma, lv->logp, lv->v, lv->sc,
                   lv->part);
  return GOGP_OK;
}

extern "C" int gogp_loo(gogp_handle *h, double *mu, double *sigma, double *logp, double *total) {
  if (!h) return GOGP_EARG;
  LooVecs lv;
  bool empty = false;
  const int rc = loo_prepare(h, "LOO", &lv, &empty);
  if (rc != GOGP_OK) return rc;
  if (total) *total = 0.0;
  if (empty) return GOGP_OK;
  hipStream_t s = h->s;
  const size_t vec = (size_t)h->n * sizeof(double);
  std::vector<double> part((size_t)(h->npad / PANEL));
  if (mu) HIPCHK(h, hipMemcpyAsync(mu, lv.mu, vec, hipMemcpyDeviceToHost, s));
  if (sigma) HIPCHK(h, hipMemcpyAsync(sigma, lv.sigma, vec, hipMemcpyDeviceToHost, s));
  if (logp) HIPCHK(h, hipMemcpyAsync(logp, lv.logp, vec, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(part.data(), lv.part, part.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  double t = 0.0;
  for (double b : part) t += b;  // the block sums, in block order
  if (total) *total = t;
  return GOGP_OK;
}

extern "C" int gogp_loo_gradient(gogp_handle *h, double *grad, int64_t len) {
  if (!h || !grad) return fail(h, GOGP_EARG, "LOO gradient: NULL");
  if (len != h->P) return fail(h, GOGP_EARG, "LOO gradient: wrong length");
  LooVecs lv;
  bool empty = false;
  int rc = loo_prepare(h, "LOO gradient", &lv, &empty);
  if (rc != GOGP_OK) return rc;
  for (int64_t i = 0; i < len; ++i) grad[i] = 0.0;
  if (empty) return GOGP_OK;
  hipStream_t s = h->s;
  const int64_t npad = h->npad, ld = npad;
  const size_t mat = (size_t)npad * (size_t)npad;
  rc = h->loo_mat.reserve(h, 2 * mat * sizeof(double));
  if (rc != GOGP_OK) return rc;
  double *B = h->loo_mat.as<double>(), *G = B + mat;
  // B = K^-1 diag(s), u = K^-1 v (its partial sums in G, which is free until the product)
  launch_loo_scale_symv(s, h->bufA, ld, h->n, npad, lv.sc, lv.v, B, ld, G, lv.u);
  // G = B B^T - u alpha^T - alpha u^T = -2 W on the lower tiles
  launch_gemm_nt(s, GEMM_LOWER, h->nblk, h->nblk, npad, 1.0, (const double *)B, ld, (const double *)B, ld, 0.0, G, ld,
                 &h->prof);
  launch_loo_rank2(s, G, ld, h->n, npad, lv.u, h->alpha);
  // sum_ab (0 0^T - G)_ab dK_ab per slot: the reduction of the LML gradient with G for K^-1 and zeros for alpha
  HIPCHK(h, hipMemsetAsync(lv.zero, 0, (size_t)npad * sizeof(double), s));
  {
    AuxTimer tm(h, GOGP_PROF_GRAD, s);
    launch_grad_reduce(s, h->devP, h->D, h->ard_dims, h->dX, lv.zero, (const double *)G, ld, h->n, npad, h->gpart, h->gout,
                       h->radial1, h->ard_mfma_min, h->ev());
  }
  double acc[NACC];
  HIPCHK(h, hipMemcpyAsync(acc, h->gout, sizeof acc, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  assemble_gradient(h, acc, h->hostP->dnoise, grad);
  return GOGP_OK;
}

// ---- per-observation noise variances (noisevar.hip) -------------------------------------------------------------------
// K = k(X, X) + s2(theta) I + diag(v), v known per observation (no reference counterpart: gp.GP has one noise level).
// Device state only: Sweep::build_gram adds v behind the Gram build, and everything behind the factorisation -- Produce,
// the gradient, LOO, the multi-output and basis calls -- works from the factor, alpha and K^-1 and never looks at the
// diagonal of K again.  gogp_append_noisy and gogp_remove, which do rebuild diagonal entries, carry v themselves.
extern "C" int gogp_noise_variances_check(const double *v, int64_t n) {
  if (n < 0 || (n > 0 && !v)) return GOGP_EARG;
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i]) || v[i] < 0.0) return GOGP_EARG;
  return GOGP_OK;
}

// NULL, or why this handle takes no noise variances
static const char *nv_refusal(const gogp_handle *h) {
  return h->prec == 32       ? "noise variances: not supported on a precision = 32 handle"
         : mixed_gradient(h) ? "noise variances: not supported with gradient_precision = 32 (its closed-form scale "
                               "component assumes K = c F + s2 I)"
         : h->dist           ? "noise variances: not supported on a sharded handle"
                             : nullptr;
}

// h->nv holds at least `cap` doubles; a new block is zero throughout (the old contents are not kept)
static int nv_reserve(gogp_handle *h, int64_t cap) {
  if (h->nv && h->nv_cap >= cap) return GOGP_OK;
  (void)hipFree(h->nv);
  h->nv = nullptr;
  h->nv_cap = 0;
  h->nv_set = false;
  HIPCHK(h, hipMalloc(&h->nv, (size_t)cap * sizeof(double)));
  h->nv_cap = cap;
  return GOGP_OK;
}

extern "C" int gogp_set_noise_variances(gogp_handle *h, const double *v, int64_t n) {
  if (!h) return GOGP_EARG;
  const bool clear = !v && n == 0;
  if (!clear)
    if (const char *why = nv_refusal(h)) return fail(h, GOGP_EARG, why);
  if (!h->have_data) return fail(h, GOGP_ESTATE, "set_noise_variances: no data (gogp_set_data)");
  if (!clear) {
    if (n != h->n) return fail(h, GOGP_EARG, "set_noise_variances: n must be gogp_n (one variance per observation)");
    if (gogp_noise_variances_check(v, n) != GOGP_OK)
      return fail(h, GOGP_EARG, "set_noise_variances: every variance must be finite and >= 0");
  }
  HIPCHK(h, hipSetDevice(h->device));
  // nothing enqueued may still read the old variances; stored results (factor, alpha, K^-1) no longer match the matrix
  for (hipStream_t q : work_streams(h)) HIPCHK(h, hipStreamSynchronize(q));
  // (dropped first: a failed upload below leaves a handle without variances and without results, never one whose
  // results belong to other variances than it holds)
  h->factored = h->have_alpha = h->have_kinv = h->observed = h->grad_valid = false;
  h->z_valid = false;
  h->multi_solved = false;
  h->basis_solved = false;
  h->lap_observed = h->lap_grad_valid = false;
  h->trtri_done = h->trtri_pending = h->alpha_pending = h->kinv_pending = false;
  h->tinv_valid = h->tinv_pending = false;
  h->nv_set = false;
  if (clear || n == 0) return GOGP_OK;
  const int rc = nv_reserve(h, std::max(h->cap_npad, h->npad));
  if (rc != GOGP_OK) return rc;
  HIPCHK(h, hipMemsetAsync(h->nv, 0, (size_t)h->nv_cap * sizeof(double), h->s));
  HIPCHK(h, hipMemcpyAsync(h->nv, v, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->s));
  HIPCHK(h, hipStreamSynchronize(h->s));
  h->nv_set = true;
  return GOGP_OK;
}

extern "C" int gogp_get_noise_variances(gogp_handle *h, double *v) {
  if (!h) return GOGP_EARG;
  if (!h->have_data) return fail(h, GOGP_ESTATE, "get_noise_variances: no data (gogp_set_data)");
  if (h->n == 0) return GOGP_OK;
  if (!v) return fail(h, GOGP_EARG, "get_noise_variances: NULL");
  if (!h->nv_set) {
    for (int64_t i = 0; i < h->n; ++i) v[i] = 0.0;
    return GOGP_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(v, h->nv, (size_t)h->n * sizeof(double), hipMemcpyDeviceToHost, h->s));
  HIPCHK(h, hipStreamSynchronize(h->s));
  return GOGP_OK;
}

// dLML/dv_i = 1/2 (alpha_i^2 - [K^-1]_ii): the preparation and the contract of gogp_loo -- K^-1 formed, nothing a later
// call reads changed -- and one launch over the diagonal.  Holds with no variances set (the derivative at v = 0).
extern "C" int gogp_noise_variances_gradient(gogp_handle *h, double *dv) {
  if (!h) return GOGP_EARG;
  if (const char *why = nv_refusal(h)) return fail(h, GOGP_EARG, why);
  if (!h->have_data) return fail(h, GOGP_ESTATE, "noise_variances_gradient: no data (gogp_set_data)");
  if (h->n == 0) return GOGP_OK;
  if (!dv) return fail(h, GOGP_EARG, "noise_variances_gradient: NULL");
  if (!h->factored) return fail(h, GOGP_ESTATE, "noise_variances_gradient: nothing absorbed");
  HIPCHK(h, hipSetDevice(h->device));
  int rc = compute_kinv(h);
  if (rc == GOGP_OK) rc = ensure_alpha(h);
  if (rc == GOGP_OK) rc = h->nv_ws.reserve(h, (size_t)std::max(h->npad, h->cap_npad) * sizeof(double));
  if (rc != GOGP_OK) return rc;
  hipStream_t s = h->s;
  launch_nv_gradient(s, h->bufA, h->npad, h->alpha, h->n, h->nv_ws.as<double>());
  HIPCHK(h, hipMemcpyAsync(dv, h->nv_ws.p, (size_t)h->n * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  return GOGP_OK;
}

// ---- leave-block-out cross-validation (blockcv.hip) -----------------------------------------------------------------
// No reference counterpart.  The contract and the data flow of the LOO calls above, with consecutive blocks of rows
// held out together: one in-LDS factorisation per group of blocks of K^-1's diagonal, and for the gradient one
// block-diagonal right-multiplication of K^-1 ahead of LOO's own product, rank-2 correction and reduction.
extern "C" int gogp_blockcv_check(const int64_t *start, int64_t F, int64_t n) {
  if (!start || F < 0 || n < 0 || start[0] != 0) return GOGP_EARG;
  for (int64_t f = 0; f < F; ++f) {
    const int64_t len = start[f + 1] - start[f];
    if (len < 1 || len > GOGP_BLOCKCV_MAX) return GOGP_EARG;
  }
  return start[F] == n ? GOGP_OK : GOGP_EARG;
}

extern "C" int gogp_blockcv_groups(const int64_t *start, int64_t F, int64_t *first, int64_t *ngroups) {
  if (!start || !first || !ngroups || F < 0) return GOGP_EARG;
  if (gogp_blockcv_check(start, F, start[F]) != GOGP_OK) return GOGP_EARG;
  *ngroups = blockcv_pack(start, F, first);
  return GOGP_OK;
}

struct BlockCvVecs {
  double *mu, *sigma, *v, *ones, *u, *zero, *logp, *Sg;
  int64_t *bstart, *gfirst;
  int ngroups;
};
// The refusals of both calls, then -- with observations -- K^-1 and alpha ordered on the main stream, the workspaces in
// place, the group kernel run and its pivots judged (the main stream is idle on return).  *empty: n == 0.
static int blockcv_prepare(gogp_handle *h, const char *who, const int64_t *start, int64_t F, BlockCvVecs *bv, bool *empty) {
  char buf[200];
  const char *refuse = h->prec == 32        ? "precision = 32 handles"
                       : mixed_gradient(h) ? "gradient_precision = 32 (a float K^-1)"
                       : h->dist           ? "sharded handles"
                                           : nullptr;
  if (refuse) {
    snprintf(buf, sizeof buf, "%s: %s are not supported", who, refuse);
    return fail(h, GOGP_EARG, buf);
  }
  if (gogp_blockcv_check(start, F, h->n) != GOGP_OK) {
    snprintf(buf, sizeof buf,
             "%s: start must hold F + 1 strictly increasing entries from 0 to n = %lld, blocks of at most %d rows", who,
             (long long)h->n, GOGP_BLOCKCV_MAX);
    return fail(h, GOGP_EARG, buf);
  }
  *empty = h->n == 0;
  if (*empty) return GOGP_OK;
  if (!h->factored) {
    snprintf(buf, sizeof buf, "%s: nothing absorbed", who);
    return fail(h, GOGP_ESTATE, buf);
  }
  HIPCHK(h, hipSetDevice(h->device));
  int rc = compute_kinv(h);
  if (rc == GOGP_OK) rc = ensure_alpha(h);
  if (rc != GOGP_OK) return rc;
  // the tables: block starts, the groups' first blocks, then room for the groups' pivots
  std::vector<int64_t> tab((size_t)(2 * F + 3));
  int64_t *first = tab.data() + F + 1;
  for (int64_t f = 0; f <= F; ++f) tab[(size_t)f] = start[f];
  const int ng = blockcv_pack(start, F, first);
  const size_t np = (size_t)h->npad, ntab = (size_t)(F + 1) + (size_t)(ng + 1);
  rc = h->bcv_vec.reserve(h, (7 * np + ntab + (size_t)ng) * sizeof(double));
  if (rc == GOGP_OK) rc = h->bcv_s.reserve(h, (size_t)ng * 128 * 128 * sizeof(double));
  if (rc != GOGP_OK) return rc;
  double *q = h->bcv_vec.as<double>();
  int64_t *dtab = reinterpret_cast<int64_t *>(q + 7 * np);
  long long *dinfo = reinterpret_cast<long long *>(dtab + ntab);
  *bv = BlockCvVecs{q, q + np, q + 2 * np, q + 3 * np, q + 4 * np, q + 5 * np, q + 6 * np, h->bcv_s.as<double>(),
                    dtab, dtab + F + 1, ng};
  hipStream_t s = h->s;
  // v, ones, u and the zero vector: zero from row n on (the LOO passes read them over all npad rows)
  HIPCHK(h, hipMemsetAsync(bv->v, 0, 4 * np * sizeof(double), s));
  HIPCHK(h, hipMemcpyAsync(dtab, tab.data(), ntab * sizeof(int64_t), hipMemcpyHostToDevice, s));
  launch_blockcv_groups(s, h->bufA, h->npad, h->alpha, h->dy, bv->bstart, bv->gfirst, ng, bv->mu, bv->sigma, bv->v, bv->ones,
                        bv->logp, bv->Sg, dinfo);
  std::vector<long long> info((size_t)ng);
  HIPCHK(h, hipMemcpyAsync(info.data(), dinfo, (size_t)ng * sizeof(long long), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  for (int g = 0; g < ng; ++g)
    if (info[(size_t)g] != 0) {  // the first failing row: the groups are in row order
      const int64_t row = (int64_t)info[(size_t)g] - 1;
      int64_t f = first[g];
      while (start[f + 1] <= row) ++f;
      h->notpd = row;
      snprintf(buf, sizeof buf,
               "%s: block %lld (rows %lld .. %lld) of K^-1 is not positive definite (pivot at row %lld): K is numerically "
               "singular", who, (long long)f, (long long)start[f], (long long)start[f + 1] - 1, (long long)row);
      h->err = buf;
      return GOGP_ENOTPD;
    }
  return GOGP_OK;
}

extern "C" int gogp_blockcv(gogp_handle *h, const int64_t *start, int64_t F, double *mu, double *sigma, double *logp,
                            double *total) {
  if (!h) return GOGP_EARG;
  BlockCvVecs bv;
  bool empty = false;
  const int rc = blockcv_prepare(h, "block CV", start, F, &bv, &empty);
  if (rc != GOGP_OK) return rc;
  if (total) *total = 0.0;
  if (empty) return GOGP_OK;
  hipStream_t s = h->s;
  const size_t vec = (size_t)h->n * sizeof(double);
  std::vector<double> lp((size_t)F);
  if (mu) HIPCHK(h, hipMemcpyAsync(mu, bv.mu, vec, hipMemcpyDeviceToHost, s));
  if (sigma) HIPCHK(h, hipMemcpyAsync(sigma, bv.sigma, vec, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(lp.data(), bv.logp, lp.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  double t = 0.0;
  for (int64_t f = 0; f < F; ++f) {  // the blocks' log densities, in block order
    t += lp[(size_t)f];
    if (logp) logp[f] = lp[(size_t)f];
  }
  if (total) *total = t;
  return GOGP_OK;
}

extern "C" int gogp_blockcv_gradient(gogp_handle *h, const int64_t *start, int64_t F, double *grad, int64_t len) {
  if (!h || !grad) return fail(h, GOGP_EARG, "block CV gradient: NULL");
  if (len != h->P) return fail(h, GOGP_EARG, "block CV gradient: wrong length");
  BlockCvVecs bv;
  bool empty = false;
  int rc = blockcv_prepare(h, "block CV gradient", start, F, &bv, &empty);
  if (rc != GOGP_OK) return rc;
  for (int64_t i = 0; i < len; ++i) grad[i] = 0.0;
  if (empty) return GOGP_OK;
  hipStream_t s = h->s;
  const int64_t npad = h->npad, ld = npad;
  const size_t mat = (size_t)npad * (size_t)npad;
  rc = h->loo_mat.reserve(h, 2 * mat * sizeof(double));
  if (rc != GOGP_OK) return rc;
  double *B = h->loo_mat.as<double>(), *G = B + mat;
  // B = K^-1 in full (a scale vector of ones), u = K^-1 v (its partial sums in G, which is free until the product) ...
  launch_loo_scale_symv(s, h->bufA, ld, h->n, npad, bv.ones, bv.v, B, ld, G, bv.u);
  // ... B <- B blockdiag(S_g) in place, and from here on gogp_loo_gradient: G = B B^T - u alpha^T - alpha u^T = -2 W
  launch_blockcv_apply(s, B, ld, h->n, bv.bstart, bv.gfirst, bv.ngroups, bv.Sg);
  launch_gemm_nt(s, GEMM_LOWER, h->nblk, h->nblk, npad, 1.0, (const double *)B, ld, (const double *)B, ld, 0.0, G, ld,
                 &h->prof);
  launch_loo_rank2(s, G, ld, h->n, npad, bv.u, h->alpha);
  {
    AuxTimer tm(h, GOGP_PROF_GRAD, s);
    launch_grad_reduce(s, h->devP, h->D, h->ard_dims, h->dX, bv.zero, (const double *)G, ld, h->n, npad, h->gpart, h->gout,
                       h->radial1, h->ard_mfma_min, h->ev());
  }
  double acc[NACC];
  HIPCHK(h, hipMemcpyAsync(acc, h->gout, sizeof acc, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  assemble_gradient(h, acc, h->hostP->dnoise, grad);
  return GOGP_OK;
}

// ---- one evaluation of many (the candidates call, batch_eval): parameters in, results out ----------------------------
// DevParams of log parameters x (gp/gp.go:378-385: theta = exp(x)).  Unusable parameters are replaced by theta = 1 and
// reported as GOGP_EARG: that evaluation is still launched with the others, and its status says so.
static int fill_params_log(const gogp_handle *h, const double *x, DevParams &p) {
  std::vector<double> th((size_t)std::max(h->P, 1));
  for (int i = 0; i < h->P; ++i) th[(size_t)i] = exp(x[i]);
  int rc = GOGP_OK;
  if (theta_refusal(h, th.data(), th.data() + h->ns)) {
    rc = GOGP_EARG;
    std::fill(th.begin(), th.end(), 1.0);
  }
  fill_params_theta(h, th.data(), th.data() + h->ns, p);
  return rc;
}

// The status of one evaluation of n observations at parameters p from its pinned row (HS_*): its LML into *lml and,
// g != nullptr, its gradient (len entries) into g; NaN and zeros when the parameters were refused (st, fill_params_log)
// or the matrix is not positive definite.  The first failure's message goes to first_msg.
static int judge_row(const gogp_handle *h, double *row, bool fp32, int64_t n, const DevParams &p, int st,
                     const char *refused, double *lml, double *g, int64_t len, std::string &first_msg) {
  *lml = NAN;
  if (g) std::fill(g, g + len, 0.0);
  if (st != GOGP_OK) {
    if (first_msg.empty()) first_msg = refused;
    return st;
  }
  const FactorResult fr = judge_scalars(h, row, fp32, fp32, n);
  if (fr.rc != GOGP_OK && first_msg.empty()) first_msg = fr.msg;
  if (fr.rc != GOGP_ENOTPD) {
    *lml = fr.lml;
    if (fp32 && std::isfinite(row[HS_TRACE]))
      fp32_gradient_identities(h, row + HS_GRAD, row[HS_TRACE], fr.yta, p.noise_var);
    if (g) assemble_gradient(h, row + HS_GRAD, p.dnoise, g);
  }
  return fr.rc;
}

// ---- several candidates at once ---------------------------------------------------------------------
// The reference's optimiser may evaluate candidates concurrently (gonum optimize.Settings.Concurrent
// = NTASKS, tutorial/tutorial.go:30,141; infer.FuncGrad closures over independent models).  Below
// N ~ 8192 one evaluation is a chain of small dependent launches that cannot fill the GPU; k
// handles (each with its own streams and buffers, same data) driven from k host threads
// overlap their chains.
extern "C" int gogp_observe_gradient_batch(gogp_handle **hs, int k, const double *xs, int64_t len,
                                           double *lmls, double *grads, int *status) {
  if (!hs || k <= 0 || !xs || !lmls || !grads) return GOGP_EARG;
  std::vector<int> st((size_t)k, GOGP_OK);
  auto body = [&](int i) {
    int rc = gogp_observe(hs[i], xs + (size_t)i * len, len, lmls + i);
    if (rc == GOGP_OK) rc = gogp_gradient(hs[i], grads + (size_t)i * len, len);
    st[(size_t)i] = rc;
  };
  std::vector<std::thread> th;
  for (int i = 1; i < k; ++i) th.emplace_back(body, i);
  body(0);
  for (auto &t : th) t.join();
  int first = GOGP_OK;
  for (int i = 0; i < k; ++i) {
    if (status) status[i] = st[(size_t)i];
    if (first == GOGP_OK && st[(size_t)i] != GOGP_OK) first = st[(size_t)i];
  }
  return first;
}

// ---- k candidates in ONE launch sequence ------------------------------------------------------------
// The same use case with one handle: k hyper-parameter vectors on the handle's data (a line search's
// trial points, the restarts of a multi-start optimisation).  Every kernel of the fused sweep is
// launched once with the candidate index on gridDim.z (common.h: Batch): the dependent chain of one
// evaluation (16 panel steps of ~230 us at N = 4096) is paid once for all k, and the GPU that one
// chain cannot fill is filled by the others -- without the k x 5 streams of the threaded form above
// competing for the hardware queues.  Each candidate works in its own arena slot; the handle's own
// buffers and state (a previous Observe / Absorb) are left untouched.
static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
constexpr int64_t GRAPH_MAX_NPAD = 1024;           // option "graph" = 1: one chain in enqueue order
constexpr int64_t GRAPH_EXPLICIT_MAX_NPAD = 8192;  // option "graph" = 2: the sweep's dependencies as edges

// the per-candidate buffers of the arena slot at `base`; *bytes: the size of a slot
static EvalBufs cand_layout(char *base, int64_t npad, size_t esz, size_t *bytes = nullptr) {
  EvalBufs b;
  size_t o = 0;
  auto take = [&](auto *&p, size_t n) {
    p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(reinterpret_cast<uintptr_t>(base) + o);
    o += align_up(n, 256);
  };
  const size_t nn = (size_t)npad * (size_t)npad * esz;  // matrices: float on the fp32 path
  take(b.devP, sizeof(DevParams));
  take(b.info, sizeof(long long));
  take(b.scalars, 8 * sizeof(double));
  take(b.gout, NACC * sizeof(double));
  take(b.z, (size_t)npad * sizeof(double));
  take(b.w, (size_t)npad * sizeof(double));
  take(b.alpha, (size_t)npad * sizeof(double));
  take(b.gpart, (size_t)grad_reduce_blocks(npad) * NACC * sizeof(double));
  take(b.Dinv, (size_t)(npad / PANEL) * PANEL * PANEL * esz);
  take(b.bufA, nn);
  take(b.bufL, nn);
  take(b.bufY, nn);
  if (bytes) *bytes = align_up(o, 4096);
  return b;
}

static int ensure_candidates(gogp_handle *h, int k) {
  if (k > h->cand_host_k) {
    drop_cand_graph(h);  // the captured graph copies from / to these pinned blocks
    (void)hipHostFree(h->cand_hostP);
    (void)hipHostFree(h->cand_hscal);
    h->cand_hostP = nullptr;
    h->cand_hscal = nullptr;
    h->cand_host_k = 0;
    HIPCHK(h, hipHostMalloc((void **)&h->cand_hostP, (size_t)k * sizeof(DevParams), hipHostMallocDefault));
    HIPCHK(h, hipHostMalloc((void **)&h->cand_hscal, (size_t)k * BATCH_ROW * sizeof(double), hipHostMallocDefault));
    h->cand_host_k = k;
  }
  if (k > h->cand_cap_k || h->npad > h->cand_cap_npad) {
    // a captured graph holds raw pointers into the arena at the OLD stride: a new arena may come back
    // at the same address with another slot size, which the pointer comparison alone would not notice
    drop_cand_graph(h);
    (void)hipFree(h->cand_arena);
    h->cand_arena = nullptr;
    h->cand_cap_k = 0;
    h->cand_cap_npad = 0;
    const int64_t cap = std::max(h->npad, h->cand_cap_npad);
    size_t stride = 0;
    (void)cand_layout(nullptr, cap, h->esz(), &stride);
    HIPCHK(h, hipMalloc((void **)&h->cand_arena, stride * (size_t)k));
    h->cand_stride = stride;
    h->cand_cap_k = k;
    h->cand_cap_npad = cap;
  }
  return GOGP_OK;
}

static CandGraphKey cand_graph_key(const gogp_handle *h, int k) {
  return {k, h->n, h->cand_cap_npad, h->cand_stride, h->cand_arena, h->dX, h->dy, h->cand_hostP, h->cand_hscal};
}

extern "C" int gogp_observe_gradient_candidates(gogp_handle *h, int k, const double *xs, int64_t len,
                                                double *lmls, double *grads, int *status) {
  if (!h || k <= 0 || !xs || !lmls || !grads) return fail(h, GOGP_EARG, "candidates: bad arguments");
  if (k > GOGP_MAX_CANDIDATES) return fail(h, GOGP_EARG, "candidates: k > GOGP_MAX_CANDIDATES");
  if (len != h->P) return fail(h, GOGP_EARG, "len(x)");  // gp/gp.go:398-400
  if (!h->have_data) return fail(h, GOGP_ESTATE, "candidates: no data (gogp_set_data)");
  if (h->nv_set)
    return fail(h, GOGP_EARG, "candidates: not supported while noise variances are set (the arena slots' sweeps do not add them)");
  if (h->dist) {
    // Sharded handle: the k candidates are evaluated one after the other in the shards' own tiles (an arena of k more
    // shards is exactly what a sharded evaluation has no memory for, and at the sizes that are sharded one evaluation
    // fills the GPUs by itself).  Collective: every rank calls with the same candidates.  Afterwards the handle holds
    // the LAST candidate's factorisation (as after gogp_observe of it) -- unlike the single-GPU form, which leaves
    // the handle's own state alone.
    HIPCHK(h, hipSetDevice(h->device));
    // the per-candidate contract of include/gogp_hip.h holds here too: every lml / gradient / status slot is written
    // before anything can fail, and a candidate with unusable parameters (GOGP_EARG: every rank sees the same
    // candidates, so every rank skips it) or a matrix that is not positive definite only marks its own slot
    for (int c = 0; c < k; ++c) {
      lmls[c] = NAN;
      if (status) status[c] = GOGP_ESTATE;  // "not evaluated": overwritten below unless the call aborts
      for (int64_t i = 0; i < len; ++i) grads[(size_t)c * len + i] = 0.0;
    }
    int first_d = GOGP_OK;
    for (int c = 0; c < k; ++c) {
      double *g = grads + (size_t)c * len;
      h->with_obs = false;
      int r = observe_theta(h, xs + (size_t)c * len, &lmls[c]);
      if (r == GOGP_OK || r == GOGP_ECOND) {
        const int rg = gogp_gradient(h, g, len);
        if (rg != GOGP_OK) r = rg;
      }
      if (r == GOGP_ENOTPD || r == GOGP_EARG) {
        lmls[c] = NAN;
        for (int64_t i = 0; i < len; ++i) g[i] = 0.0;
      } else if (r != GOGP_OK && r != GOGP_ECOND) {
        return r;  // a transport / HIP failure: nothing after it can be trusted (the later slots stay GOGP_ESTATE)
      }
      if (status) status[c] = r;
      if (first_d == GOGP_OK && r != GOGP_OK) first_d = r;
    }
    return first_d;
  }
  if (h->prec == 32 && k > 1) {
    // fp32 path: one candidate per launch sequence, k of them one after the other in ONE arena slot (the handle's own
    // factorisation stays untouched, as on the fp64 path).  The float kernels carry no candidate index: at the sizes
    // the fp32 path exists for, one evaluation fills the GPU.
    int first32 = GOGP_OK;
    for (int c = 0; c < k; ++c) {
      const int r = gogp_observe_gradient_candidates(h, 1, xs + (size_t)c * len, len, lmls + c, grads + (size_t)c * len,
                                                     status ? status + c : nullptr);
      if (r != GOGP_OK && r != GOGP_ENOTPD && r != GOGP_ECOND && r != GOGP_EARG) return r;
      if (first32 == GOGP_OK && r != GOGP_OK) first32 = r;
    }
    return first32;
  }
  if (!h->lookahead || !h->eager)
    return fail(h, GOGP_EARG, "candidates: needs the fused sweep (options lookahead and eager on)");
  if (h->n == 0) {  // gp/gp.go:101-104, 427-430
    for (int c = 0; c < k; ++c) {
      lmls[c] = 0.0;
      if (status) status[c] = GOGP_OK;
      for (int64_t i = 0; i < len; ++i) grads[(size_t)c * len + i] = 0.0;
    }
    return GOGP_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  // nothing of the handle's own evaluation may still be running: its streams and events are reused
  for (hipStream_t q : work_streams(h)) HIPCHK(h, hipStreamSynchronize(q));
  if (h->kinv_pending) h->have_kinv = true;  // the handle's own K^-1 finished accumulating
  h->trtri_pending = h->alpha_pending = h->kinv_pending = h->tinv_pending = false;
  int rc = ensure_candidates(h, k);
  if (rc != GOGP_OK) return rc;

  // ---- the handle works in arena slot 0 for the duration of the call ---------------------------------
  const EvalBufs saved_bufs = *h;
  const EvalState saved_state = *h;
  double *const saved_hscal = h->hscal;
  const int64_t saved_cap_y = h->cap_y;
  static_cast<EvalBufs &>(*h) = cand_layout(h->cand_arena, h->cand_cap_npad, h->esz());
  h->hscal = h->cand_hscal;
  h->cap_y = h->cand_cap_npad;
  h->with_obs = false;
  h->batch_k = k;
  h->batch_mode = true;
  gogp::tl_batch.k = k;
  gogp::tl_batch.stride = (long)h->cand_stride;
  std::vector<int> st((size_t)k, GOGP_OK);

  // parameters of every candidate into pinned host memory
  for (int c = 0; c < k; ++c) st[(size_t)c] = fill_params_log(h, xs + (size_t)c * len, h->cand_hostP[c]);
  // the whole launch sequence: parameter upload, fused sweep, K^-1, gradient sums, results to the host
  auto enqueue = [&]() -> int {
    for (int c = 0; c < k; ++c)
      HIPCHK(h, gogp::rec_memcpy_async((char *)h->devP + (size_t)c * h->cand_stride, h->cand_hostP + c,
                                       sizeof(DevParams), hipMemcpyHostToDevice, h->s));
    const bool f32 = h->prec == 32;
    int r = tiny_ok(h) ? tiny_factorize(h, true) : (f32 ? factorize_t<float>(h, true) : factorize_t<double>(h, true));
    if (r != GOGP_OK) return r;
    r = f32 ? compute_kinv_t<float>(h) : compute_kinv_t<double>(h);
    if (r != GOGP_OK) return r;
    r = ensure_alpha(h);
    if (r != GOGP_OK) return r;
    r = enqueue_grad_sums(h, f32 && h->trace_fp64);  // the fp32 path's closed-form components (fp32_gradient_identities)
    if (r != GOGP_OK) return r;
    // every stream joins the main one (the end of a captured graph; harmless otherwise)
    size_t slot = EV_BASE + 4 * (size_t)(h->npad / PANEL);  // the four event slots behind the panels' own
    for (hipStream_t q : {h->sp, h->s2, h->st, h->sl, h->sk}) order(h, slot++, q, h->s);
    return GOGP_OK;
  };
  auto run = [&]() -> int {
    int r = GOGP_OK;
    // option "graph": the launch sequence replayed from a hipGraph.  1 (default): one chain, captured with the work
    // streams aliased to one capture stream, up to npad = 1024 -- where an evaluation is a single dependent chain
    // anyway and the launch path is the cost.  2: an EXPLICITLY built graph (graphrec.h: one node per launch / copy,
    // the sweep's real cross-stream dependencies as edges, no stream captured), up to npad = 8192 -- bit-identical to
    // the streams, but this runtime executes parallel branches no faster than their serialisation (N = 4096: 6.1 ms
    // against 3.7 ms on the streams), so it is not the default.  0: streams.
    const bool dag = h->use_graph >= 2;  // 3: the same recorder as ONE chain in enqueue order (diagnostics)
    const bool graph = h->use_graph && h->prec == 64 && !h->prof.on && !h->graph_failed &&
                       h->npad <= (dag ? GRAPH_EXPLICIT_MAX_NPAD : GRAPH_MAX_NPAD);
    const CandGraphKey key = cand_graph_key(h, k);
    const bool hit = graph && h->cand_graph && h->cand_graph_key == key;
    // capture only a sequence that was asked for twice in a row (an expanding-window loop changes n
    // with every call: capturing each time would cost more than the replay saves)
    const bool seen = graph && h->cand_seen_key == key;
    h->cand_seen_key = key;
    if (hit || seen) {
      if (!hit) {
        drop_cand_graph(h);
        HIPCHK(h, graph_stream(h));
        hipGraph_t gr = nullptr;
        hipError_t eg = hipSuccess;
        gogp::GraphRec rec;
        if (dag) {
          // No stream is captured: the launch sequence is replayed into a recorder that adds one node per launch /
          // copy with explicit dependencies (graphrec.h), so hipStreamEndCapture's trouble with the sweep's fork / join
          // pattern (round 2) never arises.
          rec.chain = h->use_graph == 3;
          HIPCHK(h, hipGraphCreate(&rec.graph, 0));
          gogp::tl_rec = &rec;
          r = enqueue();
          gogp::tl_rec = nullptr;
          gr = rec.graph;
          eg = rec.err;
        } else {
          // Captured on ONE stream (the five work streams aliased to it for the duration): a linear
          // graph.  hipStreamEndCapture of this ROCm (7.0 runtime bundled with torch) recurses without
          // end on the sweep's fork / join pattern across streams, so the graph path is limited to
          // sizes where the evaluation is a single dependent chain anyway (see the caller).
          hipStream_t keep[6] = {h->s, h->sp, h->s2, h->st, h->sl, h->sk};
          h->s = h->sp = h->s2 = h->st = h->sl = h->sk = h->sg;
          eg = hipStreamBeginCapture(h->sg, hipStreamCaptureModeRelaxed);
          if (eg == hipSuccess) {
            r = enqueue();
            eg = hipStreamEndCapture(h->sg, &gr);
          }
          h->s = keep[0];
          h->sp = keep[1];
          h->s2 = keep[2];
          h->st = keep[3];
          h->sl = keep[4];
          h->sk = keep[5];
        }
        if (r == GOGP_OK && eg == hipSuccess) eg = hipGraphInstantiate(&h->cand_graph, gr, nullptr, nullptr, 0);
        if (gr) (void)hipGraphDestroy(gr);
        if (r != GOGP_OK) return r;
        if (eg != hipSuccess && dag) {
          // the runtime refused the graph: remember it, say why, and evaluate on the streams (never retried)
          (void)hipGetLastError();
          h->cand_graph = nullptr;
          h->graph_failed = true;
          h->graph_note = std::string("hipGraph not usable (") + hipGetErrorString(eg) + "): stream path";
          r = enqueue();
          if (r != GOGP_OK) return r;
          for (hipStream_t q : work_streams(h)) HIPCHK(h, hipStreamSynchronize(q));
          HIPCHK(h, hipGetLastError());
          return GOGP_OK;
        }
        HIPCHK(h, eg);
        if (dag) h->graph_nodes = rec.nodes;
        h->cand_graph_key = key;
      }
      HIPCHK(h, hipGraphLaunch(h->cand_graph, h->sg));
      HIPCHK(h, hipStreamSynchronize(h->sg));
    } else {
      r = enqueue();
      if (r != GOGP_OK) return r;
    }
    for (hipStream_t q : work_streams(h)) HIPCHK(h, hipStreamSynchronize(q));
    HIPCHK(h, hipGetLastError());
    return GOGP_OK;
  };
  rc = run();
  if (rc != GOGP_OK)  // a HIP failure: drain before the buffers change hands again
    for (hipStream_t q : work_streams(h)) (void)hipStreamSynchronize(q);

  std::string first_msg;
  int first = rc;
  if (rc == GOGP_OK) {
    for (int c = 0; c < k; ++c) {
      st[(size_t)c] = judge_row(h, h->hscal + (size_t)c * BATCH_ROW, h->prec == 32, h->n, h->cand_hostP[c], st[(size_t)c],
                                "candidates: parameters must be positive and finite", &lmls[c], grads + (size_t)c * len,
                                len, first_msg);
      if (first == GOGP_OK && st[(size_t)c] != GOGP_OK) first = st[(size_t)c];
    }
  }
  if (status)
    for (int c = 0; c < k; ++c) status[c] = (rc == GOGP_OK) ? st[(size_t)c] : rc;

  // ---- back to the handle's own buffers and state -----------------------------------------------------
  gogp::tl_batch.k = 1;
  gogp::tl_batch.stride = 0;
  h->batch_k = 1;
  h->batch_mode = false;
  static_cast<EvalBufs &>(*h) = saved_bufs;
  static_cast<EvalState &>(*h) = saved_state;
  h->hscal = saved_hscal;
  h->cap_y = saved_cap_y;
  h->trtri_pending = h->alpha_pending = h->kinv_pending = false;
  if (first != GOGP_OK && rc == GOGP_OK) h->err = first_msg;
  return first;
}

// ---- batches of independent small GPs: many members, each with its own n and theta, in ONE launch ---------------------
// The forecast harness of the reference (tutorial/tutorial.go:88-197) fits every prefix X[:end] of the data separately;
// each window on its own is one latency-bound evaluation of a few dozen rows.  Here the members are row ranges of one
// uploaded data set, and one call evaluates k (member, log theta) pairs: one copy of the pairs' parameters in, one launch
// (diag256.hip: batch_eval_kernel, a workgroup per pair), one copy of the results out.  fp64 whatever the precision
// options; the handle's own data, factorisation and candidates are not touched.
extern "C" int gogp_batch_set_data(gogp_handle *h, const double *X, const double *y, int64_t rows, int32_t nmembers,
                                   const int64_t *offset, const int64_t *n) {
  if (!h) return GOGP_EARG;
  if (h->dist) return fail(h, GOGP_EARG, "batch: not supported on a sharded handle");
  if (rows < 0 || nmembers < 0 || (rows > 0 && (!X || !y)) || (nmembers > 0 && (!offset || !n)))
    return fail(h, GOGP_EARG, "batch_set_data: bad arguments");
  for (int32_t b = 0; b < nmembers; ++b)
    if (n[b] < 0 || n[b] > GOGP_BATCH_MAX_N || offset[b] < 0 || offset[b] > rows - n[b])
      return fail(h, GOGP_EARG, "batch_set_data: every member needs 0 <= n <= GOGP_BATCH_MAX_N rows inside the data");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->s));
  if (rows > h->bt_cap_rows || !h->bt_X) {
    (void)hipFree(h->bt_X);
    (void)hipFree(h->bt_y);
    h->bt_X = h->bt_y = nullptr;
    h->bt_cap_rows = 0;
    h->bt_have = false;
    const int64_t cap = std::max<int64_t>(rows, 1);
    // (+ GOGP_MAX_NDIM doubles of slack, as the handle's own X)
    HIPCHK(h, hipMalloc(&h->bt_X, ((size_t)cap * h->D + GOGP_MAX_NDIM) * sizeof(double)));
    HIPCHK(h, hipMalloc(&h->bt_y, (size_t)cap * sizeof(double)));
    h->bt_cap_rows = cap;
  }
  if (rows > 0) {
    HIPCHK(h, hipMemcpy(h->bt_X, X, (size_t)rows * h->D * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->bt_y, y, (size_t)rows * sizeof(double), hipMemcpyHostToDevice));
  }
  h->bt_rows = rows;
  h->bt_off.assign(offset, offset + nmembers);
  h->bt_n.assign(n, n + nmembers);
  h->bt_have = true;
  return GOGP_OK;
}

// device + pinned staging of at least `bytes` (grown, never shrunk)
static int bt_reserve(gogp_handle *h, char **dev, char **host, size_t *cap, size_t bytes) {
  if (bytes <= *cap) return GOGP_OK;
  (void)hipFree(*dev);
  if (*host) (void)hipHostFree(*host);
  *dev = *host = nullptr;
  *cap = 0;
  HIPCHK(h, hipMalloc((void **)dev, bytes));
  HIPCHK(h, hipHostMalloc((void **)host, bytes, hipHostMallocDefault));
  *cap = bytes;
  return GOGP_OK;
}

// all four entry points: produce == (zoff != NULL); the full Observe form == (xoff != NULL): pair i is
// x[xoff[i] .. xoff[i+1]) = [log theta | X_i | y_i] and carries its own observations, no batch data, no members
static int batch_eval(gogp_handle *h, int32_t k, const int32_t *members, const double *x, int64_t len, const int64_t *xoff,
                      const int64_t *zoff, const double *Z, double *lmls, double *grads, double *mu, double *sigma,
                      int *status) {
  const bool produce = zoff != nullptr, full = xoff != nullptr;
  if (!h) return GOGP_EARG;
  if (h->dist) return fail(h, GOGP_EARG, "batch: not supported on a sharded handle");
  if (k < 0 || (k > 0 && ((!full && !members) || !x || !lmls || (!produce && !grads))))
    return fail(h, GOGP_EARG, "batch: bad arguments");
  int64_t nx = 0;  // full form: the doubles of the k vectors, x[xoff[0] .. xoff[k])
  if (full) {
    if (xoff[0] < 0) return fail(h, GOGP_EARG, "batch: xoff must be non-negative and non-decreasing");
    for (int32_t i = 0; i < k; ++i)
      if (xoff[i + 1] < xoff[i]) return fail(h, GOGP_EARG, "batch: xoff must be non-negative and non-decreasing");
    nx = xoff[k] - xoff[0];
  } else {
    if (len != h->P) return fail(h, GOGP_EARG, "len(x)");
    if (!h->bt_have) return fail(h, GOGP_ESTATE, "batch: no batch data (gogp_batch_set_data)");
    const int64_t nmem = (int64_t)h->bt_n.size();
    for (int32_t i = 0; i < k; ++i)
      if (members[i] < 0 || members[i] >= nmem) return fail(h, GOGP_EARG, "batch: member index out of range");
  }
  int64_t mz = 0;  // test points: rows 0 .. zoff[k] - 1 of Z
  if (produce) {
    if (zoff[0] < 0) return fail(h, GOGP_EARG, "batch_produce: zoff must be non-negative and non-decreasing");
    for (int32_t i = 0; i < k; ++i)
      if (zoff[i + 1] < zoff[i]) return fail(h, GOGP_EARG, "batch_produce: zoff must be non-negative and non-decreasing");
    mz = zoff[k];
    if (mz > 0 && (!Z || !mu || !sigma)) return fail(h, GOGP_EARG, "batch_produce: bad arguments");
  }
  if (k == 0) return GOGP_OK;
  HIPCHK(h, hipSetDevice(h->device));
  // the pairs: parameters with the fill of the candidates call; full form: the length rules of gp/gp.go:386-400 per pair.
  // A refused pair is launched with no observations (and theta = 1) and reported in its status.
  const int64_t P = h->P, D = h->D;
  std::vector<int> st((size_t)k, GOGP_OK);
  std::vector<const char *> why((size_t)k, "batch: parameters must be positive and finite");
  std::vector<int64_t> ns((size_t)k, 0);
  int64_t out_doubles = 0;
  if (full) {
    for (int32_t i = 0; i < k; ++i) {
      const int64_t li = xoff[i + 1] - xoff[i], rest = li - P;
      const double *xi = x + xoff[i];
      if (rest < 0 || rest % (D + 1) != 0) {
        st[(size_t)i] = GOGP_EARG;
        why[(size_t)i] = "len(x)";
      } else if (rest / (D + 1) > GOGP_BATCH_MAX_N) {
        st[(size_t)i] = GOGP_EARG;
        why[(size_t)i] = "batch: a pair needs n <= GOGP_BATCH_MAX_N observations";
      } else if (!std::all_of(xi + P, xi + li, [](double v) { return std::isfinite(v); })) {
        st[(size_t)i] = GOGP_EARG;
        why[(size_t)i] = "batch: non-finite observations";
      } else {
        ns[(size_t)i] = rest / (D + 1);
      }
      out_doubles += BATCH_ROW + (produce ? 0 : ns[(size_t)i] * (D + 1));
    }
  } else {
    out_doubles = (int64_t)k * BATCH_ROW;
  }
  const size_t items_bytes = align_up((size_t)k * sizeof(BatchItem), 256);
  const size_t z_bytes = (size_t)mz * h->D * sizeof(double);
  const size_t in_bytes = items_bytes + z_bytes + (size_t)nx * sizeof(double);
  const size_t out_bytes = ((size_t)out_doubles + 2 * (size_t)mz) * sizeof(double);
  int rc = bt_reserve(h, &h->bt_din, &h->bt_hin, &h->bt_in_cap, in_bytes);
  if (rc == GOGP_OK) rc = bt_reserve(h, (char **)&h->bt_dout, (char **)&h->bt_hout, &h->bt_out_cap, out_bytes);
  if (rc != GOGP_OK) return rc;
  BatchItem *items = reinterpret_cast<BatchItem *>(h->bt_hin);
  const std::vector<double> log_one((size_t)std::max<int64_t>(P, 1), 0.0);
  int64_t roff = 0;
  for (int32_t i = 0; i < k; ++i) {
    BatchItem &it = items[i];
    if (full) {
      const bool refused = st[(size_t)i] != GOGP_OK;
      const int fst = fill_params_log(h, refused ? log_one.data() : x + xoff[i], it.P);
      if (!refused) st[(size_t)i] = fst;
      it.off = (long)(xoff[i] - xoff[0] + P);
      it.n = (long)ns[(size_t)i];
    } else {
      st[(size_t)i] = fill_params_log(h, x + (size_t)i * len, it.P);
      it.off = (long)h->bt_off[(size_t)members[i]];
      it.n = (long)h->bt_n[(size_t)members[i]];
    }
    it.zoff = produce ? (long)zoff[i] : 0;
    it.m = produce ? (long)(zoff[i + 1] - zoff[i]) : 0;
    it.roff = (long)roff;
    roff += BATCH_ROW + ((full && !produce) ? it.n * (D + 1) : 0);
  }
  if (mz > 0) memcpy(h->bt_hin + items_bytes, Z, z_bytes);
  if (nx > 0) memcpy(h->bt_hin + items_bytes + z_bytes, x + xoff[0], (size_t)nx * sizeof(double));
  hipStream_t s = h->s;
  double *drows = h->bt_dout, *dmu = drows + out_doubles, *dsig = dmu + mz;
  const double *dZ = reinterpret_cast<const double *>(h->bt_din + items_bytes);
  HIPCHK(h, hipMemcpyAsync(h->bt_din, h->bt_hin, in_bytes, hipMemcpyHostToDevice, s));
  if (full)
    launch_batch_eval_full(s, reinterpret_cast<const BatchItem *>(h->bt_din), k,
                           reinterpret_cast<const double *>(h->bt_din + items_bytes + z_bytes), dZ, drows, dmu, dsig,
                           h->ard_dims, produce, h->ev());
  else
    launch_batch_eval(s, reinterpret_cast<const BatchItem *>(h->bt_din), k, h->bt_X, h->bt_y, dZ, drows, dmu, dsig,
                      h->ard_dims, produce, h->ev());
  HIPCHK(h, hipMemcpyAsync(h->bt_hout, h->bt_dout, out_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  // every pair judged as gogp_observe would judge a handle holding its member's data
  const double *hmu = h->bt_hout + out_doubles, *hsig = hmu + mz;
  int first = GOGP_OK;
  std::string first_msg;
  for (int32_t i = 0; i < k; ++i) {
    const BatchItem &it = items[i];
    const int64_t gl = full ? xoff[i + 1] - xoff[i] : len;
    double *g = produce ? nullptr : (full ? grads + xoff[i] : grads + (size_t)i * len);
    double *row = h->bt_hout + it.roff;
    if (st[(size_t)i] == GOGP_OK && it.n == 0) {  // gp/gp.go:101-104, 343-347, 427-430
      lmls[i] = 0.0;
      if (g) std::fill(g, g + gl, 0.0);
    } else {
      st[(size_t)i] = judge_row(h, row, false, it.n, it.P, st[(size_t)i], why[(size_t)i], &lmls[i], g, gl, first_msg);
    }
    const bool values = st[(size_t)i] == GOGP_OK || st[(size_t)i] == GOGP_ECOND;
    // gp/gp.go:118-129 (inputs) and :488-493 (outputs: -alpha), behind the slot sums of the pair's block
    if (full && g && values && it.n > 0) std::copy(row + BATCH_ROW, row + BATCH_ROW + it.n * (D + 1), g + P);
    if (produce)
      for (long j = it.zoff; j < it.zoff + it.m; ++j) {
        mu[j] = values ? (it.n == 0 ? 0.0 : hmu[j]) : NAN;
        sigma[j] = values ? hsig[j] : NAN;
      }
    if (status) status[i] = st[(size_t)i];
    if (first == GOGP_OK && st[(size_t)i] != GOGP_OK) first = st[(size_t)i];
  }
  if (first != GOGP_OK) h->err = first_msg;
  return first;
}

extern "C" int gogp_batch_observe_gradient(gogp_handle *h, int32_t k, const int32_t *members, const double *x,
                                           int64_t len, double *lmls, double *grads, int *status) {
  return batch_eval(h, k, members, x, len, nullptr, nullptr, nullptr, lmls, grads, nullptr, nullptr, status);
}

extern "C" int gogp_batch_produce(gogp_handle *h, int32_t k, const int32_t *members, const double *x, int64_t len,
                                  const int64_t *zoff, const double *Z, double *lmls, double *mu, double *sigma,
                                  int *status) {
  if (!zoff) return fail(h, GOGP_EARG, "batch_produce: zoff is NULL");
  return batch_eval(h, k, members, x, len, nullptr, zoff, Z, lmls, nullptr, mu, sigma, status);
}

// The full Observe form of the two (gp/gp.go:386-400: X and y re-sliced out of x; :118-129, 488-493: the gradient by the
// inputs and the outputs): the forecast windows of the case studies that infer their inputs or outputs
// (tutorial/anynoise/main.go:47, tutorial/warpedtime/main.go:59: OPTINP) in one launch.
extern "C" int gogp_batch_observe_full_gradient(gogp_handle *h, int32_t k, const double *x, const int64_t *xoff,
                                                double *lmls, double *grads, int *status) {
  if (h && !xoff) return fail(h, GOGP_EARG, "batch: xoff is NULL");
  return batch_eval(h, k, nullptr, x, 0, xoff, nullptr, nullptr, lmls, grads, nullptr, nullptr, status);
}

extern "C" int gogp_batch_produce_full(gogp_handle *h, int32_t k, const double *x, const int64_t *xoff, const int64_t *zoff,
                                       const double *Z, double *lmls, double *mu, double *sigma, int *status) {
  if (h && (!xoff || !zoff)) return fail(h, GOGP_EARG, "batch_produce: xoff or zoff is NULL");
  return batch_eval(h, k, nullptr, x, 0, xoff, zoff, Z, lmls, nullptr, mu, sigma, status);
}

extern "C" int gogp_graph_info(const gogp_handle *h, int64_t *nodes, int *refused) {
  if (!h) return GOGP_EARG;
  if (nodes) *nodes = h->cand_graph ? h->graph_nodes : 0;
  if (refused) *refused = h->graph_failed ? 1 : 0;
  return GOGP_OK;
}

// ---- produce ----------------------------------------------------------------------------------
static int ensure_m(gogp_handle *h, int64_t m, int64_t mpad) {
  if (m > h->cap_m || mpad * h->npad > h->cap_mp_npad || !h->dZ) {
    free_m_buffers(h);
    HIPCHK(h, hipMalloc(&h->dZ, (size_t)std::max<int64_t>(m, 1) * h->D * sizeof(double)));
    HIPCHK(h, hipMalloc(&h->pvec, (size_t)4 * std::max<int64_t>(mpad, 1) * sizeof(double)));
    if (h->npad > 0) {
      HIPCHK(h, hipMalloc(&h->KsT, (size_t)mpad * h->npad * h->esz()));
      HIPCHK(h, hipMalloc(&h->Vt, (size_t)mpad * h->npad * h->esz()));
    }
    h->cap_m = m;
    h->cap_mp_npad = mpad * h->npad;
  }
  return GOGP_OK;
}

constexpr int PRODUCE_GROUPS = 4;
// Produce's event slots, behind the factorisation's own
static inline size_t produce_event_base(int64_t npad) { return EV_BASE + 4 * (size_t)(npad / PANEL) + 8; }
// The blocked solve of Produce on matrices of element type T, from the mpad right-hand-side rows that lie in KsT (Produce:
// Kstar^T; gogp_multi_*: Y^T): V^T = R L^-T into Vt, row by row, and -- dq != nullptr -- |V_j|^2 of the first m rows
template <class T>
static void produce_substitute_t(gogp_handle *h, hipStream_t s, int64_t m, int64_t mpad, double *dq) {
  const int64_t npad = h->npad, ld = npad;
  T *R = reinterpret_cast<T *>(h->KsT), *V = reinterpret_cast<T *>(h->Vt);
  const T *L = reinterpret_cast<const T *>(h->bufL), *Dinv = reinterpret_cast<const T *>(h->Dinv);
  // V^T = Kstar^T L^-T by blocked substitution on the GEMM kernel
  // Produce launches are not part of the Observe+Gradient metric: they are event-timed only when the caller enabled
  // profiling around Produce itself (bench.py: the `produce.roofline` field)
  GemmProfile *pf = h->prof.on ? &h->prof : nullptr;
  const int mt = (int)(mpad / TILE);
  const int npanel = (int)(npad / PANEL);
  const int pw = h->produce_panels;  // super-panel width of the substitution, in 256-panels
  // in super-panels, as the factorisation: the panels of a super-panel are solved one after the other
  // (each updating the columns that are left inside it), the trailing columns then receive ONE update
  // with K = 256 * width instead of one K = 256 update per panel (M = 1024: N = 16384 6.74 -> 6.64 ms,
  // N = 32768 23.0 -> 21.7 ms).  The test points are independent of each other: their tile rows go to up to
  // PRODUCE_GROUPS streams, each running the whole substitution for its rows -- with M = 1024 one chain is 8 tile
  // rows tall and its ~130 dependent launches, not the N^2 M flops, are what the call costs; several chains fill
  // each other's gaps (option "produce_groups", default 2; 1 = round 3's single chain).
  // T^-1 of every super-panel's diagonal block: assembled by the first Produce on a factor (a chain of tiny launches
  // on stream sk that runs ahead of the solves, which wait for their super-panel's event), kept for the later ones.
  // Not behind the factorisation: its 110 launches cost an N = 16384 Observe + Gradient 0.6 ms (measured).
  bool use_tinv = h->produce_tinv && h->lookahead;
  if (use_tinv && ensure_tinv(h) != GOGP_OK) {  // no memory for T^-1: panel-by-panel substitution, and no stale message
    use_tinv = false;
    h->err.clear();
    (void)hipGetLastError();  // ... and no sticky allocation error for the final check of the call
  }
  const bool assemble = use_tinv && !(h->tinv_valid && h->tinv_sig == tinv_signature(h));
  // Right behind an eager Observe the streams of the triangular inverse (st, s2, sk) still hold two thirds of an
  // evaluation's flops that Produce does not depend on: everything on the main stream then
  const bool busy = h->trtri_pending || h->kinv_pending;
  hipStream_t sasm = busy ? s : h->sk;
  const size_t evt0 = produce_event_base(npad) + 2 * PRODUCE_GROUPS;  // one event per super-panel behind the others
  if (assemble) {
    if (sasm != s) order(h, EV_TINV, s, sasm);  // behind whatever last wrote the factor (s is ordered behind the factorisation)
    for (int P0 = 0, nsub = 0; P0 < npanel; P0 += nsub) {
      nsub = std::min(pw, npanel - P0);
      assemble_tinv<T>(h, sasm, P0, nsub);
      (void)gogp::rec_event_record(ev(h, evt0 + (size_t)P0), sasm);
    }
    h->tinv_valid = true;
    h->tinv_sig = tinv_signature(h);
  }
  hipStream_t gs[PRODUCE_GROUPS] = {s, h->s2, h->st, h->sp};
  int ngroups = (h->lookahead && !busy) ? std::min(h->produce_groups, std::min(mt, PRODUCE_GROUPS)) : 1;
  if (ngroups < 1) ngroups = 1;
  const size_t ev0 = produce_event_base(npad);
  for (int g = 1; g < ngroups; ++g) order(h, ev0 + g, s, gs[g]);  // Kstar^T (and whatever s held) first
  for (int g = 0; g < ngroups; ++g) {
    hipStream_t sg = gs[g];
    const int t0 = (int)((int64_t)mt * g / ngroups), t1 = (int)((int64_t)mt * (g + 1) / ngroups), mtg = t1 - t0;
    if (mtg <= 0) continue;
    T *Rg = R + (int64_t)t0 * TILE * ld, *Vg = V + (int64_t)t0 * TILE * ld;
    for (int P0 = 0, nsub = 0; P0 < npanel; P0 += nsub) {
      nsub = std::min(pw, npanel - P0);
      const int64_t C0 = (int64_t)P0 * PANEL, CE = C0 + (int64_t)nsub * PANEL;
      GemmGrid gtri, gup;
      gtri.ktri = h->ktri;
      gtri.small_below = gup.small_below = h->produce_small_below;
      if (use_tinv) {
        if (assemble && sg != sasm) (void)gogp::rec_stream_wait(sg, ev(h, evt0 + (size_t)P0));
        // the whole super-panel at once: V[:, C0:CE] = R[:, C0:CE] T^-T with the assembled inverse of the factor's
        // diagonal block -- the same flops as the panel-by-panel substitution (T^-1 is lower triangular: ktri), 2
        // dependent launches per super-panel instead of 2 per 256 columns
        const T *X = reinterpret_cast<const T *>(h->TX) + C0 * h->tinv_ld;
        launch_gemm_nt(sg, GEMM_RECT, mtg, (int)((CE - C0) / TILE), CE - C0, 1.0, Rg + C0, ld, X, h->tinv_ld, 0.0, Vg + C0,
                       ld, pf, &gtri);
      } else {
        for (int q = 0; q < nsub; ++q) {
          const int64_t c0 = C0 + (int64_t)q * PANEL, c2 = c0 + PANEL;
          const T *Dp = Dinv + (size_t)(P0 + q) * PANEL * PANEL;
          launch_gemm_nt(sg, GEMM_RECT, mtg, 2, PANEL, 1.0, Rg + c0, ld, Dp, PANEL, 0.0, Vg + c0, ld, pf, &gtri);
          if (c2 < CE)
            launch_gemm_nt(sg, GEMM_RECT, mtg, (int)((CE - c2) / TILE), PANEL, -1.0, Vg + c0, ld, L + c2 * ld + c0, ld,
                           1.0, Rg + c2, ld, pf, &gup);
        }
      }
      const int nt = (int)((npad - CE) / TILE);
      if (nt > 0)
        launch_gemm_nt(sg, GEMM_RECT, mtg, nt, CE - C0, -1.0, Vg + C0, ld, L + CE * ld + C0, ld, 1.0, Rg + CE, ld, pf,
                       &gup);
    }
  }
  for (int g = 1; g < ngroups; ++g) order(h, ev0 + PRODUCE_GROUPS + g, gs[g], s);
  // (Kstar^T K^-1 Kstar)_jj = |V_j|^2 : only the diagonal of gp/gp.go:341-342 is read (:356)
  if (dq) launch_rownorm_dot(s, V, ld, nullptr, npad, m, nullptr, dq);
}
// Kstar^T into KsT (zero rows from m on, zero columns from n on)
template <class T>
static void produce_cross_t(gogp_handle *h, hipStream_t s, int64_t m, int64_t mpad) {
  AuxTimer tm(h, GOGP_PROF_CROSS, s);
  launch_cross(s, h->devP, h->D, h->dX, h->n, h->npad, h->dZ, m, mpad, reinterpret_cast<T *>(h->KsT), h->npad,
               h->ev());  // gp/gp.go:322-332
}
// Kstar, mean and the blocked solve of Produce on matrices of element type T
template <class T>
static void produce_solve_t(gogp_handle *h, hipStream_t s, int64_t m, int64_t mpad, double *dmu, double *dq) {
  produce_cross_t<T>(h, s, m, mpad);
  // mean = Kstar^T alpha (gp/gp.go:335)
  launch_rownorm_dot(s, reinterpret_cast<const T *>(h->KsT), h->npad, h->alpha, h->npad, m, dmu, nullptr);
  produce_substitute_t<T>(h, s, m, mpad, dq);
}

// Few test points (option "produce_small_max", default 64; fp64 matrices): Kstar, the mean, and V = L^-1 Kstar by the
// persistent substitution kernel of trsm_small.hip -- one pass over the factor (8 N^2 / 2 bytes) instead of the
// ~36-launch GEMM chain.  The reference's forecast harness asks for ONE point per step (tutorial/tutorial.go:178-179).
// the workspace of the persistent substitution kernel: two launches of <= 32 columns side by side (33 .. 64 points);
// *one: the bytes of one launch's part
static int ensure_small_ws(gogp_handle *h, size_t *one) {
  *one = (trsm_small_workspace_bytes(std::max(h->npad, h->cap_npad)) + 255) / 256 * 256;
  return h->small_ws.reserve(h, 2 * *one);
}
static int produce_small(gogp_handle *h, hipStream_t s, int64_t m, int64_t mpad, double *dmu, double *dq) {
  const int64_t npad = h->npad, ld = npad;
  size_t one = 0;
  const int rcw = ensure_small_ws(h, &one);
  if (rcw != GOGP_OK) return rcw;
  const bool f32 = h->prec == 32;  // float factor / inverses / Kstar: widened as the kernel reads them, sums in fp64
  auto cross_and_mean = [&](auto *Ks) {
    {
      AuxTimer tm(h, GOGP_PROF_CROSS, s);
      launch_cross(s, h->devP, h->D, h->dX, h->n, npad, h->dZ, m, mpad, Ks, ld, h->ev());  // gp/gp.go:322-332
    }
    launch_rownorm_dot(s, Ks, ld, h->alpha, npad, m, dmu, nullptr);  // mean = Kstar^T alpha (gp/gp.go:335)
  };
  if (f32)
    cross_and_mean(reinterpret_cast<float *>(h->KsT));
  else
    cross_and_mean(h->KsT);
  auto solve = [&](hipStream_t q, int j0, int cnt, void *ws, unsigned **tm) {
    if (f32)
      launch_trsm_small(q, reinterpret_cast<const float *>(h->bufL), ld, reinterpret_cast<const float *>(h->Dinv),
                        reinterpret_cast<const float *>(h->KsT), ld, npad, j0, cnt, ws, dq, tm);
    else
      launch_trsm_small(q, h->bufL, ld, h->Dinv, h->KsT, ld, npad, j0, cnt, ws, dq, tm);
  };
  unsigned *tmo = nullptr, *tmo2 = nullptr;
  unsigned *htmo = hs_tmo(h);
  htmo[0] = htmo[1] = 0;
  const int m1 = (int)std::min<int64_t>(m, 32);
  const size_t ev0 = produce_event_base(npad);
  // (right behind an eager Observe s2 carries the triangular inverse: both launches on the main stream then)
  hipStream_t s2nd = (h->trtri_pending || h->kinv_pending) ? s : h->s2;
  if (m > 32) {
    // the second 32 columns on a second stream, beside the first (both launches read the same factor at the same
    // time: what one pulls into the Infinity Cache the other finds there)
    if (s2nd != s) order(h, ev0 + 1, s, s2nd);
    solve(s2nd, 32, (int)m - 32, h->small_ws.as<char>() + one, &tmo2);
    HIPCHK(h, hipMemcpyAsync(htmo + 1, tmo2, sizeof(unsigned), hipMemcpyDeviceToHost, s2nd));
  }
  solve(s, 0, m1, h->small_ws.p, &tmo);
  HIPCHK(h, hipMemcpyAsync(htmo, tmo, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  if (m > 32 && s2nd != s) order(h, ev0 + PRODUCE_GROUPS + 1, s2nd, s);
  return GOGP_OK;
}

// ---- what the Produce calls share ------------------------------------------------------------------
// The test points' vectors on the device, mpad doubles each (pvec)
struct ProducePlan {
  int64_t mpad = 0;
  double *prior = nullptr, *mu = nullptr, *q = nullptr, *sigma = nullptr;
};
// Up to the point where the handle's buffers are in place: the refusals (refuse != nullptr: fp32 and sharded handles,
// under that name; cov: more than GOGP_COV_MAX_M points), the state (under the name `who`), the device, the sizes.
// m == 0 returns GOGP_OK with nothing done; so does a sharded handle with observations, whose Produce has buffers of
// its own (gogp_dist_produce).
static int produce_prepare(gogp_handle *h, const char *refuse, const char *who, int64_t m, bool cov, ProducePlan *pp) {
  char buf[160];
  if (refuse && h->prec == 32) {
    snprintf(buf, sizeof buf, "%s: precision = 32 handles are not supported", refuse);
    return fail(h, GOGP_EARG, buf);
  }
  if (refuse && h->dist) {
    snprintf(buf, sizeof buf, "%s: sharded handles are not supported", refuse);
    return fail(h, GOGP_EARG, buf);
  }
  if (cov && m > GOGP_COV_MAX_M) {
    snprintf(buf, sizeof buf, "%s: more than GOGP_COV_MAX_M = %d test points", who, GOGP_COV_MAX_M);
    return fail(h, GOGP_EARG, buf);
  }
  if (m == 0) return GOGP_OK;
  if (h->n > 0 && !h->factored) {
    snprintf(buf, sizeof buf, "%s: nothing absorbed", who);
    return fail(h, GOGP_ESTATE, buf);
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (h->dist && h->n > 0) return GOGP_OK;
  if (cov && h->ncu <= 0) {  // the slab policy of pcov.hip
    HIPCHK(h, hipDeviceGetAttribute(&h->ncu, hipDeviceAttributeMultiprocessorCount, h->device));
    if (h->ncu <= 0) h->ncu = 1;
  }
  const int64_t mpad = ((m + TILE - 1) / TILE) * TILE;
  const int rc = ensure_m(h, m, mpad);
  if (rc != GOGP_OK) return rc;
  *pp = ProducePlan{mpad, h->pvec, h->pvec + mpad, h->pvec + 2 * mpad, h->pvec + 3 * mpad};
  return GOGP_OK;
}
// Z up, optionally the prior (gp/gp.go:269-278); with observations the main stream then waits for alpha and, `tile`,
// runs Produce's tile route: the mean into pp.mu, |V_j|^2 into pp.q, V^T into Vt row by row
static int produce_forward(gogp_handle *h, const double *Z, int64_t m, const ProducePlan &pp, bool prior, bool tile) {
  hipStream_t s = h->s;
  if (h->n == 0) {
    const int rc = gogp_upload_params(h);  // no observations: parameters may not have been uploaded yet
    if (rc != GOGP_OK) return rc;
  }
  HIPCHK(h, hipMemcpyAsync(h->dZ, Z, (size_t)m * h->D * sizeof(double), hipMemcpyHostToDevice, s));
  if (prior) launch_prior(s, h->devP, h->dZ, m, pp.prior);
  if (h->n == 0) return GOGP_OK;
  const int rc = ensure_alpha(h);
  if (rc != GOGP_OK) return rc;
  if (tile) produce_solve_t<double>(h, s, m, pp.mpad, pp.mu, pp.q);
  return GOGP_OK;
}
// No observations (gp/gp.go:343-347), behind produce_forward with the prior: sigma = sqrt(prior), mu = 0
static int produce_of_the_prior(gogp_handle *h, const ProducePlan &pp, int64_t m, double *mu, double *sigma) {
  launch_sigma(h->s, pp.prior, nullptr, m, pp.sigma);
  HIPCHK(h, hipMemcpyAsync(sigma, pp.sigma, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, h->s));
  HIPCHK(h, hipStreamSynchronize(h->s));
  for (int64_t j = 0; j < m; ++j) mu[j] = 0.0;
  return GOGP_OK;
}

extern "C" int gogp_produce(gogp_handle *h, const double *Z, int64_t m, double *mu,
                            double *sigma) {
  if (!h || m < 0 || (m > 0 && (!Z || !mu || !sigma))) return fail(h, GOGP_EARG, "produce: NULL");
  ProducePlan pp;
  int rc = produce_prepare(h, nullptr, "Produce", m, false, &pp);
  if (rc != GOGP_OK || m == 0) return rc;
  if (h->dist && h->n > 0) return gogp_dist_produce(h, Z, m, mu, sigma);
  hipStream_t s = h->s;
  rc = produce_forward(h, Z, m, pp, true, false);
  if (rc != GOGP_OK) return rc;
  if (h->n == 0) return produce_of_the_prior(h, pp, m, mu, sigma);
  // (float matrices: up to 16 test points -- measured at N = 65536: M = 1 / 16 / 64 in 4.5 / 5.0 / 11.2 ms against 7.5 on
  // the float tile-kernel chain, N = 16384: 0.92 / 0.94 / 1.53 against 1.07: the float chain is twice as fast as the fp64 one)
  const bool small = m <= h->produce_small_max && (h->prec == 64 || m <= 16);
  if (small) {
    rc = produce_small(h, s, m, pp.mpad, pp.mu, pp.q);
    if (rc != GOGP_OK) return rc;
  } else if (h->prec == 32)
    produce_solve_t<float>(h, s, m, pp.mpad, pp.mu, pp.q);
  else
    produce_solve_t<double>(h, s, m, pp.mpad, pp.mu, pp.q);
  launch_sigma(s, pp.prior, pp.q, m, pp.sigma);
  HIPCHK(h, hipMemcpyAsync(mu, pp.mu, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(sigma, pp.sigma, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  const unsigned tmo = small ? hs_tmo(h)[0] | hs_tmo(h)[1] : 0u;
  if (tmo != 0u) {
    // a workgroup of the persistent substitution gave up waiting for another one (trsm_small.hip): the numbers are
    // not to be trusted -- say so instead of returning them
    char buf[160];
    snprintf(buf, sizeof buf, "Produce: the substitution kernel timed out waiting for a workgroup (code 0x%x)", tmo);
    h->err = buf;
    return GOGP_EHIP;
  }
  return GOGP_OK;
}

// ---- produce with derivatives -------------------------------------------------------------------
// W^T = V^T L^-1 behind produce_solve_t, on the main stream: the block backward substitution over the rows of Vt
// (one test point each), from the last column panel to the first.  Per step two launches of the skinny NN kernel
// (pgrad.hip): W^T[:, p] = R[:, p] inv(L_pp) into KsT (whose Kstar^T the forward pass has consumed), then
// R[:, j] -= W^T[:, p] L[p, j] for every column j left of the panel, in place in Vt.  A step is a super-panel of
// `produce_panels` 256-panels where the forward pass has assembled T^-1 (2 launches per 1024 columns), one 256-panel
// through its Dinv block otherwise.
static void produce_backward(gogp_handle *h, hipStream_t s, int64_t m) {
  const int64_t npad = h->npad, ld = npad, rows16 = (m + 15) / 16;
  double *V = h->Vt, *W = h->KsT;
  const int npanel = (int)(npad / PANEL);
  const bool use_tinv = h->produce_tinv && h->lookahead && h->TX && h->tinv_valid && h->tinv_sig == tinv_signature(h);
  const int pw = use_tinv ? h->produce_panels : 1;
  for (int P0 = (npanel - 1) / pw * pw; P0 >= 0; P0 -= pw) {
    const int nsub = std::min(pw, npanel - P0), K = nsub * PANEL;
    const int64_t C0 = (int64_t)P0 * PANEL;
    const double *Binv = use_tinv ? h->TX + C0 * h->tinv_ld : h->Dinv + (size_t)P0 * PANEL * PANEL;
    launch_bwd_panel(s, rows16, V + C0, ld, Binv, use_tinv ? h->tinv_ld : (int64_t)PANEL, W + C0, ld, K, K, true, false);
    launch_bwd_panel(s, rows16, W + C0, ld, h->bufL + C0 * ld, ld, V, ld, C0, K, false, true);
  }
}

extern "C" int gogp_produce_gradient(gogp_handle *h, const double *Z, int64_t m, double *mu, double *sigma,
                                     double *dmu_out, double *dsigma_out) {
  if (!h || m < 0 || (m > 0 && (!Z || !mu || !sigma || !dmu_out || !dsigma_out)))
    return fail(h, GOGP_EARG, "produce_gradient: NULL");
  ProducePlan pp;
  int rc = produce_prepare(h, "produce_gradient", "ProduceGradient", m, false, &pp);
  if (rc != GOGP_OK || m == 0) return rc;
  const int D = h->D;
  hipStream_t s = h->s;
  if (h->n == 0) {
    rc = produce_forward(h, Z, m, pp, true, true);
    if (rc == GOGP_OK) rc = produce_of_the_prior(h, pp, m, mu, sigma);
    if (rc != GOGP_OK) return rc;
    for (int64_t j = 0; j < m * D; ++j) dmu_out[j] = dsigma_out[j] = 0.0;  // the prior does not depend on z
    return GOGP_OK;
  }
  const int nslab = gogp::pgrad_slabs(h->npad, m, nullptr);
  const size_t md = (size_t)m * D;
  rc = h->pg_ws.reserve(h, md * (2 * (size_t)nslab + 2) * sizeof(double));
  if (rc != GOGP_OK) return rc;
  double *part = h->pg_ws.as<double>(), *ddmu = part + 2 * (size_t)nslab * md, *ddsig = ddmu + md;
  // always the tile route of Produce, whatever m: it leaves V^T in Vt, row by row, where the backward pass starts
  // (the persistent few-point kernel keeps its solution in a layout of its own)
  rc = produce_forward(h, Z, m, pp, true, true);
  if (rc != GOGP_OK) return rc;
  launch_sigma(s, pp.prior, pp.q, m, pp.sigma);
  produce_backward(h, s, m);
  launch_pgrad(s, h->devP, D, h->dX, h->n, h->npad, h->dZ, m, h->alpha, h->KsT, h->npad, pp.sigma, part, ddmu, ddsig,
               h->ev());
  HIPCHK(h, hipMemcpyAsync(mu, pp.mu, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(sigma, pp.sigma, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(dmu_out, ddmu, md * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(dsigma_out, ddsig, md * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  return GOGP_OK;
}

// ---- T output columns on one factorisation (multi.hip) ------------------------------------------------------------
// No reference counterpart (gp.GP holds one output vector).  Y^T and the solutions A^T = (K^-1 Y)^T lie in multi_vec,
// GOGP_MULTI_MAX_T rows of npad doubles each.  The solutions come from the factor -- Y^T into KsT, Produce's forward and
// ProduceGradient's backward substitution -- on first need after a factorisation and are kept (multi_solved).  The calls
// write workspaces of their own, Produce's (whose contents no call expects to find again) and, as gogp_gradient would,
// K^-1: the handle's state afterwards is what a gogp_gradient at this point would have left.
static double *multi_yt(const gogp_handle *h) { return h->multi_vec.as<double>(); }
static double *multi_at(const gogp_handle *h) { return multi_yt(h) + (size_t)GOGP_MULTI_MAX_T * h->npad; }
// NULL, or the kind of handle the multi-output calls refuse (LOO's refusals)
static const char *multi_refusal(const gogp_handle *h) {
  return h->prec == 32        ? "precision = 32 handles"
         : mixed_gradient(h) ? "gradient_precision = 32 (a float K^-1)"
         : h->dist           ? "sharded handles"
                             : nullptr;
}

extern "C" int gogp_multi_set_outputs(gogp_handle *h, const double *Y, int64_t n, int32_t T) {
  if (!h) return GOGP_EARG;
  if (T == 0 && !Y) {  // clear
    h->multi_T = 0;
    h->multi_solved = false;
    return GOGP_OK;
  }
  if (const char *refuse = multi_refusal(h)) {
    char buf[160];
    snprintf(buf, sizeof buf, "multi_set_outputs: %s are not supported", refuse);
    return fail(h, GOGP_EARG, buf);
  }
  if (!h->have_data) return fail(h, GOGP_ESTATE, "multi_set_outputs: no data (gogp_set_data)");
  if (!Y || n != h->n || T < 1 || T > GOGP_MULTI_MAX_T)
    return fail(h, GOGP_EARG, "multi_set_outputs: need Y, n == gogp_n and 1 <= T <= GOGP_MULTI_MAX_T");
  for (int64_t i = 0; i < n * T; ++i)
    if (!std::isfinite(Y[i])) return fail(h, GOGP_EARG, "multi_set_outputs: non-finite output");
  h->multi_solved = false;
  if (n > 0) {
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t npad = h->npad;
    const size_t rows = (size_t)GOGP_MULTI_MAX_T * npad;
    h->multi_T = 0;  // until the new ones are in place
    const int rc = h->multi_vec.reserve(h, 2 * rows * sizeof(double));
    if (rc != GOGP_OK) return rc;
    std::vector<double> yt((size_t)T * npad, 0.0);
    for (int64_t i = 0; i < n; ++i)
      for (int t = 0; t < T; ++t) yt[(size_t)t * npad + i] = Y[i * T + t];
    HIPCHK(h, hipMemsetAsync(multi_yt(h), 0, rows * sizeof(double), h->s));
    HIPCHK(h, hipMemcpyAsync(multi_yt(h), yt.data(), yt.size() * sizeof(double), hipMemcpyHostToDevice, h->s));
    HIPCHK(h, hipStreamSynchronize(h->s));
  }
  h->multi_T = T;
  return GOGP_OK;
}

// A^T = (K^-1 Y)^T of the current factor into its buffer, on the main stream
static int multi_solve(gogp_handle *h) {
  if (h->multi_solved) return GOGP_OK;
  const int T = h->multi_T;
  int rc = ensure_alpha(h);  // the main stream behind the factorisation
  if (rc == GOGP_OK) rc = ensure_m(h, T, TILE);
  if (rc != GOGP_OK) return rc;
  hipStream_t s = h->s;
  const size_t row = (size_t)h->npad * sizeof(double);
  static_assert(GOGP_MULTI_MAX_T == TILE, "the outputs are one tile row of right-hand sides");
  HIPCHK(h, hipMemcpyAsync(h->KsT, multi_yt(h), TILE * row, hipMemcpyDeviceToDevice, s));
  produce_substitute_t<double>(h, s, T, TILE, nullptr);  // V^T = Y^T L^-T into Vt
  produce_backward(h, s, T);                             // A^T = V^T L^-1 into KsT
  HIPCHK(h, hipMemcpyAsync(multi_at(h), h->KsT, (size_t)T * row, hipMemcpyDeviceToDevice, s));
  if (T < TILE) HIPCHK(h, hipMemsetAsync(multi_at(h) + (size_t)T * h->npad, 0, (size_t)(TILE - T) * row, s));
  h->multi_solved = true;
  return GOGP_OK;
}

// The refusals and the state of the four calls that work on the outputs (under the name `who`), then -- with
// observations -- the solutions in place on the main stream.  *empty: n == 0, nothing to launch.
static int multi_prepare(gogp_handle *h, const char *who, bool *empty) {
  char buf[160];
  if (const char *refuse = multi_refusal(h)) {
    snprintf(buf, sizeof buf, "%s: %s are not supported", who, refuse);
    return fail(h, GOGP_EARG, buf);
  }
  if (h->multi_T == 0) {
    snprintf(buf, sizeof buf, "%s: no outputs (gogp_multi_set_outputs)", who);
    return fail(h, GOGP_ESTATE, buf);
  }
  *empty = h->n == 0;
  if (*empty) return GOGP_OK;
  if (!h->factored) {
    snprintf(buf, sizeof buf, "%s: nothing absorbed", who);
    return fail(h, GOGP_ESTATE, buf);
  }
  HIPCHK(h, hipSetDevice(h->device));
  return multi_solve(h);
}

extern "C" int gogp_multi_lml(gogp_handle *h, double *total, double *lml) {
  if (!h || !total) return fail(h, GOGP_EARG, "multi_lml: NULL");
  bool empty = false;
  int rc = multi_prepare(h, "multi_lml", &empty);
  if (rc != GOGP_OK) return rc;
  const int T = h->multi_T;
  *total = 0.0;
  if (empty) {
    for (int t = 0; lml && t < T; ++t) lml[t] = 0.0;
    return GOGP_OK;
  }
  rc = h->multi_mean.reserve(h, GOGP_MULTI_MAX_T * sizeof(double));
  if (rc != GOGP_OK) return rc;
  hipStream_t s = h->s;
  double dots[GOGP_MULTI_MAX_T];
  launch_multi_dots(s, multi_yt(h), multi_at(h), h->npad, h->n, T, h->multi_mean.as<double>());
  HIPCHK(h, hipMemcpyAsync(dots, h->multi_mean.p, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  double sum = 0.0;
  for (int t = 0; t < T; ++t) {  // as judge_scalars, with y_t^T alpha_t for the quadratic term; summed in column order
    const double l = -0.5 * (double)h->n * log(2 * M_PI) - 0.5 * h->logdet2 - 0.5 * dots[t];
    if (lml) lml[t] = l;
    sum += l;
  }
  *total = sum;
  return GOGP_OK;
}

extern "C" int gogp_multi_gradient(gogp_handle *h, double *grad, int64_t len) {
  if (!h || !grad) return fail(h, GOGP_EARG, "multi_gradient: NULL");
  if (len != h->P) return fail(h, GOGP_EARG, "multi_gradient: wrong length");
  bool empty = false;
  int rc = multi_prepare(h, "multi_gradient", &empty);
  if (rc != GOGP_OK) return rc;
  for (int64_t i = 0; i < len; ++i) grad[i] = 0.0;
  if (empty) return GOGP_OK;
  rc = compute_kinv(h);
  if (rc != GOGP_OK) return rc;
  hipStream_t s = h->s;
  const int64_t npad = h->npad, ld = npad;
  const size_t mat = (size_t)npad * (size_t)npad;
  rc = h->multi_mat.reserve(h, (mat + (size_t)npad) * sizeof(double));
  if (rc != GOGP_OK) return rc;
  double *G = h->multi_mat.as<double>(), *zero = G + mat;
  // G = T K^-1 - A A^T on the lower tiles
  launch_multi_weight(s, multi_at(h), npad, h->multi_T, h->bufA, ld, h->n, npad, (double)h->multi_T, G);
  // sum_ab (0 0^T - G)_ab dK_ab per slot: the reduction of the LML gradient with G for K^-1 and zeros for alpha
  HIPCHK(h, hipMemsetAsync(zero, 0, (size_t)npad * sizeof(double), s));
  {
    AuxTimer tm(h, GOGP_PROF_GRAD, s);
    launch_grad_reduce(s, h->devP, h->D, h->ard_dims, h->dX, zero, (const double *)G, ld, h->n, npad, h->gpart, h->gout,
                       h->radial1, h->ard_mfma_min, h->ev());
  }
  double acc[NACC];
  HIPCHK(h, hipMemcpyAsync(acc, h->gout, sizeof acc, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  assemble_gradient(h, acc, h->hostP->dnoise, grad);
  return GOGP_OK;
}

extern "C" int gogp_multi_get_alpha(gogp_handle *h, double *A) {
  if (!h || !A) return fail(h, GOGP_EARG, "multi_get_alpha: NULL");
  bool empty = false;
  const int rc = multi_prepare(h, "multi_get_alpha", &empty);
  if (rc != GOGP_OK || empty) return rc;
  const int T = h->multi_T;
  const int64_t n = h->n, npad = h->npad;
  std::vector<double> at((size_t)T * npad);
  HIPCHK(h, hipMemcpyAsync(at.data(), multi_at(h), at.size() * sizeof(double), hipMemcpyDeviceToHost, h->s));
  HIPCHK(h, hipStreamSynchronize(h->s));
  HIPCHK(h, hipGetLastError());
  for (int64_t i = 0; i < n; ++i)
    for (int t = 0; t < T; ++t) A[i * T + t] = at[(size_t)t * npad + i];
  return GOGP_OK;
}

extern "C" int gogp_multi_produce(gogp_handle *h, const double *Z, int64_t m, double *mu, double *sigma) {
  if (!h || m < 0 || (m > 0 && (!Z || !mu))) return fail(h, GOGP_EARG, "multi_produce: NULL");
  bool empty = false;
  int rc = multi_prepare(h, "multi_produce", &empty);
  if (rc != GOGP_OK) return rc;
  ProducePlan pp;
  rc = produce_prepare(h, "multi_produce", "multi_produce", m, false, &pp);
  if (rc != GOGP_OK || m == 0) return rc;
  const int T = h->multi_T;
  hipStream_t s = h->s;
  rc = produce_forward(h, Z, m, pp, true, false);  // Z up, the prior, the main stream behind alpha
  if (rc != GOGP_OK) return rc;
  if (empty) {  // no observations (gp/gp.go:343-347): sigma = sqrt(prior), mu = 0
    launch_sigma(s, pp.prior, nullptr, m, pp.sigma);
    if (sigma) HIPCHK(h, hipMemcpyAsync(sigma, pp.sigma, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    for (int64_t j = 0; j < m * T; ++j) mu[j] = 0.0;
    return GOGP_OK;
  }
  rc = h->multi_mean.reserve(h, (size_t)pp.mpad * GOGP_MULTI_MAX_T * sizeof(double));
  if (rc != GOGP_OK) return rc;
  // always the tile route of Produce, whatever m (as gogp_produce_gradient): Kstar^T row by row in KsT
  produce_cross_t<double>(h, s, m, pp.mpad);
  // the means, Kstar^T A, in one launch of the tile kernel -- before the substitution uses up Kstar^T
  GemmGrid gm;
  gm.small_below = h->produce_small_below;
  launch_gemm_nt(s, GEMM_RECT, (int)(pp.mpad / TILE), 1, h->npad, 1.0, (const double *)h->KsT, h->npad,
                 (const double *)multi_at(h), h->npad, 0.0, h->multi_mean.as<double>(), (int64_t)GOGP_MULTI_MAX_T,
                 h->prof.on ? &h->prof : nullptr, &gm);
  if (sigma) {
    produce_substitute_t<double>(h, s, m, pp.mpad, pp.q);
    launch_sigma(s, pp.prior, pp.q, m, pp.sigma);
    HIPCHK(h, hipMemcpyAsync(sigma, pp.sigma, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  HIPCHK(h, hipMemcpy2DAsync(mu, (size_t)T * sizeof(double), h->multi_mean.p, (size_t)GOGP_MULTI_MAX_T * sizeof(double),
                             (size_t)T * sizeof(double), (size_t)m, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  return GOGP_OK;
}

// ---- explicit basis functions: a marginalised linear mean (basis.hip) ------------------------------------------------
// No reference counterpart (gp.GP has mean zero).  Rasmussen & Williams section 2.7 in the flat-prior limit; the formulas
// are in DESIGN.md section 4, "Explicit basis functions".  basis_vec holds H^T and W^T = (K^-1 H)^T (TILE rows of npad
// doubles each, zero from row p and column n on: the tile kernel and Produce's substitution take them as they lie), the
// p + 1 rows [Q | alpha~]^T and the p x p results; everything is computed on first need after a factorisation and kept
// (basis_solved).  W comes from the explicit K^-1 by basis_symm_kernel where that matrix is there or on its way, from
// the factor by multi_solve's two substitutions otherwise (option "basis_symm").  The calls write workspaces of their
// own, Produce's and, as gogp_gradient would, K^-1: the contract of gogp_multi_*.  G shares multi_mat with
// gogp_multi_gradient: both write it whole before they read it, inside one call.
constexpr int BASIS_CROWS = (GOGP_BASIS_MAX_P + 1 + 3) / 4 * 4;
constexpr size_t BASIS_PP = (size_t)GOGP_BASIS_MAX_P * GOGP_BASIS_MAX_P, BASIS_AG = (size_t)GOGP_BASIS_MAX_P * (GOGP_BASIS_MAX_P + 1);
static_assert(GOGP_BASIS_MAX_P <= TILE, "the basis columns are one tile row of right-hand sides");
struct BasisBufs {
  double *Ht, *Wt, *Ct, *Ag, *LA, *Ainv, *beta, *scal, *gpart;
  long long *info;
};
static size_t basis_layout(double *base, int64_t npad, BasisBufs *b) {
  size_t off = 0;
  auto take = [&](size_t cnt) {
    double *q = base ? base + off : nullptr;
    off += cnt;
    return q;
  };
  b->Ht = take((size_t)TILE * npad), b->Wt = take((size_t)TILE * npad), b->Ct = take((size_t)BASIS_CROWS * npad);
  b->Ag = take(BASIS_AG), b->LA = take(BASIS_PP), b->Ainv = take(BASIS_PP), b->beta = take(GOGP_BASIS_MAX_P);
  b->scal = take(8), b->gpart = take((size_t)gogp::BASIS_GRAM_SLABS_MAX * BASIS_AG);
  b->info = reinterpret_cast<long long *>(take(1));
  return off * sizeof(double);
}
static BasisBufs basis_bufs(const gogp_handle *h) {
  BasisBufs b;
  (void)basis_layout(h->basis_vec.as<double>(), h->npad, &b);
  return b;
}

extern "C" int gogp_basis_set(gogp_handle *h, const double *H, int64_t n, int32_t p) {
  if (!h) return GOGP_EARG;
  if (p == 0 && !H) {  // clear
    h->basis_p = 0;
    h->basis_solved = false;
    return GOGP_OK;
  }
  if (const char *refuse = multi_refusal(h)) {
    char buf[160];
    snprintf(buf, sizeof buf, "basis_set: %s are not supported", refuse);
    return fail(h, GOGP_EARG, buf);
  }
  if (!h->have_data) return fail(h, GOGP_ESTATE, "basis_set: no data (gogp_set_data)");
  if (!H || n != h->n || p < 1 || p > GOGP_BASIS_MAX_P)
    return fail(h, GOGP_EARG, "basis_set: need H, n == gogp_n and 1 <= p <= GOGP_BASIS_MAX_P");
  if (n <= p) return fail(h, GOGP_EARG, "basis_set: needs more observations than basis columns (n > p)");
  for (int64_t i = 0; i < n * p; ++i)
    if (!std::isfinite(H[i])) return fail(h, GOGP_EARG, "basis_set: non-finite basis value");
  HIPCHK(h, hipSetDevice(h->device));
  const int64_t npad = h->npad;
  h->basis_p = 0;  // until the new one is in place
  h->basis_solved = false;
  BasisBufs b;
  const int rc = h->basis_vec.reserve(h, basis_layout(nullptr, std::max(npad, h->cap_npad), &b));
  if (rc != GOGP_OK) return rc;
  b = basis_bufs(h);
  std::vector<double> ht((size_t)p * npad, 0.0);
  for (int64_t i = 0; i < n; ++i)
    for (int c = 0; c < p; ++c) ht[(size_t)c * npad + i] = H[i * p + c];
  HIPCHK(h, hipMemsetAsync(b.Ht, 0, 2 * (size_t)TILE * npad * sizeof(double), h->s));  // H^T and W^T
  HIPCHK(h, hipMemcpyAsync(b.Ht, ht.data(), ht.size() * sizeof(double), hipMemcpyHostToDevice, h->s));
  HIPCHK(h, hipStreamSynchronize(h->s));
  h->basis_p = p;
  return GOGP_OK;
}

// W, [A | g], the factor of A, beta and [Q | alpha~] of the current factor and basis, on the main stream
static int basis_solve(gogp_handle *h) {
  if (h->basis_solved) return GOGP_OK;
  const int p = h->basis_p;
  const int64_t n = h->n, npad = h->npad;
  int rc = ensure_alpha(h);  // the main stream behind the factorisation
  if (rc != GOGP_OK) return rc;
  hipStream_t s = h->s;
  const BasisBufs b = basis_bufs(h);
  const size_t row = (size_t)npad * sizeof(double);
  const bool symm = h->basis_symm == 1 || (h->basis_symm < 0 && (h->have_kinv || h->kinv_pending));
  if (symm) {
    rc = compute_kinv(h);
    if (rc == GOGP_OK)
      rc = h->basis_part.reserve(h, (size_t)gogp::basis_symm_slabs(n) * (size_t)((p + 3) / 4 * 4) * row);
    if (rc != GOGP_OK) return rc;
    launch_basis_symm(s, h->bufA, npad, n, npad, b.Ht, npad, p, h->basis_part.as<double>(), b.Wt);
  } else {  // multi_solve's route: H^T into KsT, Produce's forward and ProduceGradient's backward substitution
    rc = ensure_m(h, p, TILE);
    if (rc != GOGP_OK) return rc;
    HIPCHK(h, hipMemcpyAsync(h->KsT, b.Ht, TILE * row, hipMemcpyDeviceToDevice, s));
    produce_substitute_t<double>(h, s, p, TILE, nullptr);
    produce_backward(h, s, p);
    HIPCHK(h, hipMemcpyAsync(b.Wt, h->KsT, (size_t)p * row, hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemsetAsync(b.Wt + (size_t)p * npad, 0, (size_t)(TILE - p) * row, s));
  }
  launch_basis_gram(s, b.Ht, b.Wt, npad, h->alpha, n, p, b.gpart, b.Ag);
  launch_basis_finish(s, b.Ag, p, b.LA, b.Ainv, b.beta, b.scal, b.info);
  long long info = 0;
  double scal[2];
  h->basis_beta.assign((size_t)p, 0.0);
  h->basis_cov.assign((size_t)p * p, 0.0);
  HIPCHK(h, hipMemcpyAsync(&info, b.info, sizeof info, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  if (info != 0) {
    char buf[200];
    snprintf(buf, sizeof buf,
             "basis: H^T K^-1 H is not positive definite (pivot %lld): the basis columns are linearly dependent",
             info - 1);
    h->err = buf;
    return GOGP_ECOND;
  }
  launch_basis_cols(s, b.Wt, npad, n, p, b.LA, b.beta, h->alpha, b.Ct);
  HIPCHK(h, hipMemcpyAsync(scal, b.scal, sizeof scal, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(h->basis_beta.data(), b.beta, (size_t)p * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(h->basis_cov.data(), b.Ainv, (size_t)p * p * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  h->basis_logdet = scal[0];
  h->basis_gtb = scal[1];
  h->basis_solved = true;
  return GOGP_OK;
}

// The refusals and the state of the calls that work on the basis (under the name `who`), then the solutions in place
static int basis_prepare(gogp_handle *h, const char *who) {
  char buf[160];
  if (const char *refuse = multi_refusal(h)) {
    snprintf(buf, sizeof buf, "%s: %s are not supported", who, refuse);
    return fail(h, GOGP_EARG, buf);
  }
  if (h->basis_p == 0) {
    snprintf(buf, sizeof buf, "%s: no basis (gogp_basis_set)", who);
    return fail(h, GOGP_ESTATE, buf);
  }
  if (h->n <= h->basis_p) {
    snprintf(buf, sizeof buf, "%s: needs more observations than basis columns (n > p)", who);
    return fail(h, GOGP_EARG, buf);
  }
  if (!h->factored) {
    snprintf(buf, sizeof buf, "%s: nothing absorbed", who);
    return fail(h, GOGP_ESTATE, buf);
  }
  HIPCHK(h, hipSetDevice(h->device));
  return basis_solve(h);
}

extern "C" int gogp_basis_lml(gogp_handle *h, double *lml) {
  if (!h || !lml) return fail(h, GOGP_EARG, "basis_lml: NULL");
  const int rc = basis_prepare(h, "basis_lml");
  if (rc != GOGP_OK) return rc;
  // R&W eq. 2.45: the handle's own LML, + 1/2 g^T beta - 1/2 log|A| + p/2 log 2 pi
  *lml = h->lml + 0.5 * h->basis_gtb - 0.5 * h->basis_logdet + 0.5 * (double)h->basis_p * log(2 * M_PI);
  return GOGP_OK;
}

extern "C" int gogp_basis_gradient(gogp_handle *h, double *grad, int64_t len) {
  if (!h || !grad) return fail(h, GOGP_EARG, "basis_gradient: NULL");
  if (len != h->P) return fail(h, GOGP_EARG, "basis_gradient: wrong length");
  if (h->basis_p != 0 && h->with_obs) return fail(h, GOGP_EARG, "basis_gradient: the full Observe form is not supported");
  int rc = basis_prepare(h, "basis_gradient");
  if (rc != GOGP_OK) return rc;
  for (int64_t i = 0; i < len; ++i) grad[i] = 0.0;
  rc = compute_kinv(h);
  if (rc != GOGP_OK) return rc;
  hipStream_t s = h->s;
  const int64_t npad = h->npad, ld = npad;
  const size_t mat = (size_t)npad * (size_t)npad;
  rc = h->multi_mat.reserve(h, (mat + (size_t)npad) * sizeof(double));
  if (rc != GOGP_OK) return rc;
  double *G = h->multi_mat.as<double>(), *zero = G + mat;
  // G = K^-1 - [Q | alpha~][Q | alpha~]^T on the lower tiles, then the reduction of the LML gradient with G for K^-1 and
  // zeros for alpha (gogp_multi_gradient)
  launch_multi_weight(s, basis_bufs(h).Ct, npad, h->basis_p + 1, h->bufA, ld, h->n, npad, 1.0, G);
  HIPCHK(h, hipMemsetAsync(zero, 0, (size_t)npad * sizeof(double), s));
  {
    AuxTimer tm(h, GOGP_PROF_GRAD, s);
    launch_grad_reduce(s, h->devP, h->D, h->ard_dims, h->dX, zero, (const double *)G, ld, h->n, npad, h->gpart, h->gout,
                       h->radial1, h->ard_mfma_min, h->ev());
  }
  double acc[NACC];
  HIPCHK(h, hipMemcpyAsync(acc, h->gout, sizeof acc, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  assemble_gradient(h, acc, h->hostP->dnoise, grad);
  return GOGP_OK;
}

extern "C" int gogp_basis_get_beta(gogp_handle *h, double *beta, double *cov) {
  if (!h || !beta) return fail(h, GOGP_EARG, "basis_get_beta: NULL");
  const int rc = basis_prepare(h, "basis_get_beta");
  if (rc != GOGP_OK) return rc;
  const size_t p = (size_t)h->basis_p;
  for (size_t i = 0; i < p; ++i) beta[i] = h->basis_beta[i];
  for (size_t i = 0; cov && i < p * p; ++i) cov[i] = h->basis_cov[i];
  return GOGP_OK;
}

extern "C" int gogp_basis_get_alpha(gogp_handle *h, double *alpha) {
  if (!h || !alpha) return fail(h, GOGP_EARG, "basis_get_alpha: NULL");
  const int rc = basis_prepare(h, "basis_get_alpha");
  if (rc != GOGP_OK) return rc;
  HIPCHK(h, hipMemcpyAsync(alpha, basis_bufs(h).Ct + (size_t)h->basis_p * h->npad, (size_t)h->n * sizeof(double),
                           hipMemcpyDeviceToHost, h->s));
  HIPCHK(h, hipStreamSynchronize(h->s));
  HIPCHK(h, hipGetLastError());
  return GOGP_OK;
}

extern "C" int gogp_basis_produce(gogp_handle *h, const double *Z, const double *Hz, int64_t m, double *mu, double *sigma) {
  if (!h || m < 0 || (m > 0 && (!Z || !Hz || !mu))) return fail(h, GOGP_EARG, "basis_produce: NULL");
  int rc = basis_prepare(h, "basis_produce");
  if (rc != GOGP_OK) return rc;
  const int p = h->basis_p;
  for (int64_t i = 0; i < m * p; ++i)
    if (!std::isfinite(Hz[i])) return fail(h, GOGP_EARG, "basis_produce: non-finite basis value");
  ProducePlan pp;
  rc = produce_prepare(h, "basis_produce", "basis_produce", m, false, &pp);
  if (rc != GOGP_OK || m == 0) return rc;
  hipStream_t s = h->s;
  rc = produce_forward(h, Z, m, pp, true, false);  // Z up, the prior, the main stream behind alpha
  if (rc != GOGP_OK) return rc;
  const size_t mp = (size_t)pp.mpad;
  rc = h->basis_mean.reserve(h, mp * (TILE + GOGP_BASIS_MAX_P + 1) * sizeof(double));
  if (rc != GOGP_OK) return rc;
  double *KW = h->basis_mean.as<double>(), *dHz = KW + mp * TILE, *dmu = dHz + mp * GOGP_BASIS_MAX_P;
  const BasisBufs b = basis_bufs(h);
  HIPCHK(h, hipMemcpyAsync(dHz, Hz, (size_t)m * p * sizeof(double), hipMemcpyHostToDevice, s));
  // always the tile route of Produce, whatever m (as gogp_multi_produce): Kstar^T row by row in KsT
  produce_cross_t<double>(h, s, m, pp.mpad);
  launch_rownorm_dot(s, (const double *)h->KsT, h->npad, h->alpha, h->npad, m, pp.mu, nullptr);  // mu_0 = Kstar^T alpha
  // Kstar^T W in one launch of the tile kernel -- before the substitution uses up Kstar^T
  GemmGrid gm;
  gm.small_below = h->produce_small_below;
  launch_gemm_nt(s, GEMM_RECT, (int)(pp.mpad / TILE), 1, h->npad, 1.0, (const double *)h->KsT, h->npad, (const double *)b.Wt,
                 h->npad, 0.0, KW, (int64_t)TILE, h->prof.on ? &h->prof : nullptr, &gm);
  if (sigma) produce_substitute_t<double>(h, s, m, pp.mpad, pp.q);
  launch_basis_predict(s, dHz, KW, TILE, m, p, b.beta, b.Ainv, pp.mu, pp.prior, pp.q, dmu, sigma ? pp.sigma : nullptr);
  HIPCHK(h, hipMemcpyAsync(mu, dmu, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
  if (sigma) HIPCHK(h, hipMemcpyAsync(sigma, pp.sigma, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  return GOGP_OK;
}

// ---- joint predictive covariance and posterior samples ----------------------------------------------
// Both calls: Produce's tile route for every m (it leaves V^T in Vt row by row, as gogp_produce_gradient needs it), then
// the split-K product Vt Vt^T and its finalising kernel (pcov.hip) on the main stream.  Workspace pc_ws, grown on demand:
//   covariance:  part | cov (m x m)
//   samples:     part | S = cov + diag_add I, identity-padded to mp = a multiple of 256 | C, its lower factor | one
//                block inverse | xi, zero-padded to nsp x mp (nsp a multiple of 128) | xi C^T | samples (ns x m) | pivot word
// doubles of the SYRK's partial tiles for m test points on the current factor
static size_t pcov_part_doubles(gogp_handle *h, int64_t m) {
  if (h->n == 0) return 0;
  const size_t tiles = (size_t)((m + 63) / 64), pairs = tiles * (tiles + 1) / 2;
  return (size_t)gogp::pcov_slabs(h->npad, m, h->ncu, nullptr) * pairs * 4096;
}
// Z up, the mean into pp.mu and V^T into Vt (n == 0: the mean is zero and there is no V)
static int pcov_forward(gogp_handle *h, const double *Z, int64_t m, const ProducePlan &pp) {
  const int rc = produce_forward(h, Z, m, pp, false, true);
  if (rc == GOGP_OK && h->n == 0) HIPCHK(h, hipMemsetAsync(pp.mu, 0, (size_t)m * sizeof(double), h->s));
  return rc;
}

extern "C" int gogp_produce_covariance(gogp_handle *h, const double *Z, int64_t m, double *mu, double *cov) {
  if (!h || m < 0 || (m > 0 && (!Z || !mu || !cov))) return fail(h, GOGP_EARG, "produce_covariance: NULL");
  ProducePlan pp;
  int rc = produce_prepare(h, "produce_covariance", "produce_covariance", m, true, &pp);
  if (rc != GOGP_OK || m == 0) return rc;
  const size_t npart = pcov_part_doubles(h, m), mm = (size_t)m * m;
  rc = h->pc_ws.reserve(h, (npart + mm) * sizeof(double));
  if (rc != GOGP_OK) return rc;
  double *part = h->pc_ws.as<double>(), *dcov = part + npart;
  hipStream_t s = h->s;
  rc = pcov_forward(h, Z, m, pp);
  if (rc != GOGP_OK) return rc;
  launch_pcov(s, h->devP, h->dZ, m, h->n > 0 ? h->Vt : nullptr, h->npad, h->npad, h->ncu, part, 0.0, dcov, m, m, h->ev());
  HIPCHK(h, hipMemcpyAsync(mu, pp.mu, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(cov, dcov, mm * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  return GOGP_OK;
}

extern "C" int gogp_produce_samples(gogp_handle *h, const double *Z, int64_t m, const double *xi, int64_t ns,
                                    double diag_add, double *mu, double *samples) {
  if (!h || m < 0 || ns < 0 || (m > 0 && (!Z || !mu)) || (m > 0 && ns > 0 && (!xi || !samples)))
    return fail(h, GOGP_EARG, "produce_samples: NULL");
  if (!(diag_add >= 0.0) || !std::isfinite(diag_add))
    return fail(h, GOGP_EARG, "produce_samples: diag_add must be finite and not negative");
  ProducePlan pp;
  int rc = produce_prepare(h, "produce_samples", "produce_samples", m, true, &pp);
  if (rc != GOGP_OK || m == 0) return rc;
  for (int64_t i = 0; i < ns * m; ++i)
    if (!std::isfinite(xi[i])) return fail(h, GOGP_EARG, "produce_samples: xi contains a value that is not finite");
  hipStream_t s = h->s;
  double *dmu = pp.mu;
  if (ns == 0) {  // the mean alone
    rc = pcov_forward(h, Z, m, pp);
    if (rc != GOGP_OK) return rc;
    HIPCHK(h, hipMemcpyAsync(mu, dmu, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    return GOGP_OK;
  }
  const int64_t mp = ((m + PANEL - 1) / PANEL) * PANEL, nsp = ((ns + TILE - 1) / TILE) * TILE;
  const size_t npart = pcov_part_doubles(h, m), mm = (size_t)mp * mp, nx = (size_t)nsp * mp;
  rc = h->pc_ws.reserve(h, (npart + 2 * mm + (size_t)PANEL * PANEL + 2 * nx + (size_t)ns * m + 1) * sizeof(double));
  if (rc != GOGP_OK) return rc;
  double *part = h->pc_ws.as<double>(), *S = part + npart, *C = S + mm, *Dp = C + mm, *dxi = Dp + (size_t)PANEL * PANEL,
         *G = dxi + nx, *dsamp = G + nx;
  long long *info = reinterpret_cast<long long *>(dsamp + (size_t)ns * m);
  rc = pcov_forward(h, Z, m, pp);
  if (rc != GOGP_OK) return rc;
  launch_pcov(s, h->devP, h->dZ, m, h->n > 0 ? h->Vt : nullptr, h->npad, h->npad, h->ncu, part, diag_add, S, mp, mp, h->ev());
  // S = C C^T, right-looking in 256-panels on the main stream: the diagonal block and its inverse, the panel under it
  // through that inverse, the trailing lower tiles (the factorisation's chain_split = 0 form; m <= 4096: <= 16 panels)
  HIPCHK(h, hipMemsetAsync(C, 0, mm * sizeof(double), s));
  HIPCHK(h, hipMemsetAsync(info, 0, sizeof(long long), s));
  for (int64_t c0 = 0; c0 < mp; c0 += PANEL) {
    const int64_t c2 = c0 + PANEL;
    launch_diag256(s, S + c0 * mp + c0, mp, C + c0 * mp + c0, mp, Dp, c0, m, info);
    const int mt2 = (int)((mp - c2) / TILE);
    if (mt2 > 0) {
      GemmGrid gtri;
      gtri.ktri = h->ktri;
      launch_gemm_nt(s, GEMM_RECT, mt2, 2, PANEL, 1.0, S + c2 * mp + c0, mp, Dp, PANEL, 0.0, C + c2 * mp + c0, mp, nullptr,
                     &gtri);
      launch_gemm_nt(s, GEMM_LOWER, mt2, mt2, PANEL, -1.0, C + c2 * mp + c0, mp, C + c2 * mp + c0, mp, 1.0,
                     S + c2 * mp + c2, mp, nullptr);
    }
  }
  long long *hinfo = reinterpret_cast<long long *>(h->hscal + HS_PIVOT);  // a staging word of this call's own: HS_INFO keeps K's
  HIPCHK(h, hipMemcpyAsync(hinfo, info, sizeof(long long), hipMemcpyDeviceToHost, s));
  // samples = mu + xi C^T: xi up in one copy, one product (B = C as stored: zero above the diagonal), samples down in one
  HIPCHK(h, hipMemsetAsync(dxi, 0, nx * sizeof(double), s));
  HIPCHK(h, hipMemcpy2DAsync(dxi, (size_t)mp * sizeof(double), xi, (size_t)m * sizeof(double), (size_t)m * sizeof(double),
                             (size_t)ns, hipMemcpyHostToDevice, s));
  GemmGrid gx;
  gx.ktri = h->ktri;
  gx.small_below = h->produce_small_below;
  launch_gemm_nt(s, GEMM_RECT, (int)(nsp / TILE), (int)(mp / TILE), mp, 1.0, dxi, mp, C, mp, 0.0, G, mp, nullptr, &gx);
  launch_pcov_add_mu(s, G, mp, dmu, ns, m, dsamp);
  HIPCHK(h, hipMemcpyAsync(mu, dmu, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  if (*hinfo != 0) {  // nothing is written to samples; the fitted process is untouched
    char buf[200];
    h->notpd = (int64_t)*hinfo - 1;
    snprintf(buf, sizeof buf,
             "produce_samples: the predictive covariance (+ diag_add) of the test points is not positive definite "
             "(pivot %lld of the test points)", (long long)h->notpd);
    h->err = buf;
    return GOGP_ENOTPD;
  }
  HIPCHK(h, hipMemcpyAsync(samples, dsamp, (size_t)ns * m * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  return GOGP_OK;
}

// ---- inducing-point approximation (sparse.hip) ----------------------------------------------------------------------
// No reference counterpart.  The collapsed bound of Titsias (2009) on M inducing points; the formulas are in DESIGN.md
// section 4, "Sparse".  The process on the inducing points is a private dense handle (sp_ind): Kuu + eps I is its Gram
// matrix (constant noise of std sqrt(eps)), so its factor, V^T of a chunk (Produce's forward substitution on the tile
// route with the chunk's rows as test points), Y = L^-T and the reduction over the (U, U) pairs all come from the code
// of the dense path.  Everything runs on that handle's main stream.  The M x M work on B = I + V V^T / s2 is done here
// with the tile kernel: a 256-panel Cholesky (as gogp_produce_samples), the triangular inverse panel by panel
// (the recurrence of trtri_superstep: column panel i of Y = C^-T is -Y[:i, :i] C[i, :i]^T inv(C_ii)^T), B^-1 = Y Y^T.
struct SparseBufs {
  double *Bacc, *Bm, *C, *Y, *Binv, *Pm, *Gm, *Yu;  // Mp x Mp; the gradient reuses Bacc / C / Y for T / S / a product
  double *Dinv, *tmp;                          // Mp / 256 block inverses; Mp x 256
  double *r, *g, *mvec, *zero;                 // Mp doubles each
  double *scal, *gsum, *gpart;                 // 8; NACC; SG partial rows
  long long *info;
};
// the buffers at `base` (nullptr: the sizes alone); returns the bytes they take
static size_t sparse_layout(double *base, int64_t Mp, SparseBufs *b) {
  const size_t mm = (size_t)Mp * Mp;
  size_t off = 0;
  auto take = [&](size_t cnt) {
    double *q = base ? base + off : nullptr;
    off += cnt;
    return q;
  };
  b->Bacc = take(mm), b->Bm = take(mm), b->C = take(mm), b->Y = take(mm), b->Binv = take(mm), b->Pm = take(mm);
  b->Gm = take(mm), b->Yu = take(mm);
  b->Dinv = take((size_t)(Mp / PANEL) * PANEL * PANEL);
  b->tmp = take((size_t)Mp * PANEL);
  b->r = take(Mp), b->g = take(Mp), b->mvec = take(Mp), b->zero = take(Mp);
  b->scal = take(8), b->gsum = take(NACC), b->gpart = take((size_t)SPARSE_GRAD_BLOCKS_MAX * NACC);
  b->info = reinterpret_cast<long long *>(take(1));
  return off * sizeof(double);
}
static int64_t sparse_mp(const gogp_handle *h) { return ((h->sp_M + PANEL - 1) / PANEL) * PANEL; }

// The multi-output state (gogp_sparse_multi_*): what the multi observe leaves beside the shared Mp x Mp matrices.  Every
// matrix is padded to the tile kernel's 128 (SM_TP = GOGP_SPARSE_MULTI_MAX_T columns or rows, exact zeros from T on), so
// the GEMM_RECT launches take them as they lie: Rt = R^T and Gt = Gamma^T are SM_TP x Mp (a row per output: the dots
// kernel and the products Gamma^T = Rt Binv, Mm = Yu Gt^T, mu = Vt Gt^T read them), Gam = Gamma and Mm = Yu Gamma are
// Mp x SM_TP (Gamma Gamma^T and the second pass's rank-T launch read those).
constexpr int64_t SM_TP = GOGP_SPARSE_MULTI_MAX_T;
static_assert(SM_TP == TILE, "the multi-output matrices are one tile of outputs wide");
struct SparseMultiBufs {
  double *Rt, *Gt, *Gam, *Mm;  // SM_TP x Mp, SM_TP x Mp, Mp x SM_TP, Mp x SM_TP
  double *dots;                // 2 SM_TP: r_t . gamma_t, gamma_t . gamma_t
};
static size_t sparse_multi_layout(double *base, int64_t Mp, SparseMultiBufs *b) {
  const size_t mt = (size_t)Mp * SM_TP;
  b->Rt = base, b->Gt = base ? base + mt : nullptr, b->Gam = base ? base + 2 * mt : nullptr;
  b->Mm = base ? base + 3 * mt : nullptr, b->dots = base ? base + 4 * mt : nullptr;
  return (4 * mt + 2 * SM_TP) * sizeof(double);
}
// bytes of the scratch sized by the chunk: the partials of launch_sparse_xty for every chunk length up to `chunk`, then
// (from *ypad_off doubles on) the chunk's rows of Y padded to chunk x SM_TP for the second pass
static size_t sparse_multi_scratch(int64_t chunk, int64_t M, int T, size_t *ypad_off) {
  const size_t np = sparse_xty_part_doubles(chunk, M, T);
  if (ypad_off) *ypad_off = np;
  return (np + (size_t)chunk * SM_TP) * sizeof(double);
}
static void sparse_multi_free(gogp_handle *h) {
  (void)hipFree(h->sp_Y);
  h->sp_Y = nullptr;
  h->sp_T = 0;
  h->sp_mobserved = false;
  h->sp_myty.clear();
  h->sp_mdots.clear();
  h->sp_mws.release();
  h->sp_mscr.release();
  h->sp_mmu.release();
}

static void sparse_free(gogp_handle *h) {
  if (h->sp_ind) gogp_destroy(h->sp_ind);
  h->sp_ind = nullptr;
  (void)hipFree(h->sp_X);
  (void)hipFree(h->sp_y);
  h->sp_X = h->sp_y = nullptr;
  h->sp_ws.release();
  h->sp_vec.release();
  h->sp_ug.release();
  sparse_multi_free(h);
  h->sp_N = h->sp_M = 0;
  h->sp_have = h->sp_observed = false;
}

// NULL, or the kind of handle the sparse calls refuse (events: another text for a handle with event discounts)
static const char *sparse_refusal(const gogp_handle *h, const char *events = nullptr) {
  return h->prec == 32 ? "precision = 32 handles are not supported"
         : h->dist     ? "sharded handles are not supported"
         : !h->ev()    ? nullptr
         : events      ? events
                       : "event discounts are out of scope of the inducing-point approximation (clear them with gogp_set_events)";
}
// ... which the iterative and the Vecchia calls refuse too, the event discounts in words of their own
int gogp::refuse_handle(gogp_handle *h, const char *who) {
  if (!h) return GOGP_EARG;
  const char *why = sparse_refusal(h, "event discounts are out of scope of the iterative solver (clear them with gogp_set_events)");
  return why ? refuse(h, who, GOGP_EARG, why) : GOGP_OK;
}
static int sparse_refuse(gogp_handle *h, const char *who) {
  char buf[200];
  snprintf(buf, sizeof buf, "%s: %s", who, sparse_refusal(h));
  return fail(h, GOGP_EARG, buf);
}
// an error of the inducing process under the name of the sparse call
static int sparse_fail_from(gogp_handle *h, const char *who, int rc) {
  h->err = std::string(who) + ": " + (h->sp_ind ? h->sp_ind->err : std::string("no inducing process"));
  return rc;
}

extern "C" int gogp_sparse_set_data(gogp_handle *h, const double *X, const double *y, int64_t N, const double *U, int64_t M) {
  if (!h) return GOGP_EARG;
  if (M == 0 && !U) {  // clear
    HIPCHK(h, hipSetDevice(h->device));
    sparse_free(h);
    return GOGP_OK;
  }
  if (sparse_refusal(h)) return sparse_refuse(h, "sparse_set_data");
  if (!U || M < 1 || M > GOGP_SPARSE_MAX_M)
    return fail(h, GOGP_EARG, "sparse_set_data: need U and 1 <= M <= GOGP_SPARSE_MAX_M");
  if (N < 0 || (N > 0 && (!X || !y))) return fail(h, GOGP_EARG, "sparse_set_data: need X and y for N > 0, N >= 0");
  const int D = h->D;
  for (int64_t i = 0; i < M * D; ++i)
    if (!std::isfinite(U[i])) return fail(h, GOGP_EARG, "sparse_set_data: non-finite inducing point");
  for (int64_t i = 0; i < N * D; ++i)
    if (!std::isfinite(X[i])) return fail(h, GOGP_EARG, "sparse_set_data: non-finite input");
  for (int64_t i = 0; i < N; ++i)
    if (!std::isfinite(y[i])) return fail(h, GOGP_EARG, "sparse_set_data: non-finite output");
  HIPCHK(h, hipSetDevice(h->device));
  sparse_free(h);
  // the inducing process: the handle's similarity terms, constant noise (its std is set per Observe), no tiny path (the
  // general sweep leaves Y = L^-T in its buffer)
  gogp_desc d = h->desc;
  d.noise_kind = GOGP_NOISE_CONSTANT;
  d.noise_std = pow(10.0, 0.5 * h->sp_jitter_log10);
  gogp_handle *ind = nullptr;
  int rc = gogp_create(&d, h->device, &ind);
  if (rc != GOGP_OK) return fail(h, rc, "sparse_set_data: the inducing process could not be created");
  h->sp_ind = ind;
  ind->tiny = 0;
  std::vector<double> y0((size_t)M, 0.0);
  rc = gogp_set_data(ind, U, y0.data(), M);
  if (rc != GOGP_OK) {
    rc = sparse_fail_from(h, "sparse_set_data", rc);
    sparse_free(h);
    return rc;
  }
  h->sp_M = M;
  h->sp_N = N;
  const int64_t Mp = sparse_mp(h);
  SparseBufs b;
  rc = h->sp_ws.reserve(h, sparse_layout(nullptr, Mp, &b));
  if (rc != GOGP_OK) {
    sparse_free(h);
    return rc;
  }
  sparse_layout(h->sp_ws.as<double>(), Mp, &b);
  hipStream_t s = ind->s;
  hipError_t e = hipSuccess;
  h->sp_yty = 0.0;
  if (N > 0) {
    const size_t xb = ((size_t)N * D + GOGP_MAX_NDIM) * sizeof(double);
    e = hipMalloc(&h->sp_X, xb);
    if (e == hipSuccess) e = hipMalloc(&h->sp_y, (size_t)N * sizeof(double));
    if (e == hipSuccess) e = hipMemsetAsync(h->sp_X, 0, xb, s);
    if (e == hipSuccess) e = hipMemcpyAsync(h->sp_X, X, (size_t)N * D * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(h->sp_y, y, (size_t)N * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
      launch_sparse_sumsq(s, h->sp_y, N, b.scal);
      e = hipMemcpyAsync(&h->sp_yty, b.scal, sizeof(double), hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
  }
  if (e != hipSuccess) {
    sparse_free(h);
    HIPCHK(h, e);
  }
  h->sp_have = true;
  return GOGP_OK;
}

// The T output columns of the multi flavour: N x T row-major, uploaded as given (no transpose on the host: the kernels
// take the row-major layout), y_t^T y_t of every column once, and the state buffers sized by Mp.
extern "C" int gogp_sparse_multi_set_outputs(gogp_handle *h, const double *Y, int64_t N, int32_t T) {
  if (!h) return GOGP_EARG;
  if (T == 0 && !Y) {  // clear
    HIPCHK(h, hipSetDevice(h->device));
    sparse_multi_free(h);
    return GOGP_OK;
  }
  if (sparse_refusal(h)) return sparse_refuse(h, "sparse_multi_set_outputs");
  if (T < 1 || T > GOGP_SPARSE_MULTI_MAX_T)
    return fail(h, GOGP_EARG, "sparse_multi_set_outputs: need 1 <= T <= GOGP_SPARSE_MULTI_MAX_T");
  if (!h->sp_have) return fail(h, GOGP_ESTATE, "sparse_multi_set_outputs: no sparse data (gogp_sparse_set_data)");
  if (N != h->sp_N) return fail(h, GOGP_EARG, "sparse_multi_set_outputs: N differs from the N of gogp_sparse_set_data");
  if (N > 0 && !Y) return fail(h, GOGP_EARG, "sparse_multi_set_outputs: NULL");
  for (int64_t i = 0; i < N * T; ++i)
    if (!std::isfinite(Y[i])) return fail(h, GOGP_EARG, "sparse_multi_set_outputs: non-finite output");
  HIPCHK(h, hipSetDevice(h->device));
  sparse_multi_free(h);
  SparseMultiBufs mb;
  const int rc = h->sp_mws.reserve(h, sparse_multi_layout(nullptr, sparse_mp(h), &mb));
  if (rc != GOGP_OK) return rc;
  sparse_multi_layout(h->sp_mws.as<double>(), sparse_mp(h), &mb);
  h->sp_myty.assign((size_t)T, 0.0);
  if (N > 0) {
    hipStream_t s = h->sp_ind->s;
    const size_t yb = (size_t)N * T * sizeof(double);
    hipError_t e = hipMalloc(&h->sp_Y, yb);
    if (e == hipSuccess) e = hipMemcpyAsync(h->sp_Y, Y, yb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
      launch_sparse_multi_sumsq(s, h->sp_Y, T, N, T, mb.dots);
      e = hipMemcpyAsync(h->sp_myty.data(), mb.dots, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
      sparse_multi_free(h);
      HIPCHK(h, e);
    }
  }
  h->sp_T = T;
  return GOGP_OK;
}

// C C^T = Bm (256-panel Cholesky on the main stream), Y = C^-T panel by panel, Binv = Y Y^T in full
static void sparse_factor_b(gogp_handle *ind, hipStream_t s, const SparseBufs &b, int64_t M, int64_t Mp) {
  GemmGrid gtri;
  gtri.ktri = ind->ktri;
  for (int64_t c0 = 0; c0 < Mp; c0 += PANEL) {
    const int64_t c2 = c0 + PANEL;
    double *Dp = b.Dinv + (size_t)(c0 / PANEL) * PANEL * PANEL;
    launch_diag256(s, b.Bm + c0 * Mp + c0, Mp, b.C + c0 * Mp + c0, Mp, Dp, c0, M, b.info);
    const int mt2 = (int)((Mp - c2) / TILE);
    if (mt2 > 0) {
      launch_gemm_nt(s, GEMM_RECT, mt2, 2, PANEL, 1.0, b.Bm + c2 * Mp + c0, Mp, Dp, PANEL, 0.0, b.C + c2 * Mp + c0, Mp, nullptr,
                     &gtri);
      launch_gemm_nt(s, GEMM_LOWER, mt2, mt2, PANEL, -1.0, b.C + c2 * Mp + c0, Mp, b.C + c2 * Mp + c0, Mp, 1.0,
                     b.Bm + c2 * Mp + c2, Mp, nullptr);
    }
  }
  for (int64_t c0 = 0; c0 < Mp; c0 += PANEL) {
    const double *Dp = b.Dinv + (size_t)(c0 / PANEL) * PANEL * PANEL;
    launch_ydiag(s, Dp, b.Y + c0 * Mp + c0, Mp);
    if (c0 > 0) {
      const int mt = (int)(c0 / TILE);
      launch_gemm_nt(s, GEMM_RECT, mt, 2, c0, 1.0, b.Y, Mp, b.C + c0 * Mp, Mp, 0.0, b.tmp, PANEL, nullptr);
      launch_gemm_nt(s, GEMM_RECT, mt, 2, PANEL, -1.0, b.tmp, PANEL, Dp, PANEL, 0.0, b.Y + c0, Mp, nullptr);
    }
  }
  const int nt = (int)(Mp / TILE);
  launch_gemm_nt(s, GEMM_RECT, nt, nt, Mp, 1.0, b.Y, Mp, b.Y, Mp, 0.0, b.Binv, Mp, nullptr);
}

// gogp_sparse_observe (bounds == nullptr, `multi` false) and gogp_sparse_multi_observe: one body.  The multi flavour adds
// R^T += Yc^T Vt behind every chunk's launch_sparse_syrk (whose r = V y of the single output it leaves unused), takes
// Gamma = B^-1 R in the place of g = B^-1 r and the per-output dots in the place of r^T g; everything else -- the
// cross-covariances, the substitution, B, its factor, B^-1 and the scalars of B -- is the same launches in the same order.
static int sparse_observe_impl(gogp_handle *h, const char *who, bool multi, const double *x, int64_t len, double *bound,
                               double *bounds) {
  auto msg = [&](const char *what) { return std::string(who) + what; };
  if (sparse_refusal(h)) return sparse_refuse(h, who);
  if (len != h->P) return fail(h, GOGP_EARG, msg(": len(x)").c_str());
  for (int64_t i = 0; i < len; ++i)
    if (!std::isfinite(x[i])) return fail(h, GOGP_EARG, msg(": non-finite parameter").c_str());
  if (!h->sp_have) return fail(h, GOGP_ESTATE, msg(": no sparse data (gogp_sparse_set_data)").c_str());
  if (multi && h->sp_T < 1) return fail(h, GOGP_ESTATE, msg(": no outputs (gogp_sparse_multi_set_outputs)").c_str());
  HIPCHK(h, hipSetDevice(h->device));
  gogp_handle *ind = h->sp_ind;
  const int nT = multi ? h->sp_T : 0;
  h->sp_observed = h->sp_mobserved = false;  // the last observe of either flavour owns the shared workspace
  *bound = NAN;
  for (int t = 0; t < nT && bounds; ++t) bounds[t] = NAN;
  // the parameters on the host: noise variance, its derivative, the output scales
  std::vector<double> th(h->P > 0 ? h->P : 1);
  for (int i = 0; i < h->P; ++i) th[i] = exp(x[i]);
  if (const char *why = theta_refusal(h, th.data(), th.data() + h->ns)) return fail(h, GOGP_EARG, why);
  DevParams hp;
  fill_params_theta(h, th.data(), th.data() + h->ns, hp);
  if (!(hp.noise_var > 0.0) || !std::isfinite(hp.noise_var))
    return fail(h, GOGP_EARG, msg(": the noise variance must be positive and finite").c_str());
  ind->desc.noise_std = pow(10.0, 0.5 * h->sp_jitter_log10);
  ind->cond_limit = h->cond_limit;
  int rc = gogp_observe(ind, x, ind->P, nullptr);
  if (rc == GOGP_ENOTPD) {
    char buf[200];
    h->notpd = ind->notpd;
    snprintf(buf, sizeof buf, "%s: Kuu + jitter is not positive definite (inducing point %lld)", who, (long long)h->notpd);
    h->err = buf;
    return rc;
  }
  if (rc != GOGP_OK && rc != GOGP_ECOND) return sparse_fail_from(h, who, rc);
  const int rcond = rc;
  if (rcond == GOGP_ECOND) h->err = msg(": the factor of Kuu + jitter exceeds the condition limit");
  const int64_t N = h->sp_N, M = h->sp_M, Mp = sparse_mp(h);
  const double s2 = hp.noise_var;
  h->sp_s2 = s2;
  h->sp_dnoise = hp.dnoise;
  h->sp_cterm.assign(hp.c, hp.c + h->desc.nterms);
  h->sp_csum = 0.0;
  for (int t = 0; t < h->desc.nterms; ++t) h->sp_csum += hp.c[t];
  if (N == 0) {
    *bound = 0.0;
    for (int t = 0; t < nT && bounds; ++t) bounds[t] = 0.0;
    if (multi) h->sp_mdots.assign(2 * (size_t)nT, 0.0);
    (multi ? h->sp_mobserved : h->sp_observed) = true;
    return rcond;
  }
  SparseBufs b;
  sparse_layout(h->sp_ws.as<double>(), Mp, &b);
  hipStream_t s = ind->s;
  rc = ensure_alpha(ind);  // the main stream behind the factorisation
  if (rc != GOGP_OK) return sparse_fail_from(h, who, rc);
  const size_t mm = (size_t)Mp * Mp;
  HIPCHK(h, hipMemsetAsync(b.Bacc, 0, 4 * mm * sizeof(double), s));  // Bacc, Bm, C, Y
  HIPCHK(h, hipMemsetAsync(b.r, 0, 4 * (size_t)Mp * sizeof(double), s));  // r, g, mvec, zero
  HIPCHK(h, hipMemsetAsync(b.info, 0, sizeof(long long), s));
  // first pass over the data: V^T of every chunk, B_acc += V V^T, r += V y
  const int64_t chunk = std::min(h->sp_chunk, ((N + TILE - 1) / TILE) * TILE);
  rc = ensure_m(ind, chunk, chunk);
  if (rc != GOGP_OK) return sparse_fail_from(h, who, rc);
  SparseMultiBufs mb = {};
  double *xpart = nullptr;
  if (multi) {
    // (the bound over every chunk length up to `chunk`: a ragged last chunk may take more slabs than a full one)
    const int rcw = h->sp_mscr.reserve(h, sparse_multi_scratch(chunk, M, nT, nullptr));
    if (rcw != GOGP_OK) return rcw;
    xpart = h->sp_mscr.as<double>();
    sparse_multi_layout(h->sp_mws.as<double>(), Mp, &mb);
    HIPCHK(h, hipMemsetAsync(mb.Rt, 0, (size_t)Mp * SM_TP * sizeof(double), s));
  }
  for (int64_t f0 = 0; f0 < N; f0 += chunk) {
    const int64_t m = std::min(chunk, N - f0), mpad = ((m + TILE - 1) / TILE) * TILE;
    launch_cross(s, ind->devP, ind->D, ind->dX, M, Mp, h->sp_X + f0 * ind->D, m, mpad, ind->KsT, Mp, false);
    produce_substitute_t<double>(ind, s, m, mpad, nullptr);
    launch_sparse_syrk(s, ind->Vt, Mp, m, M, Mp, h->sp_y + f0, b.Bacc, Mp, b.r);
    if (multi) launch_sparse_xty(s, ind->Vt, Mp, m, M, h->sp_Y + f0 * nT, nT, nT, xpart, mb.Rt, Mp);
  }
  // the M x M work: B, its factor, B^-1, g = B^-1 r and the scalars
  launch_sparse_finish_b(s, b.Bacc, Mp, 1.0 / s2, b.Bm);
  HIPCHK(h, hipMemcpyAsync(b.Pm, b.Bm, mm * sizeof(double), hipMemcpyDeviceToDevice, s));  // the factorisation consumes Bm
  sparse_factor_b(ind, s, b, M, Mp);
  HIPCHK(h, hipMemcpyAsync(b.Bm, b.Pm, mm * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (multi) {
    // Gamma^T = R^T B^-1 and Gamma = B^-1 R (B^-1 is symmetric in full), then the dots of every output
    const int nt = (int)(Mp / TILE);
    launch_gemm_nt(s, GEMM_RECT, 1, nt, Mp, 1.0, (const double *)mb.Rt, Mp, (const double *)b.Binv, Mp, 0.0, mb.Gt, Mp, nullptr);
    launch_gemm_nt(s, GEMM_RECT, nt, 1, Mp, 1.0, (const double *)b.Binv, Mp, (const double *)mb.Rt, Mp, 0.0, mb.Gam, SM_TP,
                   nullptr);
    launch_sparse_multi_dots(s, mb.Rt, mb.Gt, Mp, M, nT, nT, mb.dots);
    h->sp_mdots.assign(2 * (size_t)nT, 0.0);
    HIPCHK(h, hipMemcpyAsync(h->sp_mdots.data(), mb.dots, 2 * (size_t)nT * sizeof(double), hipMemcpyDeviceToHost, s));
  } else {
    launch_rownorm_dot(s, b.Binv, Mp, b.r, Mp, M, b.g, nullptr);
  }
  launch_sparse_scalars(s, b.C, b.Bm, b.Binv, b.r, b.g, M, Mp, b.scal);
  long long info = 0;
  HIPCHK(h, hipMemcpyAsync(h->sp_scal, b.scal, 5 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(&info, b.info, sizeof info, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  if (info != 0)
    return fail(h, GOGP_EHIP, msg(": the factorisation of B = I + V V^T / s2 met a non-positive pivot").c_str());
  const double logdetB = h->sp_scal[0], trBmM = h->sp_scal[1], rtg = h->sp_scal[3];
  const double t0 = (double)N * h->sp_csum;
  if (multi) {  // bound_t = c0 - y_t^T y_t / (2 s2) + r_t^T gamma_t / (2 s2^2), their sum in column order
    const double c0 = -0.5 * (double)N * log(2 * M_PI) - 0.5 * logdetB - 0.5 * (double)N * log(s2) - (t0 - s2 * trBmM) / (2 * s2);
    double total = 0.0;
    for (int t = 0; t < nT; ++t) {
      const double bt = c0 - h->sp_myty[(size_t)t] / (2 * s2) + h->sp_mdots[(size_t)t] / (2 * s2 * s2);
      if (bounds) bounds[t] = bt;
      total += bt;
    }
    *bound = total;
    h->sp_mobserved = true;
    return rcond;
  }
  *bound = -0.5 * (double)N * log(2 * M_PI) - 0.5 * logdetB - 0.5 * (double)N * log(s2) - h->sp_yty / (2 * s2) +
           rtg / (2 * s2 * s2) - (t0 - s2 * trBmM) / (2 * s2);
  h->sp_observed = true;
  return rcond;
}

extern "C" int gogp_sparse_observe(gogp_handle *h, const double *x, int64_t len, double *bound) {
  if (!h || !x || !bound) return fail(h, GOGP_EARG, "sparse_observe: NULL");
  return sparse_observe_impl(h, "sparse_observe", false, x, len, bound, nullptr);
}

extern "C" int gogp_sparse_multi_observe(gogp_handle *h, const double *x, int64_t len, double *total, double *bounds) {
  if (!h || !x || !total) return fail(h, GOGP_EARG, "sparse_multi_observe: NULL");
  return sparse_observe_impl(h, "sparse_multi_observe", true, x, len, total, bounds);
}

// gogp_sparse_gradient (dU == nullptr) and gogp_sparse_gradient_inducing: with dU, the second pass over the data also
// reduces the (U, X) pairs on dk/du (launch_sparse_ugrad: the chunk's Wt, mvec, y and s4 of launch_sparse_grad) and
// the (U, U) pairs go through the input-gradient reduction of the full Observe form (launch_xgrad) with a zero alpha
// and -G as its K^-1:  dU = 2 (U, U part) + (U, X part) -- u_a enters Kuu through row a and column a.
// The multi flavour (gogp_sparse_multi_gradient*): T and S carry the number of outputs and Gamma Gamma^T in the place of
// g g^T, the rank-one term y_f m_u / s2^2 of the weights becomes the rank-T term Yc Mm^T / s2^2, which one more
// GEMM_RECT launch adds to the chunk's Wt, and the pair reductions run unchanged with the zero vector as mvec.
static int sparse_gradient_impl(gogp_handle *h, const char *who, bool multi, double *grad, int64_t len, double *dU) {
  auto msg = [&](const char *what) { return std::string(who) + what; };
  if (sparse_refusal(h)) return sparse_refuse(h, who);
  if (len != h->P) return fail(h, GOGP_EARG, msg(": wrong length").c_str());
  if (!h->sp_have) return fail(h, GOGP_ESTATE, msg(": no sparse data (gogp_sparse_set_data)").c_str());
  if (multi && h->sp_T < 1) return fail(h, GOGP_ESTATE, msg(": no outputs (gogp_sparse_multi_set_outputs)").c_str());
  if (!(multi ? h->sp_mobserved : h->sp_observed))
    return fail(h, GOGP_ESTATE, msg(multi ? " before sparse_multi_observe" : " before sparse_observe").c_str());
  for (int64_t i = 0; i < len; ++i) grad[i] = 0.0;
  const int64_t N = h->sp_N, M = h->sp_M, Mp = sparse_mp(h);
  const int64_t md = M * h->D;
  if (dU)
    for (int64_t i = 0; i < md; ++i) dU[i] = 0.0;
  if (N == 0) return GOGP_OK;
  HIPCHK(h, hipSetDevice(h->device));
  gogp_handle *ind = h->sp_ind;
  SparseBufs b;
  sparse_layout(h->sp_ws.as<double>(), Mp, &b);
  hipStream_t s = ind->s;
  const int64_t chunk = std::min(h->sp_chunk, ((N + TILE - 1) / TILE) * TILE);
  double *upart = nullptr, *dux = nullptr, *duu = nullptr;  // the slab partials, the (U, X) and the (U, U) part
  if (dU) {
    // (the bound over every chunk length up to `chunk`: a ragged last chunk may take more slabs than a full one)
    const size_t np = (size_t)sparse_ugrad_slabs_bound(chunk, M) * (size_t)md;
    const int rcw = h->sp_ug.reserve(h, (np + 2 * (size_t)md) * sizeof(double));
    if (rcw != GOGP_OK) return rcw;
    upart = h->sp_ug.as<double>(), dux = upart + np, duu = dux + md;
  }
  const int nT = multi ? h->sp_T : 1;
  const int64_t kT = ((nT + GEMM_BK - 1) / GEMM_BK) * GEMM_BK;  // the K of the rank-T launch: T padded with zeros
  SparseMultiBufs mb = {};
  double *ypad = nullptr;
  if (multi) {
    size_t yoff = 0;
    const int rcw = h->sp_mscr.reserve(h, sparse_multi_scratch(chunk, M, nT, &yoff));
    if (rcw != GOGP_OK) return rcw;
    ypad = h->sp_mscr.as<double>() + yoff;
    sparse_multi_layout(h->sp_mws.as<double>(), Mp, &mb);
  }
  int rc = compute_kinv(ind);  // Y = L^-T of the inducing process in its bufY, the main stream behind it
  if (rc != GOGP_OK) return sparse_fail_from(h, who, rc);
  const double s2 = h->sp_s2, s4 = 1.0 / (s2 * s2);
  // (the upper triangle of the inducing process's bufY: what lies below its super-panels is not part of Y)
  launch_sparse_copy_upper(s, ind->bufY, Mp, b.Yu);
  const double *Yu = b.Yu;
  double *T = b.Bacc, *S = b.C, *W1 = b.Y;
  const int nt = (int)(Mp / TILE);
  // T and S, then P = Yu T Yu^T / (2 s2), G = Yu S Yu^T / 2 (both triangles), m = Yu g
  if (multi) {  // (Gamma Gamma^T goes through W1, which the next product overwrites)
    launch_gemm_nt(s, GEMM_RECT, nt, nt, SM_TP, 1.0, (const double *)mb.Gam, SM_TP, (const double *)mb.Gam, SM_TP, 0.0, W1, Mp,
                   nullptr);
    launch_sparse_multi_weights(s, b.Bm, b.Binv, W1, Mp, nT, s4, T, S);
  } else {
    launch_sparse_weights(s, b.Bm, b.Binv, b.g, Mp, s4, T, S);
  }
  launch_gemm_nt(s, GEMM_RECT, nt, nt, Mp, 1.0, Yu, Mp, T, Mp, 0.0, W1, Mp, nullptr);
  launch_gemm_nt(s, GEMM_RECT, nt, nt, Mp, 1.0 / (2 * s2), W1, Mp, Yu, Mp, 0.0, b.Pm, Mp, nullptr);
  launch_gemm_nt(s, GEMM_RECT, nt, nt, Mp, 1.0, Yu, Mp, S, Mp, 0.0, W1, Mp, nullptr);
  // (the reduction of the LML gradient forms sum_ab (alpha_a alpha_b - Kinv_ab) dK_ab: G goes in negated, alpha zero)
  launch_gemm_nt(s, GEMM_RECT, nt, nt, Mp, -0.5, W1, Mp, Yu, Mp, 0.0, b.Gm, Mp, nullptr);
  if (multi)  // Mm = Yu Gamma, M x T
    launch_gemm_nt(s, GEMM_RECT, nt, 1, Mp, 1.0, Yu, Mp, (const double *)mb.Gt, Mp, 0.0, mb.Mm, SM_TP, nullptr);
  else
    launch_rownorm_dot(s, Yu, Mp, b.g, Mp, M, b.mvec, nullptr);
  const double *mvec = multi ? b.zero : b.mvec;
  launch_grad_reduce(s, ind->devP, ind->D, ind->ard_dims, ind->dX, b.zero, (const double *)b.Gm, Mp, M, Mp, ind->gpart,
                     ind->gout, ind->radial1, ind->ard_mfma_min, false);
  // (launch_xgrad mirrors its matrix in place: behind the reduction that has read Gm)
  if (dU) launch_xgrad(s, ind->devP, ind->D, ind->dX, b.zero, b.Gm, Mp, M, Mp, duu, false);
  // second pass over the data: the chunk's cross-covariance again, Wt = Ks^T 2 P, the pair reduction
  rc = ensure_m(ind, chunk, chunk);
  if (rc != GOGP_OK) return sparse_fail_from(h, who, rc);
  GemmGrid gw;
  gw.small_below = ind->produce_small_below;
  for (int64_t f0 = 0; f0 < N; f0 += chunk) {
    const int64_t m = std::min(chunk, N - f0), mpad = ((m + TILE - 1) / TILE) * TILE;
    launch_cross(s, ind->devP, ind->D, ind->dX, M, Mp, h->sp_X + f0 * ind->D, m, mpad, ind->KsT, Mp, false);
    launch_gemm_nt(s, GEMM_RECT, (int)(mpad / TILE), nt, Mp, 2.0, (const double *)ind->KsT, Mp, (const double *)b.Pm, Mp,
                   0.0, ind->Vt, Mp, nullptr, &gw);
    if (multi) {  // Wt += Yc Mm^T / s2^2
      // (mpad is a multiple of TILE and kT of GEMM_BK: whole workgroups of 256 elements, which the launcher requires)
      static_assert((TILE * GEMM_BK) % 256 == 0, "launch_sparse_multi_pad launches nothing unless rpad * kp % 256 == 0");
      launch_sparse_multi_pad(s, h->sp_Y + f0 * nT, nT, m, nT, kT, mpad, ypad, SM_TP);
      launch_gemm_nt(s, GEMM_RECT, (int)(mpad / TILE), nt, kT, s4, (const double *)ypad, SM_TP, (const double *)mb.Mm, SM_TP,
                     1.0, ind->Vt, Mp, nullptr, &gw);
    }
    launch_sparse_grad(s, ind->devP, ind->D, ind->ard_dims, h->sp_X + f0 * ind->D, m, ind->dX, M, ind->Vt, Mp, h->sp_y + f0,
                       mvec, s4, b.gpart, b.gsum, f0 > 0);
    if (dU)
      launch_sparse_ugrad(s, ind->devP, ind->D, h->sp_X + f0 * ind->D, m, ind->dX, M, ind->Vt, Mp, h->sp_y + f0, mvec, s4,
                          upart, dux, f0 > 0);
  }
  double acc[NACC], accu[NACC];
  std::vector<double> hu;
  HIPCHK(h, hipMemcpyAsync(acc, b.gsum, sizeof acc, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(accu, ind->gout, sizeof accu, hipMemcpyDeviceToHost, s));
  if (dU) {
    hu.resize((size_t)md);
    HIPCHK(h, hipMemcpyAsync(dU, dux, (size_t)md * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(hu.data(), duu, (size_t)md * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  if (dU)
    for (int64_t i = 0; i < md; ++i) dU[i] = 2.0 * hu[(size_t)i] + dU[i];
  // assemble_gradient halves the slot sums (the LML's 1/2 tr): (W, dKuf) + (G, dKuu) go in doubled
  for (int q = 0; q < NACC; ++q) acc[q] = 2.0 * (acc[q] + accu[q]);
  acc[ACC_TRACE] = 0.0;
  assemble_gradient(h, acc, 0.0, grad);
  // the diagonal term -1/(2 s2) sum_f dk(x_f, x_f): the output scales alone
  for (int t = 0; t < h->desc.nterms; ++t)
    if (h->desc.terms[t].scale_idx >= 0) grad[h->desc.terms[t].scale_idx] -= (double)nT * (double)N * h->sp_cterm[t] / (2 * s2);
  if (h->nn > 0 && multi) {  // the sums over the outputs in column order
    double yty = 0.0, rtg = 0.0, gtg = 0.0;
    for (int t = 0; t < nT; ++t) yty += h->sp_myty[(size_t)t], rtg += h->sp_mdots[(size_t)t], gtg += h->sp_mdots[(size_t)(nT + t)];
    const double trBmM = h->sp_scal[1], trBinv = h->sp_scal[2];
    const double t0 = (double)N * h->sp_csum, s6 = s2 * s2 * s2;
    const double dF = (double)nT * (((double)M - trBinv) / (2 * s2) - (double)N / (2 * s2) + (t0 - s2 * trBmM) / (2 * s2 * s2)) +
                      yty / (2 * s2 * s2) - rtg / s6 + (rtg - gtg) / (2 * s6);
    grad[h->ns] = h->sp_dnoise * dF;
  } else if (h->nn > 0) {
    const double trBmM = h->sp_scal[1], trBinv = h->sp_scal[2], rtg = h->sp_scal[3], gtg = h->sp_scal[4];
    const double t0 = (double)N * h->sp_csum, s6 = s2 * s2 * s2;
    const double dF = ((double)M - trBinv) / (2 * s2) - (double)N / (2 * s2) + h->sp_yty / (2 * s2 * s2) - rtg / s6 +
                      (rtg - gtg) / (2 * s6) + (t0 - s2 * trBmM) / (2 * s2 * s2);
    grad[h->ns] = h->sp_dnoise * dF;
  }
  return GOGP_OK;
}

extern "C" int gogp_sparse_gradient(gogp_handle *h, double *grad, int64_t len) {
  if (!h || !grad) return fail(h, GOGP_EARG, "sparse_gradient: NULL");
  return sparse_gradient_impl(h, "sparse_gradient", false, grad, len, nullptr);
}

extern "C" int gogp_sparse_multi_gradient(gogp_handle *h, double *grad, int64_t len) {
  if (!h || !grad) return fail(h, GOGP_EARG, "sparse_multi_gradient: NULL");
  return sparse_gradient_impl(h, "sparse_multi_gradient", true, grad, len, nullptr);
}

extern "C" int gogp_sparse_gradient_inducing(gogp_handle *h, double *grad, int64_t len, double *dU) {
  if (!h || !grad || !dU) return fail(h, GOGP_EARG, "sparse_gradient_inducing: NULL");
  return sparse_gradient_impl(h, "sparse_gradient_inducing", false, grad, len, dU);
}

extern "C" int gogp_sparse_multi_gradient_inducing(gogp_handle *h, double *grad, int64_t len, double *dU) {
  if (!h || !grad || !dU) return fail(h, GOGP_EARG, "sparse_multi_gradient_inducing: NULL");
  return sparse_gradient_impl(h, "sparse_multi_gradient_inducing", true, grad, len, dU);
}

// The inducing points alone: the inducing process is given (U, y = 0) again -- its buffers are sized by M, which stays --
// and X, y, the workspaces and the options are kept.
extern "C" int gogp_sparse_set_inducing(gogp_handle *h, const double *U, int64_t M) {
  if (!h) return GOGP_EARG;
  if (sparse_refusal(h)) return sparse_refuse(h, "sparse_set_inducing");
  if (!U) return fail(h, GOGP_EARG, "sparse_set_inducing: NULL");
  if (!h->sp_have) return fail(h, GOGP_ESTATE, "sparse_set_inducing: no sparse data (gogp_sparse_set_data)");
  if (M != h->sp_M) return fail(h, GOGP_EARG, "sparse_set_inducing: M differs from the M of gogp_sparse_set_data");
  for (int64_t i = 0; i < M * h->D; ++i)
    if (!std::isfinite(U[i])) return fail(h, GOGP_EARG, "sparse_set_inducing: non-finite inducing point");
  HIPCHK(h, hipSetDevice(h->device));
  h->sp_observed = h->sp_mobserved = false;
  std::vector<double> y0((size_t)M, 0.0);
  const int rc = gogp_set_data(h->sp_ind, U, y0.data(), M);
  return rc == GOGP_OK ? rc : sparse_fail_from(h, "sparse_set_inducing", rc);
}

extern "C" int gogp_sparse_produce(gogp_handle *h, const double *Z, int64_t m, double *mu, double *sigma) {
  if (!h || m < 0 || (m > 0 && (!Z || !mu || !sigma))) return fail(h, GOGP_EARG, "sparse_produce: NULL");
  if (sparse_refusal(h)) return sparse_refuse(h, "sparse_produce");
  if (!h->sp_have) return fail(h, GOGP_ESTATE, "sparse_produce: no sparse data (gogp_sparse_set_data)");
  if (!h->sp_observed) return fail(h, GOGP_ESTATE, "sparse_produce before sparse_observe");
  for (int64_t i = 0; i < m * h->D; ++i)
    if (!std::isfinite(Z[i])) return fail(h, GOGP_EARG, "sparse_produce: non-finite test point");
  if (m == 0) return GOGP_OK;
  gogp_handle *ind = h->sp_ind;
  const int64_t M = h->sp_M, Mp = sparse_mp(h);
  ProducePlan pp;
  int rc = produce_prepare(ind, nullptr, "sparse_produce", m, false, &pp);
  if (rc != GOGP_OK) return sparse_fail_from(h, "sparse_produce", rc);
  rc = h->sp_vec.reserve(h, (size_t)pp.mpad * sizeof(double));
  if (rc != GOGP_OK) return rc;
  hipStream_t s = ind->s;
  const bool empty = h->sp_N == 0;
  // the tile route of Produce on the inducing process, whatever m: it leaves v^T = (L^-1 k(U, z))^T in Vt row by row
  // and |v|^2 in pp.q
  rc = produce_forward(ind, Z, m, pp, true, !empty);
  if (rc != GOGP_OK) return sparse_fail_from(h, "sparse_produce", rc);
  if (empty) {  // no observations: the prior
    rc = produce_of_the_prior(ind, pp, m, mu, sigma);
    return rc == GOGP_OK ? rc : sparse_fail_from(h, "sparse_produce", rc);
  }
  SparseBufs b;
  sparse_layout(h->sp_ws.as<double>(), Mp, &b);
  double *dot = h->sp_vec.as<double>();
  launch_rownorm_dot(s, (const double *)ind->Vt, Mp, b.g, Mp, m, dot, nullptr);
  GemmGrid gm;
  gm.small_below = ind->produce_small_below;
  launch_gemm_nt(s, GEMM_RECT, (int)(pp.mpad / TILE), (int)(Mp / TILE), Mp, 1.0, (const double *)ind->Vt, Mp,
                 (const double *)b.Binv, Mp, 0.0, ind->KsT, Mp, nullptr, &gm);
  launch_sparse_predict(s, ind->KsT, ind->Vt, Mp, M, m, pp.prior, pp.q, dot, 1.0 / h->sp_s2, pp.mu, pp.sigma);
  HIPCHK(h, hipMemcpyAsync(mu, pp.mu, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(sigma, pp.sigma, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  return GOGP_OK;
}

// gogp_sparse_produce for the T outputs of the multi observe: sigma as there (the outputs share it), the m x T means
// from one product, mu = Vt Gamma / s2.
extern "C" int gogp_sparse_multi_produce(gogp_handle *h, const double *Z, int64_t m, double *mu, double *sigma) {
  if (!h || m < 0 || (m > 0 && (!Z || !mu || !sigma))) return fail(h, GOGP_EARG, "sparse_multi_produce: NULL");
  if (sparse_refusal(h)) return sparse_refuse(h, "sparse_multi_produce");
  if (!h->sp_have) return fail(h, GOGP_ESTATE, "sparse_multi_produce: no sparse data (gogp_sparse_set_data)");
  if (h->sp_T < 1) return fail(h, GOGP_ESTATE, "sparse_multi_produce: no outputs (gogp_sparse_multi_set_outputs)");
  if (!h->sp_mobserved) return fail(h, GOGP_ESTATE, "sparse_multi_produce before sparse_multi_observe");
  for (int64_t i = 0; i < m * h->D; ++i)
    if (!std::isfinite(Z[i])) return fail(h, GOGP_EARG, "sparse_multi_produce: non-finite test point");
  if (m == 0) return GOGP_OK;
  gogp_handle *ind = h->sp_ind;
  const int64_t M = h->sp_M, Mp = sparse_mp(h);
  const int nT = h->sp_T;
  ProducePlan pp;
  int rc = produce_prepare(ind, nullptr, "sparse_multi_produce", m, false, &pp);
  if (rc != GOGP_OK) return sparse_fail_from(h, "sparse_multi_produce", rc);
  rc = h->sp_mmu.reserve(h, (size_t)pp.mpad * SM_TP * sizeof(double));
  if (rc != GOGP_OK) return rc;
  hipStream_t s = ind->s;
  const bool empty = h->sp_N == 0;
  rc = produce_forward(ind, Z, m, pp, true, !empty);
  if (rc != GOGP_OK) return sparse_fail_from(h, "sparse_multi_produce", rc);
  if (empty) {  // no observations: the prior, a zero mean for every output
    std::vector<double> mu0((size_t)m);
    rc = produce_of_the_prior(ind, pp, m, mu0.data(), sigma);
    for (int64_t i = 0; i < m * nT; ++i) mu[i] = 0.0;
    return rc == GOGP_OK ? rc : sparse_fail_from(h, "sparse_multi_produce", rc);
  }
  SparseBufs b;
  sparse_layout(h->sp_ws.as<double>(), Mp, &b);
  SparseMultiBufs mb;
  sparse_multi_layout(h->sp_mws.as<double>(), Mp, &mb);
  double *dmu = h->sp_mmu.as<double>();
  GemmGrid gm;
  gm.small_below = ind->produce_small_below;
  launch_gemm_nt(s, GEMM_RECT, (int)(pp.mpad / TILE), 1, Mp, 1.0 / h->sp_s2, (const double *)ind->Vt, Mp, (const double *)mb.Gt,
                 Mp, 0.0, dmu, SM_TP, nullptr, &gm);
  launch_gemm_nt(s, GEMM_RECT, (int)(pp.mpad / TILE), (int)(Mp / TILE), Mp, 1.0, (const double *)ind->Vt, Mp,
                 (const double *)b.Binv, Mp, 0.0, ind->KsT, Mp, nullptr, &gm);
  launch_sparse_multi_sigma(s, ind->KsT, ind->Vt, Mp, M, m, pp.prior, pp.q, pp.sigma);
  HIPCHK(h, hipMemcpy2DAsync(mu, (size_t)nT * sizeof(double), dmu, (size_t)SM_TP * sizeof(double), (size_t)nT * sizeof(double),
                             (size_t)m, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(sigma, pp.sigma, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  return GOGP_OK;
}

// ---- choosing the inducing points (select.hip) ------------------------------------------------------------------------
// gogp_sparse_select_inducing (X given: uploaded for the call) and gogp_sparse_select_inducing_resident (X == nullptr
// with resident: the rows of sp_X): one body.  Every buffer is the call's own -- the parameters too, so that devP keeps
// what the last evaluation uploaded -- on the handle's main stream, freed before the call returns: nothing of the handle
// changes but its error string.
static int sparse_select_impl(gogp_handle *h, const char *who, bool resident, const double *x, int64_t len, const double *X,
                              int64_t N, int64_t M, double tol, int64_t *idx, double *pivots, double *U, int64_t *m_out,
                              double *trace) {
  auto msg = [&](const char *what) { return std::string(who) + what; };
  if (!h) return GOGP_EARG;
  if (!x || !idx || !m_out) return fail(h, GOGP_EARG, msg(": NULL").c_str());
  if (sparse_refusal(h)) return sparse_refuse(h, who);
  if (len != h->P) return fail(h, GOGP_EARG, msg(": len(x)").c_str());
  for (int64_t i = 0; i < len; ++i)
    if (!std::isfinite(x[i])) return fail(h, GOGP_EARG, msg(": non-finite parameter").c_str());
  if (M < 1 || M > GOGP_SPARSE_MAX_M) return fail(h, GOGP_EARG, msg(": need 1 <= M <= GOGP_SPARSE_MAX_M").c_str());
  if (std::isnan(tol) || tol == INFINITY) return fail(h, GOGP_EARG, msg(": tol must be finite or negative").c_str());
  const int D = h->D;
  if (resident) {
    if (!h->sp_have) return fail(h, GOGP_ESTATE, msg(": no sparse data (gogp_sparse_set_data)").c_str());
    N = h->sp_N;
  } else {
    if (N < 0 || (N > 0 && !X)) return fail(h, GOGP_EARG, msg(": need X for N > 0, N >= 0").c_str());
    for (int64_t i = 0; i < N * D; ++i)
      if (!std::isfinite(X[i])) return fail(h, GOGP_EARG, msg(": non-finite input").c_str());
  }
  std::vector<double> th(h->P > 0 ? h->P : 1);
  for (int i = 0; i < h->P; ++i) th[i] = exp(x[i]);
  if (const char *why = theta_refusal(h, th.data(), th.data() + h->ns)) return fail(h, GOGP_EARG, why);
  if (tol < 0.0) tol = pow(10.0, (double)h->sp_jitter_log10);
  *m_out = 0;
  if (N == 0) {
    if (trace) *trace = 0.0;
    return GOGP_OK;
  }
  DevParams hp;
  fill_params_theta(h, th.data(), th.data() + h->ns, hp);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->s;
  const int64_t cols = std::min(M, N);
  SelectBufs b;
  const size_t small = select_layout(nullptr, N, M, D, &b);
  const size_t xbytes = resident ? 0 : (size_t)N * D * sizeof(double);
  const size_t lbytes = (size_t)cols * (size_t)b.ldn * sizeof(double);
  char *work = nullptr;
  double *dXc = nullptr, *Lt = nullptr;
  DevParams *dP = nullptr;
  auto release = [&]() {
    (void)hipFree(work);
    (void)hipFree(dXc);
    (void)hipFree(Lt);
    (void)hipFree(dP);
  };
  hipError_t e = hipMalloc(&Lt, lbytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    char buf[200];
    snprintf(buf, sizeof buf, "%s: the transient factor (%lld columns of %lld doubles, %.3f GB) could not be allocated: %s",
             who, (long long)cols, (long long)b.ldn, (double)lbytes * 1e-9, hipGetErrorString(e));
    h->err = buf;
    return e == hipErrorOutOfMemory ? GOGP_ENOMEM : GOGP_EHIP;
  }
  e = hipMalloc(&work, small);
  if (e == hipSuccess && !resident) e = hipMalloc(&dXc, xbytes);
  if (e == hipSuccess) e = hipMalloc(&dP, sizeof(DevParams));
  if (e == hipSuccess) e = hipMemcpyAsync(dP, &hp, sizeof hp, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && !resident) e = hipMemcpyAsync(dXc, X, xbytes, hipMemcpyHostToDevice, s);
  int64_t m = 0;
  if (e == hipSuccess) {
    select_layout(work, N, M, D, &b);
    b.Lt = Lt;
    e = select_run(s, dP, D, resident ? h->sp_X : dXc, N, M, tol, 0, nullptr, b, &m);
  }
  std::vector<long long> hpiv((size_t)(m > 0 ? m : 1));
  if (e == hipSuccess && m > 0) {
    e = hipMemcpyAsync(hpiv.data(), b.piv, (size_t)m * sizeof(long long), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && pivots) e = hipMemcpyAsync(pivots, b.pv, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && U) e = hipMemcpyAsync(U, b.U, (size_t)m * D * sizeof(double), hipMemcpyDeviceToHost, s);
  }
  if (e == hipSuccess && trace) e = hipMemcpyAsync(trace, b.trace, sizeof(double), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  else (void)hipStreamSynchronize(s);  // nothing enqueued may outlive the buffers
  release();
  HIPCHK(h, e);
  for (int64_t j = 0; j < m; ++j) idx[j] = (int64_t)hpiv[(size_t)j];
  *m_out = m;
  return GOGP_OK;
}

extern "C" int gogp_sparse_select_inducing(gogp_handle *h, const double *x, int64_t len, const double *X, int64_t N, int64_t M,
                                           double tol, int64_t *idx, double *pivots, double *U, int64_t *m_out,
                                           double *trace) {
  return sparse_select_impl(h, "sparse_select_inducing", false, x, len, X, N, M, tol, idx, pivots, U, m_out, trace);
}

extern "C" int gogp_sparse_select_inducing_resident(gogp_handle *h, const double *x, int64_t len, int64_t M, double tol,
                                                    int64_t *idx, double *pivots, double *U, int64_t *m_out, double *trace) {
  return sparse_select_impl(h, "sparse_select_inducing_resident", true, x, len, nullptr, 0, M, tol, idx, pivots, U, m_out,
                            trace);
}

// ---- non-Gaussian likelihoods by the Laplace approximation (laplace.hip) -----------------------------------------------
// No reference counterpart.  The formulas are in laplace.hip and DESIGN.md section 4 "Laplace".  Every Newton step is
// one non-eager factorize_t<double> of B = I + diag(sw) K diag(sw) -- the Gram stage scales K (Sweep::build_gram), the
// sweep's working copy is the step's right-hand side, so z = L^-1 rhs and beta = B^-1 rhs (in h->alpha) come with the
// factor -- around two matrix-free products with K and a few passes over vectors; the host reads five doubles per
// evaluation of psi.  The general sweep runs at every n (the one-launch path of tiny_factorize builds K itself).
struct LapVecs {
  double *a, *f, *a1, *f1, *at, *ft, *g, *W, *sw, *b, *rho, *kv, *rhs, *sv, *u, *awarm, *kpart, *part, *out;
};
static size_t lap_layout(double *q, int64_t npad, LapVecs *v) {
  const size_t np = (size_t)npad;
  double **vec[] = {&v->a, &v->f, &v->a1, &v->f1, &v->at, &v->ft, &v->g, &v->W, &v->sw, &v->b, &v->rho, &v->kv, &v->rhs,
                    &v->sv, &v->u, &v->awarm};
  size_t off = 0;
  auto at = [&](size_t count) {  // (q == nullptr: the size alone is asked for)
    double *p = q ? q + off : nullptr;
    off += count;
    return p;
  };
  for (double **p : vec) *p = at(np);
  v->kpart = at((size_t)REFINE_SLABS * np);  // the slabs of launch_kmatvec_share
  v->part = at(5 * (np / PANEL));
  v->out = at(8);
  return off * sizeof(double);
}
static int lap_vecs(gogp_handle *h, LapVecs *v) {
  const int rc = h->lap_ws.reserve(h, lap_layout(nullptr, std::max(h->npad, h->cap_npad), v));
  if (rc != GOGP_OK) return rc;
  lap_layout(h->lap_ws.as<double>(), h->npad, v);
  return GOGP_OK;
}
static inline bool lap_lik_ok(int32_t lik) { return lik == GOGP_LIK_BERNOULLI_LOGIT || lik == GOGP_LIK_POISSON_LOG; }
static const char *lap_refusal(const gogp_handle *h) {
  return h->prec == 32         ? "precision = 32 handles"
         : h->grad_prec == 32 ? "gradient_precision = 32"
         : h->dist            ? "sharded handles"
                              : nullptr;
}
static int lap_refuse(gogp_handle *h, const char *who) {
  const char *why = lap_refusal(h);
  if (!why) return GOGP_OK;
  char buf[160];
  snprintf(buf, sizeof buf, "%s: %s are not supported", who, why);
  return fail(h, GOGP_EARG, buf);
}

extern "C" int gogp_laplace_check(int32_t lik, const double *y, int64_t n) {
  if (!lap_lik_ok(lik) || n < 0 || (n > 0 && !y)) return GOGP_EARG;
  for (int64_t i = 0; i < n; ++i) {
    const double v = y[i];
    const bool ok = lik == GOGP_LIK_BERNOULLI_LOGIT ? (v == 0.0 || v == 1.0)
                                                    : (v >= 0.0 && v <= 9007199254740992.0 && v == floor(v));
    if (!ok) return GOGP_EARG;
  }
  return GOGP_OK;
}

// v -> K v on the main stream (kv and kpart of the workspace are free between the steps)
static void lap_kmatvec(gogp_handle *h, const LapVecs &v, const double *in, double *out) {
  launch_kmatvec_share(h->s, h->devP, h->D, h->dX, h->n, h->npad, in, 0, 1, v.kpart, REFINE_SLABS, out, h->radial1, h->ev());
}
// The site functions at (a, f) into the workspace and hs[0 .. 4] (laplace.hip: launch_lap_site) on the host
static int lap_sites(gogp_handle *h, const LapVecs &v, int lik, const double *a, const double *f, double *hs) {
  launch_lap_site(h->s, lik, f, h->dy, a, h->n, h->npad, v.g, v.W, v.sw, v.b, v.rho, v.part, v.out);
  HIPCHK(h, hipMemcpyAsync(hs, v.out, 5 * sizeof(double), hipMemcpyDeviceToHost, h->s));
  HIPCHK(h, hipStreamSynchronize(h->s));
  HIPCHK(h, hipGetLastError());
  return GOGP_OK;
}
// One factorisation of B at the site vectors in the workspace, with rhs as the sweep's right-hand side: beta = B^-1 rhs
// is in h->alpha and ordered on the main stream afterwards.  What it says about a REGRESSION state is taken back.
static int lap_factorize(gogp_handle *h, const LapVecs &v) {
  h->lap_sw = v.sw;
  h->lap_rhs = v.rhs;
  int rc = factorize_t<double>(h, false);
  h->lap_sw = h->lap_rhs = nullptr;
  if (rc == GOGP_OK || rc == GOGP_ECOND) {
    const int rca = ensure_alpha(h);
    if (rca != GOGP_OK) rc = rca;
  }
  h->factored = h->have_alpha = h->observed = h->with_obs = h->z_valid = false;
  return rc;
}

// The Newton iteration from a = 0 (or, `warm`, the stored a^); on return *conv says whether the tolerance was reached.
// GOGP_OK / GOGP_ECOND: B's factor at the last iterate is in place, h->lap_iters and *psi belong to it.
static int lap_newton(gogp_handle *h, const LapVecs &v, int lik, bool warm, bool *conv, double *psi_out) {
  hipStream_t s = h->s;
  const int64_t n = h->n, npad = h->npad;
  const size_t vec = (size_t)npad * sizeof(double);
  const double tol = pow(10.0, (double)h->lap_tol_log10);
  if (warm) {
    HIPCHK(h, hipMemcpyAsync(v.a, v.awarm, vec, hipMemcpyDeviceToDevice, s));
    lap_kmatvec(h, v, v.a, v.f);
  } else {
    HIPCHK(h, hipMemsetAsync(v.a, 0, vec, s));
    HIPCHK(h, hipMemsetAsync(v.f, 0, vec, s));
  }
  double hs[5];
  int rc = lap_sites(h, v, lik, v.a, v.f, hs);
  if (rc != GOGP_OK) return rc;
  if (hs[4] >= 0.0) {
    char buf[160];
    snprintf(buf, sizeof buf, "laplace_observe: y[%lld] is not a value of the likelihood", (long long)hs[4]);
    return fail(h, GOGP_EARG, buf);
  }
  double psi = -0.5 * hs[1] + hs[0];
  bool stuck = false;
  int rcf = GOGP_OK;
  h->lap_iters = 0;
  *conv = false;
  for (;;) {
    *conv = hs[2] <= tol * std::max(1.0, hs[3]);
    const bool stop = *conv || stuck || h->lap_iters >= h->lap_max_iter;
    // rhs = sw o (K b); at the last iterate the factor alone is wanted and the right-hand side is whatever rhs holds
    if (!stop) {
      lap_kmatvec(h, v, v.b, v.kv);
      launch_lap_vec(s, nullptr, v.sw, v.kv, n, npad, v.rhs);
    } else {
      HIPCHK(h, hipMemsetAsync(v.rhs, 0, vec, s));
    }
    rcf = lap_factorize(h, v);
    if (rcf != GOGP_OK && rcf != GOGP_ECOND) return rcf;
    if (stop) break;
    // a+ = b - sw o beta, f+ = K a+
    launch_lap_vec(s, v.b, v.sw, h->alpha, n, npad, v.a1);
    lap_kmatvec(h, v, v.a1, v.f1);
    // damping: f is linear in a, so a halving costs passes over vectors only
    double t = 1.0;
    int halvings = 0;
    for (;;) {
      launch_lap_interp(s, v.a, v.a1, v.f, v.f1, t, n, npad, v.at, v.ft);
      rc = lap_sites(h, v, lik, v.at, v.ft, hs);
      if (rc != GOGP_OK) return rc;
      const double psit = -0.5 * hs[1] + hs[0];
      // "psi does not increase", to the rounding of its two sums: a step that gains less than that is taken as it is
      if (psit >= psi - 1e-12 * std::max(1.0, fabs(psi))) {
        psi = psit;
        break;
      }
      if (++halvings > 20) {
        stuck = true;
        break;
      }
      t *= 0.5;
    }
    if (stuck) {  // back to the iterate the step started from, and its site vectors
      rc = lap_sites(h, v, lik, v.a, v.f, hs);
      if (rc != GOGP_OK) return rc;
      hs[2] = INFINITY;  // (not converged, whatever the residual says)
      continue;
    }
    HIPCHK(h, hipMemcpyAsync(v.a, v.at, vec, hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemcpyAsync(v.f, v.ft, vec, hipMemcpyDeviceToDevice, s));
    ++h->lap_iters;
  }
  if (stuck) *conv = false;
  *psi_out = psi;
  return rcf;
}

extern "C" int gogp_laplace_observe(gogp_handle *h, int32_t lik, const double *x, int64_t len, double *lml) {
  if (!h || !x) return fail(h, GOGP_EARG, "laplace_observe: NULL");
  if (lml) *lml = NAN;
  if (len != h->P) return fail(h, GOGP_EARG, "laplace_observe: len(x)");
  if (!lap_lik_ok(lik)) return fail(h, GOGP_EARG, "laplace_observe: unknown likelihood");
  int rc = lap_refuse(h, "laplace_observe");
  if (rc != GOGP_OK) return rc;
  if (!h->have_data) return fail(h, GOGP_ESTATE, "laplace_observe: no data (gogp_set_data)");
  if (h->nv_set)
    return fail(h, GOGP_EARG, "laplace_observe: not supported while noise variances are set (its matrix-free products with K do not carry them)");
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<double> th(h->P > 0 ? h->P : 1);
  for (int i = 0; i < h->P; ++i) th[i] = exp(x[i]);
  rc = set_theta_natural(h, th.data(), th.data() + h->ns);
  if (rc != GOGP_OK) return rc;
  // the regression state goes, as with gogp_set_data; so does an earlier Laplace fit
  h->factored = h->have_alpha = h->observed = h->with_obs = h->grad_valid = h->z_valid = false;
  h->multi_solved = false;
  h->basis_solved = false;
  h->lap_observed = h->lap_grad_valid = false;
  h->lap_lik = lik;
  h->lap_iters = 0;
  if (h->n == 0) {
    h->lap_observed = true;
    if (lml) *lml = 0.0;
    return GOGP_OK;
  }
  LapVecs v;
  rc = lap_vecs(h, &v);
  if (rc == GOGP_OK) rc = gogp_upload_params(h);  // the products with K come before the first factorisation's own upload
  if (rc != GOGP_OK) return rc;
  const bool warm = h->lap_warm && h->lap_warm_valid && h->lap_warm_lik == lik && h->lap_warm_n == h->n;
  bool conv = false;
  double psi = NAN;
  rc = lap_newton(h, v, lik, warm, &conv, &psi);
  // a warm start that went nowhere (theta moved far): once more from a = 0
  if (warm && !conv && (rc == GOGP_OK || rc == GOGP_ECOND)) rc = lap_newton(h, v, lik, false, &conv, &psi);
  if (rc != GOGP_OK && rc != GOGP_ECOND) return rc;
  const double z = psi - 0.5 * h->logdet2;
  h->lml = z;
  h->lap_observed = true;
  if (conv) {
    HIPCHK(h, hipMemcpyAsync(v.awarm, v.a, (size_t)h->npad * sizeof(double), hipMemcpyDeviceToDevice, h->s));
    HIPCHK(h, hipStreamSynchronize(h->s));
    h->lap_warm_valid = true;
    h->lap_warm_lik = lik;
    h->lap_warm_n = h->n;
  }
  if (lml) *lml = z;
  if (rc == GOGP_ECOND) return rc;
  if (!conv) return fail(h, GOGP_ENOCONV, "laplace_observe: Newton did not reach the tolerance");
  return GOGP_OK;
}

extern "C" int gogp_laplace_gradient(gogp_handle *h, double *grad, int64_t len) {
  if (!h || !grad) return fail(h, GOGP_EARG, "laplace_gradient: NULL");
  if (len != h->P) return fail(h, GOGP_EARG, "laplace_gradient: wrong length");
  int rc = lap_refuse(h, "laplace_gradient");
  if (rc != GOGP_OK) return rc;
  if (!h->lap_observed) return fail(h, GOGP_ESTATE, "laplace_gradient before laplace_observe");
  for (int64_t i = 0; i < len; ++i) grad[i] = 0.0;
  if (h->n == 0) return GOGP_OK;
  if (!h->lap_grad_valid) {
    HIPCHK(h, hipSetDevice(h->device));
    LapVecs v;
    rc = lap_vecs(h, &v);
    if (rc == GOGP_OK) rc = compute_kinv(h);  // B^-1 = Y Y^T into bufA, as after an Absorb
    if (rc != GOGP_OK) return rc;
    hipStream_t s = h->s;
    const int64_t n = h->n, npad = h->npad, ld = npad;
    // s from the diagonal; u = s - sw o (B^-1 (sw o (K s))) -- the symmetric product's slot sums go through Y, which is
    // done with once B^-1 exists
    launch_lap_weight_vectors(s, h->bufA, ld, v.rho, n, npad, v.sv);
    lap_kmatvec(h, v, v.sv, v.kv);
    launch_lap_vec(s, nullptr, v.sw, v.kv, n, npad, v.rhs);
    launch_lap_symv_u(s, h->bufA, ld, n, npad, v.rhs, v.sv, v.sw, h->bufY, v.u);
    h->trtri_done = h->ydone_valid = false;
    // G over B^-1, in place, then the LML gradient's reduction with a^ for alpha and G for K^-1
    launch_lap_weight(s, h->bufA, ld, n, npad, v.sw, v.u, v.a);
    h->have_kinv = false;
    {
      AuxTimer tm(h, GOGP_PROF_GRAD, s);
      launch_grad_reduce(s, h->devP, h->D, h->ard_dims, h->dX, v.a, (const double *)h->bufA, ld, n, npad, h->gpart, h->gout,
                         h->radial1, h->ard_mfma_min, h->ev());
    }
    double acc[NACC];
    HIPCHK(h, hipMemcpyAsync(acc, h->gout, sizeof acc, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    h->lap_grad.assign(h->P, 0.0);
    assemble_gradient(h, acc, h->hostP->dnoise, h->lap_grad.data());
    h->lap_grad_valid = true;
  }
  for (int i = 0; i < h->P; ++i) grad[i] = h->lap_grad[i];
  return GOGP_OK;
}

extern "C" int gogp_laplace_get_mode(gogp_handle *h, double *f, double *a, int32_t *iterations) {
  if (!h) return GOGP_EARG;
  if (!h->lap_observed) return fail(h, GOGP_ESTATE, "laplace_get_mode before laplace_observe");
  if (iterations) *iterations = h->lap_iters;
  if (h->n == 0 || (!f && !a)) return GOGP_OK;
  HIPCHK(h, hipSetDevice(h->device));
  LapVecs v;
  const int rc = lap_vecs(h, &v);
  if (rc != GOGP_OK) return rc;
  const size_t bytes = (size_t)h->n * sizeof(double);
  if (f) HIPCHK(h, hipMemcpyAsync(f, v.f, bytes, hipMemcpyDeviceToHost, h->s));
  if (a) HIPCHK(h, hipMemcpyAsync(a, v.a, bytes, hipMemcpyDeviceToHost, h->s));
  HIPCHK(h, hipStreamSynchronize(h->s));
  return GOGP_OK;
}

extern "C" int gogp_laplace_produce(gogp_handle *h, const double *Z, int64_t m, double *mu, double *sigma, double *mean) {
  if (!h || m < 0 || (m > 0 && (!Z || !mu || !sigma))) return fail(h, GOGP_EARG, "laplace_produce: NULL");
  int rc = lap_refuse(h, "laplace_produce");
  if (rc != GOGP_OK) return rc;
  if (!h->lap_observed) return fail(h, GOGP_ESTATE, "laplace_produce before laplace_observe");
  if (m == 0) return GOGP_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const int64_t mpad = ((m + TILE - 1) / TILE) * TILE;
  rc = ensure_m(h, m, mpad);
  if (rc != GOGP_OK) return rc;
  const ProducePlan pp{mpad, h->pvec, h->pvec + mpad, h->pvec + 2 * mpad, h->pvec + 3 * mpad};
  hipStream_t s = h->s;
  if (h->n == 0) {
    rc = gogp_upload_params(h);
    if (rc != GOGP_OK) return rc;
  }
  HIPCHK(h, hipMemcpyAsync(h->dZ, Z, (size_t)m * h->D * sizeof(double), hipMemcpyHostToDevice, s));
  launch_prior(s, h->devP, h->dZ, m, pp.prior);
  if (h->n == 0) {
    launch_sigma(s, pp.prior, nullptr, m, pp.sigma);
    HIPCHK(h, hipMemsetAsync(pp.mu, 0, (size_t)m * sizeof(double), s));
  } else {
    LapVecs v;
    rc = lap_vecs(h, &v);
    if (rc != GOGP_OK) return rc;
    // the tile route for every m: the mean from the unscaled cross-covariance, its columns scaled by sw ahead of the
    // forward substitution with B's factor
    produce_cross_t<double>(h, s, m, mpad);
    launch_rownorm_dot(s, (const double *)h->KsT, h->npad, v.a, h->npad, m, pp.mu, nullptr);
    launch_lap_colscale(s, h->KsT, h->npad, mpad, h->npad, v.sw);
    produce_substitute_t<double>(h, s, m, mpad, pp.q);
    launch_sigma(s, pp.prior, pp.q, m, pp.sigma);
  }
  const size_t bytes = (size_t)m * sizeof(double);
  if (mean) {
    launch_lap_mean(s, h->lap_lik, pp.mu, pp.sigma, m, pp.q);  // (q is done with)
    HIPCHK(h, hipMemcpyAsync(mean, pp.q, bytes, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(h, hipMemcpyAsync(mu, pp.mu, bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(sigma, pp.sigma, bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  return GOGP_OK;
}

// ---- cached state --------------------------------------------------------------------------------
extern "C" int gogp_get_alpha(gogp_handle *h, double *alpha) {
  if (!h || (h->n > 0 && !alpha)) return GOGP_EARG;
  if (h->n == 0) return GOGP_OK;
  if (!h->factored) return fail(h, GOGP_ESTATE, "Alpha: nothing absorbed");
  HIPCHK(h, hipSetDevice(h->device));
  int rc = ensure_alpha(h);
  if (rc != GOGP_OK) return rc;
  HIPCHK(h, hipMemcpyAsync(alpha, h->alpha, (size_t)h->n * sizeof(double), hipMemcpyDeviceToHost, h->s));
  HIPCHK(h, hipStreamSynchronize(h->s));
  return GOGP_OK;
}

extern "C" int gogp_get_factor(gogp_handle *h, double *Lout) {
  if (!h || (h->n > 0 && !Lout)) return GOGP_EARG;
  if (h->n == 0) return GOGP_OK;
  if (!h->factored) return fail(h, GOGP_ESTATE, "L: nothing absorbed");
  if (h->dist) {  // collective: the tiles are gathered, every rank gets the whole factor
    HIPCHK(h, hipSetDevice(h->device));
    return gogp_dist_get_factor(h, Lout);
  }
  HIPCHK(h, hipSetDevice(h->device));
  double *tmp = nullptr;
  HIPCHK(h, hipMalloc(&tmp, (size_t)h->n * h->n * sizeof(double)));
  if (h->prec == 32)
    launch_extract_lower(h->s, reinterpret_cast<const float *>(h->bufL), h->npad, h->n, tmp);
  else
    launch_extract_lower(h->s, h->bufL, h->npad, h->n, tmp);
  hipError_t e = hipMemcpyAsync(Lout, tmp, (size_t)h->n * h->n * sizeof(double),
                                hipMemcpyDeviceToHost, h->s);
  if (e == hipSuccess) e = hipStreamSynchronize(h->s);
  (void)hipFree(tmp);
  HIPCHK(h, e);
  return GOGP_OK;
}

extern "C" int gogp_get_factor_rows(gogp_handle *h, const int64_t *rows, int64_t nrows,
                                    double *out) {
  if (!h || nrows < 0 || (nrows > 0 && (!rows || !out))) return GOGP_EARG;
  if (nrows == 0 || h->n == 0) return GOGP_OK;
  if (!h->factored) return fail(h, GOGP_ESTATE, "L: nothing absorbed");
  HIPCHK(h, hipSetDevice(h->device));
  const int64_t n = h->n;
  for (int64_t r = 0; r < nrows; ++r)
    if (rows[r] < 0 || rows[r] >= n) return fail(h, GOGP_EARG, "get_factor_rows: row out of range");
  if (h->dist) return gogp_dist_get_factor_part(h, rows, nrows, out);  // collective: the tiles' owners contribute
  std::vector<float> tmp32(h->prec == 32 ? (size_t)n : 0);
  for (int64_t r = 0; r < nrows; ++r) {
    const int64_t i = rows[r];
    double *o = out + r * n;
    if (h->prec == 32) {
      HIPCHK(h, hipMemcpy(tmp32.data(), reinterpret_cast<const float *>(h->bufL) + (size_t)i * h->npad,
                          (size_t)(i + 1) * sizeof(float), hipMemcpyDeviceToHost));
      for (int64_t j = 0; j <= i; ++j) o[j] = (double)tmp32[(size_t)j];
    } else {
      HIPCHK(h, hipMemcpyAsync(o, h->bufL + (size_t)i * h->npad, (size_t)(i + 1) * sizeof(double),
                               hipMemcpyDeviceToHost, h->s));
    }
    for (int64_t j = i + 1; j < n; ++j) o[j] = 0.0;
  }
  HIPCHK(h, hipStreamSynchronize(h->s));
  return GOGP_OK;
}

extern "C" int gogp_get_factor_diag(gogp_handle *h, double *diag) {
  if (!h || (h->n > 0 && !diag)) return GOGP_EARG;
  if (h->n == 0) return GOGP_OK;
  if (!h->factored) return fail(h, GOGP_ESTATE, "L: nothing absorbed");
  HIPCHK(h, hipSetDevice(h->device));
  if (h->dist) return gogp_dist_get_factor_part(h, nullptr, 0, diag);  // collective
  if (h->prec == 32) {
    std::vector<float> d32((size_t)h->n);
    HIPCHK(h, hipMemcpy2D(d32.data(), sizeof(float), h->bufL, (size_t)(h->npad + 1) * sizeof(float),
                          sizeof(float), (size_t)h->n, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < h->n; ++i) diag[i] = (double)d32[(size_t)i];
    return GOGP_OK;
  }
  HIPCHK(h, hipMemcpy2DAsync(diag, sizeof(double), h->bufL, (size_t)(h->npad + 1) * sizeof(double),
                             sizeof(double), (size_t)h->n, hipMemcpyDeviceToHost, h->s));
  HIPCHK(h, hipStreamSynchronize(h->s));
  return GOGP_OK;
}

extern "C" int gogp_set_factor(gogp_handle *h, const double *theta_simil,
                               const double *theta_noise, const double *Lin,
                               const double *alpha) {
  if (!h || !theta_simil || (h->nn > 0 && !theta_noise)) return fail(h, GOGP_EARG, "set_factor: NULL");
  if (!h->have_data) return fail(h, GOGP_ESTATE, "set_factor: no data");
  if (h->n > 0 && (!Lin || !alpha)) return fail(h, GOGP_EARG, "set_factor: NULL");
  HIPCHK(h, hipSetDevice(h->device));
  int rc = set_theta_natural(h, theta_simil, theta_noise);
  if (rc != GOGP_OK) return rc;
  h->observed = false;
  h->grad_valid = false;
  h->have_kinv = false;
  for (hipStream_t q : work_streams(h)) HIPCHK(h, hipStreamSynchronize(q));
  h->trtri_done = h->trtri_pending = h->kinv_pending = false;
  h->tinv_valid = false;  // Produce on a restored factor substitutes panel by panel
  h->z_valid = false;     // no z = L^-1 y comes with a restored factor (gogp_append recomputes it)
  h->kinv_c1 = 0;         // ... and no partial K^-1 of an earlier sweep belongs to it (compute_kinv: gogp_loo)
  h->multi_solved = false;  // ... nor do the solutions of gogp_multi_*
  h->basis_solved = false;  // ... or of gogp_basis_*
  h->lap_observed = h->lap_grad_valid = false;  // ... nor does a Laplace fit, whose factor this one replaces
  if (h->n == 0) return GOGP_OK;
  if (h->dist) return gogp_dist_set_factor(h, Lin, alpha);  // collective: every rank keeps its own tiles
  rc = gogp_upload_params(h);
  if (rc != GOGP_OK) return rc;
  hipStream_t s = h->s;
  const int64_t n = h->n, npad = h->npad;
  double *tmp = nullptr;
  HIPCHK(h, hipMalloc(&tmp, (size_t)n * n * sizeof(double)));
  hipError_t e = hipMemcpyAsync(tmp, Lin, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    auto pack = [&](auto *L, auto *Dv) {  // the factor and its block inverses in the handle's element type
      launch_pack_lower(s, tmp, n, npad, L, npad);
      for (int b = 0; b < (int)(npad / PANEL); ++b)
        diag_inv_only(h, s, L + (size_t)b * PANEL * npad + (size_t)b * PANEL, npad, Dv + (size_t)b * PANEL * PANEL);
    };
    if (h->prec == 32)
      pack(reinterpret_cast<float *>(h->bufL), reinterpret_cast<float *>(h->Dinv));
    else
      pack(h->bufL, h->Dinv);
    e = hipMemsetAsync(h->alpha, 0, (size_t)npad * sizeof(double), s);
  }
  if (e == hipSuccess)
    e = hipMemcpyAsync(h->alpha, alpha, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s);
  // z = L^T alpha is not needed: Produce uses alpha for the mean
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(tmp);
  HIPCHK(h, e);
  h->factored = true;
  h->have_alpha = true;
  h->alpha_pending = false;
  // LML of the restored state: -n/2 log 2pi - sum log L_ii - 1/2 y^T alpha
  if (h->prec == 32)
    launch_lml_scalars(s, reinterpret_cast<const float *>(h->bufL), npad, h->alpha, h->dy, h->alpha, n,
                       h->scalars);
  else
    launch_lml_scalars(s, h->bufL, npad, h->alpha, h->dy, h->alpha, n, h->scalars);
  HIPCHK(h, hipMemcpyAsync(h->hscal, h->scalars, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  h->lml = -0.5 * (double)n * log(2 * M_PI) - 0.5 * h->hscal[0] - 0.5 * h->hscal[2];
  h->logdet2 = h->hscal[0];
  return GOGP_OK;
}

// ---- append ---------------------------------------------------------------------------------------
// m observations join the factored process at the parameters of the last Absorb / Observe / set_factor (no reference
// counterpart: tutorial/tutorial.go:118-142 refactorises).  With K = [K11 B^T; B C] and K11 = L11 L11^T:
//   L21 = B L11^-T,  S = C - L21 L21^T,  L22 = chol(S),  z2 = L22^-1 (y2 - L21 z1),  alpha = L^-T z
// in chunks of <= 64 rows: the cross kernel builds B, the persistent substitution kernel (trsm_small.hip) V = L21^T in
// one pass over the factor, append.hip's two kernels the rest; the block inverses the new rows touch are refreshed
// between chunks; ONE backward substitution, the LML and the host copy at the end.
// Leading dimension: ld = npad, so a call that crosses a multiple of 256 restrides the factor ONCE, for the final
// npad, into bufA -- dead here: K was consumed by the factorisation and a K^-1 in it is invalidated anyway -- and swaps
// the two pointers; beyond the capacity a new set of buffers is allocated (an eighth more than needed: a stream of
// single appends then reallocates rarely).  The chunks pass over the rows that exist so far only.
// Rollback (a pivot of S <= 0, in any chunk): the old factor was never written -- restrided: it still lies in the
// other buffer, the pointers are swapped back; in place: the new rows lay on identity padding rows, which are put back
// -- the one old block inverse the new rows share is restored from a copy, the data tails are zeroed again.
struct AppendSaved {
  NBufs bufs;
  int64_t cap_npad, n, npad;
  int nblk;
  EvalState es;
};

// What gogp_append and gogp_remove start with: nothing of an earlier call may still run -- an eager Observe's inverse
// reads bufL and writes bufA -- and nothing that was pending or assembled for the old factor holds for the new one
static int begin_factor_update(gogp_handle *h) {
  for (hipStream_t q : work_streams(h)) HIPCHK(h, hipStreamSynchronize(q));
  h->trtri_pending = h->alpha_pending = h->kinv_pending = false;
  h->tinv_valid = h->tinv_pending = false;
  h->ydone_valid = false;
  h->kinv_c1 = 0;
  h->multi_T = 0;  // the outputs of gogp_multi_set_outputs belong to the rows as they were
  h->multi_solved = false;
  h->basis_p = 0;  // ... and so does the basis of gogp_basis_set
  h->basis_solved = false;
  h->lap_observed = h->lap_grad_valid = h->lap_warm_valid = false;  // a Laplace fit (and its warm start) belongs to the rows as they were
  return GOGP_OK;
}
// ... and end with, on the main stream s behind z of the n1 rows: alpha = L^-T z over the whole new factor L (leading
// dimension ld = its npad), the LML from y^T alpha as gogp_set_factor, one host copy, one synchronise; then `adopt` --
// the caller's part that must not run before the device is done: freeing what the old factor lay in, making L the
// handle's -- and the judging of the scalars
template <class Adopt>
static int finish_factor_update(gogp_handle *h, const double *L, int64_t ld, int64_t n1, hipStream_t s, Adopt adopt) {
  const int np1 = (int)(ld / PANEL);
  HIPCHK(h, hipMemcpyAsync(h->w, h->z, (size_t)ld * sizeof(double), hipMemcpyDeviceToDevice, s));
  for (int b = np1 - 1; b >= 0; --b) launch_trsv_bwd_step(s, L, ld, h->Dinv, b, np1, h->w, h->alpha);
  launch_lml_scalars(s, L, ld, h->z, h->dy, h->alpha, n1, h->scalars);
  HIPCHK(h, hipMemcpyAsync(h->hscal, h->scalars, 7 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  adopt();
  h->hscal[6] = h->hscal[2];  // y^T alpha where judge_scalars looks for the quadratic term of a refined alpha
  const long long zero = 0;
  memcpy(h->hscal + HS_INFO, &zero, sizeof zero);
  const FactorResult fr = judge_scalars(h, h->hscal, false, true);
  h->lml = fr.lml;
  h->logdet2 = h->hscal[0];
  h->yta = fr.yta;
  h->cond_lb = fr.cond_lb;
  h->notpd = -1;
  h->factored = h->have_alpha = true;
  h->observed = h->with_obs = h->grad_valid = h->have_kinv = h->trtri_done = false;
  h->z_valid = true;
  if (fr.rc == GOGP_ECOND) h->err = fr.msg;
  return fr.rc;
}

// v2: the new rows' noise variances (gogp_set_noise_variances), NULL: zeros.  They reach the new block's diagonal as
// -v2 folded into the first slab's partial sums (noisevar.hip), so that the commit kernel is today's; the handle's
// vector grows with the data's buffers, and a failed call leaves it as it was.
extern "C" int gogp_append_noisy(gogp_handle *h, const double *X2, const double *y2, const double *v2, int64_t m) {
  if (!h) return GOGP_EARG;
  if (m < 0) return fail(h, GOGP_EARG, "append: m < 0");
  if (m == 0) return GOGP_OK;
  if (!X2 || !y2) return fail(h, GOGP_EARG, "append: NULL");
  if (v2) {
    if (const char *why = nv_refusal(h)) return fail(h, GOGP_EARG, why);
    if (gogp_noise_variances_check(v2, m) != GOGP_OK)
      return fail(h, GOGP_EARG, "append: every noise variance must be finite and >= 0");
  }
  if (h->prec == 32)
    return fail(h, GOGP_EARG, "append: not supported on a precision = 32 handle (the update is fp64 throughout)");
  if (h->dist) return fail(h, GOGP_EARG, "append: not supported on a sharded handle");
  for (int64_t i = 0; i < m * h->D; ++i)
    if (!std::isfinite(X2[i])) return fail(h, GOGP_EARG, "append: non-finite input");
  for (int64_t i = 0; i < m; ++i)
    if (!std::isfinite(y2[i])) return fail(h, GOGP_EARG, "append: non-finite output");
  if (!h->have_data) return fail(h, GOGP_ESTATE, "append: no data (gogp_set_data)");
  if (h->n > 0 && !h->factored) return fail(h, GOGP_ESTATE, "append: nothing absorbed");
  HIPCHK(h, hipSetDevice(h->device));
  if (h->n == 0) {  // an empty process: Absorb of the m rows at the handle's parameters
    if (!h->have_theta) return fail(h, GOGP_ESTATE, "append: no parameters (Absorb, Observe or set_factor first)");
    const std::vector<double> ts = h->theta_s, tn = h->theta_n;
    int rc = gogp_set_data(h, X2, y2, m);
    if (rc != GOGP_OK) return rc;
    if (v2) rc = gogp_set_noise_variances(h, v2, m);
    if (rc == GOGP_OK) rc = gogp_absorb(h, ts.data(), tn.data());
    if (rc != GOGP_OK && rc != GOGP_ECOND) {  // empty again
      const int64_t np = h->notpd;
      const std::string e = h->err;
      (void)gogp_set_data(h, nullptr, nullptr, 0);
      h->lml = 0.0;
      h->notpd = np;
      h->err = e;
    }
    return rc;
  }
  // (begin_factor_update drops the outputs and the basis, which belong to the rows as they were: the rollback puts them
  // back with the rows; their solutions lie in workspaces of their own, which the update does not write)
  const int multi_T0 = h->multi_T, basis_p0 = h->basis_p;
  const bool multi_solved0 = h->multi_solved, basis_solved0 = h->basis_solved;
  auto keep_outputs = [&]() {  // on every return that leaves the old rows and their factor in place
    h->multi_T = multi_T0;
    h->multi_solved = multi_solved0;
    h->basis_p = basis_p0;
    h->basis_solved = basis_solved0;
  };
  int rc = begin_factor_update(h);
  if (rc != GOGP_OK) return rc;
  hipStream_t s = h->s;
  const int D = h->D;
  const int64_t n0 = h->n, npad0 = h->npad, n1 = n0 + m, npad1 = ((n1 + PANEL - 1) / PANEL) * PANEL;
  const bool restride = npad1 != npad0, grow = npad1 > h->cap_npad;
  rc = gogp_upload_params(h);
  if (rc != GOGP_OK) return keep_outputs(), rc;
  const size_t blk = (size_t)PANEL * PANEL;
  rc = h->app_ws.reserve(h, (blk + (size_t)(std::max(npad1, h->cap_npad) / PANEL) * gogp::APPEND_PART) * sizeof(double));
  if (rc != GOGP_OK) return keep_outputs(), rc;
  double *dsave = h->app_ws.as<double>(), *part = dsave + blk;
  const size_t vb0 = (size_t)npad0 * sizeof(double);
  if (!h->z_valid) {  // a restored factor: z = L^-1 y by the substitution steps
    HIPCHK(h, hipMemcpyAsync(h->w, h->dy, vb0, hipMemcpyDeviceToDevice, s));
    const int np0 = (int)(npad0 / PANEL);
    for (int b = 0; b < np0; ++b) launch_trsv_fwd_step(s, h->bufL, npad0, h->Dinv, b, np0, h->w, h->z);
    h->z_valid = true;
  }
  const AppendSaved saved{nbufs_of(h), h->cap_npad, n0, npad0, h->nblk, static_cast<const EvalState &>(*h)};
  const NBufs &old = saved.bufs;
  // the one old block inverse the new rows share
  const bool save_blk = (n0 % PANEL) != 0;
  const int64_t b0 = n0 / PANEL;
  if (save_blk) HIPCHK(h, hipMemcpyAsync(dsave, h->Dinv + (size_t)b0 * blk, blk * sizeof(double), hipMemcpyDeviceToDevice, s));
  const size_t xslack = GOGP_MAX_NDIM;
  if (grow) {
    const int64_t cap = npad1 + ((npad1 / 8 + PANEL - 1) / PANEL) * PANEL;
    NBufs nb;
    if (nbufs_alloc(h, cap, &nb) != hipSuccess) {
      (void)hipGetLastError();
      keep_outputs();
      return fail(h, GOGP_ENOMEM, "append: out of device memory");
    }
    HIPCHK(h, hipMemsetAsync(nb.dX, 0, ((size_t)cap * D + xslack) * sizeof(double), s));
    HIPCHK(h, hipMemsetAsync(nb.dy, 0, (size_t)cap * sizeof(double), s));
    HIPCHK(h, hipMemsetAsync(nb.z, 0, (size_t)cap * sizeof(double), s));
    HIPCHK(h, hipMemcpyAsync(nb.dX, old.dX, (size_t)n0 * D * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemcpyAsync(nb.dy, old.dy, (size_t)n0 * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemcpyAsync(nb.z, old.z, (size_t)n0 * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemcpyAsync(nb.Dinv, old.Dinv, (size_t)(npad0 / PANEL) * blk * sizeof(double), hipMemcpyDeviceToDevice, s));
    nbufs_put(h, nb);
    h->cap_npad = cap;
    launch_append_restride(s, old.bufL, npad0, npad0, h->bufL, npad1, npad1);
  } else {
    if (restride) {
      launch_append_restride(s, old.bufL, npad0, npad0, old.bufA, npad1, npad1);
      h->bufL = old.bufA;
      h->bufA = old.bufL;
    }
    // the data tails: the rows between the old and the new end may never have been written
    HIPCHK(h, hipMemsetAsync(h->dX + (size_t)n0 * D, 0, ((size_t)(npad1 - n0) * D + xslack) * sizeof(double), s));
    HIPCHK(h, hipMemsetAsync(h->dy + n0, 0, (size_t)(npad1 - n0) * sizeof(double), s));
    HIPCHK(h, hipMemsetAsync(h->z + n0, 0, (size_t)(npad1 - n0) * sizeof(double), s));
  }
  h->npad = npad1;
  h->nblk = (int)(npad1 / TILE);
  const int64_t ld = npad1;
  int64_t ncur = n0, touched = n0;  // rows < touched of the new factor rows may have been written
  // the noise variances: [the old rows' (zeros if none were set) | v2 (zeros if NULL) | zeros], in place where the
  // block is large enough, else in a new one of the data buffers' capacity; the old block lives until the call succeeds
  const bool nv_was_set = h->nv_set, nv_use = nv_was_set || v2 != nullptr;
  double *const nv_old = h->nv;
  const int64_t nv_old_cap = h->nv_cap;
  bool nv_fresh = false;
  auto nv_rollback = [&]() {
    if (nv_fresh) {
      (void)hipFree(h->nv);
      h->nv = nv_old;
      h->nv_cap = nv_old_cap;
    } else if (nv_use && h->nv && h->nv_cap > n0) {
      (void)hipMemsetAsync(h->nv + n0, 0, (size_t)std::min<int64_t>(m, h->nv_cap - n0) * sizeof(double), s);
    }
    h->nv_set = nv_was_set;
  };
  // put everything back as it was before the call (the factor itself was never overwritten)
  auto rollback = [&]() {
    for (hipStream_t q : {s, h->s2}) (void)hipStreamSynchronize(q);
    if (grow) {
      nbufs_free(nbufs_of(h));
      nbufs_put(h, old);
      h->cap_npad = saved.cap_npad;
    } else {
      if (!restride) launch_append_identity_rows(s, old.bufL, npad0, n0, std::min(touched, npad0), npad0);
      if (save_blk) (void)hipMemcpyAsync(h->Dinv + (size_t)b0 * blk, dsave, blk * sizeof(double), hipMemcpyDeviceToDevice, s);
      (void)hipMemsetAsync(h->dX + (size_t)n0 * D, 0, ((size_t)(npad1 - n0) * D + xslack) * sizeof(double), s);
      (void)hipMemsetAsync(h->dy + n0, 0, (size_t)(npad1 - n0) * sizeof(double), s);
      (void)hipMemsetAsync(h->z + n0, 0, (size_t)(npad1 - n0) * sizeof(double), s);
    }
    nv_rollback();
    h->bufA = old.bufA;
    h->bufL = old.bufL;
    h->n = n0;
    h->npad = npad0;
    h->nblk = saved.nblk;
    static_cast<EvalState &>(*h) = saved.es;
    if (restride && !grow) h->have_kinv = false;  // bufA held the restrided copy
    keep_outputs();
    (void)hipStreamSynchronize(s);
    free_m_buffers(h);  // sized for the npad that did not come to be
  };
  if (nv_use) {
    const int64_t need = std::max(h->cap_npad, npad1);
    hipError_t e = hipSuccess;
    if (!h->nv || h->nv_cap < need) {
      double *q = nullptr;
      e = hipMalloc(&q, (size_t)need * sizeof(double));
      if (e == hipSuccess) {
        h->nv = q;
        h->nv_cap = need;
        nv_fresh = true;
        e = hipMemsetAsync(q, 0, (size_t)need * sizeof(double), s);
      }
      if (e == hipSuccess && nv_was_set) e = hipMemcpyAsync(q, nv_old, (size_t)n0 * sizeof(double), hipMemcpyDeviceToDevice, s);
    } else if (!nv_was_set) {  // a block of earlier data: nothing in it holds
      e = hipMemsetAsync(h->nv, 0, (size_t)h->nv_cap * sizeof(double), s);
    }
    if (e == hipSuccess && v2) e = hipMemcpyAsync(h->nv + n0, v2, (size_t)m * sizeof(double), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      rollback();
      return fail(h, e == hipErrorOutOfMemory ? GOGP_ENOMEM : GOGP_EHIP, "append: the noise variances could not be stored");
    }
    h->nv_set = true;
  }
  HIPCHK(h, hipMemcpyAsync(h->dX + (size_t)n0 * D, X2, (size_t)m * D * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(h, hipMemcpyAsync(h->dy + n0, y2, (size_t)m * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(h, hipMemsetAsync(h->info, 0, sizeof(long long), s));
  rc = ensure_m(h, 64, TILE);
  size_t one = 0;
  if (rc == GOGP_OK) rc = ensure_small_ws(h, &one);
  if (rc != GOGP_OK) {
    const std::string e = h->err;
    rollback();
    h->err = e;
    return rc;
  }
  unsigned *htmo = hs_tmo(h);
  const size_t ev0 = produce_event_base(npad1);
  for (int64_t off = 0; off < m; off += 64) {
    const int mc = (int)std::min<int64_t>(64, m - off), m1 = std::min(mc, 32);
    const int64_t npc = ((ncur + PANEL - 1) / PANEL) * PANEL;  // the rows that exist so far, in whole blocks
    const double *Xc = h->dX + (size_t)ncur * D, *yc = h->dy + ncur;
    double *Lrow = h->bufL + (size_t)ncur * ld;
    touched = ncur + mc;
    launch_cross(s, h->devP, D, h->dX, ncur, npc, Xc, mc, TILE, h->KsT, ld, h->ev());  // B, as Produce's Kstar^T
    unsigned *tmo = nullptr, *tmo2 = nullptr;
    htmo[0] = htmo[1] = 0;
    if (mc > 32) {  // the second 32 columns beside the first, as Produce (every stream is idle here)
      order(h, ev0 + 1, s, h->s2);
      launch_trsm_small(h->s2, h->bufL, ld, h->Dinv, h->KsT, ld, npc, 32, mc - 32, h->small_ws.as<char>() + one, h->pvec, &tmo2);
      HIPCHK(h, hipMemcpyAsync(htmo + 1, tmo2, sizeof(unsigned), hipMemcpyDeviceToHost, h->s2));
    }
    launch_trsm_small(s, h->bufL, ld, h->Dinv, h->KsT, ld, npc, 0, m1, h->small_ws.p, h->pvec, &tmo);
    HIPCHK(h, hipMemcpyAsync(htmo, tmo, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    if (mc > 32) order(h, ev0 + PRODUCE_GROUPS + 1, h->s2, s);
    gogp::TsSolution v0 = gogp::trsm_small_solution(npc, 0, m1, h->small_ws.p), v1 = v0;
    if (mc > 32) v1 = gogp::trsm_small_solution(npc, 32, mc - 32, h->small_ws.as<char>() + one);
    launch_append_gram(s, v0, v1, m1, mc, npc, ncur, h->z, part, Lrow, ld);
    if (v2) launch_nv_append_fold(s, part, h->nv + ncur, mc);
    launch_append_commit(s, h->devP, Xc, yc, mc, ncur, part, (int)(npc / PANEL), Lrow, ld, h->z + ncur, h->info, h->ev());
    HIPCHK(h, hipMemcpyAsync(h->hscal + HS_INFO, h->info, sizeof(long long), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    if ((htmo[0] | htmo[1]) != 0u) {
      // a workgroup of the substitution kernel gave up waiting: this chunk again with one chain of substitution steps
      // per new row (solve.hip), whose solutions lie row by row in Vt
      const int nbc = (int)(npc / PANEL);
      for (int j = 0; j < mc; ++j) {
        HIPCHK(h, hipMemcpyAsync(h->w, h->KsT + (size_t)j * ld, (size_t)npc * sizeof(double), hipMemcpyDeviceToDevice, s));
        for (int b = 0; b < nbc; ++b) launch_trsv_fwd_step(s, h->bufL, ld, h->Dinv, b, nbc, h->w, h->Vt + (size_t)j * ld);
      }
      gogp::TsSolution vr;
      vr.p = h->Vt;
      vr.kind = gogp::TS_SOL_ROWS;
      vr.width = (int)ld;
      HIPCHK(h, hipMemsetAsync(h->info, 0, sizeof(long long), s));
      launch_append_gram(s, vr, vr, mc, mc, npc, ncur, h->z, part, Lrow, ld);
      if (v2) launch_nv_append_fold(s, part, h->nv + ncur, mc);
      launch_append_commit(s, h->devP, Xc, yc, mc, ncur, part, nbc, Lrow, ld, h->z + ncur, h->info, h->ev());
      HIPCHK(h, hipMemcpyAsync(h->hscal + HS_INFO, h->info, sizeof(long long), hipMemcpyDeviceToHost, s));
      HIPCHK(h, hipStreamSynchronize(s));
      HIPCHK(h, hipGetLastError());
    }
    long long info = 0;
    memcpy(&info, h->hscal + HS_INFO, sizeof info);
    if (info != 0) {
      rollback();
      h->notpd = (int64_t)info - 1;  // global: the commit kernel counts from the rows that existed
      char buf[160];
      snprintf(buf, sizeof buf, "Factorize: matrix is not positive definite (pivot %lld)", (long long)h->notpd);
      h->err = buf;
      return GOGP_ENOTPD;
    }
    for (int64_t b = ncur / PANEL; b <= (ncur + mc - 1) / PANEL; ++b)
      launch_diag256_inv_only(s, h->bufL + (size_t)b * PANEL * (ld + 1), ld, h->Dinv + (size_t)b * blk);
    ncur += mc;
  }
  h->n = n1;
  return finish_factor_update(h, h->bufL, ld, n1, s, [&] {
    if (nv_fresh) (void)hipFree(nv_old);
    if (!grow) return;
    nbufs_free(old);
    drop_cand_graph(h);
  });
}

extern "C" int gogp_append(gogp_handle *h, const double *X2, const double *y2, int64_t m) {
  return gogp_append_noisy(h, X2, y2, nullptr, m);
}

// ---- remove ---------------------------------------------------------------------------------------
// The observations idx[0] < ... < idx[m-1] leave the factored process (no reference counterpart; the counterpart of
// gogp_append).  With kept = the other rows, Lt = L[kept, kept] is lower triangular with a positive diagonal and
//   K[kept, kept] = Lt Lt^T + W W^T,  W = L[kept, idx]:
// a gather and a rank-m update by Householder reflectors (remove.hip) -- a sum, so the result is positive definite by
// construction: no GOGP_ENOTPD, no rollback.  Neither the similarity kernel nor theta is evaluated.
// Launch sequence, all on the main stream: the gather of Lt into bufA at ld = npad(n - m) -- dead here as in gogp_append
// -- and of X / y into the workspace; per pass of <= REMOVE_W columns of W (REMOVE_W_SMALL when m is that small) the
// gather of those columns from the OLD factor, a snapshot of the diagonal 128-blocks, and one launch per 128-column
// block from the block of the pass's first affected column; the block inverses from the first affected 256-block (all
// of them when npad shrinks); z by the forward chain on the compacted y, alpha by the backward chain, the LML scalars;
// one host copy, one synchronise.  The old factor is only read; the pointers are swapped at the end.
// Measured (profiles/remove.txt): slower than gogp_set_data + gogp_absorb for removals from the front at
// N = 4096 and for 64 rows at once at N = 16384; no automatic fallback.
extern "C" int gogp_remove(gogp_handle *h, const int64_t *idx, int64_t m) {
  if (!h) return GOGP_EARG;
  if (m < 0) return fail(h, GOGP_EARG, "remove: m < 0");
  if (m == 0) return GOGP_OK;
  if (!idx) return fail(h, GOGP_EARG, "remove: NULL");
  if (h->prec == 32)
    return fail(h, GOGP_EARG, "remove: not supported on a precision = 32 handle (the update is fp64 throughout)");
  if (h->dist) return fail(h, GOGP_EARG, "remove: not supported on a sharded handle");
  if (!h->have_data || h->n == 0 || !h->factored) return fail(h, GOGP_ESTATE, "remove: nothing absorbed");
  const int64_t n0 = h->n, npad0 = h->npad;
  for (int64_t j = 0; j < m; ++j) {
    if (idx[j] < 0 || idx[j] >= n0) return fail(h, GOGP_EARG, "remove: index out of range");
    if (j > 0 && idx[j] <= idx[j - 1]) return fail(h, GOGP_EARG, "remove: indices must be strictly increasing");
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (m == n0) {  // the empty process, at the parameters it had
    const int rc = gogp_set_data(h, nullptr, nullptr, 0);
    if (rc != GOGP_OK) return rc;
    h->lml = 0.0;
    h->with_obs = false;
    h->z_valid = false;
    h->notpd = -1;
    return GOGP_OK;
  }
  int rc = begin_factor_update(h);
  if (rc != GOGP_OK) return rc;
  h->have_kinv = false;  // bufA is written from here on
  hipStream_t s = h->s;
  const int D = h->D;
  const int64_t n1 = n0 - m, npad1 = ((n1 + PANEL - 1) / PANEL) * PANEL, ld = npad1;
  const bool restride = npad1 != npad0;
  std::vector<int> hmap((size_t)(n1 + m));  // new index -> old index, then the removed rows
  {
    int64_t j = 0, k = 0;
    for (int64_t i = 0; i < n0; ++i) {
      if (j < m && idx[j] == i)
        hmap[(size_t)(n1 + j++)] = (int)i;
      else
        hmap[(size_t)k++] = (int)i;
    }
  }
  const size_t nints = (size_t)((n1 + m + 1) / 2) * 2;
  const size_t need = nints * sizeof(int) +
                      ((size_t)gogp::REMOVE_W * npad1 + (size_t)npad1 * TILE + (size_t)npad1 * (D + 2)) * sizeof(double);
  rc = h->rm_ws.reserve(h, need);
  if (rc != GOGP_OK) return rc;
  int *dmap = h->rm_ws.as<int>(), *drem = dmap + n1;
  double *W = reinterpret_cast<double *>(dmap + nints), *snap = W + (size_t)gogp::REMOVE_W * npad1;
  double *Xt = snap + (size_t)npad1 * TILE, *yt = Xt + (size_t)npad1 * D, *vt = yt + npad1;  // (vt: the noise variances)
  double *Lold = h->bufL, *Lnew = h->bufA;
  HIPCHK(h, hipMemcpyAsync(dmap, hmap.data(), (size_t)(n1 + m) * sizeof(int), hipMemcpyHostToDevice, s));
  launch_remove_gather(s, Lold, npad0, dmap, n1, Lnew, npad1);
  launch_remove_rows(s, h->dX, dmap, n1, D, Xt);
  launch_remove_rows(s, h->dy, dmap, n1, 1, yt);
  if (h->nv_set) launch_remove_rows(s, h->nv, dmap, n1, 1, vt);
  const int mw = m <= gogp::REMOVE_W_SMALL ? gogp::REMOVE_W_SMALL : gogp::REMOVE_W;
  const int64_t first = std::min<int64_t>(idx[0], n1 - 1);  // the first column the call can change
  for (int64_t off = 0; off < m; off += mw) {
    const int mc = (int)std::min<int64_t>(mw, m - off);
    const int64_t c0 = idx[off] - off;  // the first kept row behind the pass's first removed one, as a new index
    if (c0 >= n1) break;                // the rest was behind every kept row: W is zero
    const int64_t cb0 = (c0 / TILE) * TILE;
    launch_remove_w(s, Lold, npad0, dmap, drem + off, mc, mw, cb0, n1, npad1, W);
    launch_remove_snap(s, Lnew, ld, (int)(cb0 / TILE), (int)((n1 + TILE - 1) / TILE - cb0 / TILE), snap);
    for (int64_t kb = cb0; kb < n1; kb += TILE) launch_remove_block(s, Lnew, ld, snap, W, mw, kb, n1);
  }
  // the data, compacted, and zero tails as gogp_set_data leaves them
  HIPCHK(h, hipMemcpyAsync(h->dX, Xt, (size_t)n1 * D * sizeof(double), hipMemcpyDeviceToDevice, s));
  HIPCHK(h, hipMemcpyAsync(h->dy, yt, (size_t)n1 * sizeof(double), hipMemcpyDeviceToDevice, s));
  HIPCHK(h, hipMemsetAsync(h->dX + (size_t)n1 * D, 0, ((size_t)(npad0 - n1) * D + GOGP_MAX_NDIM) * sizeof(double), s));
  HIPCHK(h, hipMemsetAsync(h->dy + n1, 0, (size_t)(npad0 - n1) * sizeof(double), s));
  if (h->nv_set) {
    HIPCHK(h, hipMemcpyAsync(h->nv, vt, (size_t)n1 * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemsetAsync(h->nv + n1, 0, (size_t)(npad0 - n1) * sizeof(double), s));
  }
  const int np1 = (int)(npad1 / PANEL);
  const size_t blk = (size_t)PANEL * PANEL;
  for (int b = restride ? 0 : (int)(first / PANEL); b < np1; ++b)
    launch_diag256_inv_only(s, Lnew + (size_t)b * PANEL * (ld + 1), ld, h->Dinv + (size_t)b * blk);
  const size_t vb1 = (size_t)npad1 * sizeof(double);
  HIPCHK(h, hipMemcpyAsync(h->w, h->dy, vb1, hipMemcpyDeviceToDevice, s));
  for (int b = 0; b < np1; ++b) launch_trsv_fwd_step(s, Lnew, ld, h->Dinv, b, np1, h->w, h->z);
  return finish_factor_update(h, Lnew, ld, n1, s, [&] {
    h->bufL = Lnew;
    h->bufA = Lold;
    h->n = n1;
    h->npad = npad1;
    h->nblk = (int)(npad1 / TILE);
  });
}

// ---- measurement hooks -----------------------------------------------------------------------------
extern "C" int gogp_profile_enable(gogp_handle *h, int on) {
  if (!h) return GOGP_EARG;
  h->prof.on = on != 0;
  h->prof.used = 0;
  h->prof.flops = 0;
  h->prof.launches = 0;
  h->prof.lflops.clear();
  h->prof.ltag.clear();
  for (auto &u : h->aux_used) u = 0;
  return GOGP_OK;
}

// Every launch of the tile kernel since profiling was enabled: start / end (ms since the first launch's
// start), flops, tag = mode * 1e8 + (K / 16) * 1e5 + tiles.  Does not reset (gogp_profile_read does).
extern "C" int gogp_profile_read_launches(gogp_handle *h, int64_t cap, double *t0_ms, double *t1_ms,
                                          double *flops, int64_t *tag, int64_t *n) {
  if (!h || !n) return GOGP_EARG;
  HIPCHK(h, hipSetDevice(h->device));
  for (hipStream_t q : work_streams(h)) HIPCHK(h, hipStreamSynchronize(q));
  const int64_t nl = (int64_t)std::min(h->prof.used / 2, h->prof.lflops.size());
  *n = nl;
  for (int64_t i = 0; i < nl && i < cap; ++i) {
    float d = 0.f, a = 0.f;
    (void)hipEventElapsedTime(&d, h->prof.pool[2 * i], h->prof.pool[2 * i + 1]);
    (void)hipEventElapsedTime(&a, h->prof.pool[0], h->prof.pool[2 * i]);
    if (t0_ms) t0_ms[i] = a;
    if (t1_ms) t1_ms[i] = (double)a + d;
    if (flops) flops[i] = h->prof.lflops[(size_t)i];
    if (tag) tag[i] = h->prof.ltag[(size_t)i];
  }
  return GOGP_OK;
}

extern "C" int gogp_profile_read_aux(gogp_handle *h, int cls, double *ms, int64_t *launches) {
  if (!h || cls < 0 || cls >= GOGP_PROF_NCLASS) return GOGP_EARG;
  HIPCHK(h, hipSetDevice(h->device));
  for (hipStream_t q : work_streams(h)) HIPCHK(h, hipStreamSynchronize(q));
  double sum = 0.0;
  int64_t cnt = 0;
  for (size_t i = 0; i + 1 < h->aux_used[cls]; i += 2) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, h->aux_ev[cls][i], h->aux_ev[cls][i + 1]) != hipSuccess) continue;
    sum += t;
    ++cnt;
  }
  if (ms) *ms = sum;
  if (launches) *launches = cnt;
  h->aux_used[cls] = 0;
  return GOGP_OK;
}

extern "C" int gogp_profile_read(gogp_handle *h, double *gemm_ms, int64_t *gemm_launches,
                                 double *gemm_flops, double *gemm_busy_ms) {
  if (!h) return GOGP_EARG;
  HIPCHK(h, hipSetDevice(h->device));
  for (hipStream_t q : work_streams(h)) HIPCHK(h, hipStreamSynchronize(q));
  double ms = 0.0, busy = 0.0;
  // launches run concurrently on up to four streams: besides the sum of the
  // per-launch durations report the length of the UNION of the launch intervals
  // (time during which at least one instance of the kernel is executing)
  std::vector<std::pair<double, double>> iv;
  iv.reserve(h->prof.used / 2);
  for (size_t i = 0; i + 1 < h->prof.used; i += 2) {
    float t = 0.f, t0 = 0.f;
    if (hipEventElapsedTime(&t, h->prof.pool[i], h->prof.pool[i + 1]) != hipSuccess) continue;
    ms += t;
    if (hipEventElapsedTime(&t0, h->prof.pool[0], h->prof.pool[i]) != hipSuccess) continue;
    iv.emplace_back((double)t0, (double)t0 + (double)t);
  }
  std::sort(iv.begin(), iv.end());
  double cur_b = 0, cur_e = -1;
  for (auto &p : iv) {
    if (cur_e < cur_b || p.first > cur_e) {
      if (cur_e >= cur_b) busy += cur_e - cur_b;
      cur_b = p.first;
      cur_e = p.second;
    } else if (p.second > cur_e) {
      cur_e = p.second;
    }
  }
  if (cur_e >= cur_b && !iv.empty()) busy += cur_e - cur_b;
  if (gemm_ms) *gemm_ms = ms;
  if (gemm_launches) *gemm_launches = h->prof.launches;
  if (gemm_flops) *gemm_flops = h->prof.flops;
  if (gemm_busy_ms) *gemm_busy_ms = busy;
  h->prof.used = 0;
  h->prof.flops = 0;
  h->prof.launches = 0;
  h->prof.lflops.clear();
  h->prof.ltag.clear();
  return GOGP_OK;
}

extern "C" int gogp_set_option(gogp_handle *h, const char *name, int64_t value) {
  if (!h || !name) return GOGP_EARG;
  // a captured launch sequence of the candidates path was recorded under the old options: every option decides
  // what enqueue() launches (or may, later), so none of them keeps the graph
  drop_cand_graph(h);
  if (strcmp(name, "produce_tinv") == 0) {  // Produce solves whole super-panels through T^-1 (assembled behind the factorisation)
    h->produce_tinv = value != 0;
    return GOGP_OK;
  }
  if (strcmp(name, "basis_symm") == 0) {  // gogp_basis_*: W = K^-1 H from the explicit K^-1 (1), from the factor (0), -1: whichever is there
    if (value < -1 || value > 1) return fail(h, GOGP_EARG, "basis_symm must be -1, 0 or 1");
    h->basis_symm = (int)value;
    h->basis_solved = false;
    return GOGP_OK;
  }
  if (strcmp(name, "produce_panels") == 0) {  // Produce: 256-panels per super-panel of its substitution
    if (value < 1 || value > 8) return fail(h, GOGP_EARG, "produce_panels must be 1..8");
    h->produce_panels = (int)value;
    return GOGP_OK;
  }
  if (strcmp(name, "produce_small_below") == 0) {  // Produce: launches below this many 128-tiles use 64 x 64 tiles
    if (value < 0) return fail(h, GOGP_EARG, "produce_small_below must be >= 0");
    h->produce_small_below = (int)value;
    return GOGP_OK;
  }
  if (strcmp(name, "produce_small_max") == 0) {  // Produce: up to this many test points through the persistent substitution kernel (0: never)
    if (value < 0 || value > 64) return fail(h, GOGP_EARG, "produce_small_max must be 0..64");
    h->produce_small_max = (int)value;
    return GOGP_OK;
  }
  if (strcmp(name, "produce_groups") == 0) {  // Produce: independent substitution chains over the test points' tile rows
    if (value < 1 || value > PRODUCE_GROUPS) return fail(h, GOGP_EARG, "produce_groups must be 1..4");
    h->produce_groups = (int)value;
    return GOGP_OK;
  }
  if (strcmp(name, "gradient_precision") == 0) {  // 64 (default) | 32: Y = L^-T and K^-1 on the fp32 tile kernel (fp64 handle)
    if (value != 32 && value != 64) return fail(h, GOGP_EARG, "gradient_precision must be 32 or 64");
    // Offered for ONE term with an output scale only: there the components of the gradient that cancel (trace, output
    // scale) come from closed forms and the gradient stays ~1e-8 from the fp64 one.  A SUM of terms has no closed form
    // per term: its scale components would be sums over the float K^-1 (measured 1.9e-4 on the hyperpriors kernel,
    // above the 1e-4 the reference checks its own gradient to, gp_test.go:170,248) -- refused rather than shipped.
    if (value == 32 && (h->desc.nterms != 1 || h->desc.terms[0].scale_idx < 0))
      return fail(h, GOGP_EARG, "gradient_precision = 32 is offered for one-term kernels with an output scale only");
    if (value == 32 && h->nv_set)  // its closed-form scale component assumes K = c F + s2 I
      return fail(h, GOGP_EARG, "gradient_precision = 32 is not supported while noise variances are set");
    HIPCHK(h, hipSetDevice(h->device));
    for (hipStream_t q : work_streams(h)) HIPCHK(h, hipStreamSynchronize(q));
    h->grad_prec = (int)value;
    h->have_kinv = h->grad_valid = false;  // an inverse of the other kind must not be reused
    h->trtri_done = h->trtri_pending = h->kinv_pending = false;
    return GOGP_OK;
  }
  if (strcmp(name, "trace_fp64") == 0) {  // fp32 path: trace / scale components of the gradient by their closed forms
    h->trace_fp64 = value != 0;
    return GOGP_OK;
  }
  if (strcmp(name, "krag") == 0) {  // the inverse's updates skip the zero triangle of a super-panel of Y
    h->krag = value != 0;
    return GOGP_OK;
  }
  if (strcmp(name, "lookahead") == 0) {
    h->lookahead = value != 0;
    return GOGP_OK;
  }
  if (strcmp(name, "eager") == 0) {
    h->eager = value != 0;
    return GOGP_OK;
  }
  if (strcmp(name, "precision") == 0) {
    // 64 (default): everything fp64.  32: the N x N matrices (K, L, Y, K^-1, block inverses) and
    // the O(N^3) products in fp32 on v_mfma_f32_32x32x2_f32; inputs, kernel evaluation, diagonal
    // blocks, vectors and all reductions stay fp64 (BASELINE config 5; DESIGN.md "fp32 path").
    // Changes the buffers: the data must be set again afterwards.
    if (value != 32 && value != 64) return fail(h, GOGP_EARG, "precision must be 32 or 64");
    if (h->dist && (int)value != h->prec)
      return fail(h, GOGP_EARG, "precision: set it before gogp_dist_init_* (the shard's buffers are typed)");
    if ((int)value != h->prec) {
      HIPCHK(h, hipSetDevice(h->device));
      for (hipStream_t q : work_streams(h)) HIPCHK(h, hipStreamSynchronize(q));
      free_n_buffers(h);
      free_m_buffers(h);
      free_cand_buffers(h);  // the candidates' arena slots are laid out for the matrices' element type
      h->prec = (int)value;
      h->have_data = h->factored = h->have_alpha = h->have_kinv = h->observed = h->grad_valid = false;
      h->lap_observed = h->lap_grad_valid = h->lap_warm_valid = false;  // (free_n_buffers dropped the Laplace fit too)
      h->multi_T = 0;  // (free_n_buffers dropped the outputs of gogp_multi_set_outputs; said here too)
      h->multi_solved = false;
      h->basis_p = 0;
      h->basis_solved = false;
      h->trtri_done = h->trtri_pending = h->alpha_pending = h->kinv_pending = false;
    }
    return GOGP_OK;
  }
  if (strcmp(name, "kinv_split") == 0) {  // percent of the columns of Y whose part of K^-1 is launched inside the sweep; 0: off
    if (value < 0 || value > 95) return fail(h, GOGP_EARG, "kinv_split must be 0..95");
    h->kinv_split = (int)value;
    return GOGP_OK;
  }
  if (strcmp(name, "kinv_fused") == 0) {  // -1: by size (default), 0: LAUUM in Gradient, 1: fused
    h->kinv_fused = value < 0 ? -1 : (value != 0);
    return GOGP_OK;
  }
  if (strcmp(name, "superpanel_head") == 0) {
    if (value < -1 || value > 8) return fail(h, GOGP_EARG, "superpanel_head must be -1..8");
    h->superpanel_head = (int)value;
    return GOGP_OK;
  }
  if (strcmp(name, "head_remaining") == 0) {
    if (value < 0) return fail(h, GOGP_EARG, "head_remaining must be >= 0");
    h->head_remaining = (int)value;
    return GOGP_OK;
  }
  if (strcmp(name, "ard_mfma_min_dims") == 0) {
    if (value < 1 || value > 65) return fail(h, GOGP_EARG, "ard_mfma_min_dims must be 1..65");
    h->ard_mfma_min = (int)value;
    return GOGP_OK;
  }
  if (strcmp(name, "chain_prio") == 0) {  // -1: by size, 0: off, 1: the chains' skinny launches, 2: all their launches
    if (value < -1 || value > 2) return fail(h, GOGP_EARG, "chain_prio must be -1..2");
    h->chain_prio = (int)value;
    return GOGP_OK;
  }
  if (strcmp(name, "tiny") == 0) {  // N <= 128: the whole factorisation in one launch (diag256.hip: tiny_eval_kernel); 0: the general sweep
    if (value < 0 || value > 1) return fail(h, GOGP_EARG, "tiny must be 0 or 1");
    h->tiny = (int)value;
    return GOGP_OK;
  }
  if (strcmp(name, "chain_slabs") == 0) {  // chain_split = 2: 64-row slabs per workgroup of the chain step; 0: by size (the result does not depend on it)
    if (value < 0 || value > 8) return fail(h, GOGP_EARG, "chain_slabs must be 0..8");
    h->chain_slabs = (int)value;
    return GOGP_OK;
  }
  if (strcmp(name, "chain_split") == 0) {  // -1: by size, 0: 256-block kernel, 2: panel128.hip (form 1 is gone, 2 keeps its number)
    if (value < -1 || value > 2 || value == 1) return fail(h, GOGP_EARG, "chain_split must be -1, 0 or 2");
    h->chain_split = (int)value;
    return GOGP_OK;
  }
  if (strcmp(name, "ktri") == 0) {
    h->ktri = value != 0;
    return GOGP_OK;
  }
  if (strcmp(name, "graph") == 0) {  // candidates: hipGraph replay -- 1 a chain (N <= 1024), 2 the real DAG (N <= 8192), 0 streams
    if (value < 0 || value > 3) return fail(h, GOGP_EARG, "graph must be 0..3");
    h->use_graph = (int)value;
    h->graph_failed = false;
    drop_cand_graph(h);
    return GOGP_OK;
  }
  if (strcmp(name, "diag_fp64") == 0) {  // fp32 path: the diagonal blocks' trailing updates accumulated in fp64 (diagsyrk.hip)
    if (value < 0 || value > 1) return fail(h, GOGP_EARG, "diag_fp64 must be 0 or 1");
    h->diag_fp64 = (int)value;
    return GOGP_OK;
  }
  if (strcmp(name, "refine_steps") == 0) {
    if (value < 0 || value > 8) return fail(h, GOGP_EARG, "refine_steps must be 0..8");
    h->refine_steps = (int)value;
    return GOGP_OK;
  }
  if (strcmp(name, "cond_limit_log10") == 0) {  // gonum: mat.ConditionTolerance (a package variable), 1e16
    if (value < 1 || value > 300) return fail(h, GOGP_EARG, "cond_limit_log10 must be 1..300");
    h->cond_limit = pow(10.0, (double)value);
    return GOGP_OK;
  }
  if (strcmp(name, "sparse_jitter_log10") == 0) {  // gogp_sparse_*: Kuu + 10^value I is factored (absolute), from the next sparse_observe on
    if (value < -14 || value > -2) return fail(h, GOGP_EARG, "sparse_jitter_log10 must be -14..-2");
    h->sp_jitter_log10 = (int)value;
    h->sp_observed = h->sp_mobserved = false;
    return GOGP_OK;
  }
  if (strcmp(name, "sparse_chunk") == 0) {  // gogp_sparse_*: rows of X per pass
    if (value < 256 || value > 65536 || value % 256) return fail(h, GOGP_EARG, "sparse_chunk must be a multiple of 256 in 256..65536");
    h->sp_chunk = value;
    return GOGP_OK;
  }
  if (strcmp(name, "cg_check") == 0) {  // gogp_cg_*: iterations between two looks at the status word; no result depends on it
    if (value < 1 || value > 1024) return fail(h, GOGP_EARG, "cg_check must be 1..1024");
    h->cg.check = (int)value;
    return GOGP_OK;
  }
  if (strcmp(name, "laplace_max_iter") == 0) {  // gogp_laplace_observe: Newton steps at the most
    if (value < 1 || value > 200) return fail(h, GOGP_EARG, "laplace_max_iter must be 1..200");
    h->lap_max_iter = (int)value;
    return GOGP_OK;
  }
  if (strcmp(name, "laplace_tol_log10") == 0) {  // ... its stationarity tolerance 10^value
    if (value < -14 || value > -4) return fail(h, GOGP_EARG, "laplace_tol_log10 must be -14..-4");
    h->lap_tol_log10 = (int)value;
    return GOGP_OK;
  }
  if (strcmp(name, "laplace_warm") == 0) {  // ... 1: start from the last converged mode of the same data and likelihood
    if (value < 0 || value > 1) return fail(h, GOGP_EARG, "laplace_warm must be 0 or 1");
    h->lap_warm = (int)value;
    return GOGP_OK;
  }
  if (strcmp(name, "superpanel") == 0) {
    if (value < 1 || value > 8) return fail(h, GOGP_EARG, "superpanel must be 1..8");
    h->superpanel = (int)value;
    return GOGP_OK;
  }
  return fail(h, GOGP_EARG, "unknown option");
}

