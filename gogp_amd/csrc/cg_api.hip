// cg_api.hip -- C ABI of the iterative exact GP (gogp_cg_*): host code; kernels in cg.hip, state in handle.h's CgHandleState.
// include/gogp_hip.h states the iteration and the preconditioner; DESIGN.md section 4, "Iterative (CG)".  Everything runs
// on the handle's main stream with buffers of the family's own.  Reused launchers: select_run (the factor), launch_cross
// (the right-hand sides k* of Produce, whose KsT layout is one row of N per test point), launch_prior.  The Woodbury
// products are cg.hip's own: the factor lies column-major and a block's vectors as T rows of N, which neither
// launch_sparse_xty / launch_sparse_syrk (row-major chunks of Vt) nor the tile GEMM (multiples of 128) take without
// transposed copies of N x rank and N x T doubles per application.  C = I + Ls^T Ls (rank <= 1024) is factored and inverted on
// the host, once per solve.
#include "api_internal.h"

using namespace gogp;

extern "C" int gogp_cg_set_data(gogp_handle *h, const double *X, const double *y, const double *v, int64_t N) {
  const char *who = "cg_set_data";
  if (!h) return GOGP_EARG;
  CgHandleState &cg = h->cg;
  if (N == 0 && !X && !y && !v) {  // clear
    HIPCHK(h, hipSetDevice(h->device));
    cg.release();
    return GOGP_OK;
  }
  if (const int rc = refuse_handle(h, who)) return rc;
  if (N < 1 || !X || !y) return refuse(h, who, GOGP_EARG, "need X, y and N >= 1 (N == 0 with NULLs clears)");
  const int D = h->D;
  double vmin = 0.0;
  if (const char *why = resident_data_refusal(X, y, v, N, D, &vmin)) return refuse(h, who, GOGP_EARG, why);
  HIPCHK(h, hipSetDevice(h->device));
  if (h->s) HIPCHK(h, hipStreamSynchronize(h->s));
  cg.release();
  const int64_t npad = (N + 255) / 256 * 256;
  const size_t xb = ((size_t)npad * D + GOGP_MAX_NDIM) * sizeof(double), vb = (size_t)npad * sizeof(double);
  hipStream_t s = h->s;
  hipError_t e = hipMalloc(&cg.X, xb);
  if (e == hipSuccess) e = hipMalloc(&cg.y, vb);
  if (e == hipSuccess && v) e = hipMalloc(&cg.v, vb);
  if (e == hipSuccess) e = hipMalloc(&cg.d, vb);
  if (e == hipSuccess) e = hipMalloc(&cg.dis, vb);
  if (e == hipSuccess) e = hipMalloc(&cg.alpha, vb);
  if (e == hipSuccess) e = hipMalloc(&cg.P, sizeof(DevParams));
  if (e == hipSuccess) e = hipMemsetAsync(cg.X, 0, xb, s);
  if (e == hipSuccess) e = hipMemsetAsync(cg.y, 0, vb, s);
  if (e == hipSuccess && v) e = hipMemsetAsync(cg.v, 0, vb, s);
  if (e == hipSuccess) e = hipMemcpyAsync(cg.X, X, (size_t)N * D * sizeof(double), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(cg.y, y, (size_t)N * sizeof(double), hipMemcpyHostToDevice, s);
  if (e == hipSuccess && v) e = hipMemcpyAsync(cg.v, v, (size_t)N * sizeof(double), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    cg.release();
    HIPCHK(h, e);
  }
  cg.N = N;
  cg.npad = npad;
  cg.vmin = vmin;
  cg.have = true;
  return GOGP_OK;
}

// The small device buffers of the family behind C^-1: W, Y, the state, the dots' results
struct CgSmall {
  double *Cinv, *W, *Y, *sc, *dots;
  int *st;
};
static size_t cg_small_layout(char *base, int rp, CgSmall *b) {
  Carve c{base};
  const size_t rr = (size_t)std::max(rp, 16);
  b->Cinv = c.take<double>(rr * rr);
  b->W = c.take<double>((size_t)CG_MAX_T * rr);
  b->Y = c.take<double>((size_t)CG_MAX_T * rr);
  b->sc = c.take<double>((size_t)CG_SC_ROWS * CG_MAX_T);
  b->dots = c.take<double>((size_t)CG_MAX_T);
  b->st = c.take<int>((size_t)CG_ST_ROWS * CG_MAX_T);
  return c.off;
}

// z = P^-1 r for a block (T rows of ld = npad doubles)
static void cg_apply_precond(gogp_handle *h, const CgSmall &sm, const double *R, int T, double *Z) {
  const CgHandleState &cg = h->cg;
  hipStream_t s = h->s;
  const int r = cg.rank, rp = cg.rp;
  const double *Ls = cg.L.as<double>();
  if (r > 0) {
    launch_cg_lst(s, Ls, cg.ldn, cg.N, r, rp, cg.dis, R, cg.npad, T, cg.part.as<double>(), sm.W);
    launch_cg_small_mm(s, sm.Cinv, r, rp, sm.W, T, sm.Y);
  }
  launch_cg_precond(s, Ls, cg.ldn, cg.N, r, rp, cg.dis, R, sm.Y, cg.npad, T, Z);
}

// the scratch the product and the skinny transposed product share: sized for CG_MAX_T columns once
static int cg_reserve_part(gogp_handle *h, int T) {
  CgHandleState &cg = h->cg;
  const int64_t n = cg.N;
  const size_t kmm = (size_t)kmm_slabs(n, n) * (size_t)T * (size_t)((n + 63) / 64 * 64);
  const size_t lst = (size_t)cg_lst_slabs(n) * (size_t)((T + 15) / 16 * 16) * (size_t)std::max(cg.rp, 16);
  return cg.part.reserve(h, std::max(kmm, lst) * sizeof(double));
}

// One lock-step block: K^ x_t = b_t for the T <= CG_MAX_T rows of dB (device, ld = npad, zero from column n on); the
// solutions are left in the first T rows of the workspace's x (returned through *xout).  GOGP_OK, GOGP_ENOCONV (every
// output written) or an error.  With `keep` (gogp_cg_lml_gradient) the block also holds on to w = P^-1 b (a seventh
// vector behind the dots' partials, returned through keep->w), records every iteration's a and beta (keep->hist, device:
// 2 max_iter rows of CG_MAX_T) and leaves rho0 = b^T w per column in keep->rho0 (device, CG_MAX_T); no bit of x depends on it.
struct CgKeep {
  double *hist = nullptr, *rho0 = nullptr;  // in: device buffers
  double *w = nullptr;                      // out
};
static int cg_block_solve(gogp_handle *h, const char *who, const double *dB, int T, double tol, int max_iter, double **xout,
                          gogp_cg_col *cols, int col0, CgKeep *keep = nullptr) {
  CgHandleState &cg = h->cg;
  const int64_t n = cg.N, ld = cg.npad;
  hipStream_t s = h->s;
  const int nb = cg_dot_blocks(n);
  const size_t vec = (size_t)T * (size_t)ld;
  int rc = cg.vec.reserve(h, ((keep ? 6 : 5) * vec + (size_t)CG_MAX_T * nb) * sizeof(double));
  if (rc == GOGP_OK) rc = cg_reserve_part(h, T);
  if (rc != GOGP_OK) return rc;
  CgSmall sm;
  cg_small_layout(cg.small.as<char>(), cg.rp, &sm);
  double *x = cg.vec.as<double>(), *r = x + vec, *p = r + vec, *z = p + vec, *q = z + vec, *dpart = q + vec;
  double *kpart = cg.part.as<double>();
  const CgState cs{sm.sc, sm.st};
  const int nslab = kmm_slabs(n, n);
  const DevParams *P = cg.P;
  const int D = h->D;
  HIPCHK(h, hipMemsetAsync(x, 0, 5 * vec * sizeof(double), s));
  HIPCHK(h, hipMemcpyAsync(r, dB, vec * sizeof(double), hipMemcpyDeviceToDevice, s));
  launch_cg_dots(s, r, r, ld, n, T, CG_DOT_BNORM, 0, tol, dpart, nullptr, cs);
  cg_apply_precond(h, sm, r, T, z);
  HIPCHK(h, hipMemcpyAsync(p, z, vec * sizeof(double), hipMemcpyDeviceToDevice, s));
  double *hist = nullptr;
  if (keep) {
    keep->w = dpart + (size_t)CG_MAX_T * nb;
    hist = keep->hist;
    HIPCHK(h, hipMemcpyAsync(keep->w, z, vec * sizeof(double), hipMemcpyDeviceToDevice, s));
  }
  launch_cg_dots(s, r, z, ld, n, T, CG_DOT_RHO0, 0, tol, dpart, keep ? keep->rho0 : nullptr, cs);
  int status[2] = {T, 0};
  const int check = std::max(1, cg.check);
  for (int it = 1; it <= max_iter; ++it) {
    launch_kmm(s, P, D, cg.X, n, cg.X, n, p, ld, T, cg.d, nslab, 0, kpart, q, ld);
    ++cg.products;
    launch_cg_dots(s, p, q, ld, n, T, CG_DOT_PQ, it, tol, dpart, nullptr, cs, hist);
    launch_cg_update_xr(s, x, r, p, q, ld, n, T, cs);
    launch_cg_dots(s, r, r, ld, n, T, CG_DOT_RR, it, tol, dpart, nullptr, cs);
    cg_apply_precond(h, sm, r, T, z);
    launch_cg_dots(s, r, z, ld, n, T, CG_DOT_BETA, it, tol, dpart, nullptr, cs, hist);
    launch_cg_update_p(s, p, z, ld, n, T, cs);
    if (it % check == 0 || it == max_iter) {
      launch_cg_status(s, T, cs);
      HIPCHK(h, hipMemcpyAsync(status, sm.st + CG_ST_STATUS * CG_MAX_T, sizeof status, hipMemcpyDeviceToHost, s));
      HIPCHK(h, hipStreamSynchronize(s));
      if (status[0] == 0 || status[1] != 0) break;
    }
  }
  // the true residual: one more product; b - K^ x into z, its squared norms through the plain dots
  launch_kmm(s, P, D, cg.X, n, cg.X, n, x, ld, T, cg.d, nslab, 0, kpart, q, ld);
  ++cg.products;
  launch_cg_scale(s, dB, nullptr, q, ld, n, T, z);
  launch_cg_dots(s, z, z, ld, n, T, CG_DOT_PLAIN, 0, tol, dpart, sm.dots, cs);
  double hsc[CG_SC_ROWS * CG_MAX_T], hdots[CG_MAX_T];
  int hst[CG_ST_ROWS * CG_MAX_T];
  // (the three copies land in locals: the stream is drained before any return, whatever failed)
  hipError_t ce = hipMemcpyAsync(hsc, sm.sc, sizeof hsc, hipMemcpyDeviceToHost, s);
  if (ce == hipSuccess) ce = hipMemcpyAsync(hdots, sm.dots, sizeof hdots, hipMemcpyDeviceToHost, s);
  if (ce == hipSuccess) ce = hipMemcpyAsync(hst, sm.st, sizeof hst, hipMemcpyDeviceToHost, s);
  const hipError_t se = hipStreamSynchronize(s);
  HIPCHK(h, ce);
  HIPCHK(h, se);
  HIPCHK(h, hipGetLastError());
  ++cg.blocks;
  *xout = x;
  int bad = -1;
  bool all = true;
  for (int t = 0; t < T; ++t) {
    const bool isbad = hst[CG_ST_BAD * CG_MAX_T + t] != 0;
    if (isbad && bad < 0) bad = t;
    const bool conv = hst[CG_ST_FROZEN * CG_MAX_T + t] != 0 && !isbad;
    all = all && conv;
    if (cols) {
      gogp_cg_col &c = cols[t];
      const double bn = sqrt(hsc[CG_SC_BNORM2 * CG_MAX_T + t]);
      c.iterations = hst[CG_ST_ITERS * CG_MAX_T + t];
      c.converged = conv ? 1 : 0;
      c.rel_residual = bn > 0.0 ? sqrt(hdots[t]) / bn : 0.0;
      c.rel_residual_recurrence = bn > 0.0 ? sqrt(hsc[CG_SC_RR * CG_MAX_T + t]) / bn : 0.0;
    }
  }
  char buf[200];
  if (bad >= 0) {
    snprintf(buf, sizeof buf, "%s: p^T K p of column %d is not positive and finite (%g): the matrix is not positive definite",
             who, col0 + bad, hsc[CG_SC_PQ * CG_MAX_T + bad]);
    return fail(h, GOGP_ENOTPD, buf);
  }
  if (!all) {
    snprintf(buf, sizeof buf, "%s: a column did not reach the tolerance within %d iterations", who, max_iter);
    return fail(h, GOGP_ENOCONV, buf);
  }
  return GOGP_OK;
}

static const char *cg_tol_refusal(double tol, int32_t max_iter) {
  if (!(tol > 0.0) || !std::isfinite(tol)) return "tol must be positive and finite";
  if (max_iter < 1) return "max_iter must be at least 1";
  return nullptr;
}

extern "C" int gogp_cg_solve(gogp_handle *h, const double *x, int64_t len, int32_t rank, double piv_tol, double tol,
                             int32_t max_iter, gogp_cg_info *info, gogp_cg_col *col) {
  const char *who = "cg_solve";
  if (!h) return GOGP_EARG;
  CgHandleState &cg = h->cg;
  if (!x || !info) return refuse(h, who, GOGP_EARG, "NULL");
  if (const int rc = refuse_handle(h, who)) return rc;
  if (len != h->P) return refuse(h, who, GOGP_EARG, "len(x)");
  for (int64_t i = 0; i < len; ++i)
    if (!std::isfinite(x[i])) return refuse(h, who, GOGP_EARG, "non-finite parameter");
  if (rank < 0 || rank > GOGP_CG_MAX_RANK) return refuse(h, who, GOGP_EARG, "need 0 <= rank <= GOGP_CG_MAX_RANK");
  if (std::isnan(piv_tol) || piv_tol == INFINITY) return refuse(h, who, GOGP_EARG, "piv_tol must be finite or negative");
  if (const char *why = cg_tol_refusal(tol, max_iter)) return refuse(h, who, GOGP_EARG, why);
  if (!cg.have) return refuse(h, who, GOGP_ESTATE, "no data (gogp_cg_set_data)");
  std::vector<double> th(h->P > 0 ? h->P : 1);
  for (int i = 0; i < h->P; ++i) th[i] = exp(x[i]);
  if (const char *why = theta_refusal(h, th.data(), th.data() + h->ns)) return refuse(h, who, GOGP_EARG, why);
  DevParams hp;
  fill_params_theta(h, th.data(), th.data() + h->ns, hp);
  // D = diag(noise_var + v_i) is inverted: its smallest entry must be positive
  if (!(hp.noise_var + cg.vmin > 0.0)) return refuse(h, who, GOGP_EARG, "noise_var + min v_i must be positive");
  if (piv_tol < 0.0) piv_tol = pow(10.0, (double)h->sp_jitter_log10);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->s;
  const int64_t N = cg.N, npad = cg.npad;
  const int D = h->D;
  cg.solved = false;
  cg.products = cg.blocks = 0;
  cg.rank = cg.rp = 0;
  cg.logdet_c = 0.0;
  cg.dnoise = hp.dnoise;
  *info = gogp_cg_info();
  HIPCHK(h, hipMemcpyAsync(cg.P, &hp, sizeof hp, hipMemcpyHostToDevice, s));
  HIPCHK(h, hipStreamSynchronize(s));  // hp is a local
  launch_cg_diag(s, cg.P, cg.v, N, npad, cg.d, cg.dis);
  // ---- the preconditioner: pivoted Cholesky of k(X, X), scaled, and the inverse of its capacitance matrix -----------------
  int64_t m = 0;
  const int64_t cap = std::min<int64_t>(rank, N);
  if (cap > 0) {
    SelectBufs b;
    const size_t small = select_layout(nullptr, N, cap, D, &b);
    const size_t lbytes = (size_t)cap * (size_t)b.ldn * sizeof(double);
    if (const int rl = cg.L.reserve(h, lbytes)) {
      if (rl != GOGP_ENOMEM) return rl;
      char buf[240];
      snprintf(buf, sizeof buf, "cg_solve: the factor (%lld columns of %lld doubles, %.3f GB) could not be allocated: %s",
               (long long)cap, (long long)b.ldn, (double)lbytes * 1e-9, h->err.c_str());
      h->err = buf;
      return GOGP_ENOMEM;
    }
    char *work = nullptr;
    HIPCHK(h, hipMalloc(&work, small));
    select_layout(work, N, cap, D, &b);
    b.Lt = cg.L.as<double>();
    const hipError_t e = select_run(s, cg.P, D, cg.X, N, cap, piv_tol, 0, nullptr, b, &m);
    (void)hipFree(work);
    HIPCHK(h, e);
    cg.ldn = b.ldn;
  }
  const int r = (int)m, rp = (r + 15) / 16 * 16;
  CgSmall sm;
  int rc = cg.small.reserve(h, cg_small_layout(nullptr, rp, &sm));
  if (rc != GOGP_OK) return rc;
  cg_small_layout(cg.small.as<char>(), rp, &sm);
  if (r > 0) {
    launch_cg_scale_factor(s, cg.L.as<double>(), cg.ldn, N, r, cg.dis);
    launch_cg_capacitance(s, cg.L.as<double>(), cg.ldn, N, r, rp, sm.Cinv);
    std::vector<double> C((size_t)rp * rp), G((size_t)rp * rp, 0.0);
    HIPCHK(h, hipMemcpyAsync(C.data(), sm.Cinv, C.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    // C = G G^T (C >= I: every pivot is at least 1 up to rounding), Ginv = G^-1, C^-1 = Ginv^T Ginv -- on the host
    for (int j = 0; j < rp; ++j) {
      double dj = C[(size_t)j * rp + j];
      for (int k = 0; k < j; ++k) dj -= G[(size_t)j * rp + k] * G[(size_t)j * rp + k];
      if (!(dj > 0.0) || !std::isfinite(dj)) return refuse(h, who, GOGP_ENOTPD, "the capacitance matrix of the preconditioner is not positive definite");
      dj = sqrt(dj);
      G[(size_t)j * rp + j] = dj;
      for (int i = j + 1; i < rp; ++i) {
        double v = C[(size_t)i * rp + j];
        const double *gi = &G[(size_t)i * rp], *gj = &G[(size_t)j * rp];
        for (int k = 0; k < j; ++k) v -= gi[k] * gj[k];
        G[(size_t)i * rp + j] = v / dj;
      }
    }
    // G^-1 kept TRANSPOSED (Gt[c][k] = (G^-1)[k][c], upper): every inner loop below runs along rows of G and of Gt
    std::vector<double> Gt((size_t)rp * rp, 0.0);
    for (int c = 0; c < rp; ++c) {
      double *gt = &Gt[(size_t)c * rp];
      gt[c] = 1.0 / G[(size_t)c * rp + c];
      for (int i = c + 1; i < rp; ++i) {
        double v = 0.0;
        const double *gi = &G[(size_t)i * rp];
        for (int k = c; k < i; ++k) v -= gi[k] * gt[k];
        gt[i] = v / gi[i];
      }
    }
    for (int i = 0; i < rp; ++i)
      for (int j = 0; j <= i; ++j) {  // C^-1[i][j] = sum_{k >= i} (G^-1)[k][i] (G^-1)[k][j]
        double v = 0.0;
        const double *ti = &Gt[(size_t)i * rp], *tj = &Gt[(size_t)j * rp];
        for (int k = i; k < rp; ++k) v += ti[k] * tj[k];
        C[(size_t)i * rp + j] = C[(size_t)j * rp + i] = v;
      }
    HIPCHK(h, hipMemcpyAsync(sm.Cinv, C.data(), C.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));  // C is a local
    double ldc = 0.0;  // log |C| = 2 sum_j log G_jj (gogp_cg_lml_gradient; the padded pivots are 1)
    for (int j = 0; j < r; ++j) ldc += log(G[(size_t)j * rp + j]);
    cg.logdet_c = 2.0 * ldc;
  }
  cg.rank = r;
  cg.rp = rp;
  // ---- K^ alpha = y ------------------------------------------------------------------------------------------------------------
  double *xs = nullptr;
  gogp_cg_col c1{};
  rc = cg_block_solve(h, who, cg.y, 1, tol, max_iter, &xs, &c1, 0);
  if (col) *col = c1;
  info->rank_used = r;
  info->products = cg.products;
  info->blocks = cg.blocks;
  if (rc != GOGP_OK && rc != GOGP_ENOCONV) return rc;  // (GOGP_ENOCONV: its error text stays, nothing below writes one and goes on)
  HIPCHK(h, hipMemsetAsync(cg.alpha, 0, (size_t)npad * sizeof(double), s));
  HIPCHK(h, hipMemcpyAsync(cg.alpha, xs, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, s));
  CgState cs{sm.sc, sm.st};
  launch_cg_dots(s, cg.y, cg.alpha, npad, N, 1, CG_DOT_PLAIN, 0, tol, xs + 5 * (size_t)npad, sm.dots, cs);
  HIPCHK(h, hipMemcpyAsync(&cg.yta, sm.dots, sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  info->yt_alpha = cg.yta;
  cg.solved = true;
  return rc;
}

extern "C" int gogp_cg_last_info(gogp_handle *h, gogp_cg_info *info) {
  if (!h) return GOGP_EARG;
  CgHandleState &cg = h->cg;
  if (!info) return fail(h, GOGP_EARG, "cg_last_info: NULL");
  info->rank_used = cg.rank;
  info->products = cg.products;
  info->blocks = cg.blocks;
  info->yt_alpha = cg.yta;
  return GOGP_OK;
}

extern "C" int gogp_cg_get_alpha(gogp_handle *h, double *alpha, int64_t n) {
  const char *who = "cg_get_alpha";
  if (!h) return GOGP_EARG;
  CgHandleState &cg = h->cg;
  if (!alpha) return refuse(h, who, GOGP_EARG, "NULL");
  if (const int rc = refuse_handle(h, who)) return rc;
  if (!cg.have || !cg.solved) return refuse(h, who, GOGP_ESTATE, "no solution (gogp_cg_solve)");
  if (n != cg.N) return refuse(h, who, GOGP_EARG, "n is not the number of observations");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(alpha, cg.alpha, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->s));
  HIPCHK(h, hipStreamSynchronize(h->s));
  return GOGP_OK;
}

extern "C" int gogp_cg_solve_columns(gogp_handle *h, const double *B, int64_t T, double tol, int32_t max_iter, double *S,
                                     gogp_cg_col *cols) {
  const char *who = "cg_solve_columns";
  if (const int rc = refuse_handle(h, who)) return rc;
  CgHandleState &cg = h->cg;
  if (T < 0 || (T > 0 && (!B || !S))) return refuse(h, who, GOGP_EARG, "need B and S for T > 0, T >= 0");
  if (const char *why = cg_tol_refusal(tol, max_iter)) return refuse(h, who, GOGP_EARG, why);
  if (!cg.have || !cg.solved) return refuse(h, who, GOGP_ESTATE, "no preconditioner (gogp_cg_solve)");
  const int64_t N = cg.N, npad = cg.npad;
  for (int64_t i = 0; i < T * N; ++i)
    if (!std::isfinite(B[i])) return refuse(h, who, GOGP_EARG, "non-finite right-hand side");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->s;
  cg.products = cg.blocks = 0;
  int rc = GOGP_OK;
  std::string first_err;
  for (int64_t t0 = 0; t0 < T; t0 += CG_MAX_T) {
    const int cnt = (int)std::min<int64_t>(CG_MAX_T, T - t0);
    int r1 = cg.ks.reserve(h, (size_t)CG_MAX_T * (size_t)npad * sizeof(double));
    if (r1 != GOGP_OK) return r1;
    double *dB = cg.ks.as<double>();
    HIPCHK(h, hipMemsetAsync(dB, 0, (size_t)cnt * npad * sizeof(double), s));
    HIPCHK(h, hipMemcpy2DAsync(dB, (size_t)npad * sizeof(double), B + t0 * N, (size_t)N * sizeof(double),
                               (size_t)N * sizeof(double), (size_t)cnt, hipMemcpyHostToDevice, s));
    double *xs = nullptr;
    r1 = cg_block_solve(h, who, dB, cnt, tol, max_iter, &xs, cols ? cols + t0 : nullptr, (int)t0);
    if (r1 != GOGP_OK && r1 != GOGP_ENOCONV) return r1;
    if (r1 != GOGP_OK && rc == GOGP_OK) rc = r1, first_err = h->err;
    HIPCHK(h, hipMemcpy2DAsync(S + t0 * N, (size_t)N * sizeof(double), xs, (size_t)npad * sizeof(double),
                               (size_t)N * sizeof(double), (size_t)cnt, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
  }
  if (rc != GOGP_OK) h->err = first_err;
  return rc;
}

extern "C" int gogp_cg_produce(gogp_handle *h, const double *Z, int64_t m, double *mu, double *sigma, double tol,
                               int32_t max_iter, gogp_cg_col *cols) {
  const char *who = "cg_produce";
  if (const int rc = refuse_handle(h, who)) return rc;
  CgHandleState &cg = h->cg;
  if (m < 0 || (m > 0 && (!Z || !mu))) return refuse(h, who, GOGP_EARG, "need Z and mu for m > 0, m >= 0");
  if (sigma)
    if (const char *why = cg_tol_refusal(tol, max_iter)) return refuse(h, who, GOGP_EARG, why);
  if (!cg.have || !cg.solved) return refuse(h, who, GOGP_ESTATE, "no solution (gogp_cg_solve)");
  const int D = h->D;
  for (int64_t i = 0; i < m * D; ++i)
    if (!std::isfinite(Z[i])) return refuse(h, who, GOGP_EARG, "non-finite test point");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->s;
  cg.products = cg.blocks = 0;
  if (m == 0) return GOGP_OK;
  const int64_t N = cg.N, npad = cg.npad;
  // layout of cg_ks: 64 rows of k* (npad each), 64 test points, prior, q, mu, sigma (64 each)
  int rc = cg.ks.reserve(h, ((size_t)CG_MAX_T * npad + (size_t)CG_MAX_T * (D + 4)) * sizeof(double));
  if (rc == GOGP_OK) rc = cg_reserve_part(h, CG_MAX_T);
  if (rc == GOGP_OK) rc = cg.part.reserve(h, (size_t)kmm_slabs(CG_MAX_T, N) * 64 * sizeof(double));
  if (rc != GOGP_OK) return rc;
  double *Ks = cg.ks.as<double>(), *dZ = Ks + (size_t)CG_MAX_T * npad, *prior = dZ + (size_t)CG_MAX_T * D;
  double *dq = prior + CG_MAX_T, *dmu = dq + CG_MAX_T, *dsg = dmu + CG_MAX_T;
  CgSmall sm;
  cg_small_layout(cg.small.as<char>(), cg.rp, &sm);
  const CgState cs{sm.sc, sm.st};
  std::string first_err;
  int ret = GOGP_OK;
  for (int64_t j0 = 0; j0 < m; j0 += CG_MAX_T) {
    const int cnt = (int)std::min<int64_t>(CG_MAX_T, m - j0);
    HIPCHK(h, hipMemsetAsync(dZ, 0, (size_t)CG_MAX_T * D * sizeof(double), s));
    HIPCHK(h, hipMemcpyAsync(dZ, Z + j0 * D, (size_t)cnt * D * sizeof(double), hipMemcpyHostToDevice, s));
    // the mean: rows = the test points, columns = X, one right-hand side alpha
    launch_kmm(s, cg.P, D, dZ, cnt, cg.X, N, cg.alpha, npad, 1, nullptr, kmm_slabs(cnt, N), 0,
               cg.part.as<double>(), dmu, CG_MAX_T);
    ++cg.products;
    HIPCHK(h, hipMemcpyAsync(mu + j0, dmu, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, s));
    if (sigma) {
      launch_cross(s, cg.P, D, cg.X, N, npad, dZ, cnt, CG_MAX_T, Ks, npad, false);
      launch_prior(s, cg.P, dZ, cnt, prior);
      double *xs = nullptr;
      rc = cg_block_solve(h, who, Ks, cnt, tol, max_iter, &xs, cols ? cols + j0 : nullptr, (int)j0);
      if (rc != GOGP_OK && rc != GOGP_ENOCONV) {
        (void)hipStreamSynchronize(s);  // the copy of mu into the caller's array must not outlive the call
        return rc;
      }
      if (rc != GOGP_OK && ret == GOGP_OK) ret = rc, first_err = h->err;
      launch_cg_dots(s, Ks, xs, npad, N, cnt, CG_DOT_PLAIN, 0, tol, xs + 5 * (size_t)cnt * npad, dq, cs);
      launch_sigma(s, prior, dq, cnt, dsg);
      HIPCHK(h, hipMemcpyAsync(sigma + j0, dsg, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, s));
    } else if (cols) {
      for (int t = 0; t < cnt; ++t) cols[j0 + t] = gogp_cg_col();
    }
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
  }
  if (ret != GOGP_OK) h->err = first_err;
  return ret;
}

// The LML and its gradient at the theta, preconditioner and alpha of the last gogp_cg_solve (include/gogp_hip.h states
// the estimator).  Per block of CG_MAX_T probes: the rows of Xi go up, cg_probe_kernel forms z = D^1/2 (Ls xi1 + xi2), one
// lock-step block solves K^ u = z and keeps w = P^-1 z, rho0 and the a / beta history; the host turns each column's history
// into its quadrature value, and the pair reduction adds the block's (-u_s / t, w_s) to the (alpha, alpha) pass that went
// first -- the order of the passes depends on t alone.
extern "C" int gogp_cg_lml_gradient(gogp_handle *h, const double *Xi, int64_t t, int64_t ldxi, double tol, int32_t max_iter,
                                    double *grad, int64_t len, double *quad, gogp_cg_lml_info *info, gogp_cg_col *cols) {
  const char *who = "cg_lml_gradient";
  if (const int rc = refuse_handle(h, who)) return rc;
  CgHandleState &cg = h->cg;
  if (!Xi || !info) return refuse(h, who, GOGP_EARG, "NULL");
  if (t < 1 || t > (1 << 20)) return refuse(h, who, GOGP_EARG, "need 1 <= t <= 2^20 probes");
  if (const char *why = cg_tol_refusal(tol, max_iter)) return refuse(h, who, GOGP_EARG, why);
  if (grad && len != h->P) return refuse(h, who, GOGP_EARG, "len(grad)");
  if (!cg.have || !cg.solved) return refuse(h, who, GOGP_ESTATE, "no solution (gogp_cg_solve)");
  const int64_t N = cg.N, npad = cg.npad;
  const int r = cg.rank, D = h->D;
  const int64_t nx = N + r;
  if (ldxi < nx) return refuse(h, who, GOGP_EARG, "ldxi is less than N + rank_used");
  if (grad && N >= (1 << 21)) return refuse(h, who, GOGP_EARG, "the gradient's pair reduction counts its tiles in 32 bits: N < 2^21 (grad == NULL computes the LML alone)");
  for (int64_t sI = 0; sI < t; ++sI)
    for (int64_t i = 0; i < nx; ++i)
      if (!std::isfinite(Xi[sI * ldxi + i])) return refuse(h, who, GOGP_EARG, "non-finite normal");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->s;
  *info = gogp_cg_lml_info();
  // the counters of the last solve / columns / produce call stay what gogp_cg_last_info reports
  struct Restore {
    CgHandleState &cg;
    const int p = cg.products, b = cg.blocks;
    ~Restore() { cg.products = p, cg.blocks = b; }
  } restore{cg};
  cg.products = cg.blocks = 0;
  const int gblocks = cg_grad_blocks(N);
  const size_t n_xi = (size_t)CG_MAX_T * (size_t)nx, n_hist = (size_t)2 * (size_t)max_iter * CG_MAX_T;
  int rc = cg.lml.reserve(h, (n_xi + n_hist + CG_MAX_T + NACC + (size_t)gblocks * NACC) * sizeof(double));
  if (rc == GOGP_OK) rc = cg.ks.reserve(h, (size_t)CG_MAX_T * (size_t)npad * sizeof(double));
  if (rc != GOGP_OK) return rc;
  double *dXi = cg.lml.as<double>(), *dhist = dXi + n_xi, *drho0 = dhist + n_hist, *gout = drho0 + CG_MAX_T;
  double *gpart = gout + NACC;
  double *dZ = cg.ks.as<double>();
  // log |P| = sum_i log D_i + log |C|: the diagonal comes down once and is summed in index order
  std::vector<double> hd((size_t)N);
  HIPCHK(h, hipMemcpyAsync(hd.data(), cg.d, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  double ldp = 0.0;
  for (int64_t i = 0; i < N; ++i) ldp += log(hd[(size_t)i]);
  ldp += cg.logdet_c;
  if (grad)
    launch_cg_grad(s, cg.P, D, h->ard_dims, cg.X, N, cg.alpha, cg.alpha, npad, 1, 1.0, gpart, gout, false);
  std::vector<double> hhist, q((size_t)t);
  double hrho0[CG_MAX_T];
  std::vector<gogp_cg_col> lcols((size_t)CG_MAX_T);
  int ret = GOGP_OK, lmax = 0;
  std::string first_err;
  const double *Ls = cg.L.as<double>();
  for (int64_t t0 = 0; t0 < t; t0 += CG_MAX_T) {
    const int cnt = (int)std::min<int64_t>(CG_MAX_T, t - t0);
    HIPCHK(h, hipMemcpy2DAsync(dXi, (size_t)nx * sizeof(double), Xi + t0 * ldxi, (size_t)ldxi * sizeof(double),
                               (size_t)nx * sizeof(double), (size_t)cnt, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemsetAsync(dZ, 0, (size_t)cnt * npad * sizeof(double), s));
    launch_cg_probes(s, Ls, cg.ldn, N, r, cg.d, dXi, nx, npad, cnt, dZ);
    CgKeep keep;
    keep.hist = dhist, keep.rho0 = drho0;
    double *xs = nullptr;
    rc = cg_block_solve(h, who, dZ, cnt, tol, max_iter, &xs, lcols.data(), (int)t0, &keep);
    if (rc != GOGP_OK && rc != GOGP_ENOCONV) return rc;
    if (rc != GOGP_OK && ret == GOGP_OK) ret = rc, first_err = h->err;
    int mmax = 0;
    for (int c = 0; c < cnt; ++c) mmax = std::max(mmax, (int)lcols[(size_t)c].iterations);
    lmax = std::max(lmax, mmax);
    hhist.resize((size_t)2 * (size_t)std::max(mmax, 1) * CG_MAX_T);
    if (mmax > 0)
      HIPCHK(h, hipMemcpyAsync(hhist.data(), dhist, (size_t)2 * mmax * CG_MAX_T * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(hrho0, drho0, sizeof hrho0, hipMemcpyDeviceToHost, s));
    if (grad)
      launch_cg_grad(s, cg.P, D, h->ard_dims, cg.X, N, xs, keep.w, npad, cnt, -1.0 / (double)t, gpart, gout, true);
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    for (int c = 0; c < cnt; ++c) {
      const int m = lcols[(size_t)c].iterations;
      q[(size_t)(t0 + c)] = cg_lanczos_quadrature(hhist.data() + c, hhist.data() + CG_MAX_T + c, 2 * CG_MAX_T, m, hrho0[c]);
      if (cols) cols[t0 + c] = lcols[(size_t)c];
    }
  }
  double qsum = 0.0;
  for (int64_t c = 0; c < t; ++c) qsum += q[(size_t)c];
  const double qmean = qsum / (double)t;
  double var = 0.0;
  for (int64_t c = 0; c < t; ++c) var += (q[(size_t)c] - qmean) * (q[(size_t)c] - qmean);
  info->logdet_precond = ldp;
  info->logdet = ldp + qmean;
  info->logdet_stderr = t > 1 ? sqrt(var / (double)(t - 1)) / sqrt((double)t) : 0.0;
  info->yt_alpha = cg.yta;
  info->lml = -0.5 * cg.yta - 0.5 * info->logdet - 0.5 * (double)N * log(2.0 * M_PI);
  info->probes = (int32_t)t;
  info->blocks = cg.blocks;
  info->products = cg.products;
  info->lanczos_max = lmax;
  if (quad)
    for (int64_t c = 0; c < t; ++c) quad[c] = q[(size_t)c];
  if (grad) {
    double acc[NACC];
    HIPCHK(h, hipMemcpyAsync(acc, gout, sizeof acc, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    for (int64_t i = 0; i < len; ++i) grad[i] = 0.0;
    assemble_gradient(h, acc, cg.dnoise, grad);
  }
  if (ret != GOGP_OK) h->err = first_err;
  return ret;
}

