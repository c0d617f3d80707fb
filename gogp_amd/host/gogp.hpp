// gogp.hpp -- C++ host-side mirror of the reference's gp.GP (gp/gp.go:20-38) over
// the C ABI of include/gogp_hip.h.  Header-only; link with -lgogp_hip.
//
// The reference is Go (compiled code) and no Go toolchain exists in the build
// image, so this header is the compiled-language host layer; the Go shim a
// maintainer would add is in go/gogp/gp.go.  Method names,
// argument meaning and error behaviour follow the reference: Absorb returns an
// error code (gp/gp.go:228-230), Observe throws where the reference panics
// (gp/gp.go:398-405), Produce returns false on error (gp/gp.go:338-340).
//
// X / Y are uploaded only when they changed: assign them through SetData() (or Absorb);
// after writing into the public X / Y members directly call Touch().  Alpha is refreshed
// after every Absorb / Observe, L lazily by Factor() (the reference documents L, Alpha, X,
// ThetaSimil, ThetaNoise as the state Produce depends on: gp/gp.go:35-36,255-257).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/gogp_hip.h"

namespace gogp {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

class GP {
 public:
  // Configuration (gp/gp.go:22-23)
  int NDim;
  gogp_desc desc;  // Simil + Noise in closed form (see gogp_desc)
  // Data (gp/gp.go:26-28)
  std::vector<double> ThetaSimil, ThetaNoise;
  std::vector<std::vector<double>> X;
  std::vector<double> Y;
  bool Parallel = false;  // accepted for compatibility
  // Cached computations (gp/gp.go:34-36)
  std::vector<double> Alpha;  // K^-1 y, refreshed by Absorb / Observe

  explicit GP(const gogp_desc &d, int device = -1) : NDim(d.ndim), desc(d) {
    if (gogp_create(&desc, device, &h_) != GOGP_OK)
      throw Error(GOGP_EHIP, gogp_last_error(nullptr));
    ThetaSimil.assign(desc.ntheta_simil, 0.0);  // gp/gp.go:50-56
    ThetaNoise.assign(gogp_desc_ntheta_noise(&desc), 0.0);
  }
  ~GP() { gogp_destroy(h_); }
  GP(const GP &) = delete;
  GP &operator=(const GP &) = delete;

  // gp/gp.go:80-87.  v: the observations' noise variances (SetNoiseVariances); empty: none, also when the previous
  // data had some.
  int Absorb(const std::vector<std::vector<double>> &x, const std::vector<double> &y,
             const std::vector<double> &v = std::vector<double>()) {
    SetData(x, y);
    int rc = push();
    if (rc != GOGP_OK) return rc;
    if (!v.empty()) {
      rc = SetNoiseVariances(v);
      if (rc != GOGP_OK) return rc;
    }
    double zero = 0.0;
    rc = gogp_absorb(h_, ThetaSimil.data(), ThetaNoise.empty() ? &zero : ThetaNoise.data());
    if (rc != GOGP_OK && rc != GOGP_ECOND) return rc;  // gp/gp.go:228-230
    const int ra = fetch_alpha();
    return ra != GOGP_OK ? ra : rc;  // GOGP_ECOND: gonum's Condition error, gp/gp.go:233-236
  }

  // Append observations to the absorbed ones at the parameters of the last Absorb / Observe (gogp_append; no reference
  // counterpart: tutorial/tutorial.go:118-142 refactorises).  An empty process absorbs them at ThetaSimil / ThetaNoise.
  // GOGP_ENOTPD: nothing changed.  GOGP_ESTATE: X / Y were re-assigned since the last upload (Absorb them instead).
  // v: the new observations' noise variances (gogp_append_noisy); empty: zeros.
  int Append(const std::vector<std::vector<double>> &x, const std::vector<double> &y,
             const std::vector<double> &v = std::vector<double>()) {
    if (x.size() != y.size() || (!v.empty() && v.size() != y.size())) return GOGP_EARG;
    if (Y.empty()) {
      int rc = push();
      if (rc != GOGP_OK) return rc;
      double zero = 0.0;
      rc = gogp_absorb(h_, ThetaSimil.data(), ThetaNoise.empty() ? &zero : ThetaNoise.data());
      if (rc != GOGP_OK) return rc;
    } else if (dirty_) {
      return GOGP_ESTATE;
    }
    if (y.empty()) return GOGP_OK;
    std::vector<double> flat = pack(x);
    const int rc = v.empty() ? gogp_append(h_, flat.data(), y.data(), (int64_t)y.size())
                             : gogp_append_noisy(h_, flat.data(), y.data(), v.data(), (int64_t)y.size());
    if (rc != GOGP_OK && rc != GOGP_ECOND) return rc;
    X.insert(X.end(), x.begin(), x.end());
    Y.insert(Y.end(), y.begin(), y.end());
    const int ra = fetch_alpha();
    return ra != GOGP_OK ? ra : rc;
  }

  // Remove the observations idx (any order, no duplicates) from the absorbed ones (gogp_remove; no reference
  // counterpart): the state Absorb on the kept rows would leave, without a new factorisation.  With Append a bounded
  // window slides: Remove({0}), then Append(new).  GOGP_EARG (duplicates, out of range): nothing changed.
  // GOGP_ESTATE: X / Y were re-assigned since the last upload (Absorb them instead).
  int Remove(const std::vector<int64_t> &idx) {
    std::vector<int64_t> s(idx);
    std::sort(s.begin(), s.end());
    for (size_t j = 0; j < s.size(); ++j)
      if (s[j] < 0 || s[j] >= (int64_t)Y.size() || (j > 0 && s[j] == s[j - 1])) return GOGP_EARG;
    if (dirty_) return GOGP_ESTATE;
    if (s.empty()) return GOGP_OK;
    const int rc = gogp_remove(h_, s.data(), (int64_t)s.size());
    if (rc != GOGP_OK && rc != GOGP_ECOND) return rc;
    size_t k = 0, j = 0;
    for (size_t i = 0; i < Y.size(); ++i) {
      if (j < s.size() && s[j] == (int64_t)i) {
        ++j;
        continue;
      }
      if (k != i) {
        X[k] = std::move(X[i]);
        Y[k] = Y[i];
      }
      ++k;
    }
    X.resize(k);
    Y.resize(k);
    const int ra = fetch_alpha();
    return ra != GOGP_OK ? ra : rc;
  }

  // Per-observation noise variances: K = k(X, X) + sigma^2(theta) I + diag(v), every v[i] finite and >= 0
  // (gogp_set_noise_variances; no reference counterpart).  An empty v clears them.  Stored results are dropped: Absorb
  // or Observe again.  They belong to the data: SetData (and so Absorb without v) clears them, Append and Remove carry
  // them.  Returns the status; GOGP_EARG: a wrong length, a negative or non-finite value, a handle that takes none.
  int SetNoiseVariances(const std::vector<double> &v) {
    if (v.empty()) return dirty_ ? GOGP_OK : gogp_set_noise_variances(h_, nullptr, 0);
    if (v.size() != Y.size()) return GOGP_EARG;
    const int rc = push();
    if (rc != GOGP_OK) return rc;
    return gogp_set_noise_variances(h_, v.data(), (int64_t)v.size());
  }
  // what the device holds for the current observations (zeros when none are set)
  std::vector<double> NoiseVariances() {
    std::vector<double> v(dirty_ ? Y.size() : (size_t)gogp_n(h_), 0.0);
    if (!dirty_ && !v.empty()) check(gogp_get_noise_variances(h_, v.data()));
    return v;
  }
  // dLML / dv[i] = 1/2 (Alpha[i]^2 - [K^-1]_ii) at the current parameters and variances (gogp_noise_variances_gradient)
  std::vector<double> NoiseVariancesGradient() {
    std::vector<double> dv((size_t)gogp_n(h_), 0.0);
    check(gogp_noise_variances_gradient(h_, dv.empty() ? nullptr : dv.data()));
    return dv;
  }

  // Assign the observations (gp.GP.X / gp.GP.Y); uploaded on the next Absorb / Observe.
  void SetData(const std::vector<std::vector<double>> &x, const std::vector<double> &y) {
    X = x;
    Y = y;
    dirty_ = true;
  }
  // Call after modifying the public X / Y members in place.
  void Touch() { dirty_ = true; }

  // gp/gp.go:244-253
  double LML() {
    double v = 0;
    check(gogp_lml(h_, &v));
    return v;
  }

  // gp/gp.go:258-360
  bool Produce(const std::vector<std::vector<double>> &x, std::vector<double> &mu,
               std::vector<double> &sigma) {
    std::vector<double> flat = pack(x);
    mu.assign(x.size(), 0.0);
    sigma.assign(x.size(), 0.0);
    return gogp_produce(h_, flat.data(), (int64_t)x.size(), mu.data(), sigma.data()) == GOGP_OK;
  }

  // Produce and d mu / d x, d sigma / d x (row-major x.size() x NDim); no reference counterpart
  bool ProduceGradient(const std::vector<std::vector<double>> &x, std::vector<double> &mu, std::vector<double> &sigma,
                       std::vector<double> &dmu, std::vector<double> &dsigma) {
    std::vector<double> flat = pack(x);
    mu.assign(x.size(), 0.0);
    sigma.assign(x.size(), 0.0);
    dmu.assign(flat.size(), 0.0);
    dsigma.assign(flat.size(), 0.0);
    return gogp_produce_gradient(h_, flat.data(), (int64_t)x.size(), mu.data(), sigma.data(), dmu.data(),
                                 dsigma.data()) == GOGP_OK;
  }

  // mu and the joint covariance of the latent function at the test points (row-major x.size() x x.size(), symmetric);
  // no reference counterpart
  bool ProduceCovariance(const std::vector<std::vector<double>> &x, std::vector<double> &mu, std::vector<double> &cov) {
    std::vector<double> flat = pack(x);
    mu.assign(x.size(), 0.0);
    cov.assign(x.size() * x.size(), 0.0);
    return gogp_produce_covariance(h_, flat.data(), (int64_t)x.size(), mu.data(), cov.data()) == GOGP_OK;
  }

  // Leave-one-out cross-validation at the current parameters (gogp_loo): the prediction of Y[i] by the process fitted
  // to the other observations -- mean, standard deviation, log density -- and the sum of the log densities; no
  // reference counterpart
  double LOO(std::vector<double> &mu, std::vector<double> &sigma, std::vector<double> &logp) {
    const size_t n = (size_t)gogp_n(h_);
    mu.assign(n, 0.0);
    sigma.assign(n, 0.0);
    logp.assign(n, 0.0);
    double total = 0.0;
    check(gogp_loo(h_, mu.data(), sigma.data(), logp.data(), &total));
    return total;
  }
  // d (LOO score) / d log theta, one entry per hyperparameter (gogp_loo_gradient)
  std::vector<double> LOOGradient() {
    std::vector<double> g(ThetaSimil.size() + ThetaNoise.size(), 0.0);
    check(gogp_loo_gradient(h_, g.data(), (int64_t)g.size()));
    return g;
  }

  // Non-Gaussian likelihoods by the Laplace approximation (gogp_laplace_*; no reference counterpart).  LaplaceObserve:
  // the approximate log marginal likelihood of Y under `lik` (GOGP_LIK_BERNOULLI_LOGIT: Y in {0, 1};
  // GOGP_LIK_POISSON_LOG: counts) at x = log theta, the mode found by a damped Newton iteration; drops the regression
  // state.  Returns the status, as Absorb does (nothing is thrown here): GOGP_OK, GOGP_ECOND or GOGP_ENOCONV (Newton did
  // not reach the tolerance) store the fit and *z -- GOGP_ENOCONV is reported exactly as GOGP_ECOND is -- anything else
  // is a failure.
  int LaplaceObserve(const std::vector<double> &x, int32_t lik, double *z) {
    int rc = push();
    if (rc != GOGP_OK) return rc;
    rc = gogp_laplace_observe(h_, lik, x.data(), (int64_t)x.size(), z);
    if (rc == GOGP_OK || rc == GOGP_ECOND || rc == GOGP_ENOCONV) {
      for (size_t i = 0; i < ThetaSimil.size(); ++i) ThetaSimil[i] = std::exp(x[i]);
      for (size_t i = 0; i < ThetaNoise.size(); ++i) ThetaNoise[i] = std::exp(x[ThetaSimil.size() + i]);
    }
    return rc;
  }
  // d LaplaceObserve / d log theta, the movement of the mode included (gogp_laplace_gradient)
  std::vector<double> LaplaceGradient() {
    std::vector<double> g(ThetaSimil.size() + ThetaNoise.size(), 0.0);
    check(gogp_laplace_gradient(h_, g.data(), (int64_t)g.size()));
    return g;
  }
  // the latent values f and a = K^-1 f at the mode; returns the Newton steps of the last LaplaceObserve
  int LaplaceMode(std::vector<double> &f, std::vector<double> &a) {
    const size_t n = (size_t)gogp_n(h_);
    f.assign(n, 0.0);
    a.assign(n, 0.0);
    int32_t it = 0;
    check(gogp_laplace_get_mode(h_, f.data(), a.data(), &it));
    return (int)it;
  }
  // latent mu and sigma (no noise, as Produce) and the response-scale prediction at the test points: E[y*] (poisson),
  // P(y* = 1) (bernoulli); throws on any status but GOGP_OK, as LaplaceGradient and LaplaceMode do
  void LaplaceProduce(const std::vector<std::vector<double>> &x, std::vector<double> &mu, std::vector<double> &sigma,
                      std::vector<double> &mean) {
    std::vector<double> flat = pack(x);
    mu.assign(x.size(), 0.0);
    sigma.assign(x.size(), 0.0);
    mean.assign(x.size(), 0.0);
    check(gogp_laplace_produce(h_, flat.data(), (int64_t)x.size(), mu.data(), sigma.data(), mean.data()));
  }

  // Leave-block-out cross-validation at the current parameters (gogp_blockcv): the rows are cut into the consecutive
  // blocks [start[f], start[f + 1]) -- start[0] = 0, start[F] = n, 1 .. GOGP_BLOCKCV_MAX rows each; blocks() builds equal
  // ones -- and every block is predicted jointly by the process fitted to all the other blocks.  mu, sigma: per row; logp:
  // the joint log density per block; returns their sum.  No reference counterpart.  Folds that are not contiguous:
  // permute the rows before assigning X / Y.
  static std::vector<int64_t> blocks(int64_t n, int64_t length) {
    std::vector<int64_t> start;
    for (int64_t s = 0; s < n && length > 0; s += length) start.push_back(s);
    start.push_back(n);
    return start;
  }
  double BlockCV(const std::vector<int64_t> &start, std::vector<double> &mu, std::vector<double> &sigma,
                 std::vector<double> &logp) {
    if (start.empty()) throw std::invalid_argument("gogp: BlockCV: start needs F + 1 entries");
    const size_t n = (size_t)gogp_n(h_);
    mu.assign(n, 0.0);
    sigma.assign(n, 0.0);
    logp.assign(start.size() - 1, 0.0);
    double total = 0.0;
    check(gogp_blockcv(h_, start.data(), (int64_t)start.size() - 1, mu.data(), sigma.data(), logp.data(), &total));
    return total;
  }
  // d (BlockCV score) / d log theta, one entry per hyperparameter (gogp_blockcv_gradient)
  std::vector<double> BlockCVGradient(const std::vector<int64_t> &start) {
    if (start.empty()) throw std::invalid_argument("gogp: BlockCVGradient: start needs F + 1 entries");
    std::vector<double> g(ThetaSimil.size() + ThetaNoise.size(), 0.0);
    check(gogp_blockcv_gradient(h_, start.data(), (int64_t)start.size() - 1, g.data(), (int64_t)g.size()));
    return g;
  }

  // Multi-output (gogp_multi_*): T output columns observed at the inputs X, sharing the kernel and the hyperparameters,
  // on one factorisation; no reference counterpart.  SetOutputs: Yt row-major n x T, n = Y.size(), T <= GOGP_MULTI_MAX_T
  // (pending X / Y are uploaded first; T == 0 clears); the outputs are dropped by whatever replaces or resizes the data.
  void SetOutputs(const std::vector<double> &Yt, int T) {
    if (T == 0) {
      check(gogp_multi_set_outputs(h_, nullptr, 0, 0));
      T_ = 0;
      return;
    }
    check(push());
    if (T < 0 || Yt.size() != Y.size() * (size_t)T) throw Error(GOGP_EARG, "len(Yt)");
    const double none = 0.0;
    check(gogp_multi_set_outputs(h_, Yt.empty() ? &none : Yt.data(), (int64_t)Y.size(), T));
    T_ = T;
  }
  // the sum of the outputs' LML; lml: one entry per output
  double MultiLML(std::vector<double> &lml) {
    lml.assign((size_t)T_, 0.0);
    double total = 0.0;
    check(gogp_multi_lml(h_, &total, lml.empty() ? nullptr : lml.data()));
    return total;
  }
  // d (that sum) / d log theta, one entry per hyperparameter
  std::vector<double> MultiGradient() {
    std::vector<double> g(ThetaSimil.size() + ThetaNoise.size(), 0.0);
    check(gogp_multi_gradient(h_, g.data(), (int64_t)g.size()));
    return g;
  }
  // A = K^-1 Yt, row-major n x T
  std::vector<double> MultiAlpha() {
    std::vector<double> a((size_t)gogp_n(h_) * (size_t)T_ + 1, 0.0);
    check(gogp_multi_get_alpha(h_, a.data()));
    a.pop_back();
    return a;
  }
  // mu row-major x.size() x T, sigma (shared by the outputs) x.size()
  bool MultiProduce(const std::vector<std::vector<double>> &x, std::vector<double> &mu, std::vector<double> &sigma) {
    std::vector<double> flat = pack(x);
    mu.assign(x.size() * (size_t)T_, 0.0);
    sigma.assign(x.size(), 0.0);
    const double none = 0.0;
    return gogp_multi_produce(h_, flat.data(), (int64_t)x.size(), mu.empty() ? const_cast<double *>(&none) : mu.data(),
                              sigma.data()) == GOGP_OK;
  }

  // Sparse (gogp_sparse_*): the collapsed variational bound of Titsias (2009) for N observations on M <=
  // GOGP_SPARSE_MAX_M inducing points, O(N M^2); no reference counterpart.  SetSparse: a data set of its own (x row-major
  // N x NDim, y, u row-major M x NDim), resident on the device beside X / Y, which it does not touch; M == 0 clears it.
  void SetSparse(const std::vector<double> &x, const std::vector<double> &y, const std::vector<double> &u) {
    sparse_m_ = 0;
    sparse_t_ = 0;  // (the library drops the outputs of SetSparseOutputs with the data)
    if (u.empty()) {
      check(gogp_sparse_set_data(h_, nullptr, nullptr, 0, nullptr, 0));
      return;
    }
    if (x.size() != y.size() * (size_t)NDim || u.size() % (size_t)NDim) throw Error(GOGP_EARG, "len(x), len(u)");
    check(gogp_sparse_set_data(h_, y.empty() ? nullptr : x.data(), y.empty() ? nullptr : y.data(), (int64_t)y.size(), u.data(),
                               (int64_t)(u.size() / (size_t)NDim)));
    sparse_m_ = u.size() / (size_t)NDim;
  }
  // the bound at x = log theta
  double SparseObserve(const std::vector<double> &x) {
    double bound = 0.0;
    check(gogp_sparse_observe(h_, x.data(), (int64_t)x.size(), &bound));
    return bound;
  }
  // d bound / d log theta at the parameters of the last SparseObserve
  std::vector<double> SparseGradient() {
    std::vector<double> g(ThetaSimil.size() + ThetaNoise.size(), 0.0);
    check(gogp_sparse_gradient(h_, g.data(), (int64_t)g.size()));
    return g;
  }
  // Replace the inducing points of SetSparse by u (row-major M x NDim, the same M) and nothing else: x, y and every device
  // buffer stay.  SparseObserve has to follow before a gradient or a forecast.
  void SetInducing(const std::vector<double> &u) {
    if (u.empty() || u.size() % (size_t)NDim) throw Error(GOGP_EARG, "len(u)");
    check(gogp_sparse_set_inducing(h_, u.data(), (int64_t)(u.size() / (size_t)NDim)));
  }
  // Greedy conditional-variance selection of at most M inducing points among the n rows of x (row-major n x NDim) at
  // logtheta (gogp_sparse_select_inducing): a partial Cholesky factorisation of k(x, x) with diagonal pivoting; the noise
  // does not enter.  It stops once no residual variance exceeds tol (tol < 0: the jitter 10^"sparse_jitter_log10"), so
  // idx (the rows in pick order), u (row-major, = x[idx]) and pivots (the residual variances at the picks) hold the
  // m <= M points taken; returns the trace term t0 - tr Qff for them.  Nothing of the process's state changes.
  double SelectInducing(const std::vector<double> &logtheta, const std::vector<double> &x, int64_t M, double tol,
                        std::vector<int64_t> &idx, std::vector<double> &u, std::vector<double> &pivots) {
    if (x.size() % (size_t)NDim) throw Error(GOGP_EARG, "len(x)");
    return select(logtheta, &x, M, tol, idx, u, pivots);
  }
  // ... among the rows of the sparse data already on the device (gogp_sparse_select_inducing_resident): re-selecting at
  // the current parameters without sending the data again.  SetInducing(u) moves the points there when m == M.
  double SelectInducingResident(const std::vector<double> &logtheta, int64_t M, double tol, std::vector<int64_t> &idx,
                                std::vector<double> &u, std::vector<double> &pivots) {
    return select(logtheta, nullptr, M, tol, idx, u, pivots);
  }
  // ---- the iterative exact GP: matrix-free preconditioned conjugate gradients (gogp_cg_*) ----
  // The data of the iterative calls (x: row-major N x NDim; v: per-observation noise variances, empty = none); all
  // empty clears them.  Nothing else of the process changes.
  void SetCG(const std::vector<double> &x, const std::vector<double> &y, const std::vector<double> &v = {}) {
    if (x.empty() && y.empty() && v.empty()) {
      cg_n_ = 0;
      check(gogp_cg_set_data(h_, nullptr, nullptr, nullptr, 0));
      return;
    }
    if (x.size() != y.size() * (size_t)NDim || (!v.empty() && v.size() != y.size())) throw Error(GOGP_EARG, "SetCG: sizes");
    check(gogp_cg_set_data(h_, x.data(), y.data(), v.empty() ? nullptr : v.data(), (int64_t)y.size()));
    cg_n_ = y.size();
  }
  // K^ alpha = y at logtheta with a pivoted-Cholesky preconditioner of at most `rank` columns (0: Jacobi; piv_tol < 0: the
  // sparse calls' jitter).  Returns the status, as LaplaceObserve does: GOGP_OK or GOGP_ENOCONV (max_iter reached; every
  // output written, alpha stored); anything else throws.
  int CGSolve(const std::vector<double> &logtheta, int32_t rank, double tol, int32_t max_iter, gogp_cg_info *info,
              gogp_cg_col *col = nullptr, double piv_tol = -1.0) {
    const int rc = gogp_cg_solve(h_, logtheta.data(), (int64_t)logtheta.size(), rank, piv_tol, tol, max_iter, info, col);
    if (rc != GOGP_ENOCONV) check(rc);
    return rc;
  }
  std::vector<double> CGAlpha() {
    std::vector<double> a(cg_n_ ? cg_n_ : 1, 0.0);
    check(gogp_cg_get_alpha(h_, a.data(), (int64_t)cg_n_));
    a.resize(cg_n_);
    return a;
  }
  // K^ S[t] = B[t] for the T rows (of N) of b, in lock-step blocks of GOGP_CG_MAX_RHS; cols: one entry per row
  int CGSolveColumns(const std::vector<double> &b, double tol, int32_t max_iter, std::vector<double> &s,
                     std::vector<gogp_cg_col> *cols = nullptr) {
    const int64_t T = cg_n_ ? (int64_t)(b.size() / cg_n_) : 0;
    s.assign(b.size(), 0.0);
    if (cols) cols->assign((size_t)T, gogp_cg_col());
    const int rc = gogp_cg_solve_columns(h_, T ? b.data() : nullptr, T, tol, max_iter, T ? s.data() : nullptr,
                                         cols && T ? cols->data() : nullptr);
    if (rc != GOGP_ENOCONV) check(rc);
    return rc;
  }
  // mu and (with_sigma) sigma of the exact posterior at the test points z (row-major m x NDim); sigma stays empty without
  // it, and no system is solved then
  int CGProduce(const std::vector<double> &z, bool with_sigma, double tol, int32_t max_iter, std::vector<double> &mu,
                std::vector<double> &sigma, std::vector<gogp_cg_col> *cols = nullptr) {
    const int64_t m = (int64_t)(z.size() / (size_t)NDim);
    mu.assign((size_t)m, 0.0);
    sigma.assign(with_sigma ? (size_t)m : 0, 0.0);
    if (cols) cols->assign((size_t)m, gogp_cg_col());
    const int rc = gogp_cg_produce(h_, m ? z.data() : nullptr, m, m ? mu.data() : nullptr,
                                   with_sigma && m ? sigma.data() : nullptr, tol, max_iter, cols && m ? cols->data() : nullptr);
    if (rc != GOGP_ENOCONV) check(rc);
    return rc;
  }
  gogp_cg_info CGLastInfo() {
    gogp_cg_info info;
    check(gogp_cg_last_info(h_, &info));
    return info;
  }
  // The LML and d LML / d log theta at the parameters of the last CGSolve, from t probes: xi holds t rows of ldxi >= N +
  // rank_used standard normals [xi2 (N) | xi1 (rank_used)] (gogp_cg_lml_gradient; nothing random happens in the library).
  // grad receives the gradient (nullptr: the pair reduction is skipped), quad the per-probe quadrature values.  Returns
  // the status as CGSolve does: GOGP_OK or GOGP_ENOCONV (every output written from the columns as they stand).
  int CGLmlGradient(const std::vector<double> &xi, int64_t t, int64_t ldxi, double tol, int32_t max_iter,
                    gogp_cg_lml_info *info, std::vector<double> *grad = nullptr, std::vector<double> *quad = nullptr,
                    std::vector<gogp_cg_col> *cols = nullptr) {
    if (t < 1 || ldxi < 1 || xi.size() < (size_t)((t - 1) * ldxi) + cg_n_) throw Error(GOGP_EARG, "CGLmlGradient: sizes");
    if (grad) grad->assign(ThetaSimil.size() + ThetaNoise.size(), 0.0);
    if (quad) quad->assign((size_t)t, 0.0);
    if (cols) cols->assign((size_t)t, gogp_cg_col());
    const int rc = gogp_cg_lml_gradient(h_, xi.data(), t, ldxi, tol, max_iter, grad ? grad->data() : nullptr,
                                        grad ? (int64_t)grad->size() : 0, quad ? quad->data() : nullptr, info,
                                        cols ? cols->data() : nullptr);
    if (rc != GOGP_ENOCONV) check(rc);
    return rc;
  }
  // Vecchia's approximation (gogp_vecchia_*): log p(y) ~ sum_i log p(y_i | y_c(i)) on the conditioning rows the table
  // names -- nbr: N x m int32 row-major, m <= GOGP_VECCHIA_MAX_M, row i distinct indices below i and then -1 padding
  // (gogp_vecchia_check).  A data set of its own that stays on the device; empty x, y and nbr clear it.
  static bool VecchiaCheck(const std::vector<int32_t> &nbr, int64_t rows, int32_t m, int64_t n, bool causal) {
    return (int64_t)nbr.size() >= rows * m && gogp_vecchia_check(nbr.data(), rows, m, n, causal ? 1 : 0) == GOGP_OK;
  }
  void SetVecchia(const std::vector<double> &x, const std::vector<double> &y, const std::vector<int32_t> &nbr, int32_t m,
                  const std::vector<double> &v = {}) {
    if (x.empty() && y.empty() && nbr.empty() && v.empty()) {
      vecchia_n_ = 0;
      check(gogp_vecchia_set_data(h_, nullptr, nullptr, nullptr, 0, nullptr, 0));
      return;
    }
    if (m < 0 || x.size() != y.size() * (size_t)NDim || nbr.size() != y.size() * (size_t)m || (!v.empty() && v.size() != y.size()))
      throw Error(GOGP_EARG, "SetVecchia: sizes");
    check(gogp_vecchia_set_data(h_, x.data(), y.data(), v.empty() ? nullptr : v.data(), (int64_t)y.size(),
                                nbr.empty() ? nullptr : nbr.data(), m));
    vecchia_n_ = y.size();
    vecchia_m_ = m;
  }
  // The value at x = log theta; terms (unless nullptr) receives N x 3: mu_i, s_i, log p_i
  double VecchiaObserve(const std::vector<double> &x, std::vector<double> *terms = nullptr) {
    double v = 0.0;
    if (terms) terms->assign(3 * vecchia_n_, 0.0);
    check(gogp_vecchia_observe(h_, x.data(), (int64_t)x.size(), &v, terms ? terms->data() : nullptr));
    return v;
  }
  // d value / d log theta at the parameters of the last VecchiaObserve: the exact derivative of its value
  std::vector<double> VecchiaGradient() {
    std::vector<double> g(ThetaSimil.size() + ThetaNoise.size(), 0.0);
    check(gogp_vecchia_gradient(h_, g.data(), (int64_t)g.size()));
    return g;
  }
  // mu and (unless nullptr) sigma of the test points, each conditioned on the rows its row of nbrz (x.size() x m) names
  void VecchiaProduce(const std::vector<std::vector<double>> &x, const std::vector<int32_t> &nbrz, std::vector<double> &mu,
                      std::vector<double> *sigma = nullptr) {
    if (nbrz.size() != x.size() * (size_t)vecchia_m_) throw Error(GOGP_EARG, "VecchiaProduce: the table is x.size() x m");
    std::vector<double> flat = pack(x);
    mu.assign(x.size(), 0.0);
    if (sigma) sigma->assign(x.size(), 0.0);
    check(gogp_vecchia_produce(h_, flat.data(), (int64_t)x.size(), nbrz.empty() ? nullptr : nbrz.data(), mu.data(),
                               sigma ? sigma->data() : nullptr));
  }
  // ... with the table built on the device (gogp_vecchia_neighbours etc.): the m nearest earlier rows under the distance
  // of x / lengths (lengths: empty = unscaled, else NDim values > 0), ties to the lower index, nearest first.
  // VecchiaNeighbours: one-shot; z empty: the causal table of x (rows x m), else z.size() rows over all of x.
  std::vector<int32_t> VecchiaNeighbours(const std::vector<double> &x, int32_t m, const std::vector<double> &lengths = {},
                                         const std::vector<std::vector<double>> &z = {}) {
    if (m < 0 || x.size() % (size_t)NDim || (!lengths.empty() && lengths.size() != (size_t)NDim))
      throw Error(GOGP_EARG, "VecchiaNeighbours: sizes");
    const size_t n = x.size() / (size_t)NDim, rows = z.empty() ? n : z.size();
    std::vector<int32_t> t(rows * (size_t)m, -1);
    if (n == 0 || t.empty()) return t;
    std::vector<double> flat = pack(z);
    check(gogp_vecchia_neighbours(h_, x.data(), (int64_t)n, z.empty() ? nullptr : flat.data(), (int64_t)z.size(),
                                  lengths.empty() ? nullptr : lengths.data(), m, t.data()));
    return t;
  }
  void SetVecchiaNearest(const std::vector<double> &x, const std::vector<double> &y, int32_t m,
                         const std::vector<double> &lengths = {}, const std::vector<double> &v = {}) {
    if (m < 0 || x.size() != y.size() * (size_t)NDim || (!lengths.empty() && lengths.size() != (size_t)NDim) ||
        (!v.empty() && v.size() != y.size()))
      throw Error(GOGP_EARG, "SetVecchiaNearest: sizes");
    check(gogp_vecchia_set_data_nearest(h_, x.data(), y.data(), v.empty() ? nullptr : v.data(), (int64_t)y.size(),
                                        lengths.empty() ? nullptr : lengths.data(), m));
    vecchia_n_ = y.size();
    vecchia_m_ = m;
  }
  // the resident table rebuilt under new lengths (same m); the last VecchiaObserve is dropped
  void VecchiaReneighbour(const std::vector<double> &lengths) {
    if (!lengths.empty() && lengths.size() != (size_t)NDim) throw Error(GOGP_EARG, "VecchiaReneighbour: sizes");
    check(gogp_vecchia_reneighbour(h_, lengths.empty() ? nullptr : lengths.data()));
  }
  std::vector<int32_t> VecchiaNeighbourTable() {
    std::vector<int32_t> t(vecchia_n_ * (size_t)vecchia_m_, -1);
    check(gogp_vecchia_get_neighbours(h_, t.empty() ? nullptr : t.data()));
    return t;
  }
  // VecchiaProduce on each test point's m nearest resident rows, found on the device; lengths empty: the resident
  // table's; nbrz (unless nullptr) receives the table
  void VecchiaProduceNearest(const std::vector<std::vector<double>> &x, std::vector<double> &mu,
                             std::vector<double> *sigma = nullptr, const std::vector<double> &lengths = {},
                             std::vector<int32_t> *nbrz = nullptr) {
    if (!lengths.empty() && lengths.size() != (size_t)NDim) throw Error(GOGP_EARG, "VecchiaProduceNearest: sizes");
    std::vector<double> flat = pack(x);
    mu.assign(x.size(), 0.0);
    if (sigma) sigma->assign(x.size(), 0.0);
    if (nbrz) nbrz->assign(x.size() * (size_t)vecchia_m_, -1);
    check(gogp_vecchia_produce_nearest(h_, flat.data(), (int64_t)x.size(), lengths.empty() ? nullptr : lengths.data(),
                                       mu.data(), sigma ? sigma->data() : nullptr,
                                       nbrz && !nbrz->empty() ? nbrz->data() : nullptr));
  }
  // SparseGradient and, from the same pass over the data, d bound / d U of the inducing points of SetSparse (dU:
  // row-major M x NDim)
  std::vector<double> SparseGradientInducing(std::vector<double> &dU) {
    if (sparse_m_ < 1) throw Error(GOGP_ESTATE, "SparseGradientInducing before SetSparse");
    std::vector<double> g(ThetaSimil.size() + ThetaNoise.size(), 0.0);
    dU.assign(sparse_m_ * (size_t)NDim, 0.0);
    check(gogp_sparse_gradient_inducing(h_, g.data(), (int64_t)g.size(), dU.data()));
    return g;
  }
  // mu and sigma of the sparse approximation at the test points (latent, unclamped, as Produce)
  bool SparseProduce(const std::vector<std::vector<double>> &x, std::vector<double> &mu, std::vector<double> &sigma) {
    std::vector<double> flat = pack(x);
    mu.assign(x.size(), 0.0);
    sigma.assign(x.size(), 0.0);
    return gogp_sparse_produce(h_, flat.data(), (int64_t)x.size(), mu.data(), sigma.data()) == GOGP_OK;
  }

  // Explicit basis functions (gogp_basis_*): a mean h(x)^T beta with beta integrated out under a flat prior (Rasmussen &
  // Williams section 2.7); no reference counterpart.  SetBasis: H row-major n x p, n = Y.size(), p <= GOGP_BASIS_MAX_P,
  // p < n (pending X / Y are uploaded first; p == 0 clears); the basis is dropped by whatever replaces or resizes the data.
  void SetBasis(const std::vector<double> &H, int p) {
    if (p == 0) {
      check(gogp_basis_set(h_, nullptr, 0, 0));
      p_ = 0;
      return;
    }
    check(push());
    if (p < 0 || H.size() != Y.size() * (size_t)p) throw Error(GOGP_EARG, "len(H)");
    const double none = 0.0;
    check(gogp_basis_set(h_, H.empty() ? &none : H.data(), (int64_t)Y.size(), p));
    p_ = p;
  }
  // the log marginal likelihood with beta integrated out, at the parameters of the last Absorb / Observe
  double BasisLML() {
    double lml = 0.0;
    check(gogp_basis_lml(h_, &lml));
    return lml;
  }
  // d BasisLML / d log theta, one entry per hyperparameter
  std::vector<double> BasisGradient() {
    std::vector<double> g(ThetaSimil.size() + ThetaNoise.size(), 0.0);
    check(gogp_basis_gradient(h_, g.data(), (int64_t)g.size()));
    return g;
  }
  // beta (p) and its covariance (H^T K^-1 H)^-1 (row-major p x p)
  std::vector<double> BasisBeta(std::vector<double> &cov) {
    std::vector<double> beta((size_t)p_ + 1, 0.0);
    cov.assign((size_t)p_ * (size_t)p_ + 1, 0.0);
    check(gogp_basis_get_beta(h_, beta.data(), cov.data()));
    beta.pop_back();
    cov.pop_back();
    return beta;
  }
  // alpha~ = K^-1 (y - H beta)
  std::vector<double> BasisAlpha() {
    std::vector<double> a((size_t)gogp_n(h_) + 1, 0.0);
    check(gogp_basis_get_alpha(h_, a.data()));
    a.pop_back();
    return a;
  }
  // mu and sigma at the test points x whose basis functions are the rows of Hz (row-major x.size() x p)
  bool BasisProduce(const std::vector<std::vector<double>> &x, const std::vector<double> &Hz, std::vector<double> &mu,
                    std::vector<double> &sigma) {
    if (Hz.size() != x.size() * (size_t)p_) throw Error(GOGP_EARG, "len(Hz)");
    std::vector<double> flat = pack(x);
    mu.assign(x.size(), 0.0);
    sigma.assign(x.size(), 0.0);
    return gogp_basis_produce(h_, flat.data(), Hz.data(), (int64_t)x.size(), mu.data(), sigma.data()) == GOGP_OK;
  }

  // Sparse multi-output (gogp_sparse_multi_*): T <= GOGP_SPARSE_MULTI_MAX_T output columns at the inputs of SetSparse on
  // one pass over the data; no reference counterpart.  SetSparseOutputs: Yt row-major N x T with the N of SetSparse, kept
  // on the device as given; T == 0 clears.  SetSparse drops the outputs, SetInducing keeps them.
  void SetSparseOutputs(const std::vector<double> &Yt, int T) {
    sparse_t_ = 0;
    if (T == 0) {
      check(gogp_sparse_multi_set_outputs(h_, nullptr, 0, 0));
      return;
    }
    if (T < 0 || Yt.size() % (size_t)T) throw Error(GOGP_EARG, "len(Yt)");
    const double none = 0.0;
    check(gogp_sparse_multi_set_outputs(h_, Yt.empty() ? &none : Yt.data(), (int64_t)(Yt.size() / (size_t)T), T));
    sparse_t_ = T;
  }
  // the sum of the outputs' bounds at x = log theta; bounds: one entry per output
  double SparseMultiObserve(const std::vector<double> &x, std::vector<double> &bounds) {
    bounds.assign((size_t)sparse_t_, 0.0);
    double total = 0.0;
    check(gogp_sparse_multi_observe(h_, x.data(), (int64_t)x.size(), &total, bounds.empty() ? nullptr : bounds.data()));
    return total;
  }
  // d (that sum) / d log theta at the parameters of the last SparseMultiObserve
  std::vector<double> SparseMultiGradient() {
    std::vector<double> g(ThetaSimil.size() + ThetaNoise.size(), 0.0);
    check(gogp_sparse_multi_gradient(h_, g.data(), (int64_t)g.size()));
    return g;
  }
  // SparseMultiGradient and, from the same pass over the data, d (that sum) / d U (dU: row-major M x NDim)
  std::vector<double> SparseMultiGradientInducing(std::vector<double> &dU) {
    if (sparse_m_ < 1) throw Error(GOGP_ESTATE, "SparseMultiGradientInducing before SetSparse");
    std::vector<double> g(ThetaSimil.size() + ThetaNoise.size(), 0.0);
    dU.assign(sparse_m_ * (size_t)NDim, 0.0);
    check(gogp_sparse_multi_gradient_inducing(h_, g.data(), (int64_t)g.size(), dU.data()));
    return g;
  }
  // mu row-major x.size() x T, sigma (shared by the outputs) x.size()
  bool SparseMultiProduce(const std::vector<std::vector<double>> &x, std::vector<double> &mu, std::vector<double> &sigma) {
    std::vector<double> flat = pack(x);
    mu.assign(x.size() * (size_t)sparse_t_, 0.0);
    sigma.assign(x.size(), 0.0);
    const double none = 0.0;
    return gogp_sparse_multi_produce(h_, flat.data(), (int64_t)x.size(), mu.empty() ? const_cast<double *>(&none) : mu.data(),
                                     sigma.data()) == GOGP_OK;
  }

  // ns = xi.size() / x.size() joint draws mu + C xi[s] (row-major ns x x.size()) from the caller's standard normals,
  // C the lower Cholesky factor of the covariance + diag_add I; no reference counterpart
  bool Sample(const std::vector<std::vector<double>> &x, const std::vector<double> &xi, double diag_add,
              std::vector<double> &mu, std::vector<double> &samples) {
    std::vector<double> flat = pack(x);
    const size_t m = x.size(), ns = m ? xi.size() / m : 0;
    if (m && ns * m != xi.size()) throw Error(GOGP_EARG, "len(xi)");
    mu.assign(m, 0.0);
    samples.assign(ns * m, 0.0);
    return gogp_produce_samples(h_, flat.data(), (int64_t)m, xi.data(), (int64_t)ns, diag_add, mu.data(),
                                samples.data()) == GOGP_OK;
  }

  // gp/gp.go:374-413
  double Observe(const std::vector<double> &x) {
    const size_t P = ThetaSimil.size() + ThetaNoise.size();
    if (x.size() < P) throw Error(GOGP_EARG, "len(x)");
    double lml = 0;
    if (x.size() == P) {
      check(push());  // uploads only if X / Y changed since the last call
      check(gogp_observe(h_, x.data(), (int64_t)x.size(), &lml));
    } else {
      if ((x.size() - P) % (NDim + 1)) throw Error(GOGP_EARG, "len(x)");  // gp/gp.go:398-400
      const int rc = gogp_observe_full(h_, x.data(), (int64_t)x.size(), &lml);
      // gp/gp.go:391-396: X, Y are re-sliced from x (the device holds them now)
      const size_t n = (x.size() - P) / (size_t)(NDim + 1);
      X.assign(n, std::vector<double>((size_t)NDim));
      for (size_t i = 0; i < n; ++i)
        for (int d = 0; d < NDim; ++d) X[i][d] = x[P + i * NDim + d];
      Y.assign(x.begin() + (long)(P + n * NDim), x.end());
      dirty_ = rc != GOGP_OK;
      check(rc);
    }
    check(fetch_alpha());
    for (size_t i = 0; i < ThetaSimil.size(); ++i) ThetaSimil[i] = std::exp(x[i]);
    for (size_t i = 0; i < ThetaNoise.size(); ++i) ThetaNoise[i] = std::exp(x[ThetaSimil.size() + i]);
    last_len_ = x.size();
    return lml;
  }

  // gp/gp.go:418-499
  std::vector<double> Gradient() {
    std::vector<double> g(last_len_, 0.0);
    check(gogp_gradient(h_, g.data(), (int64_t)g.size()));
    return g;
  }

  // k candidate log-theta vectors (hyperparameters-only form) on this GP's data in ONE launch
  // sequence (gogp_observe_gradient_candidates); the GP's own state is not touched.  lml[c] is NaN
  // and grad[c] zero where status[c] == GOGP_ENOTPD.  Counterpart: candidates evaluated
  // concurrently by the reference's optimiser (optimize.Settings.Concurrent, tutorial/tutorial.go:30,141).
  struct Candidates {
    std::vector<double> lml;
    std::vector<std::vector<double>> grad;
    std::vector<int> status;
  };
  Candidates ObserveGradientCandidates(const std::vector<std::vector<double>> &xs) {
    const size_t k = xs.size(), P = ThetaSimil.size() + ThetaNoise.size();
    std::vector<double> flat(k * P), lml(k), grads(k * P);
    for (size_t c = 0; c < k; ++c) {
      if (xs[c].size() != P) throw Error(GOGP_EARG, "len(x)");
      std::copy(xs[c].begin(), xs[c].end(), flat.begin() + (long)(c * P));
    }
    Candidates out;
    out.status.assign(k, GOGP_OK);
    check(push());
    const int rc = gogp_observe_gradient_candidates(h_, (int)k, flat.data(), (int64_t)P, lml.data(), grads.data(),
                                                    out.status.data());
    if (rc != GOGP_OK && rc != GOGP_ENOTPD && rc != GOGP_ECOND) check(rc);
    out.lml = lml;
    for (size_t c = 0; c < k; ++c)
      out.grad.emplace_back(grads.begin() + (long)(c * P), grads.begin() + (long)((c + 1) * P));
    return out;
  }

  // gp.GP.L (gp/gp.go:35): lower factor, row-major n x n, fetched on demand
  std::vector<double> Factor() {
    const size_t n = (size_t)gogp_n(h_);
    std::vector<double> L(n * n);
    check(gogp_get_factor(h_, L.data()));
    return L;
  }

  // gogp_set_option (no reference counterpart), e.g. ("gradient_precision", 32): Observe's LML, Alpha and Produce stay
  // fp64, what only Gradient needs runs on the fp32 matrix cores (one-term kernels with an output scale only: refused --
  // an exception -- for sums of terms, whose scale components would come off the float K^-1 at 1.9e-4)
  void SetOption(const char *name, int64_t value) { check(gogp_set_option(h_, name, value)); }

  // event discounts of tutorial/events/kernel/kernel.go:14-44 (gogp_set_events): events holds nevents
  // {from, to, discount} triples on input dimension `axis`; an empty vector clears them
  void SetEvents(const std::vector<double> &events, int axis = 0) {
    if (events.size() % 3) throw Error(GOGP_EARG, "SetEvents: events must be {from, to, discount} triples");
    check(gogp_set_events(h_, events.empty() ? nullptr : events.data(), (int)(events.size() / 3), axis));
  }

  gogp_handle *handle() { return h_; }

 private:
  gogp_handle *h_ = nullptr;
  size_t last_len_ = 0;
  bool dirty_ = true;
  int T_ = 0;  // output columns of SetOutputs
  int p_ = 0;  // basis columns of SetBasis
  size_t sparse_m_ = 0;  // inducing points of SetSparse
  int sparse_t_ = 0;     // output columns of SetSparseOutputs
  size_t cg_n_ = 0;      // observations of SetCG
  size_t vecchia_n_ = 0; // observations of SetVecchia
  int32_t vecchia_m_ = 0; // ... and the columns of its table

  std::vector<double> pack(const std::vector<std::vector<double>> &x) const {
    std::vector<double> flat(x.size() * (size_t)NDim);
    for (size_t i = 0; i < x.size(); ++i)
      for (int d = 0; d < NDim; ++d) flat[i * NDim + d] = x[i][d];
    return flat;
  }
  // the two forms of the greedy selection: x == nullptr is the resident one
  double select(const std::vector<double> &logtheta, const std::vector<double> *x, int64_t M, double tol,
                std::vector<int64_t> &idx, std::vector<double> &u, std::vector<double> &pivots) {
    const size_t cap = M > 0 ? (size_t)M : 1;
    idx.assign(cap, 0);
    pivots.assign(cap, 0.0);
    u.assign(cap * (size_t)NDim, 0.0);
    int64_t m = 0;
    double trace = 0.0;
    if (x)
      check(gogp_sparse_select_inducing(h_, logtheta.data(), (int64_t)logtheta.size(), x->empty() ? nullptr : x->data(),
                                        (int64_t)(x->size() / (size_t)NDim), M, tol, idx.data(), pivots.data(), u.data(), &m,
                                        &trace));
    else
      check(gogp_sparse_select_inducing_resident(h_, logtheta.data(), (int64_t)logtheta.size(), M, tol, idx.data(),
                                                 pivots.data(), u.data(), &m, &trace));
    idx.resize((size_t)m);
    pivots.resize((size_t)m);
    u.resize((size_t)m * (size_t)NDim);
    return trace;
  }
  int push() {
    if (!dirty_) return GOGP_OK;
    if (X.size() != Y.size()) return GOGP_EARG;
    std::vector<double> flat = pack(X);
    const int rc = gogp_set_data(h_, flat.data(), Y.data(), (int64_t)Y.size());
    if (rc == GOGP_OK) dirty_ = false;
    return rc;
  }
  int fetch_alpha() {
    Alpha.assign((size_t)gogp_n(h_), 0.0);
    return gogp_get_alpha(h_, Alpha.data());
  }
  void check(int rc) {
    if (rc != GOGP_OK) throw Error(rc, gogp_last_error(h_));
  }
};

}  // namespace gogp
