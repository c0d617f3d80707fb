/*
 * gogp_hip.h -- C ABI of the MI355X-native GP-regression hot path.
 *
 * This is the drop-in boundary for infergo-ml/gogp's gp.GP hot path
 * (reference: gp/gp.go).  Every entry point names the reference interface it
 * replaces.  The library behind it (libgogp_hip.so) is hand-written HIP for
 * gfx950; there is no CPU fallback: if no HIP device is usable every compute
 * entry point returns GOGP_EHIP.
 *
 * Conventions
 *   - all functions are extern "C", return an int status (GOGP_OK == 0),
 *     take plain pointers and sizes; no C++/torch types cross the boundary;
 *   - host pointers are borrowed for the duration of the call only (cgo rule:
 *     no Go pointer is retained); device memory is owned by the handle;
 *   - a handle is NOT safe for concurrent use (same as a gp.GP value, whose
 *     methods mutate its fields: gp/gp.go:84,384-385); different handles may
 *     be used from different threads;
 *   - matrices are row-major doubles.
 */
#ifndef GOGP_HIP_H
#define GOGP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes -------------------------------------------------------- */
#define GOGP_OK 0
#define GOGP_EARG 1   /* bad argument (wrong length, NULL, unknown kind)       */
#define GOGP_ENOTPD 2 /* K not positive definite: gp/gp.go:228-230 Factorize   */
#define GOGP_EHIP 3   /* HIP runtime error / no device / extension unusable    */
#define GOGP_ESTATE 4 /* call order (Gradient before Observe, ...)             */
#define GOGP_ENOMEM 5
#define GOGP_ECOND 6  /* K factored but numerically singular: gonum's Condition error
                         (cond > 1e16) from Cholesky.SolveVecTo / SolveTo, passed on by
                         gp/gp.go:233-236,338-340.  Here: (max L_ii/min L_ii)^2 > 1e16, a
                         lower bound of cond_2(K).  The factor, alpha and the LML are
                         still stored (as in gonum, which fills the result and returns the
                         error); the host shim decides: Absorb returns it as an error,
                         Observe panics, exactly where the reference does.          */
#define GOGP_ENOCONV 7 /* gogp_laplace_observe: Newton did not reach the tolerance; the last
                         iterate's values are returned and stored                          */

/* ---- kernel descriptors --------------------------------------------------
 * The reference accepts any Go value implementing
 *     type Kernel interface { Observe([]float64) float64; NTheta() int }
 * (gp/gp.go:14-17) and calls it once per pair (gp/gp.go:110-111).  A device
 * path needs a closed description instead: the similarity kernel is a SUM of
 * up to GOGP_MAX_TERMS terms, each  c * f(r)  with f one of the reference's
 * primitives (kernel/kernel.go).  This covers every kernel the reference
 * tree defines:
 *   kernel.Normal/Matern32/Matern52/Periodic       (kernel/kernel.go:23-92)
 *   c*Matern32                      (tutorial/barebones/kernel/kernel.go:14-16)
 *   c1*Matern52(l1)+c2*Periodic(l2,10p) (tutorial/hyperpriors/kernel/kernel.go:12-25)
 * For NDim > 1 (the reference primitives are 1-D, kernel/kernel.go:15-17) the
 * distance is  r^2 = sum_d ((xa_d-xb_d)/l_d)^2  (all l_d equal unless ard),
 * which reduces to the reference formulas at NDim == 1.
 */
#define GOGP_MAX_TERMS 4
#define GOGP_MAX_NDIM 64

enum gogp_simil_kind {
  GOGP_K_NORMAL = 0,            /* exp(-r^2/2)            kernel/kernel.go:23-26 */
  GOGP_K_MATERN32 = 1,          /* (1+s3 r)exp(-s3 r)     kernel/kernel.go:70-73 */
  GOGP_K_MATERN52 = 2,          /* (1+s5 r+1*r^2)exp(-s5 r): the reference's Go
                                   constant expression 5/3 is INTEGER division,
                                   i.e. 1 (kernel/kernel.go:91,
                                   kernel/ad/kernel.go:130)                      */
  GOGP_K_MATERN52_TEXTBOOK = 3, /* (1+s5 r+(5/3) r^2)exp(-s5 r)                  */
  GOGP_K_PERIODIC = 4           /* exp(-2 d^2), d=sin(pi|dx|/p)/l
                                                          kernel/kernel.go:44-47 */
};

enum gogp_noise_kind {
  GOGP_NOISE_CONSTANT = 0, /* kernel.ConstantNoise(std): var=std^2, NTheta=0
                              kernel/noise.go:21-34                             */
  GOGP_NOISE_UNIFORM = 1,  /* scale*kernel.UniformNoise: var=scale*std^2,
                              NTheta=1  kernel/noise.go:39-53; scale as in
                              tutorial/barebones/kernel/kernel.go:25-31         */
  GOGP_NOISE_CONSTANT_PARAM = 2 /* constant variance noise_std^2 WITH one parameter
                              the Gram matrix does not depend on (NTheta=1, its
                              gradient component is 0): the noise kernel of
                              tutorial/anynoise/kernel/kernel.go:26-35, whose
                              parameter only feeds the priors                   */
};

typedef struct gogp_term {
  int32_t kind;       /* enum gogp_simil_kind                                   */
  int32_t scale_idx;  /* index in ThetaSimil of the output scale c; -1: c == 1  */
  int32_t len_idx;    /* index in ThetaSimil of the (first) length scale        */
  int32_t ard;        /* 0: one length scale; 1: ndim consecutive length scales */
  int32_t period_idx; /* GOGP_K_PERIODIC: index of the period parameter         */
  int32_t reserved;
  double period_mult; /* effective period = period_mult * theta[period_idx]
                         (the 10*x[p] of tutorial/hyperpriors/kernel/kernel.go:24) */
} gogp_term;

typedef struct gogp_desc {
  int32_t ndim;         /* gp.GP.NDim                      gp/gp.go:22          */
  int32_t nterms;       /* 1..GOGP_MAX_TERMS                                    */
  int32_t ntheta_simil; /* gp.GP.Simil.NTheta()                                 */
  int32_t noise_kind;   /* enum gogp_noise_kind; gp.GP.Noise; nil => CONSTANT
                           with std 1e-5 (gp/gp.go:43-48)                       */
  double noise_std;     /* CONSTANT: the std                                    */
  double noise_scale;   /* UNIFORM: variance = noise_scale * std^2              */
  gogp_term terms[GOGP_MAX_TERMS];
} gogp_desc;

typedef struct gogp_handle gogp_handle;

/* ---- lifecycle ------------------------------------------------------------ */

/* Validate a descriptor; returns GOGP_OK or GOGP_EARG.  Pure host code. */
int gogp_desc_check(const gogp_desc *desc);

/* Number of noise parameters, Noise.NTheta(): 0 (CONSTANT) or 1. */
int gogp_desc_ntheta_noise(const gogp_desc *desc);

/* Create a handle on HIP device `device` (-1: the current device).
 * Replaces: constructing a gp.GP{NDim,Simil,Noise} value (gp/gp.go:20-24). */
int gogp_create(const gogp_desc *desc, int device, gogp_handle **out);
void gogp_destroy(gogp_handle *h);

/* Last error text for this handle (never NULL). With h == NULL: the text of
 * the last failed gogp_create on this thread. */
const char *gogp_last_error(const gogp_handle *h);

/* After GOGP_ENOTPD: 0-based index of the failing pivot, else -1. */
int64_t gogp_notpd_index(const gogp_handle *h);

/* ---- data ------------------------------------------------------------------
 * Replaces: assigning gp.GP.X ([][]float64, n slices of NDim) and gp.GP.Y
 * (gp/gp.go:27-28,84).  X is packed row-major n x ndim by the caller's shim.
 * The data are copied to the device; n == 0 is legal (gp/gp.go:101-104). */
int gogp_set_data(gogp_handle *h, const double *X, const double *y, int64_t n);

/* Same, but X and y already live in device memory of the handle's device
 * (used by bench.py so the timed region starts with inputs resident in HBM). */
int gogp_set_data_device(gogp_handle *h, const double *dX, const double *dy,
                         int64_t n);

/* ---- event discounts (tutorial/events/kernel/kernel.go:14-44) -------------------------
 * The similarity of two points on different sides of an event boundary is multiplied by the
 * event's discount: with xa <= xb the coordinates of the two points on input dimension `axis`,
 * the FIRST event (in list order) with  xa < from <= xb  or  xa < to <= xb  applies its
 * discount to the whole similarity (all terms; not the noise), and the walk stops.  Events are
 * constants, not parameters: NTheta, the gradient slots and the noise are unchanged, and every
 * derivative is the discount times the undiscounted one.  `axis` generalises the reference's
 * 1-D x[a], x[b] to NDim > 1 (the reference case: axis = 0, ndim = 1).  Not combined with an
 * ARD term (GOGP_EARG). */
#define GOGP_MAX_EVENTS 32
/* Pure host validation: 0 <= nevents <= GOGP_MAX_EVENTS, 0 <= axis < ndim,
 * from / to / discount finite.  GOGP_OK or GOGP_EARG. */
int gogp_events_check(const double *events /* nevents x 3: from, to, discount */,
                      int nevents, int axis, int ndim);
/* Event discounts of tutorial/events/kernel/kernel.go:14-44 on input dimension
 * `axis`, multiplying the whole similarity (all terms); nevents == 0 clears.
 * Stored results (factor, alpha) no longer match and are dropped, as by gogp_set_data.
 * On a sharded handle every rank makes the same call. */
int gogp_set_events(gogp_handle *h, const double *events, int nevents, int axis);

/* ---- the hot path ----------------------------------------------------------*/

/* gp.GP.Absorb (gp/gp.go:80-87) minus the data assignment (gogp_set_data):
 * Gram build (gp/gp.go:109-156,220-225), Cholesky (gp/gp.go:228), alpha
 * (gp/gp.go:232-236), WITHOUT gradient.  theta_* are natural-scale
 * ThetaSimil/ThetaNoise (gp/gp_test.go:29).  Non-PD => GOGP_ENOTPD. */
int gogp_absorb(gogp_handle *h, const double *theta_simil,
                const double *theta_noise);

/* gp.GP.Observe, hyperparameters-only form (gp/gp.go:370-373,374-413):
 * x = log-transformed [ThetaSimil | ThetaNoise] (len P); X, Y as set by
 * gogp_set_data.  Computes exp(x), Gram, Cholesky, alpha, and returns
 * LML (gp/gp.go:244-253) in *lml.  Unlike the reference x is NOT mutated
 * (the reference exp()s and log()s it back in place, gp/gp.go:378-381,
 * 408-410).  A following gogp_gradient returns d LML / d x.
 * Errors are returned as codes; the Go shim turns them into the reference's
 * panic (gp/gp.go:402-405). */
int gogp_observe(gogp_handle *h, const double *x, int64_t len, double *lml);

/* gp.GP.Observe, full form (gp/gp.go:366-369,386-397): x = [log theta (P) |
 * x_0..x_{n-1} (ndim each) | y_0..y_{n-1}], n = (len-P)/(ndim+1); replaces the
 * handle's data by the inputs/outputs carried in x.  len must equal
 * P + n*(ndim+1) for an integer n (reference: panic("len(x)"), gp/gp.go:398-400). */
int gogp_observe_full(gogp_handle *h, const double *x, int64_t len, double *lml);

/* gp.GP.LML (gp/gp.go:244-253) of the last absorb/observe; 0 when n == 0. */
int gogp_lml(gogp_handle *h, double *lml);

/* gp.GP.Gradient (gp/gp.go:418-499): gradient of LML w.r.t. the argument of
 * the last gogp_observe[_full]: P entries d/d log theta, then -- after
 * gogp_observe_full -- n*ndim entries d/d x_i,d and n entries d/d y_i = -alpha_i
 * (gp/gp.go:488-493).  `len` must be that length.  n == 0 => zeros
 * (gp/gp.go:427-430). */
int gogp_gradient(gogp_handle *h, double *grad, int64_t len);

/* Leave-one-out cross-validation (Rasmussen & Williams 5.4.2) at the parameters of the last gogp_absorb /
 * gogp_observe[_full] / gogp_set_factor; no reference counterpart (its forecast harness refits per prefix).  From the
 * explicit K^-1 the gradient leaves on the device, kappa_i = [K^-1]_ii, and alpha:
 *     mu_i = y_i - alpha_i / kappa_i,  sigma_i = sqrt(1 / kappa_i),
 *     logp_i = 1/2 log kappa_i - 1/2 alpha_i^2 / kappa_i - 1/2 log 2 pi,  total = sum_i logp_i
 * -- the prediction of y_i, noise included, by the process fitted to the other n - 1 observations.  mu, sigma, logp:
 * n doubles each, any of them may be NULL; total may be NULL.
 * gogp_loo_gradient: d total / d log theta, P = ntheta_simil + ntheta_noise entries (`len` must be P; also after
 * gogp_observe_full: the observations' own derivatives are not formed).  One extra symmetric product for all
 * parameters: sum_ab W_ab dK_ab with W = 1/2 (u alpha^T + alpha u^T) - K^-1 diag(w) K^-1, v_i = alpha_i / kappa_i,
 * u = K^-1 v, w_i = 1/2 (1 + alpha_i^2 / kappa_i) / kappa_i, reduced by the kernels of gogp_gradient, so every kernel
 * family, ARD and the event discounts of gogp_set_events are covered.
 * Works wherever gogp_produce works with the data on the device: after Absorb (no Observe needed), Observe in either
 * form, gogp_append, gogp_remove and gogp_set_factor.  Where K^-1 is not there yet (Absorb, option "eager" = 0, after
 * Append / Remove / set_factor) the call forms it as gogp_gradient does.  The handle is left as it was found: a
 * gogp_gradient, gogp_produce, gogp_get_factor or gogp_append made afterwards returns the bits it would have returned
 * before.  Two identical calls return identical bits (fixed-order sums, no atomics).  n == 0: total = 0, the arrays
 * are not written, the gradient is zeros.  Nothing is clamped: for a positive definite K every kappa_i > 0, otherwise
 * the values are what the divisions yield (as sigma of gogp_produce).
 * GOGP_ESTATE before anything is factored; GOGP_EARG for len != P, a precision = 32 handle, "gradient_precision" = 32
 * (a float K^-1) and a sharded handle (the restrictions of gogp_append).
 * Device memory: gogp_loo 7 vectors of npad doubles; gogp_loo_gradient also two npad x npad fp64 matrices (4.3 GB at
 * n = 16384), allocated on first use and kept until the data's buffers are released.
 * Cost, measured on one MI355X with K^-1 in place (profiles/loo.txt; D = 8, beside Observe + Gradient on the same
 * build): gogp_loo 0.08 / 0.07 / 0.10 ms at n = 1024 / 4096 / 16384 -- one 5 us kernel over the diagonal, the rest is
 * the copies and the synchronise; gogp_loo_gradient 0.13 / 1.50 / 67.8 ms against 0.68 / 3.1 / 70.9 ms for
 * Observe + Gradient, i.e. one more evaluation at n = 16384, of which the product B B^T is 65 ms (n^3 flops at
 * 68 TFLOP/s), the pass over K^-1 0.84 ms, the rank-2 correction 0.44 ms and the reduction 0.60 ms. */
int gogp_loo(gogp_handle *h, double *mu, double *sigma, double *logp, double *total);
int gogp_loo_gradient(gogp_handle *h, double *grad, int64_t len);

/* Leave-block-out ("h-block", leave-out-k; Rasmussen & Williams 5.4.2) cross-validation at the parameters of the last
 * gogp_absorb / gogp_observe[_full] / gogp_set_factor; no reference counterpart.  The rows are cut into F consecutive
 * blocks B_f = [start[f], start[f + 1]), start[0] = 0, start[F] = n, of 1 .. GOGP_BLOCKCV_MAX rows each, and every block
 * is predicted jointly by the process fitted to all the other blocks: for time-ordered data the hold-out that leave-one-
 * out is not (its held-out point sits between neighbours one step away).  From the explicit K^-1 = Q the gradient leaves
 * on the device and alpha, per block with Q_BB = C C^T (lower Cholesky), X = C^-1, w = X alpha_B, v_B = X^T w:
 *     mu_B = y_B - v_B,  sigma_i = sqrt((X^T X)_ii)  (noise included, as gogp_loo),
 *     logp_f = -1/2 |w|^2 + sum_i log C_ii - |B_f| / 2 log 2 pi = log p(y_B | every other block),  total = sum_f logp_f
 * (added in block order).  mu, sigma: n doubles; logp: F doubles; any of them and total may be NULL.  Blocks of one row
 * give gogp_loo's values.
 * gogp_blockcv_gradient: d total / d log theta, P entries (`len` must be P), as gogp_loo_gradient: sum_ab W_ab dK_ab with
 * W = 1/2 (u alpha^T + alpha u^T) - 1/2 Q M Q, v the stacked v_B, u = Q v, M = blockdiag(X^T X + v_B v_B^T), whose
 * square root S_B = X^T + gamma v_B w^T, gamma = 1 / (sqrt(1 + |w|^2) + 1), needs no second factorisation; Q blockdiag(S_B)
 * then takes the place of gogp_loo_gradient's K^-1 diag(s), so every kernel family, ARD and the event discounts of
 * gogp_set_events are covered.
 * gogp_blockcv_check (host only): GOGP_OK for a `start` as described -- start[0] == 0, strictly increasing, start[F] == n,
 * every block of at most GOGP_BLOCKCV_MAX rows -- else GOGP_EARG.  gogp_blockcv_groups (host only): how the calls pack
 * consecutive blocks, greedily and in order, into groups of at most 128 rows, each factored by one workgroup (blocks of
 * one row cost n / 128 workgroups, not n): group g holds the blocks first[g] .. first[g + 1] - 1; first has room for
 * F + 1 entries, *ngroups <= 2 n / 129 + 1.
 * Contract (gogp_loo's, restated for blocks): works wherever gogp_loo works -- after Absorb, Observe in either form,
 * gogp_append, gogp_remove and gogp_set_factor -- and forms K^-1 as gogp_gradient does where it is missing.  The handle
 * is left as it was found: a gogp_gradient, gogp_produce, gogp_get_factor, gogp_loo, gogp_loo_gradient or gogp_append made
 * afterwards returns the bits it would have returned without these calls.  Two identical calls return identical bits
 * (fixed-order sums, no atomics); the result depends on K^-1, alpha, y and start alone.  n == 0 (F == 0, start = {0}):
 * total = 0, the arrays are not written, the gradient is zeros.
 * GOGP_EARG: what gogp_blockcv_check refuses, len != P, a precision = 32 handle, "gradient_precision" = 32 and a sharded
 * handle (gogp_loo's refusals).  GOGP_ESTATE before anything is factored.  GOGP_ENOTPD: a block of K^-1 has a
 * non-positive pivot, which happens only when K is numerically singular; gogp_notpd_index is the row, gogp_last_error
 * names the block, nothing is promised for the outputs and the fitted process is untouched.  Nothing is clamped.
 * Out of scope: blocks longer than GOGP_BLOCKCV_MAX rows (the per-block factorisation lives in LDS; longer folds would
 * go through the factorisation launches of gogp_produce_samples); buffer zones around a block ("hv-block");
 * non-contiguous folds -- row order carries no meaning for the process, so a caller who wants random folds permutes the
 * rows before gogp_set_data; the fp32 and sharded paths.
 * Device memory: gogp_blockcv 7 vectors of npad doubles, the tables of start and the groups' 128 x 128 square roots
 * (ngroups x 128 KB: under 34 MB at n = 16384); gogp_blockcv_gradient also gogp_loo_gradient's two npad x npad matrices,
 * which it shares.
 * Cost, measured on one MI355X with K^-1 in place (profiles/blockcv.txt; D = 8, blocks of 1 / 16 / 128 rows, beside
 * gogp_loo, gogp_loo_gradient and Observe + Gradient on the same build): gogp_blockcv 0.13 - 0.14 ms at n = 1024 and
 * 4096, 0.15 - 0.19 ms at n = 16384, against 0.08 - 0.10 ms for gogp_loo -- the group kernel is 48 - 66 us whatever n and
 * the block length, the rest is the upload of start, the copies and two synchronises; gogp_blockcv_gradient 0.22 - 0.23 /
 * 1.70 - 1.73 / 71.2 - 71.6 ms at n = 1024 / 4096 / 16384 against 0.13 / 1.50 / 68.4 ms for gogp_loo_gradient and
 * 0.67 / 3.1 / 71.2 ms for Observe + Gradient: at n = 16384 the block multiply is 2.4 ms, 3.6 % of the product behind it
 * (66.5 ms).  For blocks of one row gogp_loo remains the call: the same numbers to 1e-14 at about half the time. */
#define GOGP_BLOCKCV_MAX 128
int gogp_blockcv_check(const int64_t *start, int64_t F, int64_t n);
int gogp_blockcv_groups(const int64_t *start, int64_t F, int64_t *first, int64_t *ngroups);
int gogp_blockcv(gogp_handle *h, const int64_t *start, int64_t F, double *mu, double *sigma, double *logp, double *total);
int gogp_blockcv_gradient(gogp_handle *h, const int64_t *start, int64_t F, double *grad, int64_t len);

/* Non-Gaussian likelihoods by the Laplace approximation (Rasmussen & Williams 3.4, 5.5.1); no reference counterpart.
 * y is the handle's y (gogp_set_data), K the Gram matrix exactly as gogp_absorb builds it -- the similarity plus the
 * noise variance on the diagonal, which acts as the latent nugget -- so every parameter keeps its slot and its
 * derivative.  With pi = 1 / (1 + exp(-f)):
 *     GOGP_LIK_BERNOULLI_LOGIT  log p(y|f) = y f - softplus(f)            y in {0, 1}
 *     GOGP_LIK_POISSON_LOG      log p(y|f) = y f - exp(f) - lgamma(y + 1) y a non-negative integer
 * gogp_laplace_observe: theta = exp(x) (`len` must be P), the mode f^ = K a^ of psi(a) = -1/2 a^T f + sum_i log p(y_i|f_i)
 * by Newton's iteration (R&W Alg. 3.1) -- per step one factorisation of B = I + W^1/2 K W^1/2 (W = -d2 log p / df2), two
 * substitutions and two products with K -- damped: the step is halved while psi does not increase beyond the rounding
 * of its sums (1e-12 max(1, |psi|)), 20 times at the most.  Converged when |a - dlog p/df|_inf <= tol max(1, |a|_inf);
 * B is then factored once more AT the mode, and *lml = Z = psi(a^) - sum_i log L_ii.
 * gogp_laplace_gradient: dZ/dlog theta, P entries, implicit part (the mode moves with theta) included.  R&W eq. 5.23 and
 * the s2 line of Alg. 5.1 carry a sign error; the sign here is the one a central difference of Z confirms.
 * gogp_laplace_get_mode: f^ and a^ (n doubles each) and the Newton steps the last observe took; any may be NULL.
 * gogp_laplace_produce: at the m test points Z the latent mean mu = k*^T a^ and standard deviation sigma, sigma^2 =
 * k(z, z) - |L^-1 (W^1/2 k*)|^2 (no noise, not clamped: as gogp_produce), and -- `mean` may be NULL -- the response-scale
 * prediction: Poisson E[y*] = exp(mu + sigma^2 / 2), Bernoulli P(y* = 1) = int pi(f) N(f | mu, sigma^2) df by a fixed
 * 32-point Gauss-Hermite rule.
 * gogp_laplace_check (host only): GOGP_OK when the likelihood accepts every y[i], else GOGP_EARG.
 * Options (gogp_set_option): "laplace_max_iter" 1..200 (50), "laplace_tol_log10" -14..-4 (-10), "laplace_warm" 0 | 1 (0;
 * 1: an observe starts from the last converged a^ of the same data and likelihood instead of a = 0).
 * State: the calls work in the handle's own N-sized buffers -- B's factor lies where K's does, B^-1 and then the
 * gradient's weight matrix where K^-1 does -- plus a few vectors.  A Laplace observe DROPS the regression state, as
 * gogp_set_data does: gogp_gradient, gogp_produce, gogp_loo, gogp_append and the rest return GOGP_ESTATE until the next
 * gogp_absorb / gogp_observe, which then return the bits a fresh handle returns.  Whatever factors or replaces the data
 * (set_data, absorb, observe, append, remove, set_factor, set_events) and the options that resize buffers drop the
 * Laplace state.  Sparse data, batch data, the candidates arena and the multi-output Y are untouched.  Two identical
 * call sequences return identical bits; with "laplace_warm" = 0 an observe does not depend on earlier Laplace calls.
 * GOGP_EARG: NULL, len != P, an unknown lik, a non-finite parameter, a y the likelihood refuses (found on the device),
 * precision = 32, gradient_precision = 32, a sharded handle.  GOGP_ESTATE: no data; gradient, mode or produce before a
 * Laplace observe.  GOGP_ENOTPD: a pivot of B failed (B >= I cannot fail in exact arithmetic), *lml = NaN.  GOGP_ECOND:
 * as gogp_absorb, on B's factor.  GOGP_ENOCONV: "laplace_max_iter" steps or 20 halvings without convergence; *lml is
 * the last iterate's, and gradient and produce work on it.  n == 0: *lml = 0, a zero gradient, mu = 0, sigma =
 * sqrt(prior), mean = the likelihood's mean at that prior.
 * Out of scope: other likelihoods, multi-class, EP / variational inference, the sparse, batch, candidates, fp32 and
 * sharded paths, the full Observe form, Append / Remove on a Laplace fit.
 * Device memory: 24 vectors of npad doubles and a few block results; no matrix beyond the handle's own.
 * Cost, measured on one MI355X (profiles/laplace.txt; D = 8, n = 1024 / 4096 / 16384, wall time with the synchronise): one
 * Newton iteration, everything included (a cold observe over its factorisations of B), 0.70 / 2.8 / 31.9 ms against 0.64 /
 * 2.9 / 30.6 ms for gogp_absorb (1.10 / 0.97 / 1.04 of it); an observe of s Newton steps factors s + 1 times: from a = 0, s = 4 - 5 (Bernoulli) 3.5 / 16.9 / 192 ms, s = 8 - 9 (Poisson) 6.3 /
 * 25.8 / 320 ms; warm at the same theta 0.69 / 3.0 / 31.9 ms; gogp_laplace_gradient 0.36 / 1.86 / 49.7 ms (the lazy inverse
 * and three passes over B^-1); gogp_laplace_produce of 1024 points 0.21 / 0.67 / 5.7 ms against 0.18 / 0.63 / 5.2 ms for
 * gogp_produce, of one point 0.13 / 0.38 / 2.04 ms against 0.09 / 0.15 / 0.43 ms (the tile route for every m). */
enum gogp_lik_kind { GOGP_LIK_BERNOULLI_LOGIT = 0, GOGP_LIK_POISSON_LOG = 1 };
int gogp_laplace_check(int32_t lik, const double *y, int64_t n);
int gogp_laplace_observe(gogp_handle *h, int32_t lik, const double *x, int64_t len, double *lml);
int gogp_laplace_gradient(gogp_handle *h, double *grad, int64_t len);
int gogp_laplace_get_mode(gogp_handle *h, double *f, double *a, int32_t *iterations);
int gogp_laplace_produce(gogp_handle *h, const double *Z, int64_t m, double *mu, double *sigma, double *mean);

/* Multi-output: T output columns Y = [y_1 .. y_T] observed at the handle's inputs, sharing its kernel and
 * hyperparameters, on ONE factorisation; no reference counterpart (gp.GP holds one output vector).  The columns are
 * independent: no cross-output covariance, no per-output theta.  With A = K^-1 Y
 *     lml_t = -1/2 y_t^T a_t - sum_i log L_ii - n/2 log 2 pi,   total = sum_t lml_t (in column order),
 *     d total / d log theta = 1/2 sum_ab (A A^T - T K^-1)_ab dK_ab,   mu[j][t] = sum_i k(z_j, x_i) A[i][t].
 * gogp_multi_set_outputs copies Y (n x T row-major, n == gogp_n(h), 1 <= T <= GOGP_MULTI_MAX_T) to the device; it needs
 * data but no factorisation and does not touch the handle's own y, alpha, LML, factor or K^-1.  T == 0 with Y == NULL
 * clears the outputs.  They are dropped by whatever replaces or resizes the data -- gogp_set_data[_device],
 * gogp_observe_full, gogp_append, gogp_remove, a change of option "precision" -- and the other calls then return
 * GOGP_ESTATE until outputs are set again.
 * The other four calls work at the parameters of the last gogp_absorb / gogp_observe[_full] / gogp_set_factor, in every
 * state in which gogp_loo works.  A comes from the factor (Produce's forward and gogp_produce_gradient's backward
 * substitution with Y^T as the right-hand sides, so lml has the accuracy of gogp_lml), is solved on first need after a
 * factorisation and kept.  gogp_multi_lml: total, and lml (T doubles) unless NULL.  gogp_multi_gradient: d total /
 * d log theta, `len` == P whichever Observe form ran last; K^-1 is formed as gogp_gradient forms it where it is not
 * there, one pass writes G = T K^-1 - A A^T and the kernels of gogp_gradient reduce it, so every kernel family, ARD and
 * the event discounts are covered.  gogp_multi_get_alpha: A, n x T row-major.  gogp_multi_produce: mu (m x T
 * row-major) and sigma (m doubles, shared by the outputs: as gogp_produce returns it, no noise, unclamped; may be NULL,
 * which saves the substitution); m == 0 is OK.
 * The handle is left as it was found: a gogp_gradient, gogp_produce, gogp_get_factor, gogp_loo or gogp_append made
 * afterwards returns the bits it would have returned without these calls.  Two identical calls return identical bits
 * (fixed-order sums, no atomics).  n == 0: total, lml and the gradient are zeros, mu zeros and sigma = sqrt(prior).
 * GOGP_ESTATE before outputs are set and before anything is factored; GOGP_EARG for NULL pointers, n != gogp_n(h), T
 * outside 1 .. GOGP_MULTI_MAX_T, a non-finite output, len != P, a precision = 32 handle, "gradient_precision" = 32 (a
 * float K^-1) and a sharded handle (the restrictions of gogp_loo).
 * Device memory: Y^T and A^T, 128 rows of npad doubles each (33 MB at n = 16384), a tile row of Produce's workspace,
 * mpad x 128 doubles for the means; gogp_multi_gradient also one npad x npad fp64 matrix (2.1 GB at n = 16384),
 * allocated on first use; all kept until the data's buffers are released.
 * Cost, measured on one MI355X (profiles/multi_output.txt; D = 8, T = 1 / 8 / 128, beside Observe + Gradient on the same
 * build, every call ending in a synchronise): at n = 16384 the first gogp_multi_lml behind a factorisation -- the two
 * substitutions and the dots -- 3.8 / 3.8 / 4.9 ms, again 0.04 - 0.08 ms; gogp_multi_gradient with K^-1 in place 1.13 /
 * 1.13 / 2.17 ms; gogp_multi_produce at m = 256 3.3 / 3.3 / 3.6 ms; a whole evaluation Observe + multi_lml +
 * multi_gradient 80.5 / 80.1 / 82.9 ms against 71.7 ms for ONE Observe + Gradient, i.e. 1.12 / 0.14 / 0.009 of T separate
 * evaluations (n = 4096: 4.3 / 4.3 / 4.7 against 3.2 ms, 1.34 / 0.18 / 0.011; n = 1024: 0.89 / 0.95 / 0.95 against
 * 0.69 ms, 1.30 / 0.18 / 0.011).  For ONE output the calls lose to gogp_observe + gogp_gradient at every size: use those.
 * gogp_multi_set_outputs and gogp_multi_get_alpha transpose on the host: 30.9 and 11.1 ms at n = 16384, T = 128
 * (0.29 and 0.17 ms at T = 8). */
#define GOGP_MULTI_MAX_T 128 /* one 128-tile of right-hand-side rows */
int gogp_multi_set_outputs(gogp_handle *h, const double *Y /* n x T row-major */, int64_t n, int32_t T);
int gogp_multi_lml(gogp_handle *h, double *total, double *lml /* T, may be NULL */);
int gogp_multi_gradient(gogp_handle *h, double *grad, int64_t len /* P */);
int gogp_multi_get_alpha(gogp_handle *h, double *A /* n x T row-major */);
int gogp_multi_produce(gogp_handle *h, const double *Z, int64_t m, double *mu /* m x T */, double *sigma /* m */);

/* Explicit basis functions: a mean h(x)^T beta whose coefficients are integrated out under a flat prior (Rasmussen &
 * Williams section 2.7, eq. 2.41 - 2.45 in the limit B^-1 -> 0); no reference counterpart (gp.GP has mean zero).  H is
 * n x p, row i holding h(x_i); with K the handle's Gram matrix (noise included) and alpha = K^-1 y
 *     W = K^-1 H,  A = H^T W = L_A L_A^T,  g = H^T alpha,  beta = A^-1 g,  cov(beta) = A^-1,  alpha~ = alpha - W beta,
 *     lml_b = gogp_lml + 1/2 g^T beta - 1/2 log|A| + p/2 log 2 pi,
 *     d lml_b / d log theta = 1/2 sum_ab (alpha~ alpha~^T + Q Q^T - K^-1)_ab dK_ab,  Q = W L_A^-T,
 *     mu_b = mu_0 + R beta,  sigma_b^2 = sigma_0^2 + diag(R A^-1 R^T),  R = H_z - Kstar^T W  (mu_0, sigma_0: gogp_produce).
 * gogp_basis_set copies H (n x p row-major, n == gogp_n(h), 1 <= p <= GOGP_BASIS_MAX_P, p < n, every entry finite) to
 * the device; it needs data but no factorisation and touches nothing of the handle's own state.  p == 0 with H == NULL
 * clears the basis.  It is dropped by whatever replaces or resizes the data (the list of gogp_multi_set_outputs), and
 * the other calls then return GOGP_ESTATE until a basis is set again.
 * The other calls work at the parameters of the last gogp_absorb / gogp_observe / gogp_set_factor, in every state in which
 * gogp_multi_lml works; W, the factor of A, beta and alpha~ are computed on first need after a factorisation and kept.
 * W = K^-1 H comes from the explicit K^-1 (one symmetric product on the matrix cores, basis.hip) where that matrix is on
 * the device or on its way -- behind gogp_observe or any gradient -- and from the factor by two substitutions otherwise,
 * so a gogp_basis_produce behind gogp_absorb or gogp_set_factor does not form an inverse; option "basis_symm" forces a
 * route.  gogp_basis_gradient (`len` == P) forms K^-1 as gogp_gradient does where it is not there, one pass writes G =
 * K^-1 - [Q | alpha~][Q | alpha~]^T and the kernels of gogp_gradient reduce it: every kernel family, ARD and the event
 * discounts are covered; it is refused behind gogp_observe_full.  gogp_basis_get_beta: beta (p) and, unless NULL, its
 * covariance A^-1 (p x p).  gogp_basis_get_alpha: alpha~ (n).  gogp_basis_produce: Hz is m x p row-major, the basis at
 * the test points; sigma may be NULL, which saves the substitution; m == 0 is OK.
 * The handle is left as a gogp_gradient (gogp_basis_produce: a gogp_produce) at this point would have left it, and two
 * identical calls return identical bits (fixed-order sums, no atomics).
 * GOGP_EARG: NULL pointers, n != gogp_n(h), p outside 1 .. GOGP_BASIS_MAX_P, n <= p, a non-finite entry of H or Hz,
 * len != P, the full Observe form, a precision = 32 handle, "gradient_precision" = 32, a sharded handle.  GOGP_ECOND: a
 * pivot of A is not positive and finite -- the basis columns are linearly dependent; gogp_last_error names the pivot.
 * Device memory: H^T and W^T, 128 rows of npad doubles each, 68 rows for [Q | alpha~]^T, the slabs of the symmetric
 * product (at most 16 x p x npad doubles); gogp_basis_gradient shares the npad x npad matrix of gogp_multi_gradient. */
#define GOGP_BASIS_MAX_P 64
int gogp_basis_set(gogp_handle *h, const double *H /* n x p row-major */, int64_t n, int32_t p);
int gogp_basis_lml(gogp_handle *h, double *lml);
int gogp_basis_gradient(gogp_handle *h, double *grad, int64_t len /* P */);
int gogp_basis_get_beta(gogp_handle *h, double *beta /* p */, double *cov /* p x p, may be NULL */);
int gogp_basis_get_alpha(gogp_handle *h, double *alpha /* n */);
int gogp_basis_produce(gogp_handle *h, const double *Z, const double *Hz /* m x p */, int64_t m, double *mu,
                       double *sigma /* m, may be NULL */);

/* Sparse (inducing-point) approximation: the collapsed variational bound of Titsias (2009) for N observations (X, y) on
 * M <= GOGP_SPARSE_MAX_M inducing points U, with the handle's kernel; no reference counterpart.  It costs O(N M^2) and
 * O(M^2 + chunk M) device memory instead of O(N^3) and O(N^2), is a lower bound of the exact LML and equals it for
 * U = X.  With k the similarity at theta, s2 the noise variance, eps the jitter:
 *     Kuu = k(U, U) + eps I = L L^T,  V = L^-1 k(U, X),  B = I + V V^T / s2,  r = V y,  g = B^-1 r,  t0 = sum_f k(x_f, x_f),
 *     bound = -N/2 log 2 pi - 1/2 log|B| - N/2 log s2 - y^T y / (2 s2) + r^T g / (2 s2^2) - (t0 - s2 (tr B - M)) / (2 s2),
 *     mu(z) = v^T g / s2,   sigma(z)^2 = k(z, z) - |v|^2 + v^T B^-1 v,   v = L^-1 k(U, z)
 * (latent and unclamped, as gogp_produce).  DESIGN.md section 4, "Sparse", has the gradient.
 * gogp_sparse_set_data copies X (N x D), y and U (M x D) to the device, where they stay: a data set of its own, as the
 * batch data is.  N == 0 is legal; M == 0 with U == NULL clears it.  gogp_sparse_observe evaluates the bound at
 * x = log theta (len == P, the handle's parameters); gogp_sparse_gradient its derivative in log theta at the parameters
 * of the last gogp_sparse_observe; gogp_sparse_produce the predictive mean and standard deviation at m test points (m == 0
 * is OK).  N == 0: bound 0, zero gradient, mu = 0, sigma = sqrt(prior).
 * The data goes through in chunks of option "sparse_chunk" rows, twice for the gradient; nothing of size N^2 is
 * allocated and nothing is copied from the host inside observe or gradient.  The handle's own data, factor, K^-1, batch
 * data, candidates arena and multi-output state are not touched: a gogp_produce or gogp_gradient made afterwards returns
 * the bits it would have returned without these calls, and the sparse data survives a gogp_set_data.  Two identical call
 * sequences return identical bits (fixed-order sums, no atomics); results across chunk sizes agree to rounding only.
 * GOGP_EARG: NULL pointers or non-finite values, M outside 1 .. GOGP_SPARSE_MAX_M, len != P, a precision = 32 handle, a
 * sharded handle, a handle with event discounts set (events are out of scope here).  GOGP_ESTATE: any call before
 * gogp_sparse_set_data; gradient or produce before observe.  GOGP_ENOTPD: Kuu + eps I has a non-positive pivot -- the
 * bound is NaN and gogp_notpd_index is the inducing point (B >= I never fails).  GOGP_ECOND: (max L_ii / min L_ii)^2 of
 * Kuu's factor exceeds the handle's limit; the values are still returned, as in gogp_absorb.
 * Options: "sparse_jitter_log10" -14 .. -2 (default -8): eps = 10^value, absolute; "sparse_chunk" a multiple of 256 in
 * 256 .. 65536 (default 8192).
 * Device memory: X and y, eight Mp x Mp fp64 matrices (Mp = M rounded up to 256; 1.1 GB at M = 4096), a dense handle for
 * the M inducing points and two chunk x Mp matrices (2 x 268 MB at the defaults and M = 4096).
 * Cost, measured on one MI355X (profiles/sparse.txt; D = 8, default options, medians, every call ending in a synchronise):
 * gogp_sparse_observe / observe + gradient at N = 65536: 14.1 / 15.5 ms (M = 512), 23.9 / 35.0 ms (M = 2048), 72.1 /
 * 115.2 ms (M = 4096); N = 262144: 53.7 / 58.7, 87.1 / 126.9, 257.4 / 403.0 ms; N = 1048576: 212.1 / 231.1, 339.1 / 491.9,
 * 999.6 / 1552.9 ms; gogp_sparse_produce of 1024 points 0.2 - 1.3 ms.  At N = 16384, M = 4096 observe + gradient takes
 * 43.0 ms beside 71.3 ms for the dense gogp_observe + gogp_gradient (bound -10664.90 beside the LML -10662.82).  The new
 * SYRK runs well below the tile kernel: 27.6 against 60.9 TFLOP/s for GEMM_LOWER at M = 4096, K = 8192 (20.4 against 45.8
 * at M = 2048, 1.6 against 7.9 at M = 512); it is not tuned.
 * Learning the inducing points.  gogp_sparse_gradient_inducing returns gogp_sparse_gradient's grad (bit for bit) and, from
 * the same second pass over the data, the derivative of the bound in the inducing points.  With W (M x N), G (M x M,
 * symmetric), P and m of DESIGN.md section 4, "Sparse" (W = 2 P Kuf + m y^T / s2^2):
 *     dU[a][d] = sum_f W_af dk(u_a, x_f)/du_ad  +  2 sum_b G_ab dk(u_a, u_b)/du_ad
 * (u_a enters Kuu through row a and column a; the jitter and t0 do not depend on U; a pair of coincident points
 * contributes exact zeros).  The same preconditions and error codes as gogp_sparse_gradient, GOGP_EARG for dU == NULL;
 * N == 0: zeros in both.  It takes, beyond the memory above, slabs x M x D doubles of slab partials and two M x D arrays;
 * slabs = min(ceil(chunk / 256), floor(2048 / ceil(M / 64))), the most any chunk of up to "sparse_chunk" rows needs (one
 * slab per 256 rows, longer slabs once M / 64 x slabs would exceed 2048 workgroups -- the count is not monotone in the
 * rows, so a ragged last chunk may take more slabs than a full one; the buffer is sized by the bound).
 * gogp_sparse_set_inducing replaces U and nothing else: X, y, every buffer and the options stay, nothing of size N is
 * copied.  M must equal the M of gogp_sparse_set_data (GOGP_EARG otherwise, as for NULL, a non-finite value or a refused
 * kind of handle; GOGP_ESTATE before gogp_sparse_set_data).  Gradient and produce return GOGP_ESTATE until the next
 * gogp_sparse_observe, from which on every sparse call returns the bits of a fresh handle given
 * gogp_sparse_set_data(X, y, U).
 * Measured on the same build (profiles/sparse_inducing.txt, the rules above): observe + gradient_inducing at N = 65536
 * 16.5 / 36.3 / 118.8 ms for M = 512 / 2048 / 4096 (observe + gradient: 15.4 / 34.6 / 115.2), N = 1048576: 244.0 / 494.6 /
 * 1590.2 ms (231.3 / 477.9 / 1557.0); gogp_sparse_set_inducing 0.06 - 0.15 ms beside 2.4 - 8.6 ms for gogp_sparse_set_data.
 * Accuracy: dU along its own direction against a central difference of the bound agrees to 8e-6 .. 6.7e-3 at
 * "sparse_jitter_log10" = -6 at every size; at the default -8 to 1e-4 .. 3e-3 for M <= 2048, but at M = 4096 (random subset
 * of the inputs, cond(Kuu + eps I) ~ 1e12) it is off by 0.09 / 0.5 / 0.9 of |dU| at N = 65536 / 262144 / 1048576: the rounding
 * of P and G, ~cond * 1e-16, against parts that cancel -- a supposition from how the error scales with the jitter (a tenth
 * to a fiftieth per decade), not isolated by forming P and G in higher precision.  The call does not refuse the
 * combination: the conditioning depends on where the points lie, not on M and the jitter alone.  Learn that many inducing
 * points at a jitter of 1e-6 or more. */
#define GOGP_SPARSE_MAX_M 4096
int gogp_sparse_set_data(gogp_handle *h, const double *X, const double *y, int64_t N, const double *U, int64_t M);
int gogp_sparse_observe(gogp_handle *h, const double *x /* log theta */, int64_t len /* P */, double *bound);
int gogp_sparse_gradient(gogp_handle *h, double *grad, int64_t len /* P */);
int gogp_sparse_produce(gogp_handle *h, const double *Z, int64_t m, double *mu, double *sigma);
/* Replace the inducing points; X, y, buffers and options stay.  M must equal the M of gogp_sparse_set_data. */
int gogp_sparse_set_inducing(gogp_handle *h, const double *U /* M x ndim */, int64_t M);
/* gogp_sparse_gradient and, from the same pass over the data, d bound / d U.  NOT a usable gradient where Kuu + eps I is
 * ill-conditioned: M = 4096 at the default "sparse_jitter_log10" = -8 is off by 0.09 .. 0.9 of |dU| (above); use -6 there. */
int gogp_sparse_gradient_inducing(gogp_handle *h, double *grad /* P */, int64_t len, double *dU /* M x ndim */);

/* Sparse multi-output: T <= GOGP_SPARSE_MULTI_MAX_T output columns Y (N x T) observed at the inputs of the sparse data, under
 * one kernel, noise, jitter and set of inducing points, on ONE pass over the data: the cross-covariances, the substitution,
 * B, its factor, B^-1 and the second pass's 2 P k(U, X) do not depend on y.  With L, V, B, Yu = L^-T, t0 of the sparse section:
 *     R = V Y (M x T),  Gamma = B^-1 R,  c0 = -N/2 log 2 pi - 1/2 log|B| - N/2 log s2 - (t0 - s2 (tr B - M)) / (2 s2),
 *     bound_t = c0 - y_t^T y_t / (2 s2) + r_t^T gamma_t / (2 s2^2),   total = sum_t bound_t (column order),
 *     mu(z)[t] = v^T gamma_t / s2,   sigma(z) as gogp_sparse_produce, shared by the outputs
 * ("Sparse multi-output", has the gradient; for T = 1 it is the single-output form).
 * gogp_sparse_multi_set_outputs copies Y to the device as given (row-major, no transpose on the host), where it stays; it
 * needs gogp_sparse_set_data first and N equal to its N.  T == 0 with Y == NULL clears the outputs; gogp_sparse_set_data
 * drops them, gogp_sparse_set_inducing keeps them.  The y of gogp_sparse_set_data does not enter any result of these calls.
 * gogp_sparse_multi_observe returns the total and (bounds != NULL) the T bounds; gogp_sparse_multi_gradient the derivative
 * of the total in log theta; gogp_sparse_multi_gradient_inducing that and d total / d U; gogp_sparse_multi_produce the
 * m x T means and the m standard deviations.  Inside observe and gradient nothing is copied from the host.
 * State: the multi calls and the single-output calls share the Mp x Mp workspace, and the last observe of either flavour
 * owns it: gradient / produce of the other flavour return GOGP_ESTATE until that flavour's own observe, and after
 * gogp_sparse_set_inducing both do.  A single-output observe / gradient / produce made after any multi sequence returns
 * the bits a fresh handle returns; the handle's dense state is not touched (as above).  Two identical call sequences return
 * identical bits; results across chunk sizes agree to rounding.  Options "sparse_chunk" and "sparse_jitter_log10" apply.
 * GOGP_EARG: NULL pointers, a non-finite value in Y / Z / x, T outside 1 .. GOGP_SPARSE_MULTI_MAX_T, N != the sparse N,
 * len != P, the kinds of handle the sparse calls refuse.  GOGP_ESTATE: before the sparse data or the outputs are set;
 * gradient / produce before the multi observe.  GOGP_ENOTPD / GOGP_ECOND: as gogp_sparse_observe (ENOTPD: total and bounds
 * are NaN).  N == 0: total 0, bounds zeros, gradient and dU zeros, mu zeros, sigma = sqrt(prior); m == 0 is OK.
 * Device memory beyond the sparse section's: Y, four 128 x Mp matrices, the slab partials of the one new pass (R += V Y:
 * slabs x T' x M' doubles, T' and M' rounded up to 64, slabs = min(ceil(chunk / 256), floor(1024 / (M'/64 T'/64))), which
 * covers every chunk length) and chunk x 128 doubles.
 * Cost, measured on one MI355X (tools/sparse_multi_probe.py, profiles/sparse_multi.txt, which carries the build id of the
 * library before these figures were written here; D = 8, default options, medians of 5 rounds, every call ending in a
 * synchronise), observe + gradient in ms for T = 1 / 8 / 128 beside the single-output observe + gradient of the same build:
 * N = 65536, M = 512: 16.14 / 16.14 / 16.33 beside 15.51; M = 4096: 117.40 / 117.26 / 118.90 beside 114.31; N = 1048576,
 * M = 512: 240.24 / 240.85 / 244.87 beside 231.41; M = 4096: 1583.9 / 1584.6 / 1610.9 beside 1550.0.  So T outputs cost 1.02 -
 * 1.06 single-output evaluations: 0.128 - 0.130 of T separate ones at T = 8, 0.0081 - 0.0083 at T = 128, and the calls win
 * from T = 8 of the T measured (1, 8, 128).  At T = 1 they LOSE by 2.2 - 4.0 %: use the single-output calls for one column.
 * observe alone (T = 1 / 128): 14.53 / 14.66, 73.70 / 74.81, 219.4 / 222.0, 1021.5 / 1036.5 ms; with dU 17.24 / 17.40,
 * 120.57 / 122.60, 252.7 / 257.5, 1616.9 / 1643.2 ms; gogp_sparse_multi_produce of 1024 points 0.20 - 0.26 ms (M = 512) and
 * 1.38 - 1.52 ms (M = 4096).  The one new pass, R += V Y with its ordered final sum, is 1.9 - 3.8 % of observe (0.065 ms per
 * chunk of 8192 rows at M = 512, 0.30 ms at M = 4096, nearly the same for every T: a tile is 64 outputs wide whatever T; 16
 * and 29 TFLOP/s at T = 128).  gogp_sparse_multi_set_outputs at T = 128: 3.7 - 3.8 ms at N = 65536, 53.7 - 65.2 ms at
 * N = 1048576 (1 GB over the host link, the finiteness check and the column sums). */
#define GOGP_SPARSE_MULTI_MAX_T 128
int gogp_sparse_multi_set_outputs(gogp_handle *h, const double *Y /* N x T row-major */, int64_t N, int32_t T);
int gogp_sparse_multi_observe(gogp_handle *h, const double *x, int64_t len /* P */, double *total, double *bounds /* T, may be NULL */);
int gogp_sparse_multi_gradient(gogp_handle *h, double *grad, int64_t len /* P */);
int gogp_sparse_multi_gradient_inducing(gogp_handle *h, double *grad, int64_t len, double *dU /* M x ndim */);
int gogp_sparse_multi_produce(gogp_handle *h, const double *Z, int64_t m, double *mu /* m x T */, double *sigma /* m */);

/* Sparse: choosing the inducing points.  Greedy conditional-variance selection (Burt, Rasmussen & van der Wilk, 2019 /
 * 2020): a partial Cholesky factorisation of k(X, X) with diagonal pivoting, which at every step takes the row whose
 * variance given the rows already chosen is largest.  X (N x ndim), the similarity k at theta = exp(x), a cap M and a
 * tolerance tol >= 0; the noise does not enter:
 *     d_i = k(x_i, x_i)                                      i < N
 *     for j = 0 .. M-1:
 *         p = the LOWEST index among the maximisers of d      (ties: lowest index; all d equal at j = 0, so idx[0] = 0)
 *         if not (d_p > tol): stop, m = j                     (also stops on NaN)
 *         idx[j] = p,  pivots[j] = d_p
 *         l_i = (k(x_i, x_p) - sum_{t<j} L[i][t] L[p][t]) / sqrt(d_p)   for rows not yet selected
 *         l_p = sqrt(d_p);  l_i = 0 exactly for rows selected earlier
 *         L[:, j] = l;  d_i -= l_i^2;  d_p = 0 exactly (selected rows keep d = 0)
 *     m = number of steps taken;  trace = sum_i d_i  (= tr K - |L|_F^2 = t0 - tr Qff for U = X[idx])
 * pivots is non-increasing up to rounding; L[idx] equals chol(k(U, U)) in pivot order, so the Cholesky pivots of Kuu stay
 * above tol; a duplicated row is never picked twice; the selection greedily minimises the trace term of the bound.
 * gogp_sparse_select_inducing uploads X for the call; gogp_sparse_select_inducing_resident selects among the rows of the
 * sparse data already on the device (GOGP_ESTATE before gogp_sparse_set_data): re-selecting at the current theta during
 * an optimisation without sending N rows again.  One body.  idx (M), pivots (M), U (M x ndim): the entries from m on are
 * left alone; pivots, U and trace may be NULL.  tol < 0 means 10^"sparse_jitter_log10": a residual variance below the
 * jitter is indistinguishable from it.  M > N is legal and gives m <= N; N == 0 gives m = 0, trace = 0 and GOGP_OK.
 * Nothing of the handle changes -- dense data / factor / K^-1, sparse data and its observed state, batch data, candidates,
 * multi-output, basis and Laplace state: every later call returns the bits it would have returned without this one.
 * Two identical calls return identical bits (one launch per step, no atomics, every sum in a fixed order).
 * GOGP_EARG: h, x, idx or m_out NULL, X NULL with N > 0, N < 0, len != P, a non-finite value in x or X, M outside
 * 1 .. GOGP_SPARSE_MAX_M, tol = +inf or NaN, the kinds of handle the sparse calls refuse (precision = 32, sharded, event
 * discounts).  GOGP_ENOMEM: the transient factor could not be allocated (gogp_last_error carries the size).
 * Device memory, allocated by the call on the handle's main stream and freed before it returns: the factor, min(M, N)
 * columns of N rounded up to 256 doubles (34 GB at N = 1048576, M = 4096), X (the first form) and O(N + M ndim) beside it.
 * Cost: one launch and one pass over the factor per step, 8 N j bytes at step j, 4 N m^2 bytes in all.  Measured on one
 * MI355X (tools/select_inducing_probe.py, profiles/select_inducing.txt, which carries the build id of the library before
 * these figures were written here; D = 8, tol = 0 so that m = M, the resident form, medians of 5): M = 512 / 2048 / 4096
 * at N = 65536 13.8 / 202 / 785 ms, at N = 262144 54.6 / 793 / 3136 ms, at N = 1048576 218 / 3040 / 11581 ms -- 5.0 .. 6.1
 * TB/s of that byte count beside the ~6.3 TB/s of HBM, and 0.9 / 6 / 7 evaluations of bound + gradient: a one-off before an
 * optimisation, not part of its loop.  Against a random subset of the same M at the same theta: (max L_ii / min L_ii)^2 of
 * the factor of Kuu + 1e-8 I falls by a factor of 50 .. 400, and at M = 4096 and the default jitter d bound / d U agrees
 * with a central difference to 7e-5 .. 4e-4 where the random subset is off by 0.09 .. 0.9 of its norm (above).  The bound
 * itself is LOWER for the greedy points in every cell of that workload (N = 65536, M = 512: -28836 against -13996; trace
 * term 61.6 against 29.3): the rows of largest residual variance of uniform inputs in eight dimensions lie near the corners.
 * On the test suite's families in one to three dimensions the trace term falls by a factor of 2 .. 17.  DESIGN.md section 4,
 * "Sparse: choosing the inducing points". */
int gogp_sparse_select_inducing(gogp_handle *h, const double *x /* log theta */, int64_t len /* P */,
                                const double *X /* N x ndim */, int64_t N, int64_t M, double tol,
                                int64_t *idx /* M */, double *pivots /* M */, double *U /* M x ndim */,
                                int64_t *m_out, double *trace);
int gogp_sparse_select_inducing_resident(gogp_handle *h, const double *x, int64_t len, int64_t M, double tol,
                                         int64_t *idx, double *pivots, double *U, int64_t *m_out, double *trace);

/* Iterative exact GP: matrix-free preconditioned conjugate gradients (cg.hip; Gardner et al. 2018, Wang et al. 2019).
 * The exact posterior at a size where no N x N matrix fits: K^ = k(X, X) + sigma^2 I + diag(v) is never stored, every
 * product recomputes it from X on the matrix cores (v_mfma_f64_16x16x4_f64: a lane evaluates one k(x_i, x_j) and feeds it
 * in as its A operand), for up to GOGP_CG_MAX_RHS right-hand sides at once.  The data are a set of their own, like the
 * sparse calls': gogp_cg_set_data copies X (N x ndim), y (N) and v (N per-observation noise variances, finite and >= 0;
 * NULL: none) to the device, where they stay; N == 0 with NULLs clears them.  Nothing else of the handle changes, and no
 * dense, sparse, batch, multi-output, basis or Laplace call sees the CG state.
 * gogp_cg_solve: theta = exp(x); the preconditioner P = L L^T + D at that theta, D = diag(sigma^2 + v_i) and L the
 * N x rank_used pivoted-Cholesky factor of k(X, X) that gogp_sparse_select_inducing describes (cap `rank`, tolerance
 * piv_tol; piv_tol < 0: 10^"sparse_jitter_log10"; rank == 0: plain Jacobi, P = D), applied by Woodbury's identity:
 * Ls = D^-1/2 L, C = I + Ls^T Ls, P^-1 R = D^-1/2 (R' - Ls C^-1 Ls^T R'), R' = D^-1/2 R; then K^ alpha = y.  alpha, theta and
 * the preconditioner stay for gogp_cg_get_alpha, gogp_cg_solve_columns and gogp_cg_produce; info->yt_alpha = y^T alpha is
 * the data-fit term (the log-determinant: gogp_cg_lml_gradient, below).  Every column c of a block runs
 *     x = 0, r = b, z = P^-1 r, p = z, rho = r^T z
 *     q = K^ p; a = rho / p^T q; x += a p; r -= a q; |r| <= tol |b|: the column FREEZES (its count is recorded, a = beta = 0
 *     from then on); z = P^-1 r; rho' = r^T z; beta = rho' / rho; p = z + beta p; rho = rho'
 * with the columns of a block advancing together.  The freeze decision is taken on the device in the iteration where it
 * happens; the host reads a status word every "cg_check" iterations (option, default 8) to stop launching, so no bit and no
 * count depends on it.  b = 0 gives zeros after 0 iterations.  After the block stops ONE more product gives the true
 * |b - K^ x| / |b| (rel_residual) beside the recurrence's value.  A column that did not freeze within max_iter: the call
 * returns GOGP_ENOCONV, every output is written, converged = 0 for it.  p^T q not positive and finite: GOGP_ENOTPD, and
 * gogp_last_error names the column.  Every sum has a fixed order (slab partials, two-stage dot products, no atomics, no
 * spin-waits): two identical calls return identical bits, and a column's solution has the same bits alone as in a block.
 * gogp_cg_solve_columns: K^ s_t = b_t for T >= 0 right-hand sides (rows of N), in blocks of GOGP_CG_MAX_RHS, at the theta
 * and preconditioner of the last gogp_cg_solve.  gogp_cg_produce: mu_j = sum_i k(z_j, x_i) alpha_i (one rectangular
 * product) and, unless sigma == NULL, sigma_j = sqrt(k(z_j, z_j) - k*_j^T K^^-1 k*_j) -- latent and unclamped as gogp_produce
 * defines it -- from one solve per 64 test points; sigma == NULL runs no solve.  gogp_cg_last_info: the counters of the
 * last of these three calls (blocks: lock-step blocks; products: matrix-free products LAUNCHED -- the one figure that
 * depends on "cg_check", because the launches run on until the host's next look at the status word: between iterations
 * + 1 and iterations + cg_check per block).
 * GOGP_ESTATE: no CG data, or columns / produce / get_alpha before a solve.  GOGP_EARG: NULLs, len != P, a non-finite
 * value in X, y, x, B or Z, a negative or non-finite v, rank outside 0 .. GOGP_CG_MAX_RANK, tol <= 0 or non-finite,
 * max_iter < 1, a size mismatch (n, T < 0, m < 0), sigma^2 + min v_i not positive (D is inverted), and the kinds of
 * handle the sparse calls refuse (precision = 32, sharded, event discounts).  GOGP_ENOMEM: the factor (8 N_pad rank bytes, N_pad = N rounded up to 256) could not be
 * allocated; gogp_last_error carries the size.
 * Device memory: X, y, v, D and alpha (N (ndim + 5) doubles), the factor, C^-1 (rank^2), and per block of T columns six
 * vectors each (x, r, p, z, q, b: 48 N T bytes; gogp_cg_lml_gradient keeps a seventh, w = P^-1 b: 56 N T bytes) plus the
 * product's slab partials (8 N T kmm slabs; one slab from N = 131072 on).  C is factored and inverted on the host (rank^3 flops, once per solve); everything per iteration runs
 * on the device.
 * Measured on one MI355X (tools/cg_probe.py, profiles/cg.txt; D = 8, medians of three): one CG iteration at rank 0 for
 * T = 1 / 16 / 64 columns: Normal 22.8 / 23.3 / 31.8 ms at N = 65536, 352 / 369 / 524 ms at N = 262144 and 5.4 / - / 8.1 s at
 * N = 1048576 (one measurement), Matern-5/2 26.6 / 27.0 / 35.3 and 409 / 431 / 576 ms: 1.6 - 2.05e11 kernel evaluations per
 * second, and 64 right-hand sides cost 1.33 - 1.52 of one.  gogp_cg_solve at N = 16384, tol = 1e-8, rank 0 / 64 / 256 / 1024:
 * Normal 437 / 140 / 38 / 7 iterations in 641 / 228 / 74 / 270 ms, Matern-5/2 778 / 356 / 166 / 62 in 1329 / 648 / 328 / 362 ms,
 * beside 30 ms for the dense gogp_absorb, which is the call at that size; the two alpha differ by 6e-9 - 1e-8 of their
 * norm.  gogp_cg_produce at rank 256: the means of 1024 points 2 ms, with sigma 1.2 s (Normal) and 4.8 s (Matern-5/2).
 * gogp_cg_lml_gradient (after gogp_cg_solve; its theta, preconditioner and alpha): the log marginal likelihood and
 * d LML / d log theta by stochastic Lanczos quadrature and probe vectors (Gardner et al. 2018).  Nothing random happens
 * in the library: row s of Xi holds standard normals [xi2 (N) | xi1 (rank_used)], ldxi >= N + rank_used, and probe s is
 * z_s = D^1/2 (Ls xi1 + xi2) ~ N(0, P).  One lock-step solve K^ u_s = z_s per probe (blocks of GOGP_CG_MAX_RHS, the freeze
 * rule above); w_s = P^-1 z_s, the block's first preconditioned residual, is kept, rho0_s = z_s^T w_s, and the device
 * records a and beta of every iteration and column (2 max_iter GOGP_CG_MAX_RHS doubles).  From a column's own coefficients
 * the host recovers the Lanczos tridiagonal of P^-1/2 K^ P^-1/2 -- T_kk = 1 / a_k + beta_{k-1} / a_{k-1}, T_{k,k+1} =
 * sqrt(beta_k) / a_k, k up to the column's iteration count -- and e_1^T log(T_s) e_1 by an implicit QL sweep that carries
 * the first components of the eigenvectors only (O(m^2) per probe; nothing per iteration moves to the host):
 *     quad_s = rho0_s e_1^T log(T_s) e_1,   log|K^| = log|P| + (1/t) sum_s quad_s,   log|P| = sum_i log D_i + log|C|
 *     LML = -1/2 y^T alpha - 1/2 log|K^| - N/2 log 2 pi
 *     d LML / d log theta_p = 1/2 sum_ij W_ij dK^_ij / d log theta_p,   W = alpha alpha^T - (1/t) sum_s u_s w_s^T
 * (E[u w^T] = K^^-1 P P^-1 = K^^-1; W has rank t + 1 and is never stored).  The gradient is one matrix-free pair reduction
 * (cg.hip: cg_grad_kernel): a wave forms each 16 x 16 tile of weights from the rows (alpha, alpha) and (-u_s / t, w_s) on
 * v_mfma_f64_16x16x4_f64 and its lanes evaluate theta_p dk(x_i, x_j) / d theta_p for the four pairs in their C fragment;
 * the noise parameter takes tr W.  grad == NULL skips the reduction; quad (t, may be NULL) receives quad_s;
 * logdet_stderr is the sample standard deviation of the quad_s over sqrt(t) (0 for t = 1); lanczos_max the largest
 * iteration count of a probe; products and blocks count this call's own (gogp_cg_last_info keeps the figures of the
 * call before).  With orthogonal probes (t = N + rank_used, Xi = sqrt(t) Q) the estimator is exact.  Cost: ceil(t / 64)
 * lock-step blocks -- each iteration one product, as in gogp_cg_solve_columns -- and 1 + ceil(t / 64) passes of the pair
 * reduction (per ARD pass of 8 dimensions) over all N^2 pairs.  Every sum has a fixed order; the order of the passes
 * depends on t alone: identical calls return identical bits, and a probe's quad_s has the same bits alone as in a block.
 * The handle is left as found (alpha, preconditioner, gogp_cg_last_info).  GOGP_ESTATE before a solve; GOGP_EARG: NULL Xi
 * or info, t < 1, ldxi < N + rank_used, a non-finite value in Xi, len != P (with grad), N >= 2^21 with grad (the pair
 * reduction counts its 64 x 64 tiles in 32 bits), a bad tol or max_iter;
 * GOGP_ENOCONV with every output written from the columns as they stand; GOGP_ENOTPD naming the column.
 * Measured on one MI355X (tools/cg_lml_probe.py, profiles/cg_lml.txt; D = 8, medians of three): one pass of the pair
 * reduction over N^2 pairs for S = 1 / 16 / 64 rows of weights: Normal 24.5 / 26.4 / 44.6 ms at N = 65536 and 388 / 434 / 719 ms
 * at N = 262144, Matern-5/2 28.4 / 30.4 / 49.9 and 453 / 493 / 834 ms: 1.4 - 1.8e11 pairs per second at S = 1, and 64 rows cost
 * 1.76 - 1.85 of one.  The whole evaluation (gogp_cg_solve at rank 256 + this call with 16 probes, tol = 1e-8) at N = 16384:
 * 149 ms (Normal) and 668 ms (Matern-5/2) beside 71 ms for the dense gogp_observe + gogp_gradient, which is the call at
 * that size; the estimate lies 1.55 and 0.35 standard errors (5.4 and 34.5) from the dense LML, the gradient within 6.9e-4
 * and 1.4e-2 of the dense one's norm.  At N = 65536: 3.46 s and 19.3 s.
 * Out of scope: the symmetry of K in the product and in the pair reduction, event discounts, several GPUs.  DESIGN.md
 * section 4, "Iterative (CG)" and "Iterative (CG): LML and gradient". */
#define GOGP_CG_MAX_RANK 1024
#define GOGP_CG_MAX_RHS 64 /* systems per lock-step block */
typedef struct {
  int32_t iterations, converged;
  double rel_residual, rel_residual_recurrence;
} gogp_cg_col;
typedef struct {
  int32_t rank_used, products, blocks;
  double yt_alpha;
} gogp_cg_info;
int gogp_cg_set_data(gogp_handle *h, const double *X, const double *y, const double *v /* may be NULL */, int64_t N);
int gogp_cg_solve(gogp_handle *h, const double *x /* log theta */, int64_t len, int32_t rank, double piv_tol, double tol,
                  int32_t max_iter, gogp_cg_info *info, gogp_cg_col *col /* 1, may be NULL */);
int gogp_cg_get_alpha(gogp_handle *h, double *alpha, int64_t n);
int gogp_cg_solve_columns(gogp_handle *h, const double *B /* T rows of N */, int64_t T, double tol, int32_t max_iter,
                          double *S /* T rows of N */, gogp_cg_col *cols /* T, may be NULL */);
int gogp_cg_produce(gogp_handle *h, const double *Z, int64_t m, double *mu, double *sigma /* may be NULL */, double tol,
                    int32_t max_iter, gogp_cg_col *cols /* m, may be NULL */);
int gogp_cg_last_info(gogp_handle *h, gogp_cg_info *info);
typedef struct {
  double lml, yt_alpha, logdet, logdet_precond, logdet_stderr;
  int32_t probes, blocks, products, lanczos_max;
} gogp_cg_lml_info;
int gogp_cg_lml_gradient(gogp_handle *h, const double *Xi /* t rows of ldxi */, int64_t t, int64_t ldxi, double tol,
                         int32_t max_iter, double *grad /* len, may be NULL */, int64_t len,
                         double *quad /* t, may be NULL: rho0_s e1^T log(T_s) e1 */, gogp_cg_lml_info *info,
                         gogp_cg_col *cols /* t, may be NULL */);

/* Vecchia's approximation, also known as the nearest-neighbour GP (vecchia.hip; Vecchia 1988, Datta et al. 2016, Katzfuss &
 * Guinness 2021):
 *     log p(y) ~ sum_i log p(y_i | y_c(i)),    c(i) a set of at most m earlier rows,
 * a product of N exact Gaussian conditionals on blocks of at most m + 1 <= 64 rows.  It is a valid joint density, not a
 * bound; it equals the exact LML when c(i) holds every earlier row; its gradient is the exact derivative of its value.
 * Cost: O(N m^3) flops and N (m + 1)^2 / 2 similarity evaluations, one wave per target.  Per target i with block b =
 * [c(i) in the table's order, i]:  K_b = k(X_b, X_b) + sigma^2 I + diag(v_b), L = chol(K_b), z = L^-1 y_b, and the terms
 *     mu_i = y_i - L_qq z_q,   s_i = L_qq,   log p_i = -1/2 log 2 pi - log L_qq - 1/2 z_q^2         (q = |c(i)|):
 * the one-step-ahead forecast of y_i from its conditioning rows (noisy: s_i includes the noise) and its log density.
 * The table: `rows` rows of m int32, 0 <= m <= GOGP_VECCHIA_MAX_M; a row holds distinct indices, then -1 padding (trailing
 * only); causal: every index of row i is < i (row 0 is empty); otherwise every index is in [0, n).  The order within a
 * row is kept: it fixes the bits, not the value beyond rounding.  gogp_vecchia_check (host only) returns GOGP_EARG for a
 * table that breaks this; gogp_vecchia_set_data and gogp_vecchia_produce call it and name the first offending row in
 * gogp_last_error.  The data are a set of their own, like the iterative calls': gogp_vecchia_set_data copies X (N x
 * ndim), y (N), v (N per-observation noise variances, finite and >= 0; NULL: none) and the table to the device, where
 * they stay (N (ndim + 2) doubles, 4 N m bytes, the 3 N terms, at most 2048 partial rows); N == 0 with NULLs clears them.
 * Nothing else of the handle changes: a dense, sparse or iterative call made afterwards returns the bits it would have
 * returned without these calls.
 * gogp_vecchia_observe: the value at x = log theta into *lml and, unless NULL, the terms (N x 3: mu, s, log p).
 * gogp_vecchia_gradient: d value / d log theta at the last observe's theta, the noise parameter's component included
 * (d / dv and d / dX are out of scope); it runs the kernel again with the gradient's stages.
 * gogp_vecchia_produce: mu_j and, unless NULL, sigma_j of the test points Z (mz x ndim), each conditioned on the rows of the
 * data its row of nbrz (mz x m, same m) names: the target row is z_j with k(z_j, z_j) on its diagonal, no noise and no y --
 * the latent sigma, unclamped, as gogp_produce defines it.  It uses the last observe's theta.
 * Identical calls give identical bits (fixed-order sums, no atomics), and a target's terms have the same bits whatever
 * else is in the call.  GOGP_EARG: NULL pointers, non-finite values, a bad table, len != P, a precision = 32 handle, a
 * sharded handle, a handle with event discounts.  GOGP_ESTATE: observe before set_data; gradient or produce before
 * observe.  GOGP_ENOTPD: a block has a pivot that is not positive and finite; gogp_notpd_index is the LOWEST such target
 * (row of the data; test point for produce), that target's outputs are NaN, every other target's are written, *lml is NaN.
 * DESIGN.md section 4, "Vecchia". */
#define GOGP_VECCHIA_MAX_M 63
int gogp_vecchia_check(const int32_t *nbr, int64_t rows, int32_t m, int64_t n, int causal);
int gogp_vecchia_set_data(gogp_handle *h, const double *X, const double *y, const double *v /* may be NULL */, int64_t N,
                          const int32_t *nbr /* N x m, row-major */, int32_t m);
int gogp_vecchia_observe(gogp_handle *h, const double *x /* log theta */, int64_t len, double *lml,
                         double *terms /* N x 3: mu, s, logp; may be NULL */);
int gogp_vecchia_gradient(gogp_handle *h, double *grad, int64_t len);
int gogp_vecchia_produce(gogp_handle *h, const double *Z, int64_t mz, const int32_t *nbrz /* mz x m */, double *mu,
                         double *sigma /* may be NULL */);

/* Neighbour tables built on the device (vecchia_knn.hip): the exact brute-force search of gogp_amd/vecchia.py, nearest
 * and nearest_to, and the same table integer for integer.  xs = x / lengths per dimension (lengths: ndim values, > 0 and
 * finite; NULL: unscaled); d2(a, b) = sum_d (a_d - b_d)^2 from the differences, in index order of d, every product
 * rounded before it is added; row i of the causal table holds the m smallest keys (d2(xs_i, xs_j), j) over j < i, a row
 * of the query form the m smallest over all j < N; keys are ordered by value, then by index; nearest first, then -1; a
 * distance that is not finite is never taken.  0 <= m <= GOGP_VECCHIA_MAX_M; m == 0 writes nothing.  The key is a strict
 * total order: identical calls give identical tables, whatever the launch.  Cost: N^2 / 2 (causal) or mz N pairs of
 * 3 ndim fp64 operations; the search of a few targets is cut over the candidates; the scratch beside the scaled copies
 * stays under 36 MiB.
 * gogp_vecchia_neighbours: one-shot, nothing of the handle changes; Z == NULL (mz == 0): the causal table of X (N x m),
 * else mz rows over all of X.
 * gogp_vecchia_set_data_nearest: gogp_vecchia_set_data, with the table built on the device from the uploaded X; it stays
 * there beside the scaled copy of X (N ndim doubles more).
 * gogp_vecchia_reneighbour: rebuilds the resident table from the resident X under new lengths (same m; also a table that
 * gogp_vecchia_set_data brought, which it replaces); the last observe is dropped, so gogp_vecchia_gradient and the produce
 * calls want a new one.
 * gogp_vecchia_get_neighbours: the resident table (N x m).
 * gogp_vecchia_produce_nearest: finds each test point's m nearest resident rows on the device, then gogp_vecchia_produce's
 * launch on that table; lengths NULL: those the resident table was built with (GOGP_ESTATE if a caller brought it); nbrz,
 * unless NULL, receives the table (mz x m).
 * GOGP_EARG (gogp_last_error names the argument): m outside 0 .. 63, a length that is not positive and finite, N >= 2^31,
 * NULL pointers, and the handles the other Vecchia calls refuse.  GOGP_ESTATE: reneighbour, get_neighbours and
 * produce_nearest without resident data; produce_nearest before an observe.
 * DESIGN.md section 4, "Vecchia: neighbour tables on the device". */
int gogp_vecchia_neighbours(gogp_handle *h, const double *X, int64_t N, const double *Z /* may be NULL */, int64_t mz,
                            const double *lengths /* ndim; may be NULL */, int32_t m, int32_t *nbr);
int gogp_vecchia_set_data_nearest(gogp_handle *h, const double *X, const double *y, const double *v /* may be NULL */,
                                  int64_t N, const double *lengths /* may be NULL */, int32_t m);
int gogp_vecchia_reneighbour(gogp_handle *h, const double *lengths /* may be NULL */);
int gogp_vecchia_get_neighbours(gogp_handle *h, int32_t *nbr /* N x m */);
int gogp_vecchia_produce_nearest(gogp_handle *h, const double *Z, int64_t mz, const double *lengths /* may be NULL */,
                                 double *mu, double *sigma /* may be NULL */, int32_t *nbrz /* mz x m, may be NULL */);

/* k independent Observe + Gradient evaluations at once: handle hs[i] (each created and given
 * its data separately; they may hold the same data) evaluates x[i*len .. (i+1)*len) from its own
 * host thread, so the dependent launch chains of the k evaluations overlap on the GPU.
 * Counterpart: the reference's optimiser evaluating candidates concurrently
 * (optimize.Settings.Concurrent = NTASKS, tutorial/tutorial.go:30,141).  status (may be NULL)
 * receives the k return codes; the result is the first non-zero one. */
int gogp_observe_gradient_batch(gogp_handle **hs, int k, const double *x, int64_t len,
                                double *lmls /* k */, double *grads /* k*len */,
                                int *status /* k */);

/* k candidate parameter vectors on ONE handle's data, evaluated in one launch sequence: x is
 * k x len row-major (len = P: log theta only), lmls[c] and grads[c*len ..] receive what
 * gogp_observe + gogp_gradient would return for candidate c.  Every kernel of the sweep is launched
 * once for all candidates (candidate index on the grid's z axis), so the dependent chain of small
 * launches that bounds one evaluation below N ~ 8192 is paid once per batch.  Same counterpart as
 * above (concurrently evaluated candidates of the reference's optimiser: a line search's trial
 * points, multi-start restarts).  The handle's own state -- data, the factorisation of an earlier
 * Absorb / Observe, Produce -- is not touched; the candidates live in k arena slots of
 * ~3 x 8 N^2 bytes each that stay allocated until the handle is destroyed.  status[c] (may be
 * NULL): GOGP_OK, GOGP_ENOTPD (lmls[c] = NaN, gradient zeros), GOGP_ECOND (values still
 * returned) or GOGP_EARG (parameters not finite); the result is the first non-zero one.
 * k <= GOGP_MAX_CANDIDATES.  fp64 handle on one GPU: as described.  precision = 32: the candidates pass through
 * ONE arena slot one after the other (same results and the same untouched handle; the float kernels carry no
 * candidate index).  Sharded handle (collective: every rank with the same candidates): evaluated one after the
 * other in the shards' own tiles, and the handle afterwards holds the factorisation of the last candidate that was
 * factorised (one refused with GOGP_EARG is skipped; after a last candidate that is not positive definite the handle
 * holds no factorisation).  The per-candidate contract is the same on every kind of handle: all k slots of lmls /
 * grads / status are written, GOGP_EARG and GOGP_ENOTPD mark their own candidate only; only a transport or HIP
 * failure ends the call early (status of the candidates not reached: GOGP_ESTATE). */
#define GOGP_MAX_CANDIDATES 16
int gogp_observe_gradient_candidates(gogp_handle *h, int k, const double *x, int64_t len,
                                     double *lmls /* k */, double *grads /* k*len */,
                                     int *status /* k */);

/* Diagnostics of the candidates' launch graph (option "graph"): nodes of the graph in use (0: none yet, or the
 * stream path), whether the runtime refused an explicitly built graph (then the stream path is used for good).
 * No reference counterpart. */
int gogp_graph_info(const gogp_handle *h, int64_t *nodes, int *refused);

/* Batches of independent small GPs: many data sets, each with its own n and its own theta, evaluated in ONE launch
 * (one workgroup per (member, theta) pair; one host-to-device copy of the pairs' parameters, one device-to-host copy
 * of the results).  Counterpart: the reference's forecast harness, which fits the hyperparameters separately on every
 * prefix X[:end] of the data (tutorial/tutorial.go:88-197), and any set of short series fitted with one kernel.
 * The batch is fp64 whatever the options "precision" and "gradient_precision" are; "cond_limit_log10" and the
 * handle's event discounts (gogp_set_events) apply.  Sharded handle: GOGP_EARG.  Hyperparameters-only form (the full
 * form: gogp_batch_observe_full_gradient / gogp_batch_produce_full below). */
#define GOGP_BATCH_MAX_N 128
/* Members are row ranges [offset[b], offset[b]+n[b]) of one uploaded X (rows x ndim) / y; ranges may
   overlap (forecast windows are prefixes of the same data).  n[b] <= GOGP_BATCH_MAX_N (else GOGP_EARG).
   Replaces the previous batch data; the handle's own data, factorisation, candidates arena are untouched. */
int gogp_batch_set_data(gogp_handle *h, const double *X, const double *y, int64_t rows,
                        int32_t nmembers, const int64_t *offset, const int64_t *n);
/* k evaluations: member members[i] at log theta x[i*len .. +len) (len = P; hyperparameters-only form).
   lmls[i], grads[i*len ..], status[i] as gogp_observe + gogp_gradient on a handle holding that member's
   data would give, with the per-candidate contract of gogp_observe_gradient_candidates (ENOTPD: NaN and
   zeros; ECOND: values returned; EARG: non-finite parameters).  Members may repeat.  ONE launch.
   A member with n = 0: LML 0 and a zero gradient (gp/gp.go:101-104, 427-430).  A pair's results do not depend on
   the other pairs of the call (bit for bit).  Returns the first non-zero status; status may be NULL. */
int gogp_batch_observe_gradient(gogp_handle *h, int32_t k, const int32_t *members, const double *x,
                                int64_t len, double *lmls, double *grads, int *status);
/* Same k (member, log theta) pairs; test points of pair i are rows zoff[i] .. zoff[i+1] of Z (m x ndim):
   LML at x and mu / sigma as gogp_observe + gogp_produce would give.  ONE launch.
   zoff (k + 1 entries) is non-negative and non-decreasing; mu[j], sigma[j] belong to row j of Z.  sigma is unclamped
   as in gogp_produce; n = 0: mu = 0, sigma = sqrt(prior) (gp/gp.go:343-347).  ENOTPD / EARG: lml, mu, sigma NaN. */
int gogp_batch_produce(gogp_handle *h, int32_t k, const int32_t *members, const double *x, int64_t len,
                       const int64_t *zoff /* k+1 */, const double *Z, double *lmls, double *mu,
                       double *sigma, int *status);

/* The full Observe form of the batch (gp/gp.go:366-369, 386-400): every pair carries its own observations in its
 * parameter vector, x_i = [log theta | X_i (n_i x ndim) | y_i (n_i)] = x[xoff[i] .. xoff[i+1]), n_i = (len_i - P) /
 * (ndim + 1) <= GOGP_BATCH_MAX_N; the vectors differ in length.  Counterpart: the forecast windows of the case studies
 * that infer their inputs or outputs (OPTINP: tutorial/anynoise/main.go:47, tutorial/warpedtime/main.go:59;
 * tutorial/tutorial.go:100-110), one gogp_observe_full + gogp_gradient each in the reference's order of work.  No batch
 * data is needed or touched, nor the handle's own data, factorisation and candidates arena.  fp64 whatever "precision"
 * and "gradient_precision" are.  Sharded handle: GOGP_EARG.  Still one copy in, ONE launch, one copy out. */
/* lmls[i] and grads[xoff[i] .. xoff[i+1]) (laid out as x: hyperparameters, dLML/dX_i of gp/gp.go:118-129, dLML/dy_i =
   -alpha of :488-493) as gogp_observe_full + gogp_gradient on a handle of its own would return them; the hyperparameter
   part is bit for bit that of gogp_batch_observe_gradient on the same data.  Per pair, with the others still evaluated:
   len_i < P, a remainder (the reference: panic("len(x)"), gp/gp.go:398-400), n_i > GOGP_BATCH_MAX_N, non-finite
   parameters or observations: GOGP_EARG (LML NaN, gradient zeros); GOGP_ENOTPD: LML NaN, gradient zeros; GOGP_ECOND:
   values returned; n_i = 0: LML 0, zeros.  A pair's results do not depend on the other pairs of the call (bit for bit).
   xoff (k + 1 entries) is non-negative and non-decreasing.  Returns the first non-zero status; status may be NULL. */
int gogp_batch_observe_full_gradient(gogp_handle *h, int32_t k, const double *x, const int64_t *xoff /* k+1 */,
                                     double *lmls /* k */, double *grads /* xoff[k], laid out as x */, int *status);
/* The same pairs with test points as gogp_batch_produce: LML at x_i and mu / sigma as gogp_observe_full + gogp_produce
   would give (gp/gp.go:269-278, 322-357); n_i = 0: mu = 0, sigma = sqrt(prior).  ENOTPD / EARG: lml, mu, sigma NaN. */
int gogp_batch_produce_full(gogp_handle *h, int32_t k, const double *x, const int64_t *xoff /* k+1 */,
                            const int64_t *zoff /* k+1 */, const double *Z, double *lmls, double *mu, double *sigma,
                            int *status);

/* gp.GP.Produce (gp/gp.go:258-360): predictive mean and standard deviation of
 * the latent function at m points Z (row-major m x ndim).  sigma_j =
 * sqrt(k(z_j,z_j) - (Kstar^T K^-1 Kstar)_jj), unclamped like the reference
 * (gp/gp.go:356: a rounding-negative argument yields NaN).  With no
 * observations: mu = 0, sigma = sqrt(prior) (gp/gp.go:343-347). */
int gogp_produce(gogp_handle *h, const double *Z, int64_t m, double *mu,
                 double *sigma);
/* gogp_produce and the derivatives of the forecast with respect to the test points (no reference counterpart):
 *   dmu[j][d]    = d mu_j / d z_jd    = sum_i alpha_i dk(z_j, x_i)/dz_jd
 *   dsigma[j][d] = d sigma_j / d z_jd = -2 sum_i (K^-1 Kstar)_ij dk(z_j, x_i)/dz_jd / (2 sigma_j)
 * both row-major m x ndim.  mu and sigma are what gogp_produce returns for the same Z; sigma is not clamped, so a row
 * of dsigma with sigma_j^2 <= 0 is what the division yields (NaN / inf).  With event discounts the pair's derivative
 * carries the pair's discount (piecewise constant in z; undefined for a z exactly on a boundary).  Same preconditions
 * and error codes as gogp_produce: m == 0 is OK, GOGP_ESTATE before anything is absorbed; with no observations
 * mu = 0, sigma = sqrt(prior) and both derivative arrays are zero.  GOGP_EARG for a precision = 32 handle and for a
 * sharded handle (the restriction of gogp_append).  Works in every state in which gogp_produce works and leaves the
 * handle's state as it found it.  Two calls with the same arguments return bit-identical arrays. */
int gogp_produce_gradient(gogp_handle *h, const double *Z, int64_t m, double *mu, double *sigma,
                          double *dmu /* m x ndim */, double *dsigma /* m x ndim */);

#define GOGP_COV_MAX_M 4096
/* gogp_produce's mu and the joint covariance of the latent function at the m test points (no reference counterpart):
 *   cov[i][j] = k(z_i, z_j) - sum_r V_ri V_rj,  V = L^-1 Kstar;   row-major m x m, both triangles written, cov[i][j] and
 *   cov[j][i] the same bits; no noise term (as sigma of gogp_produce: sqrt(cov[j][j]) is that sigma to rounding);
 *   with event discounts k(z_i, z_j) and Kstar carry the pairs' discounts.
 * m == 0 is OK.  GOGP_EARG for NULL pointers, m > GOGP_COV_MAX_M, a precision = 32 handle and a sharded handle;
 * GOGP_ESTATE before anything is absorbed; with no observations mu = 0 and cov = k(Z, Z).  Works in every state in which
 * gogp_produce works and leaves the handle's state as it found it.  Two calls with the same arguments return
 * bit-identical arrays.  The call takes Produce's tile route for every m (as gogp_produce_gradient: few points cost what
 * that call's forward half costs, not what gogp_produce's one-pass kernel costs -- measured at N = 16384, D = 8, m = 1:
 * 2.04 ms against 0.43 ms for gogp_produce and 3.09 ms for gogp_produce_gradient; m = 64: 2.05 against 1.52 and 3.75;
 * m = 1024: 6.0 against 5.2 and 11.1; DESIGN.md section 4, "ProduceCovariance / Sample"). */
int gogp_produce_covariance(gogp_handle *h, const double *Z, int64_t m, double *mu, double *cov /* m x m */);

/* ns joint draws at the m test points from caller-supplied standard normals xi (ns x m, row-major):
 *   samples[s][:] = mu + C xi[s][:],  C = lower Cholesky factor of cov + diag_add * I,  samples ns x m row-major.
 * diag_add >= 0, finite: 0 draws the latent function; the noise variance draws noisy observations; a small value
 * is the caller's jitter where cov is numerically singular (test points on or between dense observations).
 * Preconditions and error codes of gogp_produce_covariance; also GOGP_EARG for a negative or non-finite diag_add and for
 * a non-finite value in xi.  ns == 0 is OK (mu is still filled when m > 0).  GOGP_ENOTPD when cov + diag_add * I has a
 * pivot that is not positive: nothing is written to samples, gogp_notpd_index is the failing pivot's index among the
 * test points, gogp_last_error names the predictive covariance, and the fitted process is untouched. */
int gogp_produce_samples(gogp_handle *h, const double *Z, int64_t m, const double *xi, int64_t ns, double diag_add,
                         double *mu /* m */, double *samples /* ns x m */);

/* ---- cached state (gp.GP.L, gp.GP.Alpha: gp/gp.go:35-36,255-257) ---------- */
int64_t gogp_n(const gogp_handle *h);
int gogp_get_alpha(gogp_handle *h, double *alpha /* n */);
/* Lower Cholesky factor, row-major n x n, upper triangle zero-filled.
 * (gonum stores U = L^T; the Go shim transposes when filling gp.GP.L.) */
int gogp_get_factor(gogp_handle *h, double *L /* n*n */);
/* Selected rows of the factor: out is nrows x n row-major, row r = L[rows[r], 0..n-1]
 * (zeros right of the diagonal); and its diagonal (n doubles).  gp.GP.L at sizes where
 * the whole n x n matrix is not wanted on the host (2*sum(log diag) is the LogDet of
 * gp/gp.go:250). */
int gogp_get_factor_rows(gogp_handle *h, const int64_t *rows, int64_t nrows,
                         double *out /* nrows*n */);
int gogp_get_factor_diag(gogp_handle *h, double *diag /* n */);
/* Restore stored results so that gogp_produce works without re-absorbing
 * ("Produce on stored results", gp/gp.go:255-257). */
int gogp_set_factor(gogp_handle *h, const double *theta_simil,
                    const double *theta_noise, const double *L /* n*n */,
                    const double *alpha /* n */);

/* Append m observations to the factored process at the parameters of the last
 * Absorb / Observe / set_factor: afterwards the handle is in the state gogp_absorb on the
 * n + m observations would leave (factor, alpha, LML, Produce; no gradient: gogp_gradient
 * returns GOGP_ESTATE as after Absorb), in O((n + m)^2 m) work and two passes over the factor.
 * No reference counterpart (the reference refactorises: tutorial/tutorial.go:118-142).
 * m == 0: nothing happens.  An empty process (n == 0, data set, parameters given): Absorb of the m rows.
 * GOGP_EARG: NULL or non-finite inputs, a precision = 32 handle, a sharded handle.  GOGP_ESTATE: not factored.
 * GOGP_ENOTPD: the handle holds exactly the state it had before the call (gogp_n, factor, Produce);
 * gogp_notpd_index is the global index of the failing pivot.  GOGP_ECOND: stored and reported, as Absorb. */
int gogp_append(gogp_handle *h, const double *X2 /* m x ndim */, const double *y2 /* m */, int64_t m);

/* Remove the observations idx[0] < idx[1] < ... < idx[m-1] from the factored process: afterwards the handle is in
 * the state gogp_absorb on the kept rows, in their original order, would leave -- gogp_n = n - m, the device-side X / y
 * compacted, factor, alpha, LML and the block inverses of Produce in place (gogp_produce, gogp_produce_gradient,
 * gogp_append, gogp_get_factor* and gogp_get_alpha work; no gradient: gogp_gradient returns GOGP_ESTATE as after
 * Absorb, and a stored K^-1 is invalidated) -- in O(n^2 m) work: a gather of the kept rows and columns of the factor
 * and a rank-m update of it by orthogonal (Householder) transformations, ceil(m / 32) passes over the trailing factor.
 * The counterpart of gogp_append; no reference counterpart (the reference refactorises: tutorial/tutorial.go:118-142).
 * Neither the similarity kernel nor the parameters are evaluated: theta stays that of the last Absorb / Observe /
 * set_factor, and the call works after each of them and after gogp_append alike, with or without event discounts.
 * The kept matrix is positive definite by construction (a sum, never a downdate): there is no GOGP_ENOTPD.  Rows of
 * the factor above idx[0] keep their bits.  Batch data, the candidates arena and event discounts are untouched.  Two
 * identical call sequences return bit-identical factors.
 * m == 0: nothing happens.  m == n: the empty process (gogp_n = 0, LML 0, Produce: mu = 0, sigma = sqrt(prior); a
 * following gogp_append absorbs).
 * GOGP_EARG: idx == NULL with m > 0, an index outside [0, n), indices not strictly increasing, a precision = 32
 * handle, a sharded handle (the restrictions of gogp_append); the handle is exactly as it was.  GOGP_ESTATE: not
 * factored.  GOGP_ECOND: stored and reported, as Absorb ((max L_ii / min L_ii)^2 against cond_limit_log10).
 * Measured on one MI355X (profiles/remove.txt, D = 8): at N = 16384 one row from the front 20 ms, one from the middle
 * 12 ms, the last 4.5 ms against 31 ms for gogp_set_data + gogp_absorb of the kept rows.  SLOWER than refactorising,
 * and there is no automatic fallback: the first 64 rows at N = 16384 (52 ms against 31; the first 16: 30 against 31),
 * and at N = 4096 every removal from the front (1 / 16 / 64 rows: 4.7 / 7.2 / 12.6 ms against 2.9).  The cost is one
 * dependent launch per 128 columns behind the first removed row, per pass of 32 removed rows. */
int gogp_remove(gogp_handle *h, const int64_t *idx /* m, strictly increasing */, int64_t m);

/* ---- per-observation noise variances ----------------------------------------------------------
 * K = k_theta(X, X) + sigma^2(theta) I + diag(v): every observation carries a known noise variance v_i, finite and
 * >= 0, on top of the handle's noise kind, which keeps its parameter slot and its derivative -- measurements with their
 * own error bars, means of n_i replicates (sigma^2 / n_i), series from instruments of different quality.  No reference
 * counterpart (gp.GP has one noise level on every observation).  A fixed diag(v) has no derivative in theta, and every
 * call behind the factorisation works from the factor, alpha and K^-1: with variances set, gogp_absorb / gogp_observe,
 * gogp_gradient, gogp_produce*, gogp_loo*, gogp_blockcv*, gogp_multi_*, gogp_basis_* and gogp_get_factor* are those of
 * the model above at no extra cost but one or two O(n) launches behind the Gram build.  Handles with variances and
 * n <= 128 take the general sweep instead of the one-launch form (option "tiny").  With none set no launch changes.
 *
 * gogp_noise_variances_check: host only; GOGP_OK when every v_i is finite and >= 0 (n == 0: OK), else GOGP_EARG.
 *
 * gogp_set_noise_variances: needs data (GOGP_ESTATE before gogp_set_data) and n == gogp_n(h) (GOGP_EARG); the values are
 * copied to the device.  v == NULL with n == 0 clears.  Stored results no longer match and are dropped, exactly as by
 * gogp_set_events: until the next gogp_absorb / gogp_observe the calls gogp_gradient, gogp_produce, gogp_loo ... return
 * GOGP_ESTATE.  Clearing, followed by an Observe, returns the bits of a handle that never had variances.
 *   Dropped by: whatever replaces the data -- gogp_set_data[_device], gogp_observe_full with observations in x -- and
 *               a change of option "precision" (the list that applies to gogp_multi_set_outputs).
 *   Carried by: gogp_append* (new rows: v2, or zeros) and gogp_remove (compacted with the rows).
 *   Untouched by: the sparse, batch, multi-output and basis setters and gogp_set_factor.  A restore that wants to
 *               append later calls gogp_set_data, then gogp_set_noise_variances, then gogp_set_factor.
 * GOGP_EARG, each said in gogp_last_error: a negative or non-finite variance; a precision = 32 handle; gradient_precision
 * = 32 (its closed-form scale component assumes K = c F + sigma^2 I; the option is refused in turn while variances are
 * set); a sharded handle.  While variances are set gogp_observe_gradient_candidates (the arena slots' sweeps do not add
 * them) and gogp_laplace_observe (its matrix-free products with K do not carry them) return GOGP_EARG.  The batches of
 * small GPs (gogp_batch_*) and the sparse calls (gogp_sparse_*) have data of their own: the variances do not apply to
 * them.
 *
 * gogp_get_noise_variances: what the device holds for the gogp_n observations; zeros when none are set.
 *
 * gogp_noise_variances_gradient: dv_i = dLML/dv_i = 1/2 (alpha_i^2 - [K^-1]_ii), one kernel over the diagonal of the
 * explicit K^-1.  Works wherever gogp_loo works, by the same preparation, also with no variances set (the derivative at
 * v = 0), and leaves the handle as gogp_loo leaves it: K^-1 formed, nothing a later call reads changed.  Two identical
 * calls return identical bits.  n == 0: nothing is written.  With it the variances can be learnt through any host-side
 * noise model v(phi): dLML/dphi = sum_i dv_i dv_i/dphi (gogp_amd/gp.py: HeteroscedasticModel).
 *
 * gogp_append_noisy: gogp_append with the new rows' variances v2 (m values, checked as above) on the diagonal of the new
 * block; gogp_append is this call with v2 == NULL, which means zeros.  With v2 given on a handle without variances the
 * vector is created with zeros for the old rows.  The vector grows with the data's buffers.  The empty process absorbs
 * the m rows with v2 set.  On GOGP_ENOTPD the handle, its variances included, is exactly as it was before the call.
 *
 * Measured on one MI355X (profiles/noise_variances.txt, D = 8, medians of alternating rounds): Observe + Gradient with
 * variances against without 0.678 / 3.185 / 71.40 ms against 0.684 / 3.163 / 71.25 ms at N = 1024 / 4096 / 16384, every
 * difference inside the spread of repeated identical runs (0.09 / 0.42 / 1.16 ms); N = 64 / 128, general sweep against one
 * launch: 0.37 / 0.36 ms against 0.19 / 0.21 ms; gogp_noise_variances_gradient with K^-1 in place 0.03 ms beside 0.08 -
 * 0.10 ms for gogp_loo; gogp_append_noisy of 1 / 64 rows at N = 16384 2.47 / 3.92 ms against 2.49 / 3.96 ms for gogp_append. */
int gogp_noise_variances_check(const double *v, int64_t n);
int gogp_set_noise_variances(gogp_handle *h, const double *v /* n; NULL with n == 0 clears */, int64_t n);
int gogp_get_noise_variances(gogp_handle *h, double *v /* gogp_n */);
int gogp_noise_variances_gradient(gogp_handle *h, double *dv /* gogp_n */);
int gogp_append_noisy(gogp_handle *h, const double *X2 /* m x ndim */, const double *y2 /* m */,
                      const double *v2 /* m, may be NULL */, int64_t m);

/* ---- one evaluation sharded over several GPUs: 2-D block-cyclic ---------------------
 * One process per GPU.  The ranks form a Pr x Pc process grid (rank = pr*Pc + pc; Pr must
 * divide Pc: 1x1, 1x2, 2x2, 2x4 for 1/2/4/8 GPUs, gogp_dist_grid).  The Gram matrix is cut into
 * 512x512 tiles; tile (I,J) lives on the GPU at grid position (I mod Pr, J mod Pc), and every
 * rank allocates ONLY its own tiles (of K, of the factor L and of Y = L^-T): memory per rank
 * is 1/(Pr*Pc) of the single-GPU footprint (gogp_dist_local_bytes).  X, y (a few MB) are
 * replicated, so every rank builds its own tiles of K with no communication.  Per block
 * column P of the blocked right-looking Cholesky: the owner of the diagonal tile factors and
 * inverts it and sends the inverse out; the process column that owns block column P solves
 * its tiles of the panel; the panel is then sent along the process rows (each rank gets the
 * tiles of its own tile rows) and, transposed, along the process columns (the tiles of its
 * own tile columns); every rank updates its trailing tiles on MFMA.  The triangular inverse
 * Y = L^-T and K^-1 = Y Y^T run right behind on the same layout with the same exchange, the
 * gradient reduction runs on the local tiles of K^-1, and the partial sums meet in one
 * all-reduce.  All ranks call the SAME sequence of gogp_set_data / gogp_absorb / gogp_observe
 * / gogp_gradient / gogp_produce collectively and get the same LML, gradient, alpha, mu, sigma.
 * The reference has no counterpart (single process, goroutines only: gp/gp.go:165-213).
 *
 * Transport, chosen at initialisation (call right after gogp_create, before gogp_set_data):
 *   gogp_dist_init_rccl       RCCL over xGMI from inside the library: grouped ncclSend /
 *                             ncclRecv between peers and ncclAllReduce, enqueued on a
 *                             communication stream and ordered against the compute streams
 *                             by events (no host synchronisation per panel).  The host layer
 *                             only has to hand every rank the same 128-byte unique id
 *                             (made on one rank by gogp_dist_unique_id).
 *   gogp_dist_init_callbacks  host-synchronous exchange through two callbacks over HOST
 *                             buffers (the library stages payloads through pinned memory):
 *                               exchange(user, ops, nops): perform all transfers of the list
 *                                 (is_send: send `bytes` from buf to rank `peer`; else receive
 *                                 into buf); returns after all have completed.  Every pair of
 *                                 ranks lists its mutual transfers in the same order.
 *                               allreduce(user, host_buf, count): sum doubles over the ranks.
 *                             For rehearsals where RCCL cannot run (several ranks sharing one
 *                             GPU, gloo) and for hosts with their own transport (MPI, sockets). */
#define GOGP_UNIQUE_ID_BYTES 128
typedef struct gogp_xfer {
  int32_t peer;    /* rank of the other side                                       */
  int32_t is_send; /* 1: send from buf, 0: receive into buf                        */
  void *buf;       /* host memory, valid until the callback returns                */
  int64_t bytes;
} gogp_xfer;
typedef int (*gogp_exchange_fn)(void *user, const gogp_xfer *ops, int32_t nops);
typedef int (*gogp_allreduce_fn)(void *user, double *host_buf, int64_t count);
/* Default process grid for `nranks` GPUs: 1x1, 1x2, 2x2, 2x4, (16: 4x4). */
int gogp_dist_grid(int nranks, int *prow, int *pcol);
int gogp_dist_unique_id(void *id128 /* GOGP_UNIQUE_ID_BYTES */);
int gogp_dist_init_rccl(gogp_handle *h, int rank, int nranks, int prow, int pcol,
                        const void *id128);
int gogp_dist_init_callbacks(gogp_handle *h, int rank, int nranks, int prow, int pcol,
                             gogp_exchange_fn exchange, gogp_allreduce_fn allreduce,
                             void *user);
/* Ranks of the communicator as the transport itself counts them (RCCL: ncclCommCount; callbacks:
 * nranks), *is_rccl (may be NULL) = 1 for the RCCL transport; -1 on an unsharded handle. */
int gogp_dist_comm_ranks(const gogp_handle *h, int *is_rccl);
/* Pre-flight of the transport, collective: phase 0 = ONE group with a send of `count` doubles to rank+1
 * and a receive from rank-1 (the shape of every panel exchange of the sweep), phase 1 = one all-reduce of
 * `count` doubles; payloads are checked.  Returns after the communication stream has drained, so a
 * transport that hangs shows up as a call that does not return (bench.py runs both under a watchdog
 * before the first sharded evaluation).  No reference counterpart. */
int gogp_dist_selftest(gogp_handle *h, int phase, int64_t count);
/* Device bytes this rank holds for the N-dependent state (its tiles of K / L / Y, panel
 * buffers, block inverses); 0 before gogp_set_data or on an unsharded handle. */
int64_t gogp_dist_local_bytes(const gogp_handle *h);

/* ---- measurement hooks (bench.py / tests; not part of the reference API) --- */

/* Enable (1) / disable (0) HIP-event timing of every launch of the dominant
 * kernel family (the fp64 MFMA GEMM/SYRK tile kernel) on the stream it is
 * launched on. */
int gogp_profile_enable(gogp_handle *h, int on);
/* Since the last reset: sum of the event-measured launch durations (ms), number
 * of launches, flops launched, and the length (ms) of the union of the launch
 * intervals (launches overlap: the hot path runs on several streams).  Resets
 * the accumulators. */
int gogp_profile_read(gogp_handle *h, double *gemm_ms, int64_t *gemm_launches,
                      double *gemm_flops, double *gemm_busy_ms);

/* Every launch of that kernel family since gogp_profile_enable(h, 1), in launch order: start and end in
 * ms since the first launch started, flops launched, tag = mode * 1e8 + (K / 16) * 1e5 + tiles (mode 0
 * rectangular, 1 lower/SYRK, 2 LAUUM).  *n = number of launches (may exceed cap; cap entries are
 * written).  The timeline behind roofline.achieved; tools/launch_timeline.py bins it. */
int gogp_profile_read_launches(gogp_handle *h, int64_t cap, double *t0_ms, double *t1_ms, double *flops,
                               int64_t *tag, int64_t *n);

/* The same for the bandwidth-bound O(N^2) kernels: sum of the event-measured durations
 * (ms) and number of timed launch groups of one class since the last read. */
#define GOGP_PROF_GRAM 0  /* Gram build (the main-stream part: all but the first 512 columns) */
#define GOGP_PROF_GRAD 1  /* fused gradient reduction over K^-1 */
#define GOGP_PROF_CROSS 2 /* cross-covariance build of Produce */
#define GOGP_PROF_NCLASS 4
int gogp_profile_read_aux(gogp_handle *h, int cls, double *ms, int64_t *launches);

/* Scheduling knobs (the results do not depend on them beyond rounding; the defaults are the
 * measured optimum).  Unknown name or out-of-range value: GOGP_EARG.
 *   "lookahead"    1 | 0   panel chain on its own high-priority stream / everything in order
 *                          on one stream                                           (default 1)
 *   "eager"        1 | 0   Observe also runs the triangular inverse (gradient preparation)
 *                          behind the Cholesky sweep / Gradient computes it lazily  (default 1)
 *   "superpanel"   1..8    256-wide panels per trailing update (K = 256 * value)    (default 2)
 *   "precision"    64 | 32 fp64 throughout / the N x N matrices and the O(N^3) products in fp32
 *                          (v_mfma_f32_32x32x2_f32) with fp64 inputs, kernel evaluation, diagonal
 *                          blocks, vectors and reductions: BASELINE configs[4].  Set it before
 *                          gogp_set_data (it re-sizes the buffers) and before gogp_dist_init_*
 *                          (a shard then holds float tiles and exchanges float panels)  (default 64)
 *   "refine_steps" 0..8    precision 32 only: steps of iterative refinement of alpha against
 *                          the exact (fp64, recomputed) Gram matrix                    (default 1)
 *   "cond_limit_log10" 1..300  GOGP_ECOND threshold 10^value -- gonum's package variable
 *                          mat.ConditionTolerance                                   (default 16)
 *   "laplace_max_iter" 1..200   gogp_laplace_observe: Newton steps at the most                (default 50)
 *   "laplace_tol_log10" -14..-4 ... its stationarity tolerance 10^value                     (default -10)
 *   "laplace_warm" 0 | 1        ... 1: start from the last converged mode of the same data and likelihood
 *                          instead of a = 0 (back to a = 0 where that start does not converge)  (default 0)
 *   "superpanel_head" -1..8, "head_remaining" >= 0   wider super-panels while more than head_remaining
 *                          panels are still to come (the chain has slack there; bulk updates with a longer
 *                          K are more efficient); 0 switches it off; -1: 3, on the fp32 path 4
 *                                                                                         (default -1, 16)
 *   "kinv_fused"   -1|0|1  K^-1 accumulated behind the triangular inverse as one rank-k update per
 *                          super-panel of Y (1) or formed by one launch over the finished Y in
 *                          gogp_gradient (0); -1: fused up to N = 10240                    (default -1)
 *   "kinv_split"   0..95   where K^-1 is not fused (fp64, N > 10240): once this percentage of the columns of Y is
 *                          final, their part of K^-1 = Y Y^T is one launch inside the sweep and gogp_gradient's launch
 *                          adds the rest (same sums, same order: bit-identical); 0: one launch       (default 60)
 *   "chain_prio"   -1..2   the chains' tile-kernel launches raise their waves' issue priority: 0 never, 1 the
 *                          skinny (64x64-tile) ones, 2 all of them, -1 the skinny ones up to N = 6144  (default -1)
 *   "ktri"         1 | 0   panel solves skip the zero half of the (lower triangular) block inverse (default 1)
 *   "ard_mfma_min_dims" 1..65  ARD kernels with one radial term and at least this many dimensions run
 *                          the gradient reduction with distances and per-dimension sums on the matrix
 *                          cores (grad_mfma.hip); 65: never                                 (default 1)
 *   "graph"        0..2    gogp_observe_gradient_candidates: on its second identical use the launch sequence
 *                          becomes a hipGraph and is replayed (parameters and data may change, sizes may not).
 *                          1: round 2's linear graph from stream capture, N <= 1024 (larger sizes: streams);
 *                          2: an explicitly built graph -- one node per launch / copy, the sweep's real
 *                          cross-stream dependencies as edges, no stream capture -- up to N = 8192:
 *                          bit-identical to the stream path and, on this runtime, slower than it (DESIGN.md
 *                          section 4); 3: the same recorder as ONE chain in enqueue order (diagnostics);
 *                          0: streams                                                       (default 1)
 *   "produce_tinv", "produce_panels", "produce_groups", "produce_small_below"
 *                          gogp_produce: whole super-panels of `produce_panels` 256-column panels solved through
 *                          the inverse of the factor's diagonal block (1) or panel by panel (0); the test
 *                          points' tile rows on `produce_groups` independent chains; 64 x 64 tiles for launches
 *                          below that many 128-tiles                                  (default 1, 4, 2, 1024)
 *   "gradient_precision" 64 | 32   on an fp64 handle: 32 runs what only the gradient needs -- Y = L^-T and
 *                          K^-1 = Y Y^T, 2/3 of an evaluation's flops -- on the fp32 tile kernel from a float copy of
 *                          the fp64 factor; factorisation, LML, alpha and Produce stay fp64 bit for bit (default 64).
 *                          Offered for kernels of ONE term with an output scale (GOGP_EARG otherwise): there the
 *                          cancelling components come from closed forms and the gradient stays ~1e-8 from the fp64
 *                          one (1e-6 from the oracle in the tests); a sum of terms would read its scale components
 *                          off the float K^-1 (1.9e-4 measured), beyond the reference's own 1e-4 (gp_test.go:170,248)
 *   "trace_fp64"   1 | 0   float K^-1 (precision = 32, gradient_precision = 32): tr(alpha alpha^T - K^-1) summed in
 *                          fp64 from Y and the output-scale component from its closed form          (default 1)
 *   "diag_fp64"    1 | 0   fp32 path (single GPU and float shards): the diagonal blocks' / tiles' trailing updates are
 *                          summed in fp64 from the float panels (diagsyrk.hip) and the fp64 diagonal-block kernel
 *                          factors THAT image; 0: it widens the float matrix's block (rounds 2-4)    (default 1)
 *   "krag"         1 | 0   the triangular inverse's updates skip the zero triangle of a super-panel of Y (default 1)
 *   "chain_split"  -1 | 0 | 2   fp64, the factorisation's dependency chain per 256-panel: 0 one workgroup factors and
 *                          inverts the 256 x 256 diagonal block, the panel solve is a K = 256 product with that inverse;
 *                          2 per 128 columns ONE launch factors the diagonal 128-block and forward-substitutes every
 *                          panel row on the way (panel128.hip), the block inverses are formed off the chain from the
 *                          finished factor; -1: 2 where the evaluation is latency-bound (N <= 8192) or no fp64 inverse
 *                          runs beside the factorisation (Absorb, eager = 0), 0 above that beside the inverse (default -1)
 *   "tiny"         1 | 0   fp64, one GPU, N <= 128 observations (the reference's own case studies): Gram matrix, factor, block
 *                          inverse, z, alpha and K^-1 in ONE launch of one workgroup instead of the general sweep's ~15
 *                          dependent launches; 0: the general sweep                                   (default 1)
 *   "chain_slabs"  0..8    chain_split = 2: 64-row slabs of the panel per workgroup of the chain step; the result does
 *                          not depend on it; 0: one while the launch has at most a workgroup per compute unit, up to 4
 *                          beyond (measured at N = 16384: 1 / 2 / 4 slabs 30.1 / 32.0 / 35.4 ms Observe only) (default 0)
 *   "produce_small_max" 0..64   gogp_produce with up to this many test points (fp32 path: up to 16 of them): ONE
 *                          persistent launch that reads the factor once (trsm_small.hip; float factors are widened in
 *                          registers, the sums are fp64) instead of the tile-kernel chain; 0: never  (default 64)
 *   "basis_symm"   -1 | 0 | 1   gogp_basis_*: W = K^-1 H by the symmetric product with the explicit K^-1 (1: formed first
 *                          where it is not there), by two substitutions through the factor (0), -1: the product where
 *                          K^-1 is on the device or on its way, the substitutions otherwise       (default -1)
 *   "sparse_jitter_log10" -14..-2   gogp_sparse_*: eps = 10^value (absolute) on the diagonal of Kuu (default -8)
 *   "sparse_chunk" 256..65536, a multiple of 256   gogp_sparse_*: rows of X per pass         (default 8192)
 * No reference counterpart (gp.GP.Parallel, gp/gp.go:30-31, only switches goroutines on). */
int gogp_set_option(gogp_handle *h, const char *name, int64_t value);

/* Library build info: "gogp_hip <version> gfx950 ..." */
const char *gogp_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GOGP_HIP_H */
