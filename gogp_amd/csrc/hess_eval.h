// hess_eval.h -- device evaluation of the FIRST and SECOND derivatives of the similarity kernel w.r.t. the LOG of its
// hyperparameters, for the Hessian of the LML (hessian.hip).  Beside kern_eval.h, which it leaves alone: every kernel
// built from that header compiles to the code it compiled to before.
//
// A term is  k = c F(S):
//   radial kinds   S = sum_d u_d^2, u_d = (xa_d - xb_d) / l_d,            F = f (kern_eval.h: radial_eval)
//   periodic       S = sum_d sin^2(phi_d) / l_d^2, phi_d = w |xa_d - xb_d|,  F = exp(-2 S), F' = -2 F, F'' = 4 F
// With D_a = theta_a d/d theta_a, A_a = D_a S and B_ab = D_a D_b S:
//   D_a k = c F' A_a,      D_a D_b k = c (F'' A_a A_b + F' B_ab),
//   D_c k = k,  D_c D_a k = D_a k,  D_c D_c k = k       (the output scale c)
// and S is so simple in the logs that A and B are a handful of sums shared by all parameters of the term:
//   one length l:      A = -2 S,        B_ll = 4 S
//   ARD length l_d:    A = -2 S_d,      B_dd = 4 S_d,   B_de = 0 (d != e)          S_d: dimension d's share of S
//   period p:          A = -2 G,        B_pp = Q,       B_pl = 4 G,  B_pd = 4 G_d
//                      G = sum_d sin phi_d cos phi_d phi_d / l_d^2  (G_d its share),
//                      Q = sum_d (2 phi_d^2 cos 2 phi_d + phi_d sin 2 phi_d) / l_d^2     (D_p phi_d = -phi_d)
// Parameters of different terms of a sum have a zero mixed derivative; the caller never asks for one.
//
// f'' of the two Matern kinds whose f is only once differentiable at 0 (3/2 and the reference's 5/2 with coefficient 1)
// grows like 1 / r; it only ever multiplies A_a A_b = O(r^4), so r = 0 takes f'' = 0.
#pragma once
#include "kern_eval.h"

namespace gogp {

// Derivative slots that share one radial evaluation (hessian.hip: an accumulator set each): 3 of a radial term, 2 of a
// periodic one, whose sincos takes the registers of the third set -- the largest groups at which hess_kmm_kernel stays
// within 256 VGPRs without spills (4 / 3: 2 .. 42 spilled VGPRs).
constexpr int HESS_G = 3;
__host__ __device__ constexpr int hess_group_max(bool periodic) { return periodic ? 2 : HESS_G; }
enum { HESS_VALUE = 0, HESS_LEN = 1, HESS_ARD = 2, HESS_PERIOD = 3 };

// Up to HESS_G parameters ("slots") of ONE term: type[q] and, for HESS_ARD, the dimension dim[q].  Passed by value:
// every field is wave-uniform.
struct HessGroup {
  int term, n;
  int type[HESS_G], dim[HESS_G];
};

// what the parameters of a term share at one pair
struct HessRadial {
  double cF, cF1, cF2;  // c F(S), c F'(S), c F''(S)
  double S, G, Q;       // G, Q: periodic only (0 otherwise)
};

// PER: the term is periodic (an instance per class: the radial kinds carry no sincos, the periodic one no sqrt)
template <bool PER, class FA, class FB>
__device__ __forceinline__ HessRadial hess_radial(const DevParams &P, int t, FA xa, FB xb) {
  const int D = P.ndim, kind = P.kind[t];
  const double c = P.c[t];
  HessRadial R;
  R.G = 0.0, R.Q = 0.0;
  double s = 0.0;
  if (PER) {
    const double w = P.w[t];
    for (int d = 0; d < D; ++d) {
      const double phi = w * fabs(xa(d) - xb(d));
      double sn, cs;
      sincos(phi, &sn, &cs);
      const double il = P.inv_len[t][d], il2 = il * il;
      s += sn * sn * il2;
      R.G += sn * cs * phi * il2;
      R.Q += (2.0 * phi * phi * (cs * cs - sn * sn) + 2.0 * phi * sn * cs) * il2;
    }
    R.cF = c * exp(-2.0 * s);
    R.cF1 = -2.0 * R.cF;
    R.cF2 = 4.0 * R.cF;
  } else {
    for (int d = 0; d < D; ++d) {
      const double u = (xa(d) - xb(d)) * P.inv_len[t][d];
      s += u * u;
    }
    // one exp for every radial kind, the polynomials by selects on the (wave-uniform) kind
    const bool nrm = kind == GOGP_K_NORMAL, m32 = kind == GOGP_K_MATERN32, m52 = kind == GOGP_K_MATERN52;
    const double a = m32 ? GOGP_SQRT3 : GOGP_SQRT5;
    const double r = sqrt(s), ir = r > 0.0 ? 1.0 / r : 0.0, ar = a * r;
    const double e = exp(nrm ? -0.5 * s : -ar);
    const double q = m52 ? 1.0 : 5.0 / 3.0;  // the reference's Go constant 5 / 3 is 1 (kern_eval.h)
    const double f = nrm ? e : (m32 ? (1.0 + ar) * e : (1.0 + ar + q * s) * e);
    const double f1 = nrm ? -0.5 * e : (m32 ? -1.5 * e : (m52 ? -0.5 * (3.0 + ar) * e : -(5.0 / 6.0) * (1.0 + ar) * e));
    const double f2 = nrm ? 0.25 * e
                          : (m32 ? 0.75 * GOGP_SQRT3 * e * ir
                                 : (m52 ? 0.25 * (2.0 * GOGP_SQRT5 * ir + (r > 0.0 ? 5.0 : 0.0)) * e : (25.0 / 12.0) * e));
    R.cF = c * f, R.cF1 = c * f1, R.cF2 = c * f2;
  }
  R.S = s;
  return R;
}

// Of one slot: A = D_a S, Bs = D_a D_a S and C = D_p D_a S (a length slot of a periodic term; 0 otherwise).
struct HessSlot {
  double A, Bs, C;
};
template <bool PER, class FA, class FB>
__device__ __forceinline__ HessSlot hess_slot(const DevParams &P, int t, int type, int dim, const HessRadial &R, FA xa,
                                              FB xb) {
  // one dimension's share (HESS_ARD; dimension 0's otherwise, unused)
  const double il = P.inv_len[t][dim], dx = xa(dim) - xb(dim);
  double Sd, Gd = 0.0;
  if (PER) {
    const double phi = P.w[t] * fabs(dx);
    double sn, cs;
    sincos(phi, &sn, &cs);
    Sd = sn * sn * il * il;
    Gd = sn * cs * phi * il * il;
  } else {
    Sd = dx * il * dx * il;
  }
  const bool len = type == HESS_LEN, ard = type == HESS_ARD, per = PER && type == HESS_PERIOD;
  const double Sq = len ? R.S : (ard ? Sd : 0.0), Gq = len ? R.G : (ard ? Gd : 0.0);
  HessSlot o;
  o.A = per ? -2.0 * R.G : -2.0 * Sq;
  o.Bs = per ? R.Q : 4.0 * Sq;
  o.C = 4.0 * Gq;
  return o;
}

// theta_a dk/dtheta_a of the group's slots (exact zeros behind g.n): one radial evaluation for all of them.
template <int G, bool PER, class FA, class FB>
__device__ __forceinline__ void hess_first(const DevParams &P, const HessGroup &g, FA xa, FB xb, double (&out)[G]) {
  const HessRadial R = hess_radial<PER>(P, g.term, xa, xb);
#pragma unroll
  for (int q = 0; q < G; ++q) {
    out[q] = 0.0;
    if (q < g.n) {
      const HessSlot o = hess_slot<PER>(P, g.term, g.type[q], g.dim[q], R, xa, xb);
      out[q] = g.type[q] == HESS_VALUE ? R.cF : R.cF1 * o.A;
    }
  }
}

// The second derivatives of two groups ga, gb of the SAME term, as sums the host combines (hessian.hip: no branch per
// pair of slots here): with w the pair's weight, into acc (HESS_NMOM doubles)
//   [0] w c F    [1 + q] w c F' A_q (ga)    [1 + G + q] w c F' A_q (gb)    [1 + 2G + q] w c F' Bs_q (ga)
//   [1 + 3G + q] w c F' C_q (ga)    [1 + 4G + q] w c F' C_q (gb)    [1 + 5G + a G + b] w c F'' A_a (ga) A_b (gb),  G = HESS_G.
// theta_a theta_b d2k / dtheta_a dtheta_b = c F'' A_a A_b + c F' B_ab with B_ab = Bs_a (the same slot), C_b (a the period),
// C_a (b the period), 0 otherwise; a value slot turns the other's derivative into its first one (A = Bs = C = 0 for it).
constexpr int HESS_NMOM = 1 + 5 * HESS_G + HESS_G * HESS_G;
template <bool PER, class FA, class FB>
__device__ __forceinline__ void hess_moments(const DevParams &P, const HessGroup &ga, const HessGroup &gb, FA xa, FB xb,
                                             double w, double (&acc)[HESS_NMOM]) {
  constexpr int G = HESS_G;
  const int t = ga.term;
  const HessRadial R = hess_radial<PER>(P, t, xa, xb);
  const double w1 = w * R.cF1, w2 = w * R.cF2;
  double Aa[G], Ab[G];
  acc[0] += w * R.cF;
#pragma unroll
  for (int q = 0; q < G; ++q) {
    HessSlot oa = {0.0, 0.0, 0.0}, ob = {0.0, 0.0, 0.0};
    if (q < ga.n) oa = hess_slot<PER>(P, t, ga.type[q], ga.dim[q], R, xa, xb);
    if (q < gb.n) ob = hess_slot<PER>(P, t, gb.type[q], gb.dim[q], R, xa, xb);
    Aa[q] = oa.A, Ab[q] = ob.A;
    acc[1 + q] += w1 * oa.A;
    acc[1 + G + q] += w1 * ob.A;
    acc[1 + 2 * G + q] += w1 * oa.Bs;
    acc[1 + 3 * G + q] += w1 * oa.C;
    acc[1 + 4 * G + q] += w1 * ob.C;
  }
#pragma unroll
  for (int a = 0; a < G; ++a)
#pragma unroll
    for (int b = 0; b < G; ++b) acc[1 + 5 * G + a * G + b] += w2 * Aa[a] * Ab[b];
}

}  // namespace gogp
