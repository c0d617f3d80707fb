// Drives gogp::GP::Remove of the C++ host mirror (gogp_amd/host/gogp.hpp): c * Matern32 + sigma^2 on one input
// dimension, Absorb of n rows, Remove of m of them, then LML, Alpha, the factor and Produce are printed
// (tests/test_remove_gpu.py compares them with the oracle's Absorb of the kept rows).
// Input file: "n m nz", "c l sigma", then n inputs, n outputs, nz test points, m indices (any order).
#include <cstdio>
#include <fstream>

#include "../gogp_amd/host/gogp.hpp"

int main(int argc, char **argv) {
  if (argc < 2) return 1;
  std::ifstream in(argv[1]);
  int n = 0, m = 0, nz = 0;
  double c = 0, l = 0, sd = 0;
  in >> n >> m >> nz >> c >> l >> sd;
  std::vector<std::vector<double>> X((size_t)n, std::vector<double>(1)), Z((size_t)nz, std::vector<double>(1));
  std::vector<double> y((size_t)n);
  std::vector<int64_t> idx((size_t)m);
  for (auto &r : X) in >> r[0];
  for (auto &v : y) in >> v;
  for (auto &r : Z) in >> r[0];
  for (auto &i : idx) in >> i;
  if (!in) return 1;
  gogp_desc d{};
  d.ndim = 1;
  d.nterms = 1;
  d.ntheta_simil = 2;
  d.noise_kind = GOGP_NOISE_UNIFORM;
  d.noise_scale = 1.0;
  d.terms[0].kind = GOGP_K_MATERN32;
  d.terms[0].scale_idx = 0;
  d.terms[0].len_idx = 1;
  d.terms[0].period_idx = -1;
  d.terms[0].period_mult = 1.0;
  try {
    gogp::GP gp(d, 0);
    gp.ThetaSimil = {c, l};
    gp.ThetaNoise = {sd};
    if (gp.Absorb(X, y) != GOGP_OK) return 2;
    if (gp.Remove({(int64_t)n}) != GOGP_EARG || (int)gp.Y.size() != n) return 3;  // refused before the library
    if (gp.Remove(idx) != GOGP_OK) return 2;
    if ((int)gp.Y.size() != n - m || (int)gp.X.size() != n - m || (int)gp.Alpha.size() != n - m) return 3;
    std::printf("%.17g\n", gp.LML());
    for (double a : gp.Alpha) std::printf("%.17g\n", a);
    for (double v : gp.Factor()) std::printf("%.17g\n", v);
    std::vector<double> mu, sigma;
    if (!gp.Produce(Z, mu, sigma)) return 2;
    for (double v : mu) std::printf("%.17g\n", v);
    for (double v : sigma) std::printf("%.17g\n", v);
  } catch (const gogp::Error &e) {
    std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
    return 2;
  }
  return 0;
}
