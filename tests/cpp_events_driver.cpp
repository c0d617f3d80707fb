// Drives gogp::GP::SetEvents of the C++ host mirror (gogp_amd/host/gogp.hpp): a flat vector that is not made of
// {from, to, discount} triples is refused, the selfcheck events of tutorial/events/Makefile are set and one Observe +
// Gradient of c * Matern52 * discount + 0.01 sigma^2 is printed (tests/test_events_gpu.py compares it).
#include <cmath>
#include <cstdio>

#include "../gogp_amd/host/gogp.hpp"

int main() {
  gogp_desc d{};
  d.ndim = 1;
  d.nterms = 1;
  d.ntheta_simil = 2;
  d.noise_kind = GOGP_NOISE_UNIFORM;
  d.noise_scale = 0.01;
  d.terms[0].kind = GOGP_K_MATERN52;
  d.terms[0].scale_idx = 0;
  d.terms[0].len_idx = 1;
  d.terms[0].period_idx = -1;
  d.terms[0].period_mult = 1.0;
  try {
    gogp::GP gp(d, 0);
    try {
      gp.SetEvents({1.0, 1.0, 0.5, 4.2});
      std::printf("short vector accepted\n");
      return 1;
    } catch (const gogp::Error &e) {
      if (e.code != GOGP_EARG) return 1;
    }
    gp.SetEvents({1.0, 1.0, 0.5, 4.2, 6.7, 0.25});
    std::vector<std::vector<double>> X;
    std::vector<double> y;
    for (int i = 0; i < 43; ++i) {
      X.push_back({0.1 + 0.2 * i});
      y.push_back(std::sin(0.1 + 0.2 * i));
    }
    gp.SetData(X, y);
    const double lml = gp.Observe({std::log(1.5), std::log(0.8), std::log(0.6)});
    const std::vector<double> g = gp.Gradient();
    std::printf("%.17g %.17g %.17g %.17g\n", lml, g[0], g[1], g[2]);
  } catch (const gogp::Error &e) {
    std::printf("error %d: %s\n", e.code, e.what());
    return 2;
  }
  return 0;
}
