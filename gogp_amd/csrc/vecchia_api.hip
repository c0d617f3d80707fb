// vecchia_api.hip -- C ABI of Vecchia's approximation (gogp_vecchia_*): host code; kernels in vecchia.hip and vecchia_knn.hip.
// include/gogp_hip.h states the approximation and the table; DESIGN.md section 4, "Vecchia".  One kernel does all the
// work; everything runs on the handle's main stream with buffers of the family's own, and the parameters are a copy of
// the family's own, so that devP keeps what the last dense evaluation uploaded.
#include "api_internal.h"

using namespace gogp;

// the first row of the table that breaks the format of include/gogp_hip.h, or -1
static int64_t vecchia_bad_row(const int32_t *nbr, int64_t rows, int32_t m, int64_t n, int causal) {
  for (int64_t i = 0; i < rows; ++i) {
    const int32_t *r = nbr + i * m;
    const int64_t lim = causal ? i : n;
    bool pad = false;
    for (int32_t a = 0; a < m; ++a) {
      if (r[a] == -1) {
        pad = true;
        continue;
      }
      if (pad || r[a] < 0 || (int64_t)r[a] >= lim) return i;
      for (int32_t b = 0; b < a; ++b)
        if (r[b] == r[a]) return i;
    }
  }
  return -1;
}

extern "C" int gogp_vecchia_check(const int32_t *nbr, int64_t rows, int32_t m, int64_t n, int causal) {
  if (m < 0 || m > GOGP_VECCHIA_MAX_M || rows < 0 || n < 0 || (causal && rows > n)) return GOGP_EARG;
  if (rows > 0 && m > 0 && !nbr) return GOGP_EARG;
  return vecchia_bad_row(nbr, rows, m, n, causal) < 0 ? GOGP_OK : GOGP_EARG;
}

// gogp_vecchia_check with the first offending row named in the handle's error text
static int vecchia_check_named(gogp_handle *h, const char *who, const int32_t *nbr, int64_t rows, int32_t m, int64_t n,
                               int causal) {
  if (gogp_vecchia_check(nbr, rows, m, n, causal) == GOGP_OK) return GOGP_OK;
  char buf[320];
  const int64_t bad = (nbr && m >= 0 && m <= GOGP_VECCHIA_MAX_M && rows >= 0) ? vecchia_bad_row(nbr, rows, m, n, causal) : -1;
  if (bad >= 0)
    snprintf(buf, sizeof buf,
             "%s: row %lld of the table is not %s: distinct indices %s, then -1 padding (gogp_vecchia_check)", who,
             (long long)bad, causal ? "causal" : "valid", causal ? "below the row's own" : "in [0, N)");
  else
    snprintf(buf, sizeof buf, "%s: need a table of rows x m int32 with 0 <= m <= %d (gogp_vecchia_check)", who,
             GOGP_VECCHIA_MAX_M);
  return fail(h, GOGP_EARG, buf);
}

// the small device buffers behind an observe: the value, the info word, the slot sums, then per workgroup the value, the
// failure word and the partial row
struct VecchiaSmall {
  double *value, *gout, *vpart, *partials;
  long long *info, *fpart;
};
static size_t vecchia_small_layout(char *base, int blocks, VecchiaSmall *b) {
  Carve c{base};
  b->value = c.take<double>(1);
  b->info = c.take<long long>(1);
  b->gout = c.take<double>(NACC);
  b->vpart = c.take<double>((size_t)blocks);
  b->fpart = c.take<long long>((size_t)blocks);
  b->partials = c.take<double>((size_t)blocks * NACC);
  return c.off;
}

extern "C" int gogp_vecchia_set_data(gogp_handle *h, const double *X, const double *y, const double *v, int64_t N,
                                     const int32_t *nbr, int32_t m) {
  const char *who = "vecchia_set_data";
  if (!h) return GOGP_EARG;
  VecchiaState &vc = h->vc;
  if (N == 0 && !X && !y && !v && !nbr) {  // clear
    HIPCHK(h, hipSetDevice(h->device));
    vc.release();
    return GOGP_OK;
  }
  if (const int rc = refuse_handle(h, who)) return rc;
  if (N < 1 || !X || !y) return refuse(h, who, GOGP_EARG, "need X, y and N >= 1 (N == 0 with NULLs clears)");
  if (N > INT32_MAX) return refuse(h, who, GOGP_EARG, "the table's indices are int32: N <= 2^31 - 1");
  if (const int rc = vecchia_check_named(h, who, nbr, N, m, N, 1)) return rc;
  const int D = h->D;
  if (const char *why = resident_data_refusal(X, y, v, N, D)) return refuse(h, who, GOGP_EARG, why);
  HIPCHK(h, hipSetDevice(h->device));
  if (h->s) HIPCHK(h, hipStreamSynchronize(h->s));
  vc.release();
  const size_t xb = (size_t)N * D * sizeof(double), vb = (size_t)N * sizeof(double);
  const size_t tb = std::max<size_t>((size_t)N * (size_t)m * sizeof(int32_t), 256);
  hipStream_t s = h->s;
  hipError_t e = hipMalloc(&vc.X, xb);
  if (e == hipSuccess) e = hipMalloc(&vc.y, vb);
  if (e == hipSuccess && v) e = hipMalloc(&vc.v, vb);
  if (e == hipSuccess) e = hipMalloc(&vc.nbr, tb);
  if (e == hipSuccess) e = hipMalloc(&vc.P, sizeof(DevParams));
  if (e == hipSuccess) e = hipMemcpyAsync(vc.X, X, xb, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(vc.y, y, vb, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && v) e = hipMemcpyAsync(vc.v, v, vb, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && m > 0) e = hipMemcpyAsync(vc.nbr, nbr, (size_t)N * (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    vc.release();
    HIPCHK(h, e);
  }
  vc.N = N;
  vc.m = m;
  vc.have = true;
  return GOGP_OK;
}

// One pass of the kernel over the stored data: the value's (grad false: terms, *value, *info) or the gradient's (the
// slot sums into acc; nothing else is written).  The stream is idle on return.
static int vecchia_run(gogp_handle *h, bool grad, double *dterms, double *value, long long *info, double *acc) {
  VecchiaState &vc = h->vc;
  hipStream_t s = h->s;
  const int blocks = vecchia_blocks(vc.N);
  VecchiaSmall sm;
  const size_t bytes = vecchia_small_layout(nullptr, blocks, &sm);
  if (const int rc = vc.small.reserve(h, bytes)) return rc;
  vecchia_small_layout(vc.small.as<char>(), blocks, &sm);
  launch_vecchia_observe(s, vc.P, h->D, h->ard_dims, vc.X, vc.y, vc.v, vc.N, vc.nbr, vc.m, dterms,
                         grad ? sm.partials : nullptr, sm.vpart, sm.fpart, sm.gout, grad ? nullptr : sm.value,
                         grad ? nullptr : sm.info);
  if (grad) {
    HIPCHK(h, hipMemcpyAsync(acc, sm.gout, NACC * sizeof(double), hipMemcpyDeviceToHost, s));
  } else {
    HIPCHK(h, hipMemcpyAsync(value, sm.value, sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(info, sm.info, sizeof(long long), hipMemcpyDeviceToHost, s));
  }
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  return GOGP_OK;
}

static int vecchia_notpd(gogp_handle *h, const char *who, long long info, const char *what) {
  char buf[240];
  snprintf(buf, sizeof buf, "%s: the block of %s %lld has a pivot that is not positive and finite", who, what, info - 1);
  h->notpd = (int64_t)(info - 1);
  return fail(h, GOGP_ENOTPD, buf);
}

extern "C" int gogp_vecchia_observe(gogp_handle *h, const double *x, int64_t len, double *lml, double *terms) {
  const char *who = "vecchia_observe";
  if (!h) return GOGP_EARG;
  if (!x || !lml) return refuse(h, who, GOGP_EARG, "NULL");
  if (const int rc = refuse_handle(h, who)) return rc;
  if (len != h->P) return refuse(h, who, GOGP_EARG, "len(x)");
  for (int64_t i = 0; i < len; ++i)
    if (!std::isfinite(x[i])) return refuse(h, who, GOGP_EARG, "non-finite parameter");
  VecchiaState &vc = h->vc;
  if (!vc.have) return refuse(h, who, GOGP_ESTATE, "no data (gogp_vecchia_set_data)");
  std::vector<double> th(h->P > 0 ? h->P : 1);
  for (int i = 0; i < h->P; ++i) th[i] = exp(x[i]);
  if (const char *why = theta_refusal(h, th.data(), th.data() + h->ns)) return refuse(h, who, GOGP_EARG, why);
  DevParams hp;
  fill_params_theta(h, th.data(), th.data() + h->ns, hp);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->s;
  vc.observed = false;
  vc.dnoise = hp.dnoise;
  HIPCHK(h, hipMemcpyAsync(vc.P, &hp, sizeof hp, hipMemcpyHostToDevice, s));
  HIPCHK(h, hipStreamSynchronize(s));  // hp is a local
  double *dterms = nullptr;
  if (terms) {
    if (const int rc = vc.terms.reserve(h, (size_t)vc.N * 3 * sizeof(double))) return rc;
    dterms = vc.terms.as<double>();
  }
  double value = 0.0;
  long long info = 0;
  if (const int rc = vecchia_run(h, false, dterms, &value, &info, nullptr)) return rc;
  if (terms) HIPCHK(h, hipMemcpy(terms, dterms, (size_t)vc.N * 3 * sizeof(double), hipMemcpyDeviceToHost));
  if (info != 0) {
    *lml = NAN;
    return vecchia_notpd(h, who, info, "row");
  }
  *lml = value;
  vc.observed = true;
  return GOGP_OK;
}

extern "C" int gogp_vecchia_gradient(gogp_handle *h, double *grad, int64_t len) {
  const char *who = "vecchia_gradient";
  if (!h) return GOGP_EARG;
  if (!grad) return refuse(h, who, GOGP_EARG, "NULL");
  if (const int rc = refuse_handle(h, who)) return rc;
  if (len != h->P) return refuse(h, who, GOGP_EARG, "len(grad)");
  VecchiaState &vc = h->vc;
  if (!vc.have || !vc.observed) return refuse(h, who, GOGP_ESTATE, "nothing observed (gogp_vecchia_observe)");
  HIPCHK(h, hipSetDevice(h->device));
  double acc[NACC];
  if (const int rc = vecchia_run(h, true, nullptr, nullptr, nullptr, acc)) return rc;
  for (int64_t i = 0; i < len; ++i) grad[i] = 0.0;
  assemble_gradient(h, acc, vc.dnoise, grad);
  return GOGP_OK;
}

// ---- Vecchia: neighbour tables built on the device (vecchia_knn.hip) ------------------------------------------------------
// The exact search of gogp_amd/vecchia.py (nearest / nearest_to) on the handle's main stream; DESIGN.md section 4,
// "Vecchia: neighbour tables on the device".  The resident forms keep the table, the scaled copy of X and the partial
// lists on the device: nothing but the length scales crosses the bus.
static int vecchia_knn_args(gogp_handle *h, const char *who, const double *lengths, int32_t m) {
  if (m < 0 || m > GOGP_VECCHIA_MAX_M) return refuse(h, who, GOGP_EARG, "m: need 0 <= m <= 63 conditioning rows");
  if (lengths)
    for (int d = 0; d < h->D; ++d)
      if (!(lengths[d] > 0.0) || !std::isfinite(lengths[d]))
        return refuse(h, who, GOGP_EARG, "lengths: every length scale must be positive and finite");
  return GOGP_OK;
}

// the scratch of one search: the lengths, the scaled copies of X and Z, the partial lists of a split search
struct VecchiaKnnBufs {
  double *len, *Xs, *Zs;
  void *ws;
};
static size_t vecchia_knn_layout(char *base, int D, int64_t N, int64_t mz, size_t ws_bytes, VecchiaKnnBufs *b) {
  Carve c{base};
  b->len = c.take<double>(GOGP_MAX_NDIM);
  b->Xs = c.take<double>((size_t)N * D);
  b->Zs = c.take<double>((size_t)mz * D);
  b->ws = c.take<char>(ws_bytes);
  return c.off;
}
static size_t vecchia_knn_bytes(int D, int64_t N, int64_t mz, int m) {
  VecchiaKnnBufs b;
  return vecchia_knn_layout(nullptr, D, N, mz, vknn_plan(mz > 0 ? mz : N, N, m).ws_bytes, &b);
}

// The launches of one search on device rows: dX (N x D) and dZ (mz x D; nullptr: the causal table of dX) into dnbr, with
// vecchia_knn_bytes of scratch at base.  lengths: the host's, or nullptr.  The caller synchronises before it returns.
static int vecchia_knn_launch(gogp_handle *h, char *base, const double *dX, int64_t N, const double *dZ, int64_t mz,
                              const double *lengths, int m, int *dnbr) {
  hipStream_t s = h->s;
  const int D = h->D;
  const int64_t targets = dZ ? mz : N;
  VecchiaKnnBufs b;
  vecchia_knn_layout(base, D, N, dZ ? mz : 0, vknn_plan(targets, N, m).ws_bytes, &b);
  if (lengths) HIPCHK(h, hipMemcpyAsync(b.len, lengths, (size_t)D * sizeof(double), hipMemcpyHostToDevice, s));
  launch_vknn_scale(s, dX, N, D, lengths ? b.len : nullptr, b.Xs);
  if (dZ) launch_vknn_scale(s, dZ, mz, D, lengths ? b.len : nullptr, b.Zs);
  launch_vknn(s, b.Xs, N, dZ ? b.Zs : nullptr, targets, D, m, 0, 0, b.ws, dnbr, nullptr);
  return GOGP_OK;
}

// What the two Produce calls do behind their own checks, for a resident and observed data set: the test points go up, the
// table is the caller's (nbrz) or, with `search`, found on the device in its place under `lengths` (nullptr: unscaled) and
// handed back through nbrz_out (nullptr: not wanted); then one launch
static int vecchia_produce_run(gogp_handle *h, const char *who, const double *Z, int64_t mz, const int32_t *nbrz, bool search,
                               const double *lengths, double *mu, double *sigma, int32_t *nbrz_out) {
  VecchiaState &vc = h->vc;
  const int D = h->D, m = vc.m;
  for (int64_t i = 0; i < mz * D; ++i)
    if (!std::isfinite(Z[i])) return refuse(h, who, GOGP_EARG, "non-finite test point");
  if (mz == 0) return GOGP_OK;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->s;
  const int blocks = vecchia_blocks(mz);
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t zb = up((size_t)mz * D * sizeof(double)), vb = up((size_t)mz * sizeof(double));
  const size_t tb = up(std::max<size_t>((size_t)mz * (size_t)m * sizeof(int32_t), 4)), fb = up((size_t)blocks * sizeof(long long));
  if (const int rc = vc.prod.reserve(h, zb + 2 * vb + tb + fb + 256)) return rc;
  if (const int rc = search ? vc.knn.reserve(h, vecchia_knn_bytes(D, vc.N, mz, m)) : GOGP_OK) return rc;
  char *base = vc.prod.as<char>();
  double *dZ = reinterpret_cast<double *>(base), *dmu = reinterpret_cast<double *>(base + zb);
  double *dsig = reinterpret_cast<double *>(base + zb + vb);
  int *dnb = reinterpret_cast<int *>(base + zb + 2 * vb);
  long long *dfp = reinterpret_cast<long long *>(base + zb + 2 * vb + tb), *dinfo = dfp + blocks;
  HIPCHK(h, hipMemcpyAsync(dZ, Z, (size_t)mz * D * sizeof(double), hipMemcpyHostToDevice, s));
  if (search) {
    if (const int rc = vecchia_knn_launch(h, vc.knn.as<char>(), vc.X, vc.N, dZ, mz, lengths, m, dnb)) return rc;
  } else if (m > 0) {
    HIPCHK(h, hipMemcpyAsync(dnb, nbrz, (size_t)mz * (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, s));
  }
  launch_vecchia_produce(s, vc.P, D, vc.X, vc.y, vc.v, dZ, mz, dnb, m, dmu, sigma ? dsig : nullptr, dfp, dinfo);
  long long info = 0;
  HIPCHK(h, hipMemcpyAsync(mu, dmu, (size_t)mz * sizeof(double), hipMemcpyDeviceToHost, s));
  if (sigma) HIPCHK(h, hipMemcpyAsync(sigma, dsig, (size_t)mz * sizeof(double), hipMemcpyDeviceToHost, s));
  if (nbrz_out && m > 0) HIPCHK(h, hipMemcpyAsync(nbrz_out, dnb, (size_t)mz * (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(&info, dinfo, sizeof info, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  if (info != 0) return vecchia_notpd(h, who, info, "test point");
  return GOGP_OK;
}

extern "C" int gogp_vecchia_produce(gogp_handle *h, const double *Z, int64_t mz, const int32_t *nbrz, double *mu,
                                    double *sigma) {
  const char *who = "vecchia_produce";
  if (const int rc = refuse_handle(h, who)) return rc;
  if (mz < 0 || (mz > 0 && (!Z || !mu))) return refuse(h, who, GOGP_EARG, "need Z and mu for mz > 0, mz >= 0");
  VecchiaState &vc = h->vc;
  if (!vc.have || !vc.observed) return refuse(h, who, GOGP_ESTATE, "nothing observed (gogp_vecchia_observe)");
  if (const int rc = vecchia_check_named(h, who, nbrz, mz, vc.m, vc.N, 0)) return rc;
  return vecchia_produce_run(h, who, Z, mz, nbrz, false, nullptr, mu, sigma, nullptr);
}

extern "C" int gogp_vecchia_neighbours(gogp_handle *h, const double *X, int64_t N, const double *Z, int64_t mz,
                                       const double *lengths, int32_t m, int32_t *nbr) {
  const char *who = "vecchia_neighbours";
  if (const int rc = refuse_handle(h, who)) return rc;
  if (N < 1 || !X) return refuse(h, who, GOGP_EARG, "need X and N >= 1");
  if (N > INT32_MAX) return refuse(h, who, GOGP_EARG, "N: the table's indices are int32: N <= 2^31 - 1");
  if (Z ? mz < 0 : mz != 0) return refuse(h, who, GOGP_EARG, "mz: the rows of Z, 0 without Z");
  if (const int rc = vecchia_knn_args(h, who, lengths, m)) return rc;
  const int64_t targets = Z ? mz : N;
  if (targets == 0 || m == 0) return GOGP_OK;
  if (!nbr) return refuse(h, who, GOGP_EARG, "nbr: NULL");
  const int D = h->D;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->s;
  // buffers of the call's own: nothing of the handle changes
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t xb = up((size_t)N * D * sizeof(double)), zb = up((size_t)(Z ? mz : 0) * D * sizeof(double));
  const size_t tb = up((size_t)targets * (size_t)m * sizeof(int32_t));
  Workspace w;
  struct Release {
    Workspace &w;
    ~Release() { w.release(); }
  } release{w};
  if (const int rc = w.reserve(h, xb + zb + tb + vecchia_knn_bytes(D, N, Z ? mz : 0, m))) return rc;
  char *base = w.as<char>();
  double *dX = reinterpret_cast<double *>(base), *dZ = Z ? reinterpret_cast<double *>(base + xb) : nullptr;
  int *dnb = reinterpret_cast<int *>(base + xb + zb);
  HIPCHK(h, hipMemcpyAsync(dX, X, (size_t)N * D * sizeof(double), hipMemcpyHostToDevice, s));
  if (Z) HIPCHK(h, hipMemcpyAsync(dZ, Z, (size_t)mz * D * sizeof(double), hipMemcpyHostToDevice, s));
  if (const int rc = vecchia_knn_launch(h, base + xb + zb + tb, dX, N, dZ, mz, lengths, m, dnb)) return rc;
  HIPCHK(h, hipMemcpyAsync(nbr, dnb, (size_t)targets * (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  return GOGP_OK;
}

// the resident table from the resident X under `lengths` (nullptr: unscaled); the last observe is dropped
static int vecchia_rebuild(gogp_handle *h, const double *lengths) {
  VecchiaState &vc = h->vc;
  if (const int rc = vc.knn.reserve(h, vecchia_knn_bytes(h->D, vc.N, 0, vc.m))) return rc;
  vc.observed = false;
  if (const int rc = vecchia_knn_launch(h, vc.knn.as<char>(), vc.X, vc.N, nullptr, 0, lengths, vc.m, vc.nbr)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->s));
  HIPCHK(h, hipGetLastError());
  vc.built_here = true;
  vc.scaled = lengths != nullptr;
  for (int d = 0; d < h->D; ++d) vc.lengths[d] = lengths ? lengths[d] : 1.0;
  return GOGP_OK;
}

extern "C" int gogp_vecchia_set_data_nearest(gogp_handle *h, const double *X, const double *y, const double *v, int64_t N,
                                             const double *lengths, int32_t m) {
  const char *who = "vecchia_set_data_nearest";
  if (const int rc = refuse_handle(h, who)) return rc;
  if (N < 1 || !X || !y) return refuse(h, who, GOGP_EARG, "need X, y and N >= 1");
  if (N > INT32_MAX) return refuse(h, who, GOGP_EARG, "N: the table's indices are int32: N <= 2^31 - 1");
  if (const int rc = vecchia_knn_args(h, who, lengths, m)) return rc;
  // the upload and its checks are gogp_vecchia_set_data's, with an empty table; the table proper is then built in place
  if (const int rc = gogp_vecchia_set_data(h, X, y, v, N, nullptr, 0)) return rc;
  VecchiaState &vc = h->vc;
  if (m > 0) {
    (void)hipFree(vc.nbr);
    vc.nbr = nullptr;
    const hipError_t e = hipMalloc(&vc.nbr, (size_t)N * (size_t)m * sizeof(int32_t));
    if (e != hipSuccess) {
      vc.release();
      HIPCHK(h, e);
    }
  }
  vc.m = m;
  if (const int rc = vecchia_rebuild(h, lengths)) {
    vc.release();  // (the error text stays)
    return rc;
  }
  return GOGP_OK;
}

extern "C" int gogp_vecchia_reneighbour(gogp_handle *h, const double *lengths) {
  const char *who = "vecchia_reneighbour";
  if (const int rc = refuse_handle(h, who)) return rc;
  VecchiaState &vc = h->vc;
  if (!vc.have) return refuse(h, who, GOGP_ESTATE, "no data (gogp_vecchia_set_data, gogp_vecchia_set_data_nearest)");
  if (const int rc = vecchia_knn_args(h, who, lengths, vc.m)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  return vecchia_rebuild(h, lengths);
}

extern "C" int gogp_vecchia_get_neighbours(gogp_handle *h, int32_t *nbr) {
  const char *who = "vecchia_get_neighbours";
  if (const int rc = refuse_handle(h, who)) return rc;
  VecchiaState &vc = h->vc;
  if (!vc.have) return refuse(h, who, GOGP_ESTATE, "no data (gogp_vecchia_set_data, gogp_vecchia_set_data_nearest)");
  if (vc.m == 0) return GOGP_OK;
  if (!nbr) return refuse(h, who, GOGP_EARG, "nbr: NULL");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(nbr, vc.nbr, (size_t)vc.N * (size_t)vc.m * sizeof(int32_t), hipMemcpyDeviceToHost, h->s));
  HIPCHK(h, hipStreamSynchronize(h->s));
  return GOGP_OK;
}

extern "C" int gogp_vecchia_produce_nearest(gogp_handle *h, const double *Z, int64_t mz, const double *lengths, double *mu,
                                            double *sigma, int32_t *nbrz) {
  const char *who = "vecchia_produce_nearest";
  if (const int rc = refuse_handle(h, who)) return rc;
  if (mz < 0 || (mz > 0 && (!Z || !mu))) return refuse(h, who, GOGP_EARG, "need Z and mu for mz > 0, mz >= 0");
  VecchiaState &vc = h->vc;
  if (!vc.have || !vc.observed) return refuse(h, who, GOGP_ESTATE, "nothing observed (gogp_vecchia_observe)");
  if (!lengths && !vc.built_here)
    return refuse(h, who, GOGP_ESTATE, "lengths: the resident table is the caller's, so it has none to take");
  if (const int rc = vecchia_knn_args(h, who, lengths, vc.m)) return rc;
  return vecchia_produce_run(h, who, Z, mz, nullptr, true, lengths ? lengths : vc.scaled ? vc.lengths : nullptr, mu, sigma, nbrz);
}
