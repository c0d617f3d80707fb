// testhooks.hip -- measurement / diagnostic entry points (include/gogp_testhooks.h).
// Built into gogp_amd/libgogp_testhooks.so, which links libgogp_hip.so and calls its
// internal launchers; none of this is part of the product ABI (include/gogp_hip.h).
#include <cstdlib>
#include <cstring>
#include <stdio.h>
#include <vector>

#include "common.h"
#include "gemm_plan.h"  // for gogp_test_gemm_plan
#include "../../include/gogp_testhooks.h"

struct gogp_handle;
namespace gogp {
int dist_init_replay(gogp_handle *h, int rank, int nranks, int prow, int pcol);  // dist2d.hip
}
extern "C" int gogp_test_dist_init_replay(void *h, int rank, int nranks, int prow, int pcol) {
  return gogp::dist_init_replay(static_cast<gogp_handle *>(h), rank, nranks, prow, pcol);
}

namespace gogp_th {
void launch_diag256(hipStream_t s, const double *A, int64_t ld, double *Lout, int64_t ldl,
                    double *Dinv, int64_t row0, int64_t nvalid, long long *info);
void launch_diag256_stamped(hipStream_t s, const double *A, double *Lout, double *Dinv,
                            long long *info, unsigned long long *stamps);
void launch_panel128_stamped(hipStream_t s, const double *A, double *Lout, int64_t rows_below, long long *info,
                             unsigned long long *stamps);
}

namespace gogp {
typedef double f64x4 __attribute__((ext_vector_type(4)));

// ---- fp64 MFMA issue-rate microbenchmark (roofline calibration) -------------
// 8 independent accumulators held in AGPRs by inline asm (the builtin form makes
// hipcc shuttle loop-carried accumulators between VGPRs and AGPRs every
// iteration, which under-reads the rate).  Wave 0 of block 0 also reports shader
// cycles (s_memtime) and wall ticks (s_memrealtime, 100 MHz) around its loop.
__global__ __launch_bounds__(256) void mfma_f64_peak_kernel(int iters, double *sink,
                                                            unsigned long long *clk) {
  f64x4 c0 = {0, 0, 0, 0}, c1 = c0, c2 = c0, c3 = c0, c4 = c0, c5 = c0, c6 = c0, c7 = c0;
  double a = 1.0 + 1e-9 * threadIdx.x, b = 1.0 - 1e-9 * threadIdx.x;
  unsigned long long t0 = __builtin_amdgcn_s_memtime();
  unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
  int cnt = iters;
  // the whole loop lives in one asm statement so that the accumulators stay in
  // AGPRs across iterations
  asm volatile(
      "1:\n\t"
      "v_mfma_f64_16x16x4_f64 %0, %9, %10, %0\n\t"
      "v_mfma_f64_16x16x4_f64 %1, %9, %10, %1\n\t"
      "v_mfma_f64_16x16x4_f64 %2, %9, %10, %2\n\t"
      "v_mfma_f64_16x16x4_f64 %3, %9, %10, %3\n\t"
      "v_mfma_f64_16x16x4_f64 %4, %9, %10, %4\n\t"
      "v_mfma_f64_16x16x4_f64 %5, %9, %10, %5\n\t"
      "v_mfma_f64_16x16x4_f64 %6, %9, %10, %6\n\t"
      "v_mfma_f64_16x16x4_f64 %7, %9, %10, %7\n\t"
      "s_sub_u32 %8, %8, 1\n\t"
      "s_cmp_lg_u32 %8, 0\n\t"
      "s_cbranch_scc1 1b"
      : "+a"(c0), "+a"(c1), "+a"(c2), "+a"(c3), "+a"(c4), "+a"(c5), "+a"(c6), "+a"(c7),
        "+s"(cnt)
      : "v"(a), "v"(b)
      : "scc");
  unsigned long long t1 = __builtin_amdgcn_s_memtime();
  unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
  double s = c0[0] + c1[1] + c2[2] + c3[3] + c4[0] + c5[1] + c6[2] + c7[3];
  if (s == 12345.678) sink[0] = s;  // keep the chains live
  if (clk && blockIdx.x == 0 && threadIdx.x == 0) {
    clk[0] = t1 - t0;
    clk[1] = r1 - r0;
  }
}

// the fp32 twin: v_mfma_f32_32x32x2_f32 (4096 flop, 16 passes), eight independent accumulators
typedef float f32x16p __attribute__((ext_vector_type(16)));
__global__ __launch_bounds__(256) void mfma_f32_peak_kernel(int iters, float *sink, unsigned long long *clk) {
  f32x16p c0 = {0}, c1 = c0, c2 = c0, c3 = c0, c4 = c0, c5 = c0, c6 = c0, c7 = c0;
  float a = 1.0f + 1e-6f * threadIdx.x, b = 1.0f - 1e-6f * threadIdx.x;
  unsigned long long t0 = __builtin_amdgcn_s_memtime();
  unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
  int cnt = iters;
  asm volatile(
      "1:\n\t"
      "v_mfma_f32_32x32x2_f32 %0, %9, %10, %0\n\t"
      "v_mfma_f32_32x32x2_f32 %1, %9, %10, %1\n\t"
      "v_mfma_f32_32x32x2_f32 %2, %9, %10, %2\n\t"
      "v_mfma_f32_32x32x2_f32 %3, %9, %10, %3\n\t"
      "v_mfma_f32_32x32x2_f32 %4, %9, %10, %4\n\t"
      "v_mfma_f32_32x32x2_f32 %5, %9, %10, %5\n\t"
      "v_mfma_f32_32x32x2_f32 %6, %9, %10, %6\n\t"
      "v_mfma_f32_32x32x2_f32 %7, %9, %10, %7\n\t"
      "s_sub_u32 %8, %8, 1\n\t"
      "s_cmp_lg_u32 %8, 0\n\t"
      "s_cbranch_scc1 1b"
      : "+a"(c0), "+a"(c1), "+a"(c2), "+a"(c3), "+a"(c4), "+a"(c5), "+a"(c6), "+a"(c7), "+s"(cnt)
      : "v"(a), "v"(b)
      : "scc");
  unsigned long long t1 = __builtin_amdgcn_s_memtime();
  unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
  float s = c0[0] + c1[1] + c2[2] + c3[3] + c4[4] + c5[5] + c6[6] + c7[7];
  if (s == 12345.678f) sink[0] = s;
  if (clk && blockIdx.x == 0 && threadIdx.x == 0) {
    clk[0] = t1 - t0;
    clk[1] = r1 - r0;
  }
}

int mfma_f32_peak(int iters, double *tflops, double *cyc_per_mfma, double *clock_mhz) {
  float *sink = nullptr;
  unsigned long long *clk = nullptr;
  if (hipMalloc(&sink, 8) != hipSuccess) return GOGP_EHIP;
  if (hipMalloc(&clk, 16) != hipSuccess) return GOGP_EHIP;
  hipDeviceProp_t prop;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return GOGP_EHIP;
  const int blocks = prop.multiProcessorCount * 2;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  hipLaunchKernelGGL(mfma_f32_peak_kernel, dim3(blocks), dim3(256), 0, 0, iters / 4 + 1, sink,
                     (unsigned long long *)nullptr);
  (void)hipEventRecord(e0, 0);
  hipLaunchKernelGGL(mfma_f32_peak_kernel, dim3(blocks), dim3(256), 0, 0, iters, sink, clk);
  (void)hipEventRecord(e1, 0);
  if (hipEventSynchronize(e1) != hipSuccess) return GOGP_EHIP;
  float ms = 0;
  (void)hipEventElapsedTime(&ms, e0, e1);
  const double flops = (double)blocks * 4.0 * (double)iters * 8.0 * 2.0 * 32 * 32 * 2;
  *tflops = flops / (ms * 1e-3) / 1e12;
  unsigned long long h[2] = {0, 0};
  (void)hipMemcpy(h, clk, 16, hipMemcpyDeviceToHost);
  if (cyc_per_mfma) *cyc_per_mfma = (double)h[0] / ((double)iters * 8.0 * 2.0);
  if (clock_mhz) *clock_mhz = h[1] ? (double)h[0] / (double)h[1] * 100.0 : 0.0;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipFree(sink);
  (void)hipFree(clk);
  return GOGP_OK;
}

// tflops: achieved rate with every SIMD issuing; cyc_per_mfma / clock_mhz from wave 0.
int mfma_f64_peak(int iters, double *tflops, double *cyc_per_mfma, double *clock_mhz) {
  double *sink = nullptr;
  unsigned long long *clk = nullptr;
  if (hipMalloc(&sink, 8) != hipSuccess) return GOGP_EHIP;
  if (hipMalloc(&clk, 16) != hipSuccess) return GOGP_EHIP;
  hipDeviceProp_t prop;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return GOGP_EHIP;
  const int blocks = prop.multiProcessorCount * 2;  // 8 waves per CU = 2 per SIMD
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  hipLaunchKernelGGL(mfma_f64_peak_kernel, dim3(blocks), dim3(256), 0, 0, iters / 4 + 1, sink,
                     (unsigned long long *)nullptr);  // warm-up (clock ramp)
  (void)hipEventRecord(e0, 0);
  hipLaunchKernelGGL(mfma_f64_peak_kernel, dim3(blocks), dim3(256), 0, 0, iters, sink, clk);
  (void)hipEventRecord(e1, 0);
  if (hipEventSynchronize(e1) != hipSuccess) return GOGP_EHIP;
  float ms = 0;
  (void)hipEventElapsedTime(&ms, e0, e1);
  const double flops = (double)blocks * 4.0 * (double)iters * 8.0 * 2.0 * 16 * 16 * 4;
  *tflops = flops / (ms * 1e-3) / 1e12;
  unsigned long long h[2] = {0, 0};
  (void)hipMemcpy(h, clk, 16, hipMemcpyDeviceToHost);
  // two waves share a SIMD: cycles per MFMA issued on that SIMD
  if (cyc_per_mfma) *cyc_per_mfma = (double)h[0] / ((double)iters * 8.0 * 2.0);
  if (clock_mhz) *clock_mhz = h[1] ? (double)h[0] / (double)h[1] * 100.0 : 0.0;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipFree(sink);
  (void)hipFree(clk);
  return GOGP_OK;
}


}  // namespace gogp

using namespace gogp;

// ---- shared helpers of the hooks below ----------------------------------------------------------------------------------
// A gogp_test_* hook drives product launchers on host buffers, and every one has the same form.  It checks every argument
// BEFORE the device is touched: a test mistake comes back as GOGP_EARG, never as an access outside the buffers.  Then it
// hands run() one line per array and a callable that launches: each array is copied to the device whole and (in / out
// arrays) back whole, so a test sees the elements a launch must leave alone as well as those it writes.
namespace {
// off + (k - 1) * stride + (rows - 1) * ld + cols <= len, all in elements
bool covers(int64_t len, int64_t off, int64_t ld, int64_t rows, int64_t cols, int64_t k, int64_t stride) {
  if (len <= 0 || off < 0 || ld < cols || rows <= 0 || cols <= 0 || k <= 0 || stride < 0) return false;
  const int64_t hi = off + (k - 1) * stride + (rows - 1) * ld + cols;
  return hi <= len;
}
bool device_ok(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return false;
  return device < 0 || hipSetDevice(device) == hipSuccess;
}
bool prec_ok(int precision) { return precision == 64 || precision == 32; }
hipError_t launched() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? hipDeviceSynchronize() : e;
}
// the largest sizes the hooks take: of the substitution and layout kernels, of the gradient and Gram kernels, of the
// kernels that update or finish a factor, and of the element counts of the vector kernels
constexpr int64_t TH_NPAD_MAX = 1 << 17;
constexpr int64_t GR_NPAD_MAX = 1 << 15;
constexpr int64_t UP_NPAD_MAX = 1 << 15;
constexpr int64_t SH_COUNT_MAX = 1 << 26;

static_assert(GOGP_TEST_NACC == NACC, "GOGP_TEST_NACC mirrors NACC");
// the launchers' selection arguments and the parameters they go with
bool kparams_ok(const gogp_test_kparams *kp, int k, int ard_dims, int radial1, int mfma_min, int ev) {
  if (!kp || k < 1) return false;
  for (int c = 0; c < k; ++c) {
    const gogp_test_kparams &q = kp[c];
    if (q.ndim < 1 || q.ndim > GOGP_MAX_NDIM || q.nterms < 1 || q.nterms > GOGP_MAX_TERMS) return false;
    if (q.ndim != kp[0].ndim || q.nterms != kp[0].nterms) return false;  // one launch sequence: one kernel shape
    int nard = 0;
    for (int t = 0; t < q.nterms; ++t) {
      if (q.kind[t] < GOGP_K_NORMAL || q.kind[t] > GOGP_K_PERIODIC || q.kind[t] != kp[0].kind[t]) return false;
      nard += q.ard[t] != 0;
      for (int d = q.ndim; d < GOGP_MAX_NDIM; ++d)
        if (q.inv_len[t][d] != 0.0) return false;  // the ARD pass relies on it (common.h: launch_grad_reduce)
    }
    if (nard > 1 || ard_dims != (nard ? q.ndim : 0)) return false;  // one ARD term at most; ard_dims is 0 or ndim
    if (radial1 && (q.nterms != 1 || q.kind[0] == GOGP_K_PERIODIC)) return false;
    if (q.nevents < 0 || q.nevents > GOGP_MAX_EVENTS || q.ev_axis < 0 || q.ev_axis >= q.ndim) return false;
  }
  if (ev && ard_dims > 0) return false;  // no instance has both (gogp_set_events refuses ARD)
  return mfma_min >= 1;
}
DevParams to_dev(const gogp_test_kparams &q) {
  DevParams p;
  memset(&p, 0, sizeof p);
  p.ndim = q.ndim;
  p.nterms = q.nterms;
  for (int t = 0; t < GOGP_MAX_TERMS; ++t) {
    p.kind[t] = q.kind[t];
    p.ard[t] = q.ard[t];
    p.c[t] = q.c[t];
    p.w[t] = q.w[t];
    for (int d = 0; d < GOGP_MAX_NDIM; ++d) p.inv_len[t][d] = q.inv_len[t][d];
  }
  p.noise_var = q.noise_var;
  p.dnoise = q.dnoise;
  p.nevents = q.nevents;
  p.ev_axis = q.ev_axis;
  for (int e = 0; e < GOGP_MAX_EVENTS; ++e) {
    p.ev_from[e] = q.ev_from[e];
    p.ev_to[e] = q.ev_to[e];
    p.ev_disc[e] = q.ev_disc[e];
  }
  return p;
}
// the one-term-at-most ARD count kparams_ok wants stated
int ard_dims_of(const gogp_test_kparams *kp) {
  if (!kp || kp->nterms < 1 || kp->nterms > GOGP_MAX_TERMS) return 0;
  int nard = 0;
  for (int t = 0; t < kp->nterms; ++t) nard += kp->ard[t] != 0;
  return nard == 1 ? kp->ndim : 0;
}

// candidate batch of a launcher that reads tl_batch: k == 1 (stride ignored) or 2 .. 16 candidates `bstride` elements apart
bool batch_ok(int precision, int k, int64_t *bstride) {
  if (k < 1 || k > GOGP_MAX_CANDIDATES) return false;
  if (k == 1) {
    *bstride = 0;
    return true;
  }
  return precision == 64 && *bstride > 0 && *bstride % 2 == 0;  // the float launchers do not batch
}
// called inside a run() callable, which puts tl_batch back to its resting {1, 0}; bstride in elements of es bytes
void set_batch(int k, int64_t bstride, int64_t es = 8) {
  tl_batch.k = k;
  tl_batch.stride = (long)(bstride * es);
}
// k parameter blocks / k rows of NACC packed for the device: candidate c at c * stride bytes (stride 0 with k == 1)
std::vector<char> pack_strided(const void *h, size_t item, int k, size_t stride) {
  std::vector<char> buf((size_t)(k - 1) * stride + item, 0);
  for (int c = 0; c < k; ++c) memcpy(buf.data() + (size_t)c * stride, (const char *)h + (size_t)c * item, item);
  return buf;
}
void unpack_strided(const std::vector<char> &buf, void *h, size_t item, int k, size_t stride) {
  for (int c = 0; c < k; ++c) memcpy((char *)h + (size_t)c * item, buf.data() + (size_t)c * stride, item);
}

// a device buffer, freed on every path.  up() allocates max(n, room) bytes, presets them to the byte `fill` (>= 0) and
// uploads the n bytes at h (h == nullptr: none); nothing to hold: nothing is allocated.  down() copies the n bytes back.
struct DevCopy {
  char *d = nullptr;
  size_t bytes = 0;
  hipError_t up(const void *h, size_t n, size_t room = 0, int fill = -1) {
    if (!h) n = 0;
    const size_t cap = n > room ? n : room;
    if (!cap) return hipSuccess;
    bytes = n;
    hipError_t e = hipMalloc(&d, cap);
    if (e == hipSuccess && fill >= 0) e = hipMemset(d, fill, cap);
    if (e == hipSuccess && n) e = hipMemcpy(d, h, n, hipMemcpyHostToDevice);
    return e;
  }
  hipError_t down(void *h) const { return d && bytes ? hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
  template <class T>
  T *as() const {
    return reinterpret_cast<T *>(d);
  }
  ~DevCopy() { (void)hipFree(d); }
};
// one array of a hook's table: len elements of es bytes at h
struct Arr {
  const void *h;
  int64_t len;
  int es;
  bool out;     // comes back after the launch
  bool opt;     // may be NULL, with length 0
  size_t room;  // bytes of the device copy where it is larger than the host array; all of a scratch array
  int fill;     // >= 0: the byte the device copy starts from
};
Arr rd(const void *h, int64_t len, int es = 8) { return {h, len, es, false, false, 0, -1}; }  // read by the launch
Arr io(void *h, int64_t len, int es = 8) { return {h, len, es, true, false, 0, -1}; }          // in / out
Arr opt(Arr a, bool may_be_null = true) {
  a.opt = may_be_null;
  return a;
}
Arr padded(Arr a, size_t bytes, int fill) {  // `bytes` on the device, of the byte `fill` behind the host array's
  a.room = bytes;
  a.fill = fill;
  return a;
}
Arr scratch(size_t bytes, int fill = -1) { return padded(opt(rd(nullptr, 0, 1)), bytes, fill); }  // device-only
bool have(const std::vector<Arr> &arrs) {
  for (const Arr &a : arrs) {
    if (a.opt && !a.h) {
      if (a.len != 0) return false;
      continue;
    }
    if (!a.h || a.len <= 0) return false;
  }
  return true;
}
// the device copies a launch works on, in the order of the table: d[i] as double *, d.f32(i), d.as<T>(i); nullptr for an
// array that is not there
struct Dev {
  std::vector<DevCopy> c;
  template <class T>
  T *as(size_t i) const {
    return c[i].as<T>();
  }
  double *operator[](size_t i) const { return as<double>(i); }
  float *f32(size_t i) const { return as<float>(i); }
};
// uploads the arrays in the order given, runs `launch` on their device copies, puts tl_batch back, synchronises and, if
// all of that succeeded, brings the in / out arrays back
template <class F>
int run(int device, const std::vector<Arr> &arrs, F &&launch) {
  if (!device_ok(device)) return GOGP_EHIP;
  Dev d;
  d.c = std::vector<DevCopy>(arrs.size());
  hipError_t e = hipSuccess;
  size_t i = 0;
  for (const Arr &a : arrs) {
    if (e == hipSuccess) e = d.c[i].up(a.h, a.h && a.len > 0 ? (size_t)a.len * (size_t)a.es : 0, a.room, a.fill);
    ++i;
  }
  if (e == hipSuccess) {
    launch(d);
    set_batch(1, 0);
    e = launched();
  }
  i = 0;
  for (const Arr &a : arrs) {
    if (e == hipSuccess && a.out) e = d.c[i].down(const_cast<void *>(a.h));
    ++i;
  }
  return e == hipSuccess ? GOGP_OK : GOGP_EHIP;
}
}  // namespace

extern "C" int gogp_mfma_f64_peak(int device, int iters, double *tflops, double *cyc_per_mfma,
                                  double *clock_mhz) {
  if (!tflops || iters <= 0) return GOGP_EARG;
  if (!device_ok(device)) return GOGP_EHIP;
  return mfma_f64_peak(iters, tflops, cyc_per_mfma, clock_mhz);
}

extern "C" int gogp_mfma_f32_peak(int device, int iters, double *tflops, double *cyc_per_mfma,
                                  double *clock_mhz) {
  if (!tflops || iters <= 0) return GOGP_EARG;
  if (!device_ok(device)) return GOGP_EHIP;
  return mfma_f32_peak(iters, tflops, cyc_per_mfma, clock_mhz);
}

extern "C" int gogp_test_dgemm_nt(int device, int64_t M, int64_t N, int64_t K, double alpha,
                                  const double *A, const double *B, double beta, double *C) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0) return GOGP_EARG;
  if (M % TILE || N % TILE || K % GEMM_BK) return GOGP_EARG;
  return run(device, {rd(A, M * K), rd(B, N * K), io(C, M * N)}, [&](const Dev &d) {
    launch_dgemm_nt(0, GEMM_RECT, (int)(M / TILE), (int)(N / TILE), K, alpha, d[0], K, d[1], K, beta, d[2], N, nullptr);
  });
}

// ---- the product launchers of the tile kernel, the fp64 diagonal-block update and the diagonal-block kernel on host
// buffers (tests/test_tile_kernels.py)
namespace {
// the launcher's arguments proper (no buffers): false for what the kernels cannot honour
bool gemm_launch_args_ok(int precision, int mode, int mt, int nt, int64_t K, const gogp_test_gemm_opts &o) {
  if (precision != 64 && precision != 32) return false;
  if (mode < GEMM_RECT || mode > GEMM_TRAP || mt <= 0 || nt <= 0 || K <= 0) return false;
  const int64_t kstep = precision == 64 ? GEMM_BK : SGEMM_BK, al = 16 / (precision / 8);  // al: elements per 16 B
  if (K % kstep || K > (1 << 30)) return false;
  if ((mode == GEMM_LOWER || mode == GEMM_LAUUM) && mt != nt) return false;
  if (o.k < 1 || o.k > 64 || o.bstride < 0 || o.bstride % al || (o.k > 1 && o.bstride == 0)) return false;
  if (precision == 32 && (o.k > 1 || o.kbeg0 != 0)) return false;  // the fp32 kernel has neither
  if (o.kbeg0 < 0 || o.kbeg0 % kstep || o.kbeg0 > K || (o.kbeg0 && mode != GEMM_LAUUM)) return false;
  if (o.new_row0 < -1 || (o.new_row0 >= 0 && mode != GEMM_LOWER)) return false;
  if (o.ktri && mode != GEMM_RECT) return false;
  if (o.krag0 < -1 || (o.krag0 >= 0 && (o.ktri || (mode != GEMM_RECT && mode != GEMM_LOWER)))) return false;
  // the first k-step of tile row ti >= krag0 is loaded at k = (ti - krag0) * tile before the loop count is known
  if (o.krag0 >= 0 && o.krag0 < mt && K < (int64_t)(mt - o.krag0) * TILE) return false;
  if (o.rule < 0 || o.rule > 2 || (o.rule && mode != GEMM_RECT)) return false;
  if (o.rule && (o.tpb_shift < 0 || o.tpb_shift > 8 || o.rblk0 < 0 || o.cblk0 < 0 || o.Pr < 1 || o.Pc < 1 ||
                 o.pr < 0 || o.pr >= o.Pr || o.pc < 0 || o.pc >= o.Pc))
    return false;
  return true;
}
const gogp_test_gemm_opts GEMM_OPTS_DEFAULT = {0, -1, -1, 0, 384, 0, 0, 0, 0, 0, 0, 1, 0, 1, -1, 1, 0};
GemmGrid gemm_grid_of(const gogp_test_gemm_opts &o) {
  GemmGrid g;
  g.ktri = o.ktri;
  g.krag0 = o.krag0;
  g.new_row0 = o.new_row0;
  g.kbeg0 = o.kbeg0;
  g.small_below = o.small_below;
  g.prio = o.prio;
  g.rule = o.rule;
  g.tpb_shift = o.tpb_shift;
  g.rblk0 = o.rblk0;
  g.cblk0 = o.cblk0;
  g.pr = o.pr;
  g.Pr = o.Pr;
  g.pc = o.pc;
  g.Pc = o.Pc;
  g.beta0 = o.beta0;
  return g;
}
}  // namespace

extern "C" int gogp_test_gemm_plan(int precision, int mode, int mt, int nt, int64_t K, const gogp_test_gemm_opts *opt,
                                   gogp_test_gemm_plan_out *out) {
  const gogp_test_gemm_opts o = opt ? *opt : GEMM_OPTS_DEFAULT;
  if (!out || !gemm_launch_args_ok(precision, mode, mt, nt, K, o)) return GOGP_EARG;
  const GemmGrid g = gemm_grid_of(o);
  const GemmPlan p = gemm_plan((GemmMode)mode, mt, nt, K, &g, o.k, precision == 64 ? GEMM_F64 : GEMM_F32);
  out->tile = p.tile;
  out->waves = p.waves;
  out->grid_x = p.gridx;
  out->grid_z = p.gridz;
  out->flops = p.flops;
  out->tag = p.tag;
  return GOGP_OK;
}

extern "C" int gogp_test_gemm_nt(int device, int precision, int mode, int mt, int nt, int64_t K, double alpha,
                                 double beta, const void *A, int64_t a_len, int64_t a_off, int64_t lda, const void *B,
                                 int64_t b_len, int64_t b_off, int64_t ldb, void *C, int64_t c_len, int64_t c_off,
                                 int64_t ldc, const gogp_test_gemm_opts *opt) {
  const gogp_test_gemm_opts o = opt ? *opt : GEMM_OPTS_DEFAULT;
  if (!A || !B || !C || !gemm_launch_args_ok(precision, mode, mt, nt, K, o)) return GOGP_EARG;
  const int64_t es = precision / 8, al = 16 / es;  // al: elements per 16 B
  if (alpha == 0.0 || (precision == 32 && (float)alpha == 0.0f)) return GOGP_EARG;  // accumulators start at (beta/alpha) C
  if (lda % al || ldb % al || ldc % al || a_off % al || b_off % al || c_off % al) return GOGP_EARG;
  const int64_t M = (int64_t)mt * TILE, N = (int64_t)nt * TILE;
  if (!covers(a_len, a_off, lda, M, K, o.k, o.bstride) || !covers(b_len, b_off, ldb, N, K, o.k, o.bstride) ||
      !covers(c_len, c_off, ldc, M, N, o.k, o.bstride))
    return GOGP_EARG;
  return run(device, {rd(A, a_len, (int)es), rd(B, b_len, (int)es), io(C, c_len, (int)es)}, [&](const Dev &d) {
    const GemmGrid g = gemm_grid_of(o);
    set_batch(o.k, o.bstride, es);
    if (precision == 64)
      launch_gemm_nt(0, (GemmMode)mode, mt, nt, K, alpha, (const double *)d[0] + a_off, lda, (const double *)d[1] + b_off,
                     ldb, beta, d[2] + c_off, ldc, nullptr, &g);
    else
      launch_gemm_nt(0, (GemmMode)mode, mt, nt, K, alpha, (const float *)d.f32(0) + a_off, lda,
                     (const float *)d.f32(1) + b_off, ldb, beta, d.f32(2) + c_off, ldc, nullptr, &g);
  });
}

extern "C" int gogp_test_diag_syrk(int device, int bs, const float *L, int64_t l_len, int64_t l_off, int64_t ld,
                                   int64_t K, int64_t row_stride, double *D64, int64_t d_len, int nblocks) {
  if (!L || !D64 || (bs != PANEL && bs != 2 * PANEL) || nblocks < 1 || nblocks > 4096) return GOGP_EARG;
  if (K < 16 || K % 16 || ld % 4 || l_off % 4 || row_stride % 4) return GOGP_EARG;  // float4 loads, k-chunks of 16
  if (bs == PANEL && row_stride != PANEL * ld) return GOGP_EARG;  // launch_diag_syrk_f64: blocks 256 rows apart
  if (!covers(l_len, l_off, ld, bs, K, nblocks, row_stride) || d_len < (int64_t)nblocks * bs * bs) return GOGP_EARG;
  return run(device, {rd(L, l_len, 4), io(D64, d_len)}, [&](const Dev &d) {
    if (bs == PANEL)
      launch_diag_syrk_f64(0, d.f32(0) + l_off, ld, K, d[1], nblocks);
    else
      launch_diag_syrk_f64_tiles(0, d.f32(0) + l_off, ld, K, d[1], nblocks, row_stride, bs);
  });
}

extern "C" int gogp_test_diag256_product(int device, int variant, const double *A, int64_t ld, double *L, int64_t ldl,
                                         double *Dinv, int64_t row0, int64_t nvalid, long long *info) {
  if (!A || !L || !Dinv || !info || variant < 0 || variant > 3) return GOGP_EARG;
  if (ld < PANEL || ldl < PANEL || ld % 2 || ldl % 2 || row0 < 0 || nvalid < 0) return GOGP_EARG;  // 16-B loads
  const int64_t ldd = (variant & 1) ? 2 * PANEL : PANEL;  // variants 1, 3: Dinv a block of a leading dimension 512
  return run(device, {rd(A, PANEL * ld), io(L, PANEL * ldl), io(Dinv, PANEL * ldd), io(info, 1)}, [&](const Dev &d) {
    long long *dinfo = d.as<long long>(3);
    switch (variant) {
      case 0: launch_diag256(0, d[0], ld, d[1], ldl, d[2], row0, nvalid, dinfo); break;
      case 1: launch_diag256_ld512(0, d[0], ld, d[1], ldl, d[2], row0, nvalid, dinfo); break;
      case 2: launch_diag256_inv_only(0, d[0], ld, d[2]); break;
      default: launch_diag256_inv_only_ld512(0, d[0], ld, d[2]); break;
    }
  });
}

// Diagnostic: factor+invert one 256x256 SPD block (host buffers) with the stamped
// build of the diagonal kernel; returns the factor, the inverse and 24 s_memtime stamps.
extern "C" int gogp_test_diag256(int device, const double *A, double *Lout, double *Dinv,
                                 unsigned long long *stamps, double *elapsed_us) {
  if (!A || !Lout || !Dinv || !stamps) return GOGP_EARG;
  if (!device_ok(device)) return GOGP_EHIP;
  double *dA = nullptr, *dL = nullptr, *dD = nullptr;
  long long *dinfo = nullptr;
  unsigned long long *dst = nullptr;
  const size_t nb = 256 * 256 * sizeof(double);
  hipError_t e = hipMalloc(&dA, nb);
  if (e == hipSuccess) e = hipMalloc(&dL, nb);
  if (e == hipSuccess) e = hipMalloc(&dD, nb);
  if (e == hipSuccess) e = hipMalloc(&dinfo, 8);
  if (e == hipSuccess) e = hipMalloc(&dst, 32 * 8);
  if (e == hipSuccess) e = hipMemcpy(dA, A, nb, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dinfo, 0, 8);
  if (e == hipSuccess) e = hipMemset(dst, 0, 32 * 8);
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  float ms = 0.f;
  if (e == hipSuccess) {
    gogp_th::launch_diag256_stamped(0, dA, dL, dD, dinfo, dst);  // warm-up
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0, 0);
    gogp::launch_diag256(0, dA, 256, dL, 256, dD, 0, 256, dinfo);  // product build, timed
    (void)hipEventRecord(e1, 0);
    (void)hipEventSynchronize(e1);
    (void)hipEventElapsedTime(&ms, e0, e1);
    gogp_th::launch_diag256_stamped(0, dA, dL, dD, dinfo, dst);
    e = hipDeviceSynchronize();
  }
  if (e == hipSuccess) e = hipMemcpy(Lout, dL, nb, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(Dinv, dD, nb, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(stamps, dst, 32 * 8, hipMemcpyDeviceToHost);
  if (elapsed_us) *elapsed_us = ms * 1e3;
  (void)hipFree(dA); (void)hipFree(dL); (void)hipFree(dD); (void)hipFree(dinfo); (void)hipFree(dst);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return e == hipSuccess ? GOGP_OK : GOGP_EHIP;
}

// ---- instruction costs of the pivot chain (pivot16.h): cycles (s_memtime) per instruction of one wave alone on its SIMD,
// for chains of dependent and runs of independent fp64 operations.  out[0..7]: dependent v_fma_f64, independent v_fma_f64,
// dependent v_mov_b64_dpp row_newbcast, independent v_mov_b64_dpp, dependent v_rsq_f64, independent v_rsq_f64,
// dependent v_mul_f64, dpp -> fma -> dpp -> fma dependent pairs (per pair).
__global__ __launch_bounds__(64) void valu_cost_kernel(double *out, double seed) {
  double x = seed + 1e-9 * threadIdx.x, y = 1.0000001, z = 0.9999999;
  double a0 = x, a1 = x + 1, a2 = x + 2, a3 = x + 3, a4 = x + 4, a5 = x + 5, a6 = x + 6, a7 = x + 7;
  unsigned long long t[9];
#define GOGP_T(k) t[k] = __builtin_amdgcn_s_memtime(); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define REP8(X) X X X X X X X X
#define REP64(X) REP8(REP8(X))
  GOGP_T(0);
  asm volatile(REP64("v_fma_f64 %0, %0, %1, %2\n\t") : "+v"(a0) : "v"(y), "v"(z));
  GOGP_T(1);
  asm volatile(REP8("v_fma_f64 %0, %0, %8, %9\n\tv_fma_f64 %1, %1, %8, %9\n\tv_fma_f64 %2, %2, %8, %9\n\tv_fma_f64 %3, %3, %8, %9\n\t"
                    "v_fma_f64 %4, %4, %8, %9\n\tv_fma_f64 %5, %5, %8, %9\n\tv_fma_f64 %6, %6, %8, %9\n\tv_fma_f64 %7, %7, %8, %9\n\t")
               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(y), "v"(z));
  GOGP_T(2);
  asm volatile(REP64("s_nop 1\n\tv_mov_b64_dpp %0, %0 row_newbcast:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") : "+v"(a0));
  GOGP_T(3);
  asm volatile(REP8("v_mov_b64_dpp %0, %8 row_newbcast:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_mov_b64_dpp %1, %8 row_newbcast:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_mov_b64_dpp %2, %8 row_newbcast:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_mov_b64_dpp %3, %8 row_newbcast:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_mov_b64_dpp %4, %8 row_newbcast:5 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_mov_b64_dpp %5, %8 row_newbcast:6 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_mov_b64_dpp %6, %8 row_newbcast:7 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_mov_b64_dpp %7, %8 row_newbcast:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t")
               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(y));
  GOGP_T(4);
  asm volatile(REP64("v_rsq_f64 %0, %0\n\t") : "+v"(a0));
  GOGP_T(5);
  asm volatile(REP8("v_rsq_f64 %0, %8\n\tv_rsq_f64 %1, %8\n\tv_rsq_f64 %2, %8\n\tv_rsq_f64 %3, %8\n\t"
                    "v_rsq_f64 %4, %8\n\tv_rsq_f64 %5, %8\n\tv_rsq_f64 %6, %8\n\tv_rsq_f64 %7, %8\n\t")
               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(y));
  GOGP_T(6);
  asm volatile(REP64("v_mul_f64 %0, %0, %1\n\t") : "+v"(a1) : "v"(y));
  GOGP_T(7);
  asm volatile(REP64("s_nop 1\n\tv_mov_b64_dpp %1, %0 row_newbcast:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_fma_f64 %0, %1, %2, %0\n\t")
               : "+v"(a2), "+v"(a3) : "v"(y));
  GOGP_T(8);
#undef GOGP_T
#undef REP8
#undef REP64
  if (threadIdx.x == 0)
    for (int k = 0; k < 8; ++k) out[k] = (double)(t[k + 1] - t[k]) / 64.0;
  out[8 + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;
}
extern "C" int gogp_test_valu_cost(int device, double *out8) {
  if (!out8) return GOGP_EARG;
  if (!device_ok(device)) return GOGP_EHIP;
  double *d = nullptr;
  if (hipMalloc(&d, (8 + 64) * sizeof(double)) != hipSuccess) return GOGP_ENOMEM;
  for (int rep = 0; rep < 3; ++rep) hipLaunchKernelGGL(valu_cost_kernel, dim3(1), dim3(64), 0, 0, d, 1.5);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out8, d, 8 * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  return e == hipSuccess ? GOGP_OK : GOGP_EHIP;
}

// Diagnostic: one 128-column chain step (panel128.hip) on a (128 + rows_below) x 128 panel given on the host (row-major,
// ld = 128; the diagonal block's lower triangle is used): the factor of the diagonal block and the solved rows, 72
// s_memtime stamps of the diagnostic build, and the HIP-event time of `reps` launches of the product build.
extern "C" int gogp_test_panel128(int device, const double *A, double *Lout, int64_t rows_below, int reps,
                                  unsigned long long *stamps, double *elapsed_us) {
  if (!A || !Lout || !stamps || rows_below < 0 || rows_below % 64 || reps <= 0) return GOGP_EARG;
  if (!device_ok(device)) return GOGP_EHIP;
  double *dA = nullptr, *dL = nullptr;
  long long *dinfo = nullptr;
  unsigned long long *dst = nullptr;
  // the product launcher also zeroes the block right of the diagonal block: it gets a 256-wide matrix
  const size_t rows = 128 + (size_t)rows_below, nb = rows * 128 * sizeof(double), nb2 = rows * 256 * sizeof(double);
  // each buffer: the ld = 128 matrix (the stamped build's), then the ld = 256 one (the product launcher's)
  hipError_t e = hipMalloc(&dA, nb + nb2);
  if (e == hipSuccess) e = hipMalloc(&dL, nb + nb2);
  if (e == hipSuccess) e = hipMalloc(&dinfo, 8);
  if (e == hipSuccess) e = hipMalloc(&dst, 72 * 8);
  if (e == hipSuccess) e = hipMemcpy(dA, A, nb, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy2D(dA + rows * 128, 256 * sizeof(double), A, 128 * sizeof(double), 128 * sizeof(double), rows,
                                       hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dinfo, 0, 8);
  if (e == hipSuccess) e = hipMemset(dst, 0, 72 * 8);
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  float ms = 0.f;
  if (e == hipSuccess) {
    double *A2 = dA + rows * 128, *L2 = dL + rows * 128;  // the ld = 256 copy (the second halves of both buffers)
    gogp::launch_panel128(0, A2, 256, L2, 256, 0, rows_below, 0, (int64_t)rows, dinfo);  // warm-up
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0, 0);
    for (int r = 0; r < reps; ++r) gogp::launch_panel128(0, A2, 256, L2, 256, 0, rows_below, 0, (int64_t)rows, dinfo);
    (void)hipEventRecord(e1, 0);
    (void)hipEventSynchronize(e1);
    (void)hipEventElapsedTime(&ms, e0, e1);
    gogp_th::launch_panel128_stamped(0, dA, dL, rows_below, dinfo, dst);
    (void)hipDeviceSynchronize();
    gogp_th::launch_panel128_stamped(0, dA, dL, rows_below, dinfo, dst);
    e = hipDeviceSynchronize();
  }
  if (e == hipSuccess) e = hipMemcpy(Lout, dL, nb, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(stamps, dst, 72 * 8, hipMemcpyDeviceToHost);
  if (elapsed_us) *elapsed_us = ms * 1e3 / reps;
  (void)hipFree(dA); (void)hipFree(dL); (void)hipFree(dinfo); (void)hipFree(dst);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return e == hipSuccess ? GOGP_OK : GOGP_EHIP;
}

// The product build of the chain step with the number of 64-row slabs per workgroup forced (panel128.hip: the result must
// not depend on it), on a (128 + rows_below) x 128 panel given on the host; HIP-event time per launch over `reps` launches.
extern "C" int gogp_test_panel128_slabs(int device, const double *A, double *Lout, int64_t rows_below, int slabs, int reps,
                                        double *elapsed_us) {
  if (!A || !Lout || rows_below < 0 || rows_below % 64 || slabs < 0 || slabs > 8 || reps <= 0) return GOGP_EARG;
  if (!device_ok(device)) return GOGP_EHIP;
  const size_t rows = 128 + (size_t)rows_below, nb2 = rows * 256 * sizeof(double);
  double *dA = nullptr, *dL = nullptr;
  long long *dinfo = nullptr;
  hipError_t e = hipMalloc(&dA, nb2);
  if (e == hipSuccess) e = hipMalloc(&dL, nb2);
  if (e == hipSuccess) e = hipMalloc(&dinfo, 8);
  if (e == hipSuccess) e = hipMemset(dL, 0, nb2);
  if (e == hipSuccess) e = hipMemset(dinfo, 0, 8);
  if (e == hipSuccess) e = hipMemcpy2D(dA, 256 * sizeof(double), A, 128 * sizeof(double), 128 * sizeof(double), rows, hipMemcpyHostToDevice);
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  float ms = 0.f;
  if (e == hipSuccess) {
    gogp::launch_panel128_slabs(0, dA, 256, dL, 256, 0, rows_below, 0, (int64_t)rows, dinfo, slabs);
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0, 0);
    for (int r = 0; r < reps; ++r) gogp::launch_panel128_slabs(0, dA, 256, dL, 256, 0, rows_below, 0, (int64_t)rows, dinfo, slabs);
    (void)hipEventRecord(e1, 0);
    (void)hipEventSynchronize(e1);
    (void)hipEventElapsedTime(&ms, e0, e1);
    e = hipDeviceSynchronize();
  }
  if (e == hipSuccess) e = hipMemcpy2D(Lout, 128 * sizeof(double), dL, 256 * sizeof(double), 128 * sizeof(double), rows, hipMemcpyDeviceToHost);
  if (elapsed_us) *elapsed_us = ms * 1e3 / reps;
  (void)hipFree(dA); (void)hipFree(dL); (void)hipFree(dinfo);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return e == hipSuccess ? GOGP_OK : GOGP_EHIP;
}

// Benchmark hook for the tile kernel: times `reps` launches of one GEMM shape on
// device-resident pseudo-random operands (lda = ldb = K, ldc = nt*128).
extern "C" int gogp_bench_gemm(int device, int mode, int mt, int nt, int64_t K, int reps,
                               double *ms_per_launch, double *tflops) {
  if (mt <= 0 || nt <= 0 || K <= 0 || K % GEMM_BK || reps <= 0 || mode < 0 || mode > 2)
    return GOGP_EARG;
  if (!device_ok(device)) return GOGP_EHIP;
  const int64_t M = (int64_t)mt * TILE, N = (int64_t)nt * TILE;
  const int64_t Kld = (mode == GEMM_LAUUM) ? M : K;  // LAUUM: K range = matrix size
  double *dA = nullptr, *dB = nullptr, *dC = nullptr;
  hipError_t e = hipMalloc(&dA, (size_t)M * Kld * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&dB, (size_t)N * Kld * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&dC, (size_t)M * N * sizeof(double));
  if (e != hipSuccess) return GOGP_ENOMEM;
  launch_fill(0, dA, M * Kld, 0.5);
  launch_fill(0, dB, N * Kld, 0.25);
  launch_fill(0, dC, M * N, 1.0);
  GemmProfile pf;
  pf.on = true;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  if (getenv("GOGP_BENCH_GEMM_F32")) {
    // the fp32 tile kernel on the same buffers read as floats (zero-filled: the values do not matter)
    (void)hipMemsetAsync(dA, 0, (size_t)M * Kld * sizeof(double), 0);
    (void)hipMemsetAsync(dB, 0, (size_t)N * Kld * sizeof(double), 0);
    (void)hipMemsetAsync(dC, 0, (size_t)M * N * sizeof(double), 0);
    GemmProfile pf32;
    pf32.on = true;
    hipEvent_t f0, f1;
    (void)hipEventCreate(&f0);
    (void)hipEventCreate(&f1);
    const float *fA = reinterpret_cast<const float *>(dA), *fB = reinterpret_cast<const float *>(dB);
    float *fC = reinterpret_cast<float *>(dC);
    const double beta32 = (mode == GEMM_LAUUM) ? 0.0 : 1.0;
    for (int w = 0; w < 2; ++w)
      launch_gemm_nt(0, (GemmMode)mode, mt, nt, Kld, -1e-3, fA, Kld, fB, Kld, beta32, fC, N, nullptr, nullptr);
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(f0, 0);
    for (int r = 0; r < reps; ++r)
      launch_gemm_nt(0, (GemmMode)mode, mt, nt, Kld, -1e-3, fA, Kld, fB, Kld, beta32, fC, N, &pf32, nullptr);
    (void)hipEventRecord(f1, 0);
    hipError_t e32 = hipEventSynchronize(f1);
    float ms32 = 0.f;
    (void)hipEventElapsedTime(&ms32, f0, f1);
    if (ms_per_launch) *ms_per_launch = ms32 / reps;
    if (tflops) *tflops = pf32.flops / (ms32 * 1e-3) / 1e12;
    for (auto ev_ : pf32.pool) (void)hipEventDestroy(ev_);
    (void)hipEventDestroy(f0);
    (void)hipEventDestroy(f1);
    (void)hipFree(dA);
    (void)hipFree(dB);
    (void)hipFree(dC);
    return e32 == hipSuccess ? GOGP_OK : GOGP_EHIP;
  }
  // GOGP_BENCH_GEMM_BETA0=1: beta = 0, i.e. no C-tile read (what the C preload costs a tile)
  const double beta = (mode == GEMM_LAUUM || getenv("GOGP_BENCH_GEMM_BETA0")) ? 0.0 : 1.0;
  // GOGP_BENCH_GEMM_LD0=1: every operand row aliases row 0 (lda = ldb = 0): all operand loads hit in the
  // caches -- the kernel's rate with memory latency taken out (diagnostic)
  const int64_t ld = getenv("GOGP_BENCH_GEMM_LD0") ? 0 : Kld;
  for (int w = 0; w < 2; ++w)
    launch_dgemm_nt(0, (GemmMode)mode, mt, nt, Kld, -1e-3, dA, ld, dB, ld, beta, dC, N, nullptr);
  (void)hipDeviceSynchronize();
  (void)hipEventRecord(e0, 0);
  for (int r = 0; r < reps; ++r)
    launch_dgemm_nt(0, (GemmMode)mode, mt, nt, Kld, -1e-3, dA, ld, dB, ld, beta, dC, N, &pf);
  (void)hipEventRecord(e1, 0);
  e = hipEventSynchronize(e1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  if (ms_per_launch) *ms_per_launch = ms / reps;
  if (tflops) *tflops = pf.flops / (ms * 1e-3) / 1e12;
  for (auto ev_ : pf.pool) (void)hipEventDestroy(ev_);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipFree(dA);
  (void)hipFree(dB);
  (void)hipFree(dC);
  return e == hipSuccess ? GOGP_OK : GOGP_EHIP;
}

// ---- the kernels that consume the factor, through their product launchers on host buffers
// (tests/test_substitution_kernels.py): the one-pass substitution of trsm_small.hip, and of solve.hip the substitution
// steps, alpha_from_y, rownorm_dot, tinv_init and the batched 256-block product.
extern "C" int64_t gogp_test_trsm_small_workspace(int64_t npad) {
  if (npad <= 0 || npad % PANEL || npad > TH_NPAD_MAX) return -1;
  return (int64_t)trsm_small_workspace_bytes(npad);
}

extern "C" int gogp_test_trsm_small(int device, int precision, int64_t npad, const void *L, int64_t l_len, int64_t ld,
                                    const void *Dinv, const void *KsT, int64_t k_len, int64_t ldk, int j0, int cnt,
                                    double *dq, int64_t dq_len, void *sol, int64_t sol_len, int *kind, int *width,
                                    int64_t *sol_off, unsigned *tmo) {
  if (!L || !Dinv || !KsT || !dq || !sol || !kind || !width || !sol_off || !tmo || !prec_ok(precision)) return GOGP_EARG;
  if (npad <= 0 || npad % PANEL || npad > TH_NPAD_MAX || ld % 2 || j0 < 0 || cnt < 1 || cnt > 32) return GOGP_EARG;
  const bool granule = precision == 64 && j0 == 0 && cnt == 1;  // reads row 0 of KsT alone
  const int64_t krows = granule ? 1 : j0 + (cnt <= 16 ? 16 : 32);  // the counter kernels read whole 16-column tiles
  if (!covers(l_len, 0, ld, npad, npad, 1, 0) || !covers(k_len, 0, ldk, krows, npad, 1, 0) || dq_len < j0 + cnt)
    return GOGP_EARG;
  const size_t wsb = trsm_small_workspace_bytes(npad);
  if (sol_len < 0 || (size_t)sol_len != wsb) return GOGP_EARG;
  const int es = precision / 8;
  int64_t tmo_off = -1;  // the time-out word lies in the work area, which comes back whole as `sol`
  const std::vector<Arr> arrs = {rd(L, l_len, es), rd(Dinv, npad * PANEL, es), rd(KsT, k_len, es), io(dq, dq_len),
                                 io(sol, sol_len, 1)};
  const int rc = run(device, arrs, [&](const Dev &d) {
    char *ws = d.as<char>(4);
    unsigned *dtmo = nullptr;
    if (precision == 64)
      launch_trsm_small(0, d[0], ld, d[1], d[2], ldk, npad, j0, cnt, ws, d[3], &dtmo);
    else
      launch_trsm_small(0, d.f32(0), ld, d.f32(1), d.f32(2), ldk, npad, j0, cnt, ws, d[3], &dtmo);
    if (dtmo) tmo_off = (const char *)dtmo - ws;
    const TsSolution r = trsm_small_solution(npad, j0, cnt, ws, precision == 32);
    *kind = r.kind;
    *width = r.width;
    *sol_off = (int64_t)((const char *)r.p - ws);
  });
  if (rc != GOGP_OK) return rc;
  if (tmo_off < 0 || tmo_off + (int64_t)sizeof(unsigned) > sol_len) return GOGP_EHIP;
  memcpy(tmo, (const char *)sol + tmo_off, sizeof(unsigned));
  return GOGP_OK;
}

extern "C" int gogp_test_trsv_steps(int device, int precision, int dir, int64_t npad, const void *L, int64_t l_len,
                                    int64_t ld, const void *Dinv, int b0, int b1, int k, int64_t bstride, double *w,
                                    int64_t w_len, double *out, int64_t out_len) {
  if (!L || !Dinv || !w || !out || !prec_ok(precision) || (dir != 0 && dir != 1)) return GOGP_EARG;
  if (npad <= 0 || npad % PANEL || npad > TH_NPAD_MAX) return GOGP_EARG;
  const int nb = (int)(npad / PANEL);
  const int64_t al = 16 / (precision / 8);  // 16-B loads of the matrix rows
  if (ld % al || b0 < 0 || b1 < b0 || b1 >= nb || k < 1 || k > 64) return GOGP_EARG;
  if (k > 1 && (precision != 64 || dir != 0 || bstride < npad * PANEL || bstride % 2)) return GOGP_EARG;  // as the product
  if (k == 1) bstride = 0;
  if (!covers(l_len, 0, ld, npad, npad, k, bstride) || !covers(w_len, 0, npad, 1, npad, k, bstride) ||
      !covers(out_len, 0, npad, 1, npad, k, bstride))
    return GOGP_EARG;
  const int es = precision / 8;
  return run(device, {rd(L, l_len, es), rd(Dinv, (k - 1) * bstride + npad * PANEL, es), io(w, w_len), io(out, out_len)},
             [&](const Dev &d) {
               set_batch(k, bstride);
               for (int i = 0; i <= b1 - b0; ++i) {
                 const int b = dir == 0 ? b0 + i : b1 - i;
                 if (precision == 64 && dir == 0)
                   launch_trsv_fwd_step(0, d[0], ld, d[1], b, nb, d[2], d[3]);
                 else if (precision == 64)
                   launch_trsv_bwd_step(0, d[0], ld, d[1], b, nb, d[2], d[3]);
                 else if (dir == 0)
                   launch_trsv_fwd_step(0, d.f32(0), ld, d.f32(1), b, nb, d[2], d[3]);
                 else
                   launch_trsv_bwd_step(0, d.f32(0), ld, d.f32(1), b, nb, d[2], d[3]);
               }
             });
}

extern "C" int gogp_test_alpha_from_y(int device, int precision, int64_t npad, const void *Y, int64_t y_len, int64_t ld,
                                      const double *z, int64_t z_len, double *alpha, int64_t alpha_len) {
  if (!Y || !z || !alpha || !prec_ok(precision)) return GOGP_EARG;
  if (npad <= 0 || npad % 2 || npad > TH_NPAD_MAX || ld % 2) return GOGP_EARG;  // pairs of columns
  if (!covers(y_len, 0, ld, npad, npad, 1, 0) || z_len < npad || alpha_len < npad) return GOGP_EARG;
  return run(device, {rd(Y, y_len, precision / 8), rd(z, z_len), io(alpha, alpha_len)}, [&](const Dev &d) {
    if (precision == 64)
      launch_alpha_from_y(0, (const double *)d[0], ld, d[1], npad, d[2]);
    else
      launch_alpha_from_y(0, (const float *)d.f32(0), ld, d[1], npad, d[2]);
  });
}

extern "C" int gogp_test_rownorm_dot(int device, int precision, const void *V, int64_t v_len, int64_t ld, int64_t ncols,
                                     int64_t m, const double *vec, int64_t vec_len, double *dot, int64_t dot_len,
                                     double *sq, int64_t sq_len) {
  if (!V || !prec_ok(precision) || m <= 0 || m > 65535 || ncols <= 0) return GOGP_EARG;
  if (!covers(v_len, 0, ld, m, ncols, 1, 0) || (vec && vec_len < ncols) || (dot && dot_len < m) || (sq && sq_len < m))
    return GOGP_EARG;
  // vec, dot and sq may each be NULL: run() copies nothing for those and the launcher gets nullptr
  return run(device, {rd(V, v_len, precision / 8), rd(vec, vec_len), io(dot, dot_len), io(sq, sq_len)}, [&](const Dev &d) {
    if (precision == 64)
      launch_rownorm_dot(0, d[0], ld, d[1], ncols, m, d[2], d[3]);
    else
      launch_rownorm_dot(0, d.f32(0), ld, d[1], ncols, m, d[2], d[3]);
  });
}

extern "C" int gogp_test_tinv(int device, int precision, int nsub, const void *Dinv, void *X, int64_t x_len, int64_t tld,
                              int with_xt, void *XT) {
  if (!Dinv || !X || !prec_ok(precision) || nsub < 1 || nsub > 16 || (with_xt && !XT)) return GOGP_EARG;
  const int64_t n = (int64_t)nsub * PANEL;
  if (!covers(x_len, 0, tld, n, n, 1, 0)) return GOGP_EARG;
  const int es = precision / 8;
  return run(device, {rd(Dinv, n * PANEL, es), io(X, x_len, es), io(with_xt ? XT : nullptr, x_len, es)}, [&](const Dev &d) {
    if (precision == 64)
      launch_tinv_init(0, d[0], d[1], d[2], nsub, tld);
    else
      launch_tinv_init(0, d.f32(0), d.f32(1), d.f32(2), nsub, tld);
  });
}

extern "C" int gogp_test_blockmm(int device, int precision, int nprod, void *arena, int64_t arena_len, const int64_t *a_off,
                                 const int64_t *lda, const int64_t *b_off, const int64_t *ldb, const int64_t *c_off,
                                 const int64_t *ldc, const int *K, double alpha, int k, int64_t bstride) {
  if (!arena || !a_off || !lda || !b_off || !ldb || !c_off || !ldc || !K || !prec_ok(precision)) return GOGP_EARG;
  if (nprod < 1 || nprod > 6 || k < 1 || k > 64 || (k > 1 && (precision != 64 || bstride <= 0))) return GOGP_EARG;
  if (k == 1) bstride = 0;
  for (int b = 0; b < nprod; ++b) {
    if (K[b] <= 0 || K[b] % 32) return GOGP_EARG;
    if (!covers(arena_len, a_off[b], lda[b], PANEL, K[b], k, bstride) ||
        !covers(arena_len, b_off[b], ldb[b], K[b], PANEL, k, bstride) ||
        !covers(arena_len, c_off[b], ldc[b], PANEL, PANEL, k, bstride))
      return GOGP_EARG;
  }
  const int es = precision / 8;
  return run(device, {io(arena, arena_len, es)}, [&](const Dev &d) {
    set_batch(k, bstride, es);
    if (precision == 64) {
      const double *A[6], *B[6];
      double *C[6];
      for (int b = 0; b < nprod; ++b) {
        A[b] = d[0] + a_off[b];
        B[b] = d[0] + b_off[b];
        C[b] = d[0] + c_off[b];
      }
      launch_blockmm(0, nprod, A, lda, B, ldb, C, ldc, K, alpha);
    } else {
      const float *A[6], *B[6];
      float *C[6];
      for (int b = 0; b < nprod; ++b) {
        A[b] = d.f32(0) + a_off[b];
        B[b] = d.f32(0) + b_off[b];
        C[b] = d.f32(0) + c_off[b];
      }
      launch_blockmm(0, nprod, A, lda, B, ldb, C, ldc, K, alpha);
    }
  });
}

// ---- the kernels that turn K^-1 into the gradient, through their product launchers (tests/test_grad_kernels.py) ----------
namespace {
int blocks_of(int64_t npad, int64_t mrows, int64_t ncols, int max_blocks) {
  if (max_blocks < 0) return -1;
  int b;
  if (mrows == 0) {
    if (ncols != 0 || npad <= 0 || npad % 64 || npad > GR_NPAD_MAX) return -1;
    b = grad_reduce_blocks(npad);
  } else {
    if (mrows <= 0 || ncols <= 0 || mrows % 64 || ncols % 64 || mrows > GR_NPAD_MAX || ncols > GR_NPAD_MAX) return -1;
    b = grad_reduce_blocks_local(mrows, ncols);
  }
  return max_blocks > 0 && max_blocks < b ? max_blocks : b;
}
}  // namespace

extern "C" int gogp_test_grad_blocks(int64_t npad, int64_t mrows, int64_t ncols, int max_blocks) {
  return blocks_of(npad, mrows, ncols, max_blocks);
}

extern "C" int gogp_test_grad_reduce(int device, int precision, const gogp_test_kparams *kparams, int ard_dims, int radial1,
                                     int mfma_min, int ev, const double *X, int64_t x_len, const double *alpha,
                                     int64_t alpha_len, const void *Kinv, int64_t kinv_len, int64_t ld, int64_t n,
                                     int64_t npad, int max_blocks, int k, int64_t bstride, double *partials,
                                     int64_t partials_len, double *out) {
  if (!kparams || !X || !alpha || !Kinv || !partials || !out || !prec_ok(precision)) return GOGP_EARG;
  if (k < 1 || k > GOGP_MAX_CANDIDATES || (k > 1 && precision != 64)) return GOGP_EARG;  // candidates: the fp64 path's
  if (!kparams_ok(kparams, k, ard_dims, radial1, mfma_min, ev)) return GOGP_EARG;
  const int blocks = blocks_of(npad, 0, 0, max_blocks);
  if (blocks < 1 || n < 1 || n > npad || ld < npad) return GOGP_EARG;
  const int ndim = kparams[0].ndim;
  const int64_t prow = (int64_t)blocks * NACC;
  if (k == 1) bstride = 0;
  // every per-candidate buffer shares the byte stride: it must hold the largest of them
  else if (bstride < (npad - 1) * ld + npad || bstride < prow || bstride * 8 < (int64_t)sizeof(DevParams)) return GOGP_EARG;
  if (x_len < npad * ndim + GOGP_MAX_NDIM || !covers(alpha_len, 0, npad, 1, npad, k, bstride) ||
      !covers(kinv_len, 0, ld, npad, npad, k, bstride) || !covers(partials_len, 0, prow, 1, prow, k, bstride))
    return GOGP_EARG;
  std::vector<DevParams> hp;
  for (int c = 0; c < k; ++c) hp.push_back(to_dev(kparams[c]));
  const size_t sb = (size_t)bstride * 8;
  const std::vector<char> P = pack_strided(hp.data(), sizeof(DevParams), k, sb);
  std::vector<char> O = pack_strided(out, NACC * sizeof(double), k, sb);
  const std::vector<Arr> arrs = {rd(P.data(), P.size(), 1),      rd(X, x_len), rd(alpha, alpha_len), rd(Kinv, kinv_len, precision / 8),
                                 io(partials, partials_len), io(O.data(), O.size(), 1)};
  const int rc = run(device, arrs, [&](const Dev &d) {
    set_batch(k, bstride);
    if (precision == 64)
      launch_grad_reduce(0, d.as<DevParams>(0), ndim, ard_dims, d[1], d[2], d[3], ld, n, npad, d[4], d[5], radial1 != 0,
                         mfma_min, ev != 0, max_blocks);
    else
      launch_grad_reduce(0, d.as<DevParams>(0), ndim, ard_dims, d[1], d[2], d.f32(3), ld, n, npad, d[4], d[5], radial1 != 0,
                         mfma_min, ev != 0, max_blocks);
  });
  if (rc == GOGP_OK) unpack_strided(O, out, NACC * sizeof(double), k, sb);
  return rc;
}

extern "C" int gogp_test_grad_reduce_local(int device, int precision, const gogp_test_kparams *kparams, int ard_dims,
                                           int radial1, int mfma_min, int ev, const double *X, int64_t x_len,
                                           const double *alpha, int64_t alpha_len, const void *Kinv, int64_t kinv_len,
                                           int64_t ld, int64_t n, int64_t npad, int64_t mrows, int64_t ncols, int nb_shift,
                                           int pr, int Pr, int pc, int Pc, int max_blocks, int k, int64_t bstride,
                                           double *partials, int64_t partials_len, double *out) {
  (void)bstride;
  if (!kparams || !X || !alpha || !Kinv || !partials || !out || !prec_ok(precision)) return GOGP_EARG;
  if (k != 1) return GOGP_EARG;  // launch_grad_reduce_local has no candidate batch
  if (!kparams_ok(kparams, 1, ard_dims, radial1, mfma_min, ev)) return GOGP_EARG;
  if (mrows <= 0 || ncols <= 0) return GOGP_EARG;
  const int blocks = blocks_of(npad, mrows, ncols, max_blocks);
  if (blocks < 1 || npad <= 0 || npad % 64 || npad > GR_NPAD_MAX || n < 1 || n > npad || ld < ncols) return GOGP_EARG;
  if (nb_shift < 6 || nb_shift > 14 || Pr < 1 || Pc < 1 || pr < 0 || pr >= Pr || pc < 0 || pc >= Pc) return GOGP_EARG;
  BlockMap map;
  map.nb_shift = nb_shift;
  map.pr = pr;
  map.Pr = Pr;
  map.pc = pc;
  map.Pc = Pc;
  // the last local row / column must be a global one inside the padded matrix (the kernels read X and alpha there)
  if (map.grow(mrows - 1) >= npad || map.gcol(ncols - 1) >= npad) return GOGP_EARG;
  const int ndim = kparams[0].ndim;
  const int64_t prow = (int64_t)blocks * NACC;
  if (x_len < npad * ndim + GOGP_MAX_NDIM || alpha_len < npad || !covers(kinv_len, 0, ld, mrows, ncols, 1, 0) ||
      partials_len < prow)
    return GOGP_EARG;
  const DevParams hp = to_dev(kparams[0]);
  return run(device, {rd(&hp, 1, sizeof hp), rd(X, x_len), rd(alpha, alpha_len), rd(Kinv, kinv_len, precision / 8),
                      io(partials, partials_len), io(out, NACC)},
             [&](const Dev &d) {
               if (precision == 64)
                 launch_grad_reduce_local(0, d.as<DevParams>(0), ndim, ard_dims, d[1], d[2], d[3], ld, n, mrows, ncols, map,
                                          d[4], d[5], radial1 != 0, mfma_min, ev != 0, max_blocks);
               else
                 launch_grad_reduce_local(0, d.as<DevParams>(0), ndim, ard_dims, d[1], d[2], d.f32(3), ld, n, mrows, ncols,
                                          map, d[4], d[5], radial1 != 0, mfma_min, ev != 0, max_blocks);
             });
}

extern "C" int gogp_test_xgrad(int device, const gogp_test_kparams *kparams, int ev, const double *X, int64_t x_len,
                               const double *alpha, int64_t alpha_len, double *Kinv, int64_t kinv_len, int64_t ld, int64_t n,
                               int64_t npad, double *gx, int64_t gx_len) {
  if (!kparams || !X || !alpha || !Kinv || !gx) return GOGP_EARG;
  int nard = 0;
  for (int t = 0; t < GOGP_MAX_TERMS && kparams->nterms >= 1 && t < kparams->nterms; ++t) nard += kparams->ard[t] != 0;
  if (!kparams_ok(kparams, 1, nard == 1 ? kparams->ndim : 0, 0, 1, 0)) return GOGP_EARG;
  if (npad <= 0 || npad % 64 || npad > GR_NPAD_MAX || n < 1 || n > npad || ld < npad) return GOGP_EARG;
  const int ndim = kparams->ndim;
  if (x_len < npad * ndim || alpha_len < npad || !covers(kinv_len, 0, ld, npad, npad, 1, 0) || gx_len < npad * ndim)
    return GOGP_EARG;
  const DevParams hp = to_dev(*kparams);
  return run(device, {rd(&hp, 1, sizeof hp), rd(X, x_len), rd(alpha, alpha_len), io(Kinv, kinv_len), io(gx, gx_len)},
             [&](const Dev &d) {
               launch_xgrad(0, d.as<DevParams>(0), ndim, d[1], d[2], d[3], ld, n, npad, d[4], ev != 0);
             });
}

// ---- the kernels that update a factor or consume Produce's V^T, through their product launchers
// (tests/test_update_kernels.py): append_gram_kernel and append_commit_kernel (append.hip), the gather, W, snapshot and
// block kernels of remove.hip, bwd_panel_kernel (pgrad.hip) and the two kernels of launch_pcov (pcov.hip).
namespace {
// bytes a solution of `cols` right-hand sides over npc rows occupies from its first byte on; -1: not a layout
int64_t sol_bytes(int kind, int width, int cols, int64_t npc) {
  if (cols < 0 || width < 1) return -1;
  switch (kind) {
    case TS_SOL_PAIRED: return cols <= width ? npc * width * 8 : -1;  // npc is even
    case TS_SOL_COMPACT: return cols <= width ? npc * width * 8 : -1;
    case TS_SOL_GRANULE: return width == 1 && cols <= 1 ? npc * 16 : -1;
    case TS_SOL_ROWS: return width >= npc ? (cols ? ((int64_t)(cols - 1) * width + npc) * 8 : 0) : -1;
    default: return -1;
  }
}
bool sol_ok(const void *p, int64_t len, int kind, int width, int64_t off, int cols, int64_t npc) {
  const int64_t need = sol_bytes(kind, width, cols, npc);
  if (need < 0) return false;
  if (cols == 0) return true;  // never read
  return p && off >= 0 && off % (kind == TS_SOL_GRANULE ? 16 : 8) == 0 && off + need <= len;
}
// every entry of an index list names a row of a matrix of leading dimension ld0 that src (src_len elements) holds whole
bool rows_ok(const int *idx, int64_t cnt, int64_t ld0, int64_t src_len) {
  for (int64_t i = 0; i < cnt; ++i)
    if (idx[i] < 0 || idx[i] >= ld0 || ((int64_t)idx[i] + 1) * ld0 > src_len) return false;
  return true;
}
}  // namespace

extern "C" int gogp_test_append_gram(int device, const void *sol0, int64_t sol0_len, int kind0, int width0, int64_t off0,
                                     const void *sol1, int64_t sol1_len, int kind1, int width1, int64_t off1, int m0, int m,
                                     int64_t npc, int64_t n, const double *z, int64_t z_len, double *part, int64_t part_len,
                                     double *Lnew, int64_t lnew_len, int64_t ld) {
  if (!z || !part || !Lnew || m < 1 || m > 64 || m0 < 0 || m0 > m) return GOGP_EARG;
  if (npc <= 0 || npc % PANEL || npc > UP_NPAD_MAX || n < 0 || n > npc || ld < n) return GOGP_EARG;
  if (!sol_ok(sol0, sol0_len, kind0, width0, off0, m0, npc) || !sol_ok(sol1, sol1_len, kind1, width1, off1, m - m0, npc))
    return GOGP_EARG;
  if (z_len < npc || part_len < npc / PANEL * APPEND_PART || lnew_len <= 0) return GOGP_EARG;
  if (n > 0 && !covers(lnew_len, 0, ld, m, n, 1, 0)) return GOGP_EARG;
  // a source that gives no column is not uploaded: its solution pointer is nullptr
  return run(device, {rd(m0 ? sol0 : nullptr, sol0_len, 1), rd(m - m0 ? sol1 : nullptr, sol1_len, 1), rd(z, z_len),
                      io(part, part_len), io(Lnew, lnew_len)},
             [&](const Dev &d) {
               TsSolution v0, v1;
               v0.p = d.as<char>(0) ? d.as<char>(0) + off0 : nullptr;
               v0.kind = kind0;
               v0.width = width0;
               v1.p = d.as<char>(1) ? d.as<char>(1) + off1 : nullptr;
               v1.kind = kind1;
               v1.width = width1;
               launch_append_gram(0, v0, v1, m0, m, npc, n, d[2], d[3], d[4], ld);
             });
}

// v2 != nullptr: launch_nv_append_fold (noisevar.hip) on the parts first, as gogp_append_noisy does; parts_back: the
// parts come back whole
static int test_append_commit(int device, const gogp_test_kparams *kparams, int ev, const double *X2, int64_t x2_len,
                              const double *y2, int64_t y2_len, const double *v2, int64_t v2_len, int m, int64_t n,
                              const double *part, bool parts_back, int64_t part_len, int nslab, double *Lnew,
                              int64_t lnew_len, int64_t ld, double *z2, int64_t z2_len, long long *info) {
  if (!kparams || !X2 || !y2 || !part || !Lnew || !z2 || !info) return GOGP_EARG;
  if (v2 && v2_len < m) return GOGP_EARG;
  if (!kparams_ok(kparams, 1, ard_dims_of(kparams), 0, 1, ev)) return GOGP_EARG;
  if (m < 1 || m > 64 || n < 0 || n > UP_NPAD_MAX || nslab < 1 || nslab > UP_NPAD_MAX / PANEL) return GOGP_EARG;
  if (x2_len < (int64_t)m * kparams->ndim || y2_len < m || z2_len < m || part_len < (int64_t)nslab * APPEND_PART)
    return GOGP_EARG;
  if (!covers(lnew_len, 0, ld, m, n + m, 1, 0)) return GOGP_EARG;
  const DevParams hp = to_dev(*kparams);
  Arr parts = rd(part, part_len);
  parts.out = parts_back;
  return run(device, {rd(&hp, 1, sizeof hp), rd(X2, x2_len), rd(y2, y2_len), rd(v2, v2_len), parts, io(Lnew, lnew_len),
                      io(z2, z2_len), io(info, 1)},
             [&](const Dev &d) {
               if (v2) launch_nv_append_fold(0, d[4], d[3], m);
               launch_append_commit(0, d.as<DevParams>(0), d[1], d[2], m, n, d[4], nslab, d[5], ld, d[6],
                                    d.as<long long>(7), ev != 0);
             });
}

extern "C" int gogp_test_append_commit(int device, const gogp_test_kparams *kparams, int ev, const double *X2, int64_t x2_len,
                                       const double *y2, int64_t y2_len, int m, int64_t n, const double *part,
                                       int64_t part_len, int nslab, double *Lnew, int64_t lnew_len, int64_t ld, double *z2,
                                       int64_t z2_len, long long *info) {
  return test_append_commit(device, kparams, ev, X2, x2_len, y2, y2_len, nullptr, 0, m, n, part, false, part_len, nslab,
                            Lnew, lnew_len, ld, z2, z2_len, info);
}

extern "C" int gogp_test_nv_append_commit(int device, const gogp_test_kparams *kparams, int ev, const double *X2,
                                          int64_t x2_len, const double *y2, int64_t y2_len, const double *v2, int64_t v2_len,
                                          int m, int64_t n, double *part, int64_t part_len, int nslab, double *Lnew,
                                          int64_t lnew_len, int64_t ld, double *z2, int64_t z2_len, long long *info) {
  if ((v2 == nullptr) != (v2_len == 0)) return GOGP_EARG;
  return test_append_commit(device, kparams, ev, X2, x2_len, y2, y2_len, v2, v2_len, m, n, part, true, part_len, nslab,
                            Lnew, lnew_len, ld, z2, z2_len, info);
}

extern "C" int gogp_test_remove_gather(int device, const double *src, int64_t src_len, int64_t ld0, const int *map,
                                       int64_t map_len, int64_t n1, double *dst, int64_t dst_len, int64_t npad1) {
  if (!src || !map || !dst || npad1 <= 0 || npad1 % PANEL || npad1 > UP_NPAD_MAX || n1 < 1 || n1 > npad1) return GOGP_EARG;
  if (ld0 < 1 || map_len < n1 || dst_len < npad1 * npad1 || !rows_ok(map, n1, ld0, src_len)) return GOGP_EARG;
  return run(device, {rd(src, src_len), rd(map, map_len, 4), io(dst, dst_len)},
             [&](const Dev &d) { launch_remove_gather(0, d[0], ld0, d.as<int>(1), n1, d[2], npad1); });
}

extern "C" int gogp_test_remove_w(int device, const double *src, int64_t src_len, int64_t ld0, const int *map,
                                  int64_t map_len, const int *rem, int64_t rem_len, int mc, int mw, int64_t r0, int64_t n1,
                                  int64_t npad1, double *W, int64_t w_len) {
  if (!src || !map || !rem || !W || npad1 <= 0 || npad1 % PANEL || npad1 > UP_NPAD_MAX || n1 < 1 || n1 > npad1)
    return GOGP_EARG;
  if (mw < 1 || mw > REMOVE_W || mc < 1 || mc > mw || r0 < 0 || r0 >= npad1) return GOGP_EARG;
  if (ld0 < 1 || map_len < n1 || rem_len < mc || w_len < (int64_t)mw * npad1) return GOGP_EARG;
  if (!rows_ok(map, n1, ld0, src_len) || !rows_ok(rem, mc, ld0, src_len)) return GOGP_EARG;
  return run(device, {rd(src, src_len), rd(map, map_len, 4), rd(rem, rem_len, 4), io(W, w_len)}, [&](const Dev &d) {
    launch_remove_w(0, d[0], ld0, d.as<int>(1), d.as<int>(2), mc, mw, r0, n1, npad1, d[3]);
  });
}

extern "C" int gogp_test_remove_block(int device, double *L, int64_t l_len, int64_t ld, int snap_b0, int snap_nb,
                                      double *snap, int64_t snap_len, double *W, int64_t w_len, int mw, int64_t kb0,
                                      int64_t kb1, int64_t n1) {
  if (!L || !snap || !W || ld <= 0 || ld % PANEL || ld > UP_NPAD_MAX || n1 < 1 || n1 > ld) return GOGP_EARG;
  if (mw != REMOVE_W_SMALL && mw != REMOVE_W) return GOGP_EARG;
  if (kb0 < 0 || kb0 % TILE || kb1 < kb0 || kb1 % TILE || kb1 + TILE > ld) return GOGP_EARG;  // the block's rows of W: < ldw = ld
  if (snap_b0 < 0 || snap_nb < 0 || (int64_t)(snap_b0 + snap_nb) * TILE > ld) return GOGP_EARG;
  if (l_len < ld * ld || w_len < (int64_t)mw * ld || snap_len < (kb1 / TILE + 1) * (int64_t)(TILE * TILE) ||
      snap_len < (int64_t)(snap_b0 + snap_nb) * (TILE * TILE))
    return GOGP_EARG;
  return run(device, {io(L, l_len), io(snap, snap_len), io(W, w_len)}, [&](const Dev &d) {
    launch_remove_snap(0, d[0], ld, snap_b0, snap_nb, d[1]);
    for (int64_t kb = kb0; kb <= kb1; kb += TILE) launch_remove_block(0, d[0], ld, d[1], d[2], mw, kb, n1);
  });
}

extern "C" int gogp_test_bwd_panel(int device, int64_t rows16, const double *A, int64_t a_len, int64_t a_off, int64_t lda,
                                   const double *B, int64_t b_len, int64_t b_off, int64_t ldb, double *C, int64_t c_len,
                                   int64_t c_off, int64_t ldc, int64_t ncols, int64_t K, int tri, int sub) {
  if (!A || !B || !C || rows16 < 1 || rows16 > 4096 || ncols <= 0 || ncols % 64 || ncols > UP_NPAD_MAX) return GOGP_EARG;
  if (K <= 0 || K % 32 || K > UP_NPAD_MAX) return GOGP_EARG;
  // beyond 32 rows the kernel takes whole groups of 64 (common.h): A and C must hold them
  const int64_t rows = rows16 <= 2 ? 16 * rows16 : (rows16 + 3) / 4 * 64;
  if (!covers(a_len, a_off, lda, rows, K, 1, 0) || !covers(b_len, b_off, ldb, K, ncols, 1, 0) ||
      !covers(c_len, c_off, ldc, rows, ncols, 1, 0))
    return GOGP_EARG;
  return run(device, {rd(A, a_len), rd(B, b_len), io(C, c_len)}, [&](const Dev &d) {
    launch_bwd_panel(0, rows16, d[0] + a_off, lda, d[1] + b_off, ldb, d[2] + c_off, ldc, ncols, (int)K, tri != 0, sub != 0);
  });
}

extern "C" int gogp_test_pcov_slabs(int64_t npad, int64_t m, int ncu, int *cols_per_slab) {
  if (npad <= 0 || npad % PANEL || npad > (1 << 20) || m < 1 || m > GOGP_COV_MAX_M || ncu < 1 || ncu > 4096) return -1;
  return pcov_slabs(npad, m, ncu, cols_per_slab);
}

extern "C" int gogp_test_pcov(int device, const gogp_test_kparams *kparams, int ev, const double *Z, int64_t z_len, int64_t m,
                              const double *Vt, int64_t vt_len, int64_t ld, int64_t npad, int ncu, double *part,
                              int64_t part_len, double diag_add, double *out, int64_t out_len, int64_t mo, int64_t ldo) {
  if (!kparams || !Z || !out || !kparams_ok(kparams, 1, ard_dims_of(kparams), 0, 1, ev)) return GOGP_EARG;
  if (m < 1 || m > GOGP_COV_MAX_M || mo < m || mo > GOGP_COV_MAX_M || z_len < m * kparams->ndim) return GOGP_EARG;
  if (!covers(out_len, 0, ldo, mo, mo, 1, 0)) return GOGP_EARG;
  if (Vt) {
    int cps = 0;
    const int nslab = gogp_test_pcov_slabs(npad, m, ncu, &cps);
    const int64_t tiles = (m + 63) / 64, pairs = tiles * (tiles + 1) / 2;
    if (nslab < 1 || npad > UP_NPAD_MAX || ld % 2 || !covers(vt_len, 0, ld, m, npad, 1, 0)) return GOGP_EARG;  // 16-B loads
    if (!part || part_len < nslab * pairs * 4096) return GOGP_EARG;
  }
  const DevParams hp = to_dev(*kparams);
  // Vt and part may be NULL (the prior covariance alone): nothing is copied for them and the launcher gets nullptr
  return run(device, {rd(&hp, 1, sizeof hp), rd(Z, z_len), rd(Vt, vt_len), io(part, part_len), io(out, out_len)},
             [&](const Dev &d) {
               launch_pcov(0, d.as<DevParams>(0), d[1], m, d[2], ld, npad, ncu, d[3], diag_add, d[4], mo, ldo, ev != 0);
             });
}

// ---- multi_weight_kernel (multi.hip) through its product launcher (tests/test_multi_output_gpu.py).  The product keeps
// A^T with zero rows up to a multiple of 4, so the hook appends them to its device copy.
extern "C" int gogp_test_multi_weight(int device, const double *At, int64_t at_len, int64_t ld, int T, const double *Kinv,
                                      int64_t kinv_len, int64_t ldk, int64_t n, int64_t npad, double *G, int64_t g_len) {
  if (!At || !Kinv || !G || T < 1 || T > GOGP_MULTI_MAX_T) return GOGP_EARG;
  if (npad <= 0 || npad % PANEL || npad > UP_NPAD_MAX || n < 1 || n > npad) return GOGP_EARG;
  if (!covers(at_len, 0, ld, T, npad, 1, 0) || !covers(kinv_len, 0, ldk, npad, npad, 1, 0) ||
      !covers(g_len, 0, ldk, npad, npad, 1, 0))
    return GOGP_EARG;
  const int T4 = (T + 3) / 4 * 4;
  const size_t at_bytes = (size_t)std::max<int64_t>(at_len, (int64_t)T4 * ld) * sizeof(double);
  // (the rows of the caller's array: T of them, the last one possibly shorter than ld; zeros behind them)
  const Arr A = padded(rd(At, std::min<int64_t>(at_len, (int64_t)T * ld)), at_bytes, 0);
  return run(device, {A, rd(Kinv, kinv_len), io(G, g_len)}, [&](const Dev &d) {
    launch_multi_weight(0, d[0], ld, T, d[1], ldk, n, npad, (double)T, d[2]);
  });
}

// ---- sparse_syrk_kernel and sparse_grad_kernel (sparse.hip) through their product launchers
// (tests/test_sparse_gpu.py).
extern "C" int gogp_test_sparse_syrk(int device, const double *Vt, int64_t vt_len, int64_t ld, int64_t rows, int64_t M,
                                     int64_t Mp, const double *y, int64_t y_len, double *Bacc, int64_t b_len, int64_t ldb,
                                     double *r, int64_t r_len) {
  if (!Vt || !y || !Bacc || !r) return GOGP_EARG;
  if (Mp <= 0 || Mp % 64 || Mp > GOGP_SPARSE_MAX_M || M < 1 || M > Mp || rows < 1 || rows > (1 << 16)) return GOGP_EARG;
  if (!covers(vt_len, 0, ld, rows, Mp, 1, 0) || !covers(b_len, 0, ldb, Mp, Mp, 1, 0) || y_len < rows || r_len < Mp)
    return GOGP_EARG;
  return run(device, {rd(Vt, vt_len), rd(y, y_len), io(Bacc, b_len), io(r, r_len)},
             [&](const Dev &d) { launch_sparse_syrk(0, d[0], ld, rows, M, Mp, d[1], d[2], ldb, d[3]); });
}

extern "C" int gogp_test_sparse_grad(int device, const gogp_test_kparams *kparams, const double *X, int64_t x_len, int64_t rows,
                                     const double *U, int64_t u_len, int64_t M, const double *Wt, int64_t wt_len, int64_t ldw,
                                     const double *y, int64_t y_len, const double *mvec, int64_t m_len, double s4,
                                     int accumulate, double *out /* GOGP_TEST_NACC */) {
  if (!kparams || !X || !U || !Wt || !y || !mvec || !out) return GOGP_EARG;
  if (!kparams_ok(kparams, 1, ard_dims_of(kparams), 0, 1, 0) || kparams->nevents != 0) return GOGP_EARG;
  if (rows < 1 || rows > (1 << 16) || M < 1 || M > GOGP_SPARSE_MAX_M || !std::isfinite(s4)) return GOGP_EARG;
  if (x_len < rows * kparams->ndim || u_len < M * kparams->ndim || y_len < rows || m_len < M) return GOGP_EARG;
  if (!covers(wt_len, 0, ldw, rows, M, 1, 0)) return GOGP_EARG;
  const DevParams hp = to_dev(*kparams);
  return run(device, {rd(&hp, 1, sizeof hp), rd(X, x_len), rd(U, u_len), rd(Wt, wt_len), rd(y, y_len), rd(mvec, m_len),
                      io(out, NACC), scratch((size_t)sparse_grad_blocks(rows, M) * NACC * sizeof(double))},
             [&](const Dev &d) {
               launch_sparse_grad(0, d.as<DevParams>(0), kparams->ndim, ard_dims_of(kparams), d[1], rows, d[2], M, d[3], ldw,
                                  d[4], d[5], s4, d[7], d[6], accumulate != 0);
             });
}

extern "C" int gogp_test_sparse_ugrad_slabs(int64_t rows, int64_t M, int *tiles_per_slab) {
  if (rows < 1 || rows > (1 << 16) || M < 1 || M > GOGP_SPARSE_MAX_M) return 0;
  return sparse_ugrad_slabs(rows, M, tiles_per_slab);
}

extern "C" int gogp_test_sparse_ugrad_slabs_bound(int64_t rows, int64_t M) {
  if (rows < 1 || rows > (1 << 16) || M < 1 || M > GOGP_SPARSE_MAX_M) return 0;
  return sparse_ugrad_slabs_bound(rows, M);
}

extern "C" int gogp_test_sparse_ugrad(int device, const gogp_test_kparams *kparams, const double *X, int64_t x_len, int64_t rows,
                                      const double *U, int64_t u_len, int64_t M, const double *Wt, int64_t wt_len, int64_t ldw,
                                      const double *y, int64_t y_len, const double *mvec, int64_t m_len, double s4,
                                      int accumulate, double *dU, int64_t du_len) {
  if (!kparams || !X || !U || !Wt || !y || !mvec || !dU) return GOGP_EARG;
  if (!kparams_ok(kparams, 1, ard_dims_of(kparams), 0, 1, 0) || kparams->nevents != 0) return GOGP_EARG;
  if (rows < 1 || rows > (1 << 16) || M < 1 || M > GOGP_SPARSE_MAX_M || !std::isfinite(s4)) return GOGP_EARG;
  if (x_len < rows * kparams->ndim || u_len < M * kparams->ndim || y_len < rows || m_len < M || du_len < M * kparams->ndim)
    return GOGP_EARG;
  if (!covers(wt_len, 0, ldw, rows, M, 1, 0)) return GOGP_EARG;
  const DevParams hp = to_dev(*kparams);
  const size_t part_bytes = (size_t)sparse_ugrad_slabs(rows, M, nullptr) * (size_t)M * kparams->ndim * sizeof(double);
  return run(device, {rd(&hp, 1, sizeof hp), rd(X, x_len), rd(U, u_len), rd(Wt, wt_len), rd(y, y_len), rd(mvec, m_len),
                      io(dU, du_len), scratch(part_bytes)},
             [&](const Dev &d) {
               launch_sparse_ugrad(0, d.as<DevParams>(0), kparams->ndim, d[1], rows, d[2], M, d[3], ldw, d[4], d[5], s4, d[7],
                                   d[6], accumulate != 0);
             });
}

// launch_sparse_xty on host arrays: R (in / out) += Y^T Vt.  The partials are sized as the product sizes them.
extern "C" int gogp_test_sparse_xty(int device, const double *Vt, int64_t vt_len, int64_t ld, int64_t rows, int64_t M,
                                    int64_t Mp, const double *Y, int64_t y_len, int64_t ldy, int64_t T, double *R,
                                    int64_t r_len, int64_t ldr) {
  if (!Vt || !Y || !R) return GOGP_EARG;
  if (Mp <= 0 || Mp % 64 || Mp > GOGP_SPARSE_MAX_M || M < 1 || M > Mp || rows < 1 || rows > (1 << 16)) return GOGP_EARG;
  if (T < 1 || T > GOGP_SPARSE_MULTI_MAX_T) return GOGP_EARG;
  const int64_t tt = (T + 63) / 64 * 64, mc = (M + 63) / 64 * 64;
  if (!covers(vt_len, 0, ld, rows, M, 1, 0) || !covers(y_len, 0, ldy, rows, T, 1, 0) || !covers(r_len, 0, ldr, tt, mc, 1, 0))
    return GOGP_EARG;
  const size_t part_bytes = sparse_xty_part_doubles(rows, M, T) * sizeof(double);
  return run(device, {rd(Vt, vt_len), rd(Y, y_len), io(R, r_len), scratch(part_bytes)},
             [&](const Dev &d) { launch_sparse_xty(0, d[0], ld, rows, M, d[1], ldy, T, d[3], d[2], ldr); });
}

extern "C" int gogp_test_sparse_xty_slabs(int64_t rows, int64_t M, int64_t T, int64_t *rows_per_slab) {
  if (rows < 1 || rows > (1 << 16) || M < 1 || M > GOGP_SPARSE_MAX_M || T < 1 || T > GOGP_SPARSE_MULTI_MAX_T) return 0;
  return sparse_xty_slabs(rows, M, T, rows_per_slab);
}

extern "C" int gogp_test_sparse_xty_slabs_bound(int64_t rows, int64_t M, int64_t T) {
  if (rows < 1 || rows > (1 << 16) || M < 1 || M > GOGP_SPARSE_MAX_M || T < 1 || T > GOGP_SPARSE_MULTI_MAX_T) return 0;
  return sparse_xty_slabs_bound(rows, M, T);
}

// ---- greedy selection of inducing points (select.hip; tests/test_select_inducing_kernels.py) ----------------------------
namespace {
constexpr int64_t SEL_N_MAX = 1 << 22;
bool select_args_ok(const gogp_test_kparams *kp, int64_t x_len, int64_t N, double tol, int max_blocks) {
  if (!kp || !kparams_ok(kp, 1, ard_dims_of(kp), 0, 1, 0) || kp->nevents != 0) return false;
  if (N < 1 || N > SEL_N_MAX || x_len < N * kp->ndim) return false;
  return std::isfinite(tol) && tol >= 0.0 && max_blocks >= 0;
}
}  // namespace

extern "C" int gogp_test_select_step(int device, const gogp_test_kparams *kparams, const double *X, int64_t x_len, int64_t N,
                                     double *Lt, int64_t lt_len, int64_t ldn, int64_t j, double tol, double *d, int64_t d_len,
                                     unsigned char *sel, int64_t sel_len, const double *part_v, const int64_t *part_i,
                                     int64_t part_len, int max_blocks, double *out_v, int64_t *out_i, int64_t out_len,
                                     int64_t *p, double *dp) {
  if (!X || !Lt || !d || !sel || !part_v || !part_i || !out_v || !out_i || !p || !dp) return GOGP_EARG;
  if (!select_args_ok(kparams, x_len, N, tol, max_blocks)) return GOGP_EARG;
  if (j < 0 || j >= GOGP_SPARSE_MAX_M || ldn < N || ldn % 256 || lt_len < (j + 1) * ldn || d_len < N || sel_len < N)
    return GOGP_EARG;
  const int blocks = select_blocks(N, max_blocks);
  if (part_len != blocks || out_len < blocks) return GOGP_EARG;
  for (int q = 0; q < blocks; ++q)
    if (part_i[q] < 0 || part_i[q] >= N) return GOGP_EARG;  // the kernel reads row part_i of X and of the factor
  const DevParams hp = to_dev(*kparams);
  const int D = kparams->ndim;
  // the select_layout work area is packed on the host, travels as one in / out array and is unpacked afterwards
  SelectBufs b;
  const size_t small = select_layout(nullptr, N, j + 1, D, &b);
  std::vector<char> work(small, 0);
  select_layout(work.data(), N, j + 1, D, &b);
  memcpy(b.d, d, (size_t)N * sizeof(double));
  memcpy(b.sel, sel, (size_t)N);
  SelPair *pin = b.part + (size_t)(j & 1) * SELECT_BLOCKS_MAX;
  for (int q = 0; q < blocks; ++q) pin[q].v = part_v[q], pin[q].i = part_i[q];
  for (int64_t t = 0; t <= j; ++t) b.piv[t] = t < j ? 0 : -1;  // the earlier steps recorded pivots
  const int rc = run(device, {rd(&hp, 1, sizeof hp), rd(X, x_len), io(Lt, lt_len), io(work.data(), (int64_t)small, 1)},
                     [&](const Dev &dv) {
                       SelectBufs db;
                       select_layout(dv.as<char>(3), N, j + 1, D, &db);
                       db.Lt = dv[2];
                       db.ldn = ldn;
                       launch_select_step(0, dv.as<DevParams>(0), D, dv[1], N, blocks, (int)j, tol, db);
                     });
  if (rc != GOGP_OK) return rc;
  memcpy(d, b.d, (size_t)N * sizeof(double));
  memcpy(sel, b.sel, (size_t)N);
  const SelPair *pout = b.part + (size_t)((j + 1) & 1) * SELECT_BLOCKS_MAX;
  *p = b.piv[j];
  *dp = b.pv[j];
  for (int q = 0; q < blocks && *p >= 0; ++q) out_v[q] = pout[q].v, out_i[q] = pout[q].i;
  return GOGP_OK;
}

extern "C" int gogp_test_select_run(int device, const gogp_test_kparams *kparams, const double *X, int64_t x_len, int64_t N,
                                    int64_t M, double tol, int max_blocks, const double *d0, int64_t d0_len, int64_t *idx,
                                    double *pivots, double *U, int64_t u_len, double *Lt, int64_t lt_len, double *d,
                                    int64_t d_len, int64_t *m_out, double *trace) {
  if (!X || !idx || !pivots || !m_out || !trace) return GOGP_EARG;
  if (!select_args_ok(kparams, x_len, N, tol, max_blocks)) return GOGP_EARG;
  if (M < 1 || M > GOGP_SPARSE_MAX_M) return GOGP_EARG;
  const int D = kparams->ndim;
  SelectBufs b;
  const size_t small = select_layout(nullptr, N, M, D, &b);
  const int64_t cols = std::min(M, N);
  if ((d0 && d0_len < N) || (U && u_len < M * D) || (Lt && lt_len < cols * b.ldn) || (d && d_len < N)) return GOGP_EARG;
  if (!device_ok(device)) return GOGP_EHIP;
  // not on run(): select_run is the product's whole loop, which returns its own error and the count m, and the results
  // are the first m entries of pieces of its device work area, not copies of host arrays
  const DevParams hp = to_dev(*kparams);
  DevCopy dP, dX, d0c, work, dL;
  const size_t lbytes = (size_t)cols * (size_t)b.ldn * sizeof(double);
  hipError_t e = dP.up(&hp, sizeof hp);
  if (e == hipSuccess) e = dX.up(X, (size_t)x_len * sizeof(double));
  if (e == hipSuccess && d0) e = d0c.up(d0, (size_t)d0_len * sizeof(double));
  if (e == hipSuccess) e = work.up(nullptr, 0, small);
  if (e == hipSuccess) e = dL.up(nullptr, 0, lbytes, 0xff);  // NaN: what no step wrote shows
  int64_t m = 0;
  if (e == hipSuccess) {
    select_layout(work.d, N, M, D, &b);
    b.Lt = dL.as<double>();
    e = select_run(0, dP.as<DevParams>(), D, dX.as<double>(), N, M, tol, max_blocks, d0c.as<double>(), b, &m);
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  std::vector<long long> hpiv((size_t)M);
  if (e == hipSuccess) e = hipMemcpy(hpiv.data(), b.piv, (size_t)M * sizeof(long long), hipMemcpyDeviceToHost);
  if (e == hipSuccess && m > 0) e = hipMemcpy(pivots, b.pv, (size_t)m * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess && U && m > 0) e = hipMemcpy(U, b.U, (size_t)m * D * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess && Lt) e = hipMemcpy(Lt, dL.d, lbytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess && d) e = hipMemcpy(d, b.d, (size_t)N * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(trace, b.trace, sizeof(double), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return GOGP_EHIP;
  for (int64_t t = 0; t < m; ++t) idx[t] = (int64_t)hpiv[(size_t)t];
  *m_out = m;
  return GOGP_OK;
}

// ---- the small kernels that finish leave-one-out, multi-output and sparse evaluations, through their product launchers
// (tests/test_finish_kernels.py): the kernels of loo.hip, multi_dots_kernel (multi.hip) and the element-wise, scalar and
// Produce kernels of sparse.hip.
namespace {
bool fin_npad_ok(int64_t n, int64_t npad) {
  return npad > 0 && npad % PANEL == 0 && npad <= UP_NPAD_MAX && n >= 1 && n <= npad;
}
// the Mp x Mp element-wise launchers start Mp / 256 workgroups per row: any other Mp would drop columns silently
bool fin_mp_ok(int64_t Mp) { return Mp > 0 && Mp % 256 == 0 && Mp <= GOGP_SPARSE_MAX_M; }
constexpr int64_t FIN_ROWS_MAX = 1 << 24;   // rows of the sums of squares
constexpr int64_t FIN_M_MAX = 4 * 65535;    // test points of the Produce kernels: one wave each, four per workgroup
}  // namespace

extern "C" int gogp_test_loo_stats(int device, const double *Kinv, int64_t kinv_len, int64_t ld, const double *alpha,
                                   int64_t alpha_len, const double *y, int64_t y_len, int64_t n, int64_t npad, double *mu,
                                   int64_t mu_len, double *sigma, int64_t sigma_len, double *logp, int64_t logp_len, double *v,
                                   int64_t v_len, double *sc, int64_t sc_len, double *part, int64_t part_len) {
  const std::vector<Arr> arrs = {rd(Kinv, kinv_len), rd(alpha, alpha_len), rd(y, y_len),
                                           io(mu, mu_len),     io(sigma, sigma_len), io(logp, logp_len),
                                           io(v, v_len),       io(sc, sc_len),       io(part, part_len)};
  if (!have(arrs) || !fin_npad_ok(n, npad) || !covers(kinv_len, 0, ld, npad, npad, 1, 0)) return GOGP_EARG;
  if (alpha_len < n || y_len < n || mu_len < n || sigma_len < n || logp_len < n) return GOGP_EARG;
  if (v_len < npad || sc_len < npad || part_len < npad / PANEL) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    launch_loo_stats(0, d[0], ld, d[1], d[2], n, npad, d[3], d[4], d[5], d[6], d[7], d[8]);
  });
}

extern "C" int gogp_test_loo_scale_symv(int device, const double *Kinv, int64_t kinv_len, int64_t ld, int64_t n, int64_t npad,
                                        const double *sc, int64_t sc_len, const double *v, int64_t v_len, double *B,
                                        int64_t b_len, int64_t ldb, double *upart, int64_t upart_len, double *u,
                                        int64_t u_len) {
  const std::vector<Arr> arrs = {rd(Kinv, kinv_len), rd(sc, sc_len),       rd(v, v_len),
                                           io(B, b_len),       io(upart, upart_len), io(u, u_len)};
  if (!have(arrs) || !fin_npad_ok(n, npad)) return GOGP_EARG;
  if (!covers(kinv_len, 0, ld, npad, npad, 1, 0) || !covers(b_len, 0, ldb, npad, npad, 1, 0)) return GOGP_EARG;
  if (sc_len < npad || v_len < npad || u_len < npad || upart_len < npad / 64 * npad) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    launch_loo_scale_symv(0, d[0], ld, n, npad, d[1], d[2], d[3], ldb, d[4], d[5]);
  });
}

extern "C" int gogp_test_loo_rank2(int device, double *G, int64_t g_len, int64_t ld, int64_t n, int64_t npad, const double *u,
                                   int64_t u_len, const double *alpha, int64_t alpha_len) {
  const std::vector<Arr> arrs = {io(G, g_len), rd(u, u_len), rd(alpha, alpha_len)};
  if (!have(arrs) || !fin_npad_ok(n, npad) || !covers(g_len, 0, ld, npad, npad, 1, 0)) return GOGP_EARG;
  if (u_len < npad || alpha_len < n) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_loo_rank2(0, d[0], ld, n, npad, d[1], d[2]); });
}

// ---- the two kernels of leave-block-out cross-validation (blockcv.hip; tests/test_blockcv_kernels.py) ------------------
namespace {
// the block and group tables of `start` (checked), packed as api.hip lays them out on the device: [F + 1 starts | ngroups
// + 1 firsts]; they travel as one read-only array
std::vector<int64_t> bcv_tables(const int64_t *start, int64_t F, int *ngroups) {
  std::vector<int64_t> tab((size_t)(2 * F + 3));
  for (int64_t f = 0; f <= F; ++f) tab[(size_t)f] = start[f];
  *ngroups = blockcv_pack(start, F, tab.data() + F + 1);
  tab.resize((size_t)(F + 1 + *ngroups + 1));
  return tab;
}
}  // namespace

extern "C" int gogp_test_blockcv_groups(int device, const double *Kinv, int64_t kinv_len, int64_t ld, const double *alpha,
                                        int64_t alpha_len, const double *y, int64_t y_len, int64_t n, const int64_t *start,
                                        int64_t F, double *mu, int64_t mu_len, double *sigma, int64_t sigma_len, double *v,
                                        int64_t v_len, double *ones, int64_t ones_len, double *logp, int64_t logp_len,
                                        double *Sg, int64_t sg_len, int64_t *info, int64_t info_len) {
  std::vector<Arr> arrs = {rd(Kinv, kinv_len), rd(alpha, alpha_len), rd(y, y_len),       io(mu, mu_len), io(sigma, sigma_len),
                           io(v, v_len),       io(ones, ones_len),   io(logp, logp_len), io(Sg, sg_len)};
  if (!have(arrs) || !info || n < 1 || n > UP_NPAD_MAX || F < 1 || gogp_blockcv_check(start, F, n) != GOGP_OK)
    return GOGP_EARG;
  if (!covers(kinv_len, 0, ld, n, n, 1, 0) || alpha_len < n || y_len < n) return GOGP_EARG;
  if (mu_len < n || sigma_len < n || v_len < n || ones_len < n || logp_len < F) return GOGP_EARG;
  int ng = 0;
  const std::vector<int64_t> tab = bcv_tables(start, F, &ng);
  if (sg_len < (int64_t)ng * 128 * 128 || info_len < ng) return GOGP_EARG;
  arrs.push_back(rd(tab.data(), (int64_t)tab.size()));
  arrs.push_back(io(info, info_len));
  return run(device, arrs, [&](const Dev &d) {
    const int64_t *dt = d.as<int64_t>(9);
    launch_blockcv_groups(0, d[0], ld, d[1], d[2], dt, dt + F + 1, ng, d[3], d[4], d[5], d[6], d[7], d[8], d.as<long long>(10));
  });
}

extern "C" int gogp_test_blockcv_apply(int device, double *Q, int64_t q_len, int64_t q_off, int64_t ld, int64_t rows, int64_t n,
                                       const int64_t *start, int64_t F, const double *Sg, int64_t sg_len) {
  std::vector<Arr> arrs = {io(Q, q_len), rd(Sg, sg_len)};
  if (!have(arrs) || n < 1 || n > UP_NPAD_MAX || F < 1 || gogp_blockcv_check(start, F, n) != GOGP_OK) return GOGP_EARG;
  if (rows % 64 || rows < n || !covers(q_len, q_off, ld, rows, n, 1, 0)) return GOGP_EARG;
  int ng = 0;
  const std::vector<int64_t> tab = bcv_tables(start, F, &ng);
  if (sg_len < (int64_t)ng * 128 * 128) return GOGP_EARG;
  arrs.push_back(rd(tab.data(), (int64_t)tab.size()));
  return run(device, arrs, [&](const Dev &d) {
    const int64_t *dt = d.as<int64_t>(2);
    launch_blockcv_apply(0, d[0] + q_off, ld, n, dt, dt + F + 1, ng, d[1]);
  });
}

extern "C" int gogp_test_multi_dots(int device, const double *Yt, int64_t yt_len, const double *At, int64_t at_len, int64_t ld,
                                    int64_t n, int T, double *dots, int64_t dots_len) {
  const std::vector<Arr> arrs = {rd(Yt, yt_len), rd(At, at_len), io(dots, dots_len)};
  if (!have(arrs) || T < 1 || T > GOGP_MULTI_MAX_T || n < 1 || n > UP_NPAD_MAX || dots_len < T) return GOGP_EARG;
  if (!covers(yt_len, 0, ld, T, n, 1, 0) || !covers(at_len, 0, ld, T, n, 1, 0)) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_multi_dots(0, d[0], d[1], ld, n, T, d[2]); });
}

extern "C" int gogp_test_sparse_finish_b(int device, const double *Bacc, int64_t bacc_len, int64_t Mp, double inv_s2, double *B,
                                         int64_t b_len) {
  const std::vector<Arr> arrs = {rd(Bacc, bacc_len), io(B, b_len)};
  if (!have(arrs) || !fin_mp_ok(Mp) || !std::isfinite(inv_s2) || bacc_len < Mp * Mp || b_len < Mp * Mp) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_sparse_finish_b(0, d[0], Mp, inv_s2, d[1]); });
}

extern "C" int gogp_test_sparse_copy_upper(int device, const double *src, int64_t src_len, int64_t Mp, double *dst,
                                           int64_t dst_len) {
  const std::vector<Arr> arrs = {rd(src, src_len), io(dst, dst_len)};
  if (!have(arrs) || !fin_mp_ok(Mp) || src_len < Mp * Mp || dst_len < Mp * Mp) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_sparse_copy_upper(0, d[0], Mp, d[1]); });
}

extern "C" int gogp_test_sparse_weights(int device, const double *B, int64_t b_len, const double *Binv, int64_t binv_len,
                                        const double *g, int64_t g_len, int64_t Mp, double s4, double *T, int64_t t_len,
                                        double *S, int64_t s_len) {
  const std::vector<Arr> arrs = {rd(B, b_len), rd(Binv, binv_len), rd(g, g_len), io(T, t_len), io(S, s_len)};
  if (!have(arrs) || !fin_mp_ok(Mp) || !std::isfinite(s4) || g_len < Mp) return GOGP_EARG;
  if (b_len < Mp * Mp || binv_len < Mp * Mp || t_len < Mp * Mp || s_len < Mp * Mp) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_sparse_weights(0, d[0], d[1], d[2], Mp, s4, d[3], d[4]); });
}

extern "C" int gogp_test_sparse_multi_weights(int device, const double *B, int64_t b_len, const double *Binv, int64_t binv_len,
                                              const double *GG, int64_t gg_len, int64_t Mp, int T, double s4, double *Tm,
                                              int64_t tm_len, double *S, int64_t s_len) {
  const std::vector<Arr> arrs = {rd(B, b_len), rd(Binv, binv_len), rd(GG, gg_len), io(Tm, tm_len), io(S, s_len)};
  if (!have(arrs) || !fin_mp_ok(Mp) || !std::isfinite(s4) || T < 1 || T > GOGP_SPARSE_MULTI_MAX_T) return GOGP_EARG;
  if (b_len < Mp * Mp || binv_len < Mp * Mp || gg_len < Mp * Mp || tm_len < Mp * Mp || s_len < Mp * Mp) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_sparse_multi_weights(0, d[0], d[1], d[2], Mp, T, s4, d[3], d[4]); });
}

extern "C" int gogp_test_sparse_scalars(int device, const double *C, int64_t c_len, const double *B, int64_t b_len,
                                        const double *Binv, int64_t binv_len, const double *r, int64_t r_len, const double *g,
                                        int64_t g_len, int64_t M, int64_t Mp, double *out, int64_t out_len) {
  const std::vector<Arr> arrs = {rd(C, c_len), rd(B, b_len), rd(Binv, binv_len), rd(r, r_len), rd(g, g_len), io(out, out_len)};
  if (!have(arrs) || M < 1 || M > Mp || Mp > GOGP_SPARSE_MAX_M || r_len < M || g_len < M || out_len < 5) return GOGP_EARG;
  if (!covers(c_len, 0, Mp, M, M, 1, 0) || !covers(b_len, 0, Mp, M, M, 1, 0) || !covers(binv_len, 0, Mp, M, M, 1, 0))
    return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_sparse_scalars(0, d[0], d[1], d[2], d[3], d[4], M, Mp, d[5]); });
}

extern "C" int gogp_test_sparse_sumsq(int device, const double *y, int64_t y_len, int64_t n, double *out, int64_t out_len) {
  const std::vector<Arr> arrs = {rd(y, y_len), io(out, out_len)};
  if (!have(arrs) || n < 1 || n > FIN_ROWS_MAX || y_len < n) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_sparse_sumsq(0, d[0], n, d[1]); });
}

extern "C" int gogp_test_sparse_predict(int device, const double *A, int64_t a_len, const double *V, int64_t v_len, int64_t ld,
                                        int64_t ncols, int64_t m, const double *prior, int64_t prior_len, const double *q,
                                        int64_t q_len, const double *dot, int64_t dot_len, double inv_s2, double *mu,
                                        int64_t mu_len, double *sigma, int64_t sigma_len) {
  const std::vector<Arr> arrs = {rd(A, a_len),     rd(V, v_len),   rd(prior, prior_len),   rd(q, q_len),
                                 rd(dot, dot_len), io(mu, mu_len), io(sigma, sigma_len)};
  if (!have(arrs) || m < 1 || m > FIN_M_MAX || !std::isfinite(inv_s2)) return GOGP_EARG;
  if (!covers(a_len, 0, ld, m, ncols, 1, 0) || !covers(v_len, 0, ld, m, ncols, 1, 0)) return GOGP_EARG;
  if (prior_len < m || q_len < m || dot_len < m || mu_len < m || sigma_len < m) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    launch_sparse_predict(0, d[0], d[1], ld, ncols, m, d[2], d[3], d[4], inv_s2, d[5], d[6]);
  });
}

extern "C" int gogp_test_sparse_multi_dots(int device, const double *Rt, int64_t rt_len, const double *Gt, int64_t gt_len,
                                           int64_t ld, int64_t M, int T, int tstride, double *out, int64_t out_len) {
  const std::vector<Arr> arrs = {rd(Rt, rt_len), rd(Gt, gt_len), io(out, out_len)};
  if (!have(arrs) || M < 1 || M > GOGP_SPARSE_MAX_M || T < 1 || T > GOGP_SPARSE_MULTI_MAX_T) return GOGP_EARG;
  if (tstride < T || out_len < (int64_t)tstride + T) return GOGP_EARG;
  if (!covers(rt_len, 0, ld, T, M, 1, 0) || !covers(gt_len, 0, ld, T, M, 1, 0)) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_sparse_multi_dots(0, d[0], d[1], ld, M, T, tstride, d[2]); });
}

extern "C" int gogp_test_sparse_multi_sumsq(int device, const double *Y, int64_t y_len, int64_t ldy, int64_t n, int T,
                                            double *out, int64_t out_len) {
  const std::vector<Arr> arrs = {rd(Y, y_len), io(out, out_len)};
  if (!have(arrs) || n < 1 || n > FIN_ROWS_MAX || T < 1 || T > GOGP_SPARSE_MULTI_MAX_T || out_len < T) return GOGP_EARG;
  if (!covers(y_len, 0, ldy, n, T, 1, 0)) return GOGP_EARG;  // (ldy < T is refused here)
  return run(device, arrs, [&](const Dev &d) { launch_sparse_multi_sumsq(0, d[0], ldy, n, T, d[1]); });
}

extern "C" int gogp_test_sparse_multi_pad(int device, const double *Y, int64_t y_len, int64_t ldy, int64_t rows, int64_t T,
                                          int64_t kp, int64_t rpad, double *Yp, int64_t yp_len, int64_t ldp) {
  const std::vector<Arr> arrs = {rd(Y, y_len), io(Yp, yp_len)};
  if (!have(arrs) || rpad < 1 || rpad > (1 << 16) || kp < 1 || kp > (1 << 12) || rows < 1 || rows > rpad || T < 1 || T > kp)
    return GOGP_EARG;
  if ((rpad * kp) % 256) return GOGP_EARG;  // the launcher starts whole workgroups of 256 elements or none at all
  if (!covers(y_len, 0, ldy, rows, T, 1, 0) || !covers(yp_len, 0, ldp, rpad, kp, 1, 0)) return GOGP_EARG;  // ldy < T, ldp < kp
  return run(device, arrs, [&](const Dev &d) { launch_sparse_multi_pad(0, d[0], ldy, rows, T, kp, rpad, d[1], ldp); });
}

extern "C" int gogp_test_sparse_multi_sigma(int device, const double *A, int64_t a_len, const double *V, int64_t v_len,
                                            int64_t ld, int64_t ncols, int64_t m, const double *prior, int64_t prior_len,
                                            const double *q, int64_t q_len, double *sigma, int64_t sigma_len) {
  const std::vector<Arr> arrs = {rd(A, a_len), rd(V, v_len), rd(prior, prior_len), rd(q, q_len), io(sigma, sigma_len)};
  if (!have(arrs) || m < 1 || m > FIN_M_MAX) return GOGP_EARG;
  if (!covers(a_len, 0, ld, m, ncols, 1, 0) || !covers(v_len, 0, ld, m, ncols, 1, 0)) return GOGP_EARG;
  if (prior_len < m || q_len < m || sigma_len < m) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    launch_sparse_multi_sigma(0, d[0], d[1], ld, ncols, m, d[2], d[3], d[4]);
  });
}

// Benchmark hook for launch_sparse_xty (the kernel and its ordered final sum): `reps` launches on device buffers (Vt: rows
// x Mp, Mp = M rounded up to 256; Y: rows x T); ms per launch and TFLOP/s on 2 rows M T flops
extern "C" int gogp_bench_sparse_xty(int device, int64_t rows, int64_t M, int64_t T, int reps, double *ms_per_launch,
                                     double *tflops) {
  if (rows < 1 || rows > (1 << 16) || M < 1 || M > GOGP_SPARSE_MAX_M || T < 1 || T > GOGP_SPARSE_MULTI_MAX_T || reps < 1)
    return GOGP_EARG;
  if (!device_ok(device)) return GOGP_EHIP;
  const int64_t Mp = (M + PANEL - 1) / PANEL * PANEL;
  double *dV = nullptr, *dY = nullptr, *dR = nullptr, *dP = nullptr;
  hipError_t e = hipMalloc(&dV, (size_t)rows * Mp * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&dY, (size_t)rows * T * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&dR, (size_t)GOGP_SPARSE_MULTI_MAX_T * Mp * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&dP, sparse_xty_part_doubles(rows, M, T) * sizeof(double));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  float ms = 0.f;
  if (e == hipSuccess) {
    launch_fill(0, dV, rows * Mp, 0.5);
    launch_fill(0, dY, rows * T, 0.25);
    launch_fill(0, dR, GOGP_SPARSE_MULTI_MAX_T * Mp, 0.0);
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    for (int w = 0; w < 2; ++w) launch_sparse_xty(0, dV, Mp, rows, M, dY, T, T, dP, dR, Mp);
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0, 0);
    for (int r = 0; r < reps; ++r) launch_sparse_xty(0, dV, Mp, rows, M, dY, T, T, dP, dR, Mp);
    (void)hipEventRecord(e1, 0);
    e = hipEventSynchronize(e1);
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  (void)hipFree(dV);
  (void)hipFree(dY);
  (void)hipFree(dR);
  (void)hipFree(dP);
  if (e != hipSuccess) return e == hipErrorOutOfMemory ? GOGP_ENOMEM : GOGP_EHIP;
  if (ms_per_launch) *ms_per_launch = ms / reps;
  if (tflops) *tflops = 2.0 * (double)rows * (double)M * (double)T * reps / (ms * 1e-3) / 1e12;
  return GOGP_OK;
}

// Benchmark hook for sparse_syrk_kernel: `reps` launches on device buffers (Vt: rows x Mp, Mp = M rounded up to 256);
// ms per launch and TFLOP/s on the flops of the lower 64-tiles
extern "C" int gogp_bench_sparse_syrk(int device, int64_t rows, int64_t M, int reps, double *ms_per_launch, double *tflops) {
  if (rows < 1 || rows > (1 << 16) || M < 1 || M > GOGP_SPARSE_MAX_M || reps < 1) return GOGP_EARG;
  if (!device_ok(device)) return GOGP_EHIP;
  const int64_t Mp = (M + PANEL - 1) / PANEL * PANEL;
  double *dV = nullptr, *dy = nullptr, *dB = nullptr, *dr = nullptr;
  hipError_t e = hipMalloc(&dV, (size_t)rows * Mp * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&dy, (size_t)rows * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&dB, (size_t)Mp * Mp * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&dr, (size_t)Mp * sizeof(double));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  float ms = 0.f;
  if (e == hipSuccess) {
    launch_fill(0, dV, rows * Mp, 0.5);
    launch_fill(0, dy, rows, 0.25);
    launch_fill(0, dB, Mp * Mp, 0.0);
    launch_fill(0, dr, Mp, 0.0);
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    for (int w = 0; w < 2; ++w) launch_sparse_syrk(0, dV, Mp, rows, M, Mp, dy, dB, Mp, dr);
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0, 0);
    for (int r = 0; r < reps; ++r) launch_sparse_syrk(0, dV, Mp, rows, M, Mp, dy, dB, Mp, dr);
    (void)hipEventRecord(e1, 0);
    e = hipEventSynchronize(e1);
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  (void)hipFree(dV);
  (void)hipFree(dy);
  (void)hipFree(dB);
  (void)hipFree(dr);
  if (e != hipSuccess) return e == hipErrorOutOfMemory ? GOGP_ENOMEM : GOGP_EHIP;
  const int64_t nt = Mp / 64;
  const double flops = (double)(nt * (nt + 1) / 2) * 64.0 * 64.0 * 2.0 * (double)rows * reps;
  if (ms_per_launch) *ms_per_launch = ms / reps;
  if (tflops) *tflops = flops / (ms * 1e-3) / 1e12;
  return GOGP_OK;
}

// ---- the kernels of the Laplace approximation (laplace.hip; tests/test_laplace_kernels.py) --------------------------------
namespace {
bool lap_lik_known(int lik) { return lik == GOGP_LIK_BERNOULLI_LOGIT || lik == GOGP_LIK_POISSON_LOG; }
}  // namespace

extern "C" int gogp_test_lap_site(int device, int lik, const double *f, int64_t f_len, const double *y, int64_t y_len,
                                  const double *a, int64_t a_len, int64_t n, int64_t npad, double *g, int64_t g_len,
                                  double *W, int64_t w_len, double *sw, int64_t sw_len, double *b, int64_t b_len, double *rho,
                                  int64_t rho_len, double *part, int64_t part_len, double *out, int64_t out_len) {
  const std::vector<Arr> arrs = {rd(f, f_len),   rd(y, y_len), rd(a, a_len),     io(g, g_len),       io(W, w_len),
                                 io(sw, sw_len), io(b, b_len), io(rho, rho_len), io(part, part_len), io(out, out_len)};
  if (!have(arrs) || !fin_npad_ok(n, npad) || !lap_lik_known(lik)) return GOGP_EARG;
  if (f_len < n || y_len < n || a_len < n) return GOGP_EARG;
  if (g_len < npad || w_len < npad || sw_len < npad || b_len < npad || rho_len < npad) return GOGP_EARG;
  if (part_len < 5 * (npad / PANEL) || out_len < 5) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    launch_lap_site(0, lik, d[0], d[1], d[2], n, npad, d[3], d[4], d[5], d[6], d[7], d[8], d[9]);
  });
}

extern "C" int gogp_test_lap_scale_gram(int device, double *A, int64_t a_len, int64_t ld, int64_t n, int64_t npad,
                                        const double *sw, int64_t sw_len, int64_t wcols) {
  const std::vector<Arr> arrs = {io(A, a_len), rd(sw, sw_len)};
  if (!have(arrs) || !fin_npad_ok(n, npad) || !covers(a_len, 0, ld, npad, npad, 1, 0)) return GOGP_EARG;
  if (sw_len < n || wcols < 0 || wcols % 64) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_lap_scale_gram(0, 0, d[0], ld, n, npad, d[1], wcols); });
}

extern "C" int gogp_test_lap_step(int device, const double *b, int64_t b_len, const double *sw, int64_t sw_len,
                                  const double *beta, int64_t beta_len, int64_t n, int64_t npad, double *rhs, int64_t rhs_len,
                                  double *a1, int64_t a1_len) {
  const std::vector<Arr> arrs = {rd(b, b_len), rd(sw, sw_len), rd(beta, beta_len), io(rhs, rhs_len), io(a1, a1_len)};
  if (!have(arrs) || !fin_npad_ok(n, npad)) return GOGP_EARG;
  if (b_len < n || sw_len < n || beta_len < n || rhs_len < npad || a1_len < npad) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    launch_lap_vec(0, nullptr, d[1], d[2], n, npad, d[3]);  // rhs = sw o beta
    launch_lap_vec(0, d[0], d[1], d[2], n, npad, d[4]);     // a1 = b - sw o beta
  });
}

extern "C" int gogp_test_lap_interp(int device, const double *a, int64_t a_len, const double *a1, int64_t a1_len,
                                    const double *f, int64_t f_len, const double *f1, int64_t f1_len, double t, int64_t n,
                                    int64_t npad, double *at, int64_t at_len, double *ft, int64_t ft_len) {
  const std::vector<Arr> arrs = {rd(a, a_len), rd(a1, a1_len), rd(f, f_len), rd(f1, f1_len), io(at, at_len), io(ft, ft_len)};
  if (!have(arrs) || !fin_npad_ok(n, npad) || !std::isfinite(t)) return GOGP_EARG;
  if (a_len < n || a1_len < n || f_len < n || f1_len < n || at_len < npad || ft_len < npad) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_lap_interp(0, d[0], d[1], d[2], d[3], t, n, npad, d[4], d[5]); });
}

extern "C" int gogp_test_lap_weight_vectors(int device, const double *Binv, int64_t binv_len, int64_t ld, const double *rho,
                                            int64_t rho_len, int64_t n, int64_t npad, double *sv, int64_t sv_len) {
  const std::vector<Arr> arrs = {rd(Binv, binv_len), rd(rho, rho_len), io(sv, sv_len)};
  if (!have(arrs) || !fin_npad_ok(n, npad) || !covers(binv_len, 0, ld, npad, npad, 1, 0)) return GOGP_EARG;
  if (rho_len < n || sv_len < npad) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_lap_weight_vectors(0, d[0], ld, d[1], n, npad, d[2]); });
}

extern "C" int gogp_test_lap_symv_u(int device, const double *Binv, int64_t binv_len, int64_t ld, int64_t n, int64_t npad,
                                    const double *v, int64_t v_len, const double *sv, int64_t sv_len, const double *sw,
                                    int64_t sw_len, double *upart, int64_t upart_len, double *u, int64_t u_len) {
  const std::vector<Arr> arrs = {rd(Binv, binv_len), rd(v, v_len),         rd(sv, sv_len),
                                 rd(sw, sw_len),     io(upart, upart_len), io(u, u_len)};
  if (!have(arrs) || !fin_npad_ok(n, npad) || !covers(binv_len, 0, ld, npad, npad, 1, 0)) return GOGP_EARG;
  if (v_len < npad || sv_len < n || sw_len < n || u_len < npad || upart_len < npad / 64 * npad) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_lap_symv_u(0, d[0], ld, n, npad, d[1], d[2], d[3], d[4], d[5]); });
}

extern "C" int gogp_test_lap_weight(int device, double *G, int64_t g_len, int64_t ld, int64_t n, int64_t npad,
                                    const double *sw, int64_t sw_len, const double *u, int64_t u_len, const double *a,
                                    int64_t a_len) {
  const std::vector<Arr> arrs = {io(G, g_len), rd(sw, sw_len), rd(u, u_len), rd(a, a_len)};
  if (!have(arrs) || !fin_npad_ok(n, npad) || !covers(g_len, 0, ld, npad, npad, 1, 0)) return GOGP_EARG;
  if (sw_len < n || u_len < n || a_len < n) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_lap_weight(0, d[0], ld, n, npad, d[1], d[2], d[3]); });
}

extern "C" int gogp_test_lap_colscale(int device, double *KsT, int64_t k_len, int64_t ld, int64_t rows, int64_t npad,
                                      const double *sw, int64_t sw_len) {
  const std::vector<Arr> arrs = {io(KsT, k_len), rd(sw, sw_len)};
  if (!have(arrs) || npad <= 0 || npad % PANEL || npad > UP_NPAD_MAX || rows < 1 || rows > FIN_M_MAX) return GOGP_EARG;
  if (!covers(k_len, 0, ld, rows, npad, 1, 0) || sw_len < npad) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_lap_colscale(0, d[0], ld, rows, npad, d[1]); });
}

extern "C" int gogp_test_lap_mean(int device, int lik, const double *mu, int64_t mu_len, const double *sigma,
                                  int64_t sigma_len, int64_t m, double *mean, int64_t mean_len) {
  const std::vector<Arr> arrs = {rd(mu, mu_len), rd(sigma, sigma_len), io(mean, mean_len)};
  if (!have(arrs) || !lap_lik_known(lik) || m < 1 || m > FIN_M_MAX) return GOGP_EARG;
  if (mu_len < m || sigma_len < m || mean_len < m) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_lap_mean(0, lik, d[0], d[1], m, d[2]); });
}

// ---- the kernels of basis.hip through their product launchers (tests/test_basis_kernels.py)
namespace {
bool basis_p_ok(int p) { return p >= 1 && p <= GOGP_BASIS_MAX_P; }
}  // namespace
extern "C" int gogp_test_basis_symm_slabs(int64_t n) { return n >= 1 && n <= UP_NPAD_MAX ? basis_symm_slabs(n) : 0; }
extern "C" int gogp_test_basis_gram_slabs(int64_t n) { return n >= 1 && n <= UP_NPAD_MAX ? basis_gram_slabs(n) : 0; }

extern "C" int gogp_test_basis_symm(int device, const double *Kinv, int64_t kinv_len, int64_t ldk, int64_t n, int64_t npad,
                                    const double *Ht, int64_t ht_len, int64_t ld, int p, double *part, int64_t part_len,
                                    double *Wt, int64_t wt_len) {
  const std::vector<Arr> arrs = {rd(Kinv, kinv_len), rd(Ht, ht_len), io(part, part_len), io(Wt, wt_len)};
  if (!have(arrs) || !fin_npad_ok(n, npad) || !basis_p_ok(p) || ld < npad || ldk < npad) return GOGP_EARG;
  const int64_t p4 = (p + 3) / 4 * 4;
  if (!covers(kinv_len, 0, ldk, npad, npad, 1, 0) || ht_len < (int64_t)p * ld || wt_len < p4 * ld ||
      part_len < (int64_t)basis_symm_slabs(n) * p4 * ld)
    return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_basis_symm(0, d[0], ldk, n, npad, d[1], ld, p, d[2], d[3]); });
}

extern "C" int gogp_test_basis_gram(int device, const double *Ht, int64_t ht_len, const double *Wt, int64_t wt_len, int64_t ld,
                                    const double *alpha, int64_t alpha_len, int64_t n, int p, double *part, int64_t part_len,
                                    double *Ag, int64_t ag_len) {
  const std::vector<Arr> arrs = {rd(Ht, ht_len), rd(Wt, wt_len), rd(alpha, alpha_len), io(part, part_len), io(Ag, ag_len)};
  if (!have(arrs) || !basis_p_ok(p) || n < 1 || n > UP_NPAD_MAX || ld < n) return GOGP_EARG;
  const int64_t total = (int64_t)p * (p + 1);
  if (ht_len < (int64_t)p * ld || wt_len < (int64_t)p * ld || alpha_len < n || ag_len < total ||
      part_len < (int64_t)basis_gram_slabs(n) * total)
    return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_basis_gram(0, d[0], d[1], ld, d[2], n, p, d[3], d[4]); });
}

extern "C" int gogp_test_basis_finish(int device, const double *Ag, int64_t ag_len, int p, double *LA, int64_t la_len,
                                      double *Ainv, int64_t ainv_len, double *beta, int64_t beta_len, double *scal,
                                      int64_t scal_len, double *info, int64_t info_len) {
  // the info word is a long long on the device: it travels in the caller's double and is converted on the way back
  const std::vector<Arr> arrs = {rd(Ag, ag_len),     io(LA, la_len),     io(Ainv, ainv_len),
                                 io(beta, beta_len), io(scal, scal_len), io(info, info_len)};
  if (!have(arrs) || !basis_p_ok(p)) return GOGP_EARG;
  const int64_t pp = (int64_t)p * p;
  if (ag_len < pp + p || la_len < pp || ainv_len < pp || beta_len < p || scal_len < 2) return GOGP_EARG;
  const int rc = run(device, arrs, [&](const Dev &d) {
    launch_basis_finish(0, d[0], p, d[1], d[2], d[3], d[4], d.as<long long>(5));
  });
  if (rc != GOGP_OK) return rc;
  long long word;
  memcpy(&word, info, sizeof word);
  info[0] = (double)word;
  return GOGP_OK;
}

extern "C" int gogp_test_basis_cols(int device, const double *Wt, int64_t wt_len, int64_t ld, int64_t n, int p,
                                    const double *LA, int64_t la_len, const double *beta, int64_t beta_len,
                                    const double *alpha, int64_t alpha_len, double *Ct, int64_t ct_len) {
  const std::vector<Arr> arrs = {rd(Wt, wt_len), rd(LA, la_len), rd(beta, beta_len), rd(alpha, alpha_len), io(Ct, ct_len)};
  if (!have(arrs) || !basis_p_ok(p) || n < 1 || ld < n || ld > UP_NPAD_MAX) return GOGP_EARG;
  const int64_t rows = (p + 1 + 3) / 4 * 4;
  if (wt_len < (int64_t)p * ld || la_len < (int64_t)p * p || beta_len < p || alpha_len < n || ct_len < rows * ld)
    return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_basis_cols(0, d[0], ld, n, p, d[1], d[2], d[3], d[4]); });
}

extern "C" int gogp_test_basis_predict(int device, const double *Hz, int64_t hz_len, const double *KW, int64_t kw_len,
                                       int64_t ldkw, int64_t m, int p, const double *beta, int64_t beta_len,
                                       const double *Ainv, int64_t ainv_len, const double *mu0, int64_t mu0_len,
                                       const double *prior, int64_t prior_len, const double *q, int64_t q_len, double *mu,
                                       int64_t mu_len, double *sigma, int64_t sigma_len) {
  const bool ws = sigma != nullptr;
  if ((!ws && sigma_len != 0) || !basis_p_ok(p) || m < 1 || m > FIN_M_MAX || ldkw < p) return GOGP_EARG;
  if (hz_len < m * p || kw_len < (m - 1) * ldkw + p || beta_len < p || ainv_len < (int64_t)p * p || mu0_len < m ||
      prior_len < m || q_len < m || mu_len < m || (ws && sigma_len < m))
    return GOGP_EARG;
  const std::vector<Arr> arrs = {rd(Hz, hz_len),   rd(KW, kw_len),       rd(beta, beta_len), rd(Ainv, ainv_len),
                                 rd(mu0, mu0_len), rd(prior, prior_len), rd(q, q_len),       io(mu, mu_len),
                                 opt(io(sigma, sigma_len))};  // no sigma: the launcher gets nullptr
  if (!have(arrs)) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    launch_basis_predict(0, d[0], d[1], ldkw, m, p, d[2], d[3], d[4], d[5], d[6], d[7], d[8]);
  });
}

// ---- the kernels of the per-observation noise variances (noisevar.hip; tests/test_noise_variances_kernels.py) ----
extern "C" int gogp_test_nv_diag_add(int device, double *A, int64_t a_len, int64_t ld, int64_t n, int64_t npad,
                                     const double *v, int64_t v_len, int64_t wcols) {
  const std::vector<Arr> arrs = {io(A, a_len), rd(v, v_len)};
  if (!have(arrs) || !fin_npad_ok(n, npad) || !covers(a_len, 0, ld, npad, npad, 1, 0)) return GOGP_EARG;
  if (v_len < n || wcols < 0 || wcols % 64) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_nv_diag_add(0, 0, d[0], ld, n, d[1], wcols); });
}

extern "C" int gogp_test_nv_gradient(int device, const double *Kinv, int64_t kinv_len, int64_t ld, const double *alpha,
                                     int64_t alpha_len, int64_t n, int64_t npad, double *dv, int64_t dv_len) {
  const std::vector<Arr> arrs = {rd(Kinv, kinv_len), rd(alpha, alpha_len), io(dv, dv_len)};
  if (!have(arrs) || !fin_npad_ok(n, npad) || !covers(kinv_len, 0, ld, npad, npad, 1, 0)) return GOGP_EARG;
  if (alpha_len < n || dv_len < n) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_nv_gradient(0, d[0], ld, d[1], n, d[2]); });
}

// ---- the kernels of the sharded path (dist2d.hip and the "helpers of the sharded evaluation" of solve.hip) and the rest of
// solve.hip -- the LML scalars, the fp64 trace, the layout kernels around the factor, the one-line vector kernels --
// through their product launchers (tests/test_shard_kernels.py).  Arrays typed `void *` hold doubles (precision 64) or
// floats (32); lengths count elements.
namespace {
// the block map of rank (pr, pc) of a Pr x Pc grid with tiles of 2^nb_shift; false for what no rank can be
bool sh_map(int nb_shift, int Pr, int Pc, int pr, int pc, BlockMap *m) {
  if (nb_shift < 5 || nb_shift > 10 || Pr < 1 || Pr > 8 || Pc < 1 || Pc > 8 || pr < 0 || pr >= Pr || pc < 0 || pc >= Pc)
    return false;
  m->nb_shift = nb_shift;
  m->Pr = Pr;
  m->Pc = Pc;
  m->pr = pr;
  m->pc = pc;
  return true;
}
// local tile counts of one rank: the product pads so that the grid divides the tile count, NB = mloc Pr = nloc Pc
bool sh_tiles(int mloc, int nloc, const BlockMap &m) {
  return mloc >= 1 && nloc >= 1 && mloc <= 64 && nloc <= 64 && (int64_t)mloc * m.Pr == (int64_t)nloc * m.Pc;
}
}  // namespace

extern "C" int64_t gogp_test_chunk_tdot_scratch(int64_t rows, int nb) {
  if (rows < 1 || rows > SH_COUNT_MAX || nb < 64 || nb > 1024 || nb % 64) return -1;
  return chunk_tdot_scratch(rows, nb);
}

extern "C" int gogp_test_gather_rows(int device, const double *y, int64_t y_len, int64_t rows, int nb_shift, int Pr, int Pc,
                                     int pr, int pc, double *yloc, int64_t yloc_len) {
  const std::vector<Arr> arrs = {rd(y, y_len), io(yloc, yloc_len)};
  BlockMap m;
  if (!have(arrs) || !sh_map(nb_shift, Pr, Pc, pr, pc, &m)) return GOGP_EARG;
  if (rows < 1 || rows > SH_COUNT_MAX || rows % (1 << nb_shift) || yloc_len < rows || y_len < m.grow(rows - 1) + 1)
    return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_gather_rows(0, d[0], d[1], rows, m); });
}

extern "C" int gogp_test_gather_x(int device, const double *X, int64_t x_len, const double *a, int64_t a_len, int D, int64_t n,
                                  int64_t rows, int nb_shift, int Pr, int Pc, int pr, int pc, double *Xloc, int64_t xloc_len,
                                  double *aloc, int64_t aloc_len) {
  const std::vector<Arr> arrs = {rd(X, x_len), rd(a, a_len), io(Xloc, xloc_len), io(aloc, aloc_len)};
  BlockMap m;
  if (!have(arrs) || !sh_map(nb_shift, Pr, Pc, pr, pc, &m) || D < 1 || D > GOGP_MAX_NDIM) return GOGP_EARG;
  if (rows < 1 || rows > SH_COUNT_MAX || rows % (1 << nb_shift) || n < 1 || n > SH_COUNT_MAX) return GOGP_EARG;
  if (x_len < n * D || a_len < n || xloc_len < rows * D || aloc_len < rows) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_gather_x(0, d[0], d[1], D, n, rows, m, d[2], d[3]); });
}

extern "C" int gogp_test_scatter_tile(int device, int precision, const void *src, int64_t src_len, int nb, int64_t n,
                                      int64_t row0, int64_t col0, int diag, int64_t r0, double *dst, int64_t dst_len) {
  if (!prec_ok(precision)) return GOGP_EARG;
  const std::vector<Arr> arrs = {rd(src, src_len, precision / 8), io(dst, dst_len)};
  if (!have(arrs) || nb < 1 || nb > 1024 || n < 1 || n > TH_NPAD_MAX || (diag != 0 && diag != 1)) return GOGP_EARG;
  if (r0 < 0 || row0 < r0 || row0 >= n || col0 < 0 || col0 >= n || src_len < (int64_t)nb * nb) return GOGP_EARG;
  const int64_t rend = row0 + nb < n ? row0 + nb : n;  // dst is the band of the rows from r0 on
  if (dst_len < (rend - r0) * n) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    if (precision == 64)
      launch_scatter_tile(0, d[0], nb, d[1] - r0 * n, n, row0, col0, diag);
    else
      launch_scatter_tile(0, d.f32(0), nb, d[1] - r0 * n, n, row0, col0, diag);
  });
}

extern "C" int gogp_test_gather_rows_of_l(int device, int precision, const void *Lch, int64_t lch_len, int mloc, int nloc,
                                          int nb_shift, int Pr, int Pc, int pr, int pc, const int64_t *rows, int64_t rows_len,
                                          int64_t n, int diag_only, double *out, int64_t out_len) {
  if (!prec_ok(precision) || (diag_only != 0 && diag_only != 1)) return GOGP_EARG;
  const std::vector<Arr> arrs = {rd(Lch, lch_len, precision / 8), opt(rd(rows, rows_len), diag_only == 1), io(out, out_len)};
  BlockMap m;
  if (!have(arrs) || !sh_map(nb_shift, Pr, Pc, pr, pc, &m) || !sh_tiles(mloc, nloc, m)) return GOGP_EARG;
  const int64_t nb = 1 << nb_shift;
  if (diag_only && rows) return GOGP_EARG;
  if (n < 1 || n > (int64_t)mloc * Pr * nb || lch_len < (int64_t)nloc * mloc * nb * nb) return GOGP_EARG;
  if (rows_len > 65535 || out_len < (diag_only ? n : rows_len * n)) return GOGP_EARG;
  for (int64_t k = 0; k < rows_len; ++k)
    if (rows[k] < 0 || rows[k] >= n) return GOGP_EARG;  // the kernel indexes the chunks with them
  return run(device, arrs, [&](const Dev &d) {
    const int64_t *dr = d.as<int64_t>(1);
    if (precision == 64)
      launch_gather_rows_of_l(0, d[0], mloc, nloc, (int)nb, m, dr, rows_len, n, diag_only, d[2]);
    else
      launch_gather_rows_of_l(0, d.f32(0), mloc, nloc, (int)nb, m, dr, rows_len, n, diag_only, d[2]);
  });
}

extern "C" int gogp_test_scatter_stage(int device, int precision, const double *stage, int64_t stage_len, int64_t lds_,
                                       void *Lch, int64_t lch_len, int nloc, int mloc, int bi, int nb) {
  if (!prec_ok(precision)) return GOGP_EARG;
  const std::vector<Arr> arrs = {rd(stage, stage_len), io(Lch, lch_len, precision / 8)};
  if (!have(arrs) || nloc < 1 || nloc > 64 || mloc < 1 || mloc > 64 || bi < 0 || bi >= mloc || nb < 1 || nb > 1024)
    return GOGP_EARG;
  if (!covers(stage_len, 0, lds_, nb, (int64_t)nloc * nb, 1, 0) || lch_len < (int64_t)nloc * mloc * nb * nb) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    if (precision == 64)
      launch_scatter_stage(0, d[0], lds_, d[1], nloc, mloc, bi, nb);
    else
      launch_scatter_stage(0, d[0], lds_, d.f32(1), nloc, mloc, bi, nb);
  });
}

extern "C" int gogp_test_transpose_rect(int device, int precision, const void *src, int64_t src_len, int64_t lds_, void *dst,
                                        int64_t dst_len, int64_t ldd, int64_t rows, int cols) {
  if (!prec_ok(precision)) return GOGP_EARG;
  const std::vector<Arr> arrs = {rd(src, src_len, precision / 8), io(dst, dst_len, precision / 8)};
  if (!have(arrs) || rows < 32 || cols < 32 || rows % 32 || cols % 32 || rows > (1 << 16) || cols > (1 << 16))
    return GOGP_EARG;
  if (!covers(src_len, 0, lds_, rows, cols, 1, 0) || !covers(dst_len, 0, ldd, cols, rows, 1, 0)) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    if (precision == 64)
      launch_transpose_rect(0, d[0], lds_, d[1], ldd, rows, cols);
    else
      launch_transpose_rect(0, d.f32(0), lds_, d.f32(1), ldd, rows, cols);
  });
}

extern "C" int gogp_test_transpose_sq(int device, int precision, const void *src, int64_t src_len, int64_t lds_, void *dst,
                                      int64_t dst_len, int64_t ldd, int n) {
  if (!prec_ok(precision)) return GOGP_EARG;
  const std::vector<Arr> arrs = {rd(src, src_len, precision / 8), io(dst, dst_len, precision / 8)};
  if (!have(arrs) || n < 32 || n % 32 || n > (1 << 13)) return GOGP_EARG;
  if (!covers(src_len, 0, lds_, n, n, 1, 0) || !covers(dst_len, 0, ldd, n, n, 1, 0)) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    if (precision == 64)
      launch_transpose_sq(0, d[0], lds_, d[1], ldd, n);
    else
      launch_transpose_sq(0, d.f32(0), lds_, d.f32(1), ldd, n);
  });
}

extern "C" int gogp_test_copy_block(int device, double *dst, int64_t dst_len, const double *src, int64_t src_len, int64_t ld,
                                    int nb, int64_t rows) {
  const std::vector<Arr> arrs = {io(dst, dst_len), rd(src, src_len)};
  if (!have(arrs) || nb < 1 || nb > 1024 || rows < 1 || rows > (1 << 16)) return GOGP_EARG;
  if (dst_len < rows * nb || !covers(src_len, 0, ld, rows, nb, 1, 0)) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_copy_block(0, d[0], d[1], ld, nb, rows); });
}

extern "C" int gogp_test_residual_block(int device, int precision, void *W, int64_t w_len, const void *Ks, int64_t ks_len,
                                        const double *U, int64_t u_len, int64_t ld, const double *recv, int64_t recv_len,
                                        int nrecv, int nb, int64_t rows) {
  if (!prec_ok(precision) || nrecv < 0 || nrecv > 64) return GOGP_EARG;
  const std::vector<Arr> arrs = {io(W, w_len, precision / 8), rd(Ks, ks_len, precision / 8), rd(U, u_len),
                                 opt(rd(recv, recv_len), nrecv == 0)};
  if (!have(arrs) || nb < 1 || nb > 1024 || rows < 1 || rows > (1 << 16) || (nrecv == 0 && recv)) return GOGP_EARG;
  if (w_len < rows * nb || !covers(ks_len, 0, ld, rows, nb, 1, 0) || !covers(u_len, 0, ld, rows, nb, 1, 0) ||
      recv_len < (int64_t)nrecv * rows * nb)
    return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    if (precision == 64)
      launch_residual_block(0, d[0], d[1], d[2], ld, d[3], nrecv, nb, rows);
    else
      launch_residual_block(0, d.f32(0), d.f32(1), d[2], ld, d[3], nrecv, nb, rows);
  });
}

extern "C" int gogp_test_pack_blocks(int device, double *dst, int64_t dst_len, const double *src, int64_t src_len, int nblk,
                                     int64_t blk, int first, int stride) {
  const std::vector<Arr> arrs = {io(dst, dst_len), rd(src, src_len)};
  if (!have(arrs) || nblk < 1 || nblk > 65535 || blk < 2 || blk % 2 || blk > SH_COUNT_MAX || first < 0 || stride < 1 ||
      first > 4096 || stride > 4096)
    return GOGP_EARG;
  if (dst_len < (int64_t)nblk * blk || src_len < ((int64_t)first + (int64_t)(nblk - 1) * stride + 1) * blk) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_pack_blocks(0, d[0], d[1], nblk, blk, first, stride); });
}

extern "C" int gogp_test_convert_block(int device, int precision, int precision2, const void *src, int64_t src_len,
                                       int64_t lds_, void *dst, int64_t dst_len, int64_t ldd, int rows, int cols) {
  if (!prec_ok(precision) || !prec_ok(precision2) || (precision == 32 && precision2 == 32)) return GOGP_EARG;
  const std::vector<Arr> arrs = {rd(src, src_len, precision / 8), io(dst, dst_len, precision2 / 8)};
  if (!have(arrs) || rows < 1 || rows > (1 << 16) || cols < 1 || cols > (1 << 16)) return GOGP_EARG;
  if (!covers(src_len, 0, lds_, rows, cols, 1, 0) || !covers(dst_len, 0, ldd, rows, cols, 1, 0)) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    if (precision == 32)
      launch_convert_block(0, d.f32(0), lds_, d[1], ldd, rows, cols);
    else if (precision2 == 32)
      launch_convert_block(0, d[0], lds_, d.f32(1), ldd, rows, cols);
    else
      launch_convert_block(0, (const double *)d[0], lds_, d[1], ldd, rows, cols);
  });
}

extern "C" int gogp_test_chunk_tdot(int device, int precision, const void *chunk, int64_t chunk_len, int64_t rows, int nb,
                                    const double *v, int64_t v_len, double *part, int64_t part_len, double *out,
                                    int64_t out_len) {
  if (!prec_ok(precision)) return GOGP_EARG;
  const std::vector<Arr> arrs = {rd(chunk, chunk_len, precision / 8), rd(v, v_len), io(part, part_len), io(out, out_len)};
  // the grid is nb / 64 column groups: any other nb would leave columns unwritten
  if (!have(arrs) || rows < 1 || rows > (1 << 20) || nb < 64 || nb > 1024 || nb % 64) return GOGP_EARG;
  if (chunk_len < rows * nb || v_len < rows || part_len < chunk_tdot_scratch(rows, nb) || out_len < nb) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    if (precision == 64)
      launch_chunk_tdot(0, d[0], rows, nb, d[1], d[2], d[3]);
    else
      launch_chunk_tdot(0, d.f32(0), rows, nb, d[1], d[2], d[3]);
  });
}

extern "C" int gogp_test_chunk_alpha(int device, int precision, const void *Ych, int64_t ych_len, int mloc, int nloc,
                                     int nb_shift, int Pr, int Pc, int pr, int pc, const double *z, int64_t z_len, double *out,
                                     int64_t out_len) {
  if (!prec_ok(precision)) return GOGP_EARG;
  const std::vector<Arr> arrs = {rd(Ych, ych_len, precision / 8), rd(z, z_len), io(out, out_len)};
  BlockMap m;
  if (!have(arrs) || !sh_map(nb_shift, Pr, Pc, pr, pc, &m) || !sh_tiles(mloc, nloc, m)) return GOGP_EARG;
  const int64_t nb = 1 << nb_shift, npad = (int64_t)mloc * Pr * nb;
  if (ych_len < (int64_t)nloc * mloc * nb * nb || z_len < npad || out_len < npad) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    if (precision == 64)
      launch_chunk_alpha(0, d[0], mloc, nloc, (int)nb, m, d[1], d[2]);
    else
      launch_chunk_alpha(0, d.f32(0), mloc, nloc, (int)nb, m, d[1], d[2]);
  });
}

extern "C" int gogp_test_chunk_sumsq(int device, int precision, const void *Ych, int64_t ych_len, int mloc, int nloc,
                                     int nb_shift, int Pr, int Pc, int pr, int pc, int64_t n, double *part, int64_t part_len,
                                     double *out, int64_t out_len) {
  if (!prec_ok(precision)) return GOGP_EARG;
  const std::vector<Arr> arrs = {rd(Ych, ych_len, precision / 8), io(part, part_len), io(out, out_len)};
  BlockMap m;
  if (!have(arrs) || !sh_map(nb_shift, Pr, Pc, pr, pc, &m) || !sh_tiles(mloc, nloc, m)) return GOGP_EARG;
  const int64_t nb = 1 << nb_shift, npad = (int64_t)mloc * Pr * nb;
  if (n < 1 || n > npad || ych_len < (int64_t)nloc * mloc * nb * nb || part_len < mloc * nb || out_len < 1) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    if (precision == 64)
      launch_chunk_sumsq(0, d[0], mloc, nloc, (int)nb, m, n, d[1], d[2]);
    else
      launch_chunk_sumsq(0, d.f32(0), mloc, nloc, (int)nb, m, n, d[1], d[2]);
  });
}

extern "C" int gogp_test_lml_scalars(int device, int precision, const void *L, int64_t l_len, int64_t ld, const double *z,
                                     int64_t z_len, const double *y, int64_t y_len, const double *alpha, int64_t alpha_len,
                                     int64_t n, int k, int64_t bstride, double *scalars, int64_t scalars_len) {
  if (!prec_ok(precision)) return GOGP_EARG;
  const std::vector<Arr> arrs = {rd(L, l_len, precision / 8), rd(z, z_len), rd(y, y_len), opt(rd(alpha, alpha_len)),
                                 io(scalars, scalars_len)};
  if (!have(arrs) || !batch_ok(precision, k, &bstride) || n < 1 || n > TH_NPAD_MAX) return GOGP_EARG;
  if (!covers(l_len, 0, ld, n, n, k, bstride) || !covers(z_len, 0, n, 1, n, k, bstride) || y_len < n ||
      (alpha && !covers(alpha_len, 0, n, 1, n, k, bstride)) || !covers(scalars_len, 0, 5, 1, 5, k, bstride))
    return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    set_batch(k, bstride);
    if (precision == 64)
      launch_lml_scalars(0, d[0], ld, d[1], d[2], d[3], n, d[4]);
    else
      launch_lml_scalars(0, d.f32(0), ld, d[1], d[2], d[3], n, d[4]);
  });
}

extern "C" int gogp_test_alpha_from_y_batched(int device, const double *Y, int64_t y_len, int64_t ld, const double *z,
                                              int64_t z_len, int64_t npad, int k, int64_t bstride, double *alpha,
                                              int64_t alpha_len) {
  const std::vector<Arr> arrs = {rd(Y, y_len), rd(z, z_len), io(alpha, alpha_len)};
  if (!have(arrs) || !batch_ok(64, k, &bstride) || npad <= 0 || npad % 2 || npad > TH_NPAD_MAX || ld % 2) return GOGP_EARG;
  if (!covers(y_len, 0, ld, npad, npad, k, bstride) || !covers(z_len, 0, npad, 1, npad, k, bstride) ||
      !covers(alpha_len, 0, npad, 1, npad, k, bstride))
    return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    set_batch(k, bstride);
    launch_alpha_from_y(0, (const double *)d[0], ld, d[1], npad, d[2]);
  });
}

extern "C" int gogp_test_trace_from_y(int device, const float *Y, int64_t y_len, int64_t ld, int64_t n, int64_t npad,
                                      const double *alpha, int64_t alpha_len, double *part, int64_t part_len, double *out,
                                      int64_t out_len) {
  const std::vector<Arr> arrs = {rd(Y, y_len, 4), rd(alpha, alpha_len), io(part, part_len), io(out, out_len)};
  if (!have(arrs) || npad <= 0 || npad % PANEL || npad > TH_NPAD_MAX || n < 1 || n > npad) return GOGP_EARG;
  if (!covers(y_len, 0, ld, n, npad, 1, 0) || alpha_len < n || part_len < n || out_len < 1) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_trace_from_y(0, d.f32(0), ld, n, npad, d[1], d[2], d[3]); });
}

extern "C" int gogp_test_zero_upper_blocks(int device, int precision, void *R, int64_t r_len, int64_t ld, int64_t npad, int k,
                                           int64_t bstride) {
  if (!prec_ok(precision)) return GOGP_EARG;
  const std::vector<Arr> arrs = {io(R, r_len, precision / 8)};
  if (!have(arrs) || !batch_ok(precision, k, &bstride) || npad <= 0 || npad % PANEL || npad > (1 << 15) || ld % 2)
    return GOGP_EARG;
  if (!covers(r_len, 0, ld, npad, npad, k, bstride)) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    set_batch(k, bstride);
    if (precision == 64)
      launch_zero_upper_blocks(0, d[0], ld, npad);
    else
      launch_zero_upper_blocks(0, d.f32(0), ld, npad);
  });
}

extern "C" int gogp_test_ydiag(int device, int precision, const void *Dinv, int64_t dinv_len, void *Y, int64_t y_len,
                               int64_t ld, int k, int64_t bstride) {
  if (!prec_ok(precision)) return GOGP_EARG;
  const std::vector<Arr> arrs = {rd(Dinv, dinv_len, precision / 8), io(Y, y_len, precision / 8)};
  if (!have(arrs) || !batch_ok(precision, k, &bstride)) return GOGP_EARG;
  if (!covers(dinv_len, 0, PANEL, PANEL, PANEL, k, bstride) || !covers(y_len, 0, ld, PANEL, PANEL, k, bstride))
    return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    set_batch(k, bstride);
    if (precision == 64)
      launch_ydiag(0, d[0], d[1], ld);
    else
      launch_ydiag(0, d.f32(0), d.f32(1), ld);
  });
}

extern "C" int gogp_test_zero_block(int device, int precision, void *B, int64_t b_len, int64_t ld, int64_t rows, int64_t cols,
                                    int k, int64_t bstride) {
  if (!prec_ok(precision)) return GOGP_EARG;
  const std::vector<Arr> arrs = {io(B, b_len, precision / 8)};
  // pairs of columns are stored: an odd cols would write one column more, an odd ld misalign the pairs
  if (!have(arrs) || !batch_ok(precision, k, &bstride) || rows < 1 || rows > 65535 || cols < 2 || cols % 2 || ld % 2 ||
      cols > (1 << 20))
    return GOGP_EARG;
  if (!covers(b_len, 0, ld, rows, cols, k, bstride)) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    set_batch(k, bstride);
    if (precision == 64)
      launch_zero_block(0, d[0], ld, rows, cols);
    else
      launch_zero_block(0, d.f32(0), ld, rows, cols);
  });
}

extern "C" int gogp_test_extract_lower(int device, int precision, const void *L, int64_t l_len, int64_t ld, int64_t n,
                                       double *out, int64_t out_len) {
  if (!prec_ok(precision)) return GOGP_EARG;
  const std::vector<Arr> arrs = {rd(L, l_len, precision / 8), io(out, out_len)};
  if (!have(arrs) || n < 1 || n > 65535 || !covers(l_len, 0, ld, n, n, 1, 0) || out_len < n * n) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    if (precision == 64)
      launch_extract_lower(0, d[0], ld, n, d[1]);
    else
      launch_extract_lower(0, d.f32(0), ld, n, d[1]);
  });
}

extern "C" int gogp_test_pack_lower(int device, int precision, const double *src, int64_t src_len, int64_t n, int64_t npad,
                                    void *L, int64_t l_len, int64_t ld) {
  if (!prec_ok(precision)) return GOGP_EARG;
  const std::vector<Arr> arrs = {rd(src, src_len), io(L, l_len, precision / 8)};
  if (!have(arrs) || n < 1 || n > npad || npad > 65535 || src_len < n * n || !covers(l_len, 0, ld, npad, npad, 1, 0))
    return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    if (precision == 64)
      launch_pack_lower(0, d[0], n, npad, d[1], ld);
    else
      launch_pack_lower(0, d[0], n, npad, d.f32(1), ld);
  });
}

extern "C" int gogp_test_sigma(int device, const double *prior, int64_t prior_len, const double *q, int64_t q_len, int64_t m,
                               double *sigma, int64_t sigma_len) {
  const std::vector<Arr> arrs = {rd(prior, prior_len), opt(rd(q, q_len)), io(sigma, sigma_len)};
  if (!have(arrs) || m < 1 || m > SH_COUNT_MAX || prior_len < m || (q && q_len < m) || sigma_len < m) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_sigma(0, d[0], d[1], m, d[2]); });
}

extern "C" int gogp_test_logdet_block(int device, const double *L, int64_t l_len, int64_t ld, int64_t row0, int64_t n, int nb,
                                      double *acc, int64_t acc_len) {
  const std::vector<Arr> arrs = {rd(L, l_len), io(acc, acc_len)};
  if (!have(arrs) || nb < 1 || nb > 1024 || row0 < 0 || n < 0 || n > TH_NPAD_MAX || row0 > TH_NPAD_MAX) return GOGP_EARG;
  if (!covers(l_len, 0, ld, nb, nb, 1, 0) || acc_len < 1) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_logdet_block(0, d[0], ld, row0, n, nb, d[1]); });
}

extern "C" int gogp_test_dot(int device, const double *a, int64_t a_len, const double *b, int64_t b_len, int64_t n, double *out,
                             int64_t out_len) {
  const std::vector<Arr> arrs = {rd(a, a_len), rd(b, b_len), io(out, out_len)};
  if (!have(arrs) || n < 1 || n > SH_COUNT_MAX || a_len < n || b_len < n || out_len < 1) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_dot(0, d[0], d[1], n, d[2]); });
}

extern "C" int gogp_test_sumsq_info(int device, const double *z, int64_t z_len, int64_t n, const int64_t *info,
                                    int64_t info_len, double *out, int64_t out_len) {
  const std::vector<Arr> arrs = {rd(z, z_len), opt(rd(info, info_len)), io(out, out_len)};
  if (!have(arrs) || n < 1 || n > SH_COUNT_MAX || z_len < n || out_len < (info ? 2 : 1)) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) { launch_sumsq_info(0, d[0], n, d.as<long long>(1), d[2]); });
}

// the one-line vector kernels: op 0 fill (a := f), 1 axpy (a += b), 2 add_vec (a += b), 3 scale (a *= f), 4 residual_from
// (a := b - a), 5 add_inplace (a += b; the one op with a float instance), 6 info_to_double (a[0] := the int64 whose bits
// b[0] holds; count 1).  fill and scale take no b: NULL with length 0.
extern "C" int gogp_test_vector_op(int device, int op, int precision, void *a, int64_t a_len, const void *b, int64_t b_len,
                                   int64_t count, double f) {
  if (!prec_ok(precision) || op < 0 || op > 6 || (precision == 32 && op != 5)) return GOGP_EARG;
  const bool no_b = op == 0 || op == 3;
  const std::vector<Arr> arrs = {io(a, a_len, precision / 8), opt(rd(b, b_len, precision / 8), no_b)};
  if (!have(arrs) || count < 1 || count > SH_COUNT_MAX || a_len < count || (op == 6 && count != 1)) return GOGP_EARG;
  if (no_b ? b != nullptr : b_len < count) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    switch (op) {
      case 0: launch_fill(0, d[0], count, f); break;
      case 1: launch_axpy(0, d[0], d[1], count); break;
      case 2: launch_add_vec(0, d[0], d[1], count); break;
      case 3: launch_scale(0, d[0], f, count); break;
      case 4: launch_residual_from(0, d[0], d[1], count); break;
      case 5:
        if (precision == 64)
          launch_add_inplace(0, d[0], d[1], count);
        else
          launch_add_inplace(0, d.f32(0), d.f32(1), count);
        break;
      default: launch_info_to_double(0, d.as<long long>(1), d[0]); break;
    }
  });
}

// ---- the kernels of gram.hip and the forecast-derivative kernels of pgrad.hip, through their product launchers
// (tests/test_gram_kernels.py).  What they refuse beyond the arrays' lengths follows from
// the kernels (common.h states it at the launchers): whole 64 x 64 tiles are written, so npad / mpad / mrows / ncols are
// positive multiples of 64 and the output holds all of their rows; the one-radial-term paths read rows n .. npad - 1 of X
// unguarded, so X holds npad rows (and GOGP_MAX_NDIM doubles of slack, the convention of gogp_test_grad_reduce); wcols == 0
// would launch an empty grid; radial1 goes with one radial term only; no instance has events and an ARD term.
namespace {
bool gram_args_ok(const gogp_test_kparams *kp, int k, int radial1, int ev) {
  if ((ev != 0 && ev != 1) || (radial1 != 0 && radial1 != 1)) return false;
  return kparams_ok(kp, k, ard_dims_of(kp), radial1, 1, ev);  // (two ARD terms: ard_dims_of is 0, which kparams_ok refuses)
}
bool pad_ok(int64_t npad) { return npad > 0 && npad % 64 == 0 && npad <= GR_NPAD_MAX; }
}  // namespace

extern "C" int gogp_test_gram_split(int device, int precision, const gogp_test_kparams *kparams, int ev, const double *X,
                                    int64_t x_len, int64_t n, int64_t npad, int64_t wcols, int k, int64_t bstride, void *K,
                                    int64_t k_len, int64_t ld) {
  if (!kparams || !X || !K || !prec_ok(precision) || !batch_ok(precision, k, &bstride)) return GOGP_EARG;
  if (!gram_args_ok(kparams, k, 0, ev) || !pad_ok(npad) || n < 1 || n > npad || ld < npad) return GOGP_EARG;
  if (wcols < 64 || wcols % 64 || wcols > GR_NPAD_MAX) return GOGP_EARG;
  // every per-candidate buffer shares the stride: it must hold the matrix and the parameters
  if (k > 1 && (bstride < (npad - 1) * ld + npad || bstride * 8 < (int64_t)sizeof(DevParams))) return GOGP_EARG;
  const int ndim = kparams[0].ndim;
  if (x_len < npad * ndim + GOGP_MAX_NDIM || !covers(k_len, 0, ld, npad, npad, k, bstride)) return GOGP_EARG;
  std::vector<DevParams> hp;
  for (int c = 0; c < k; ++c) hp.push_back(to_dev(kparams[c]));
  const std::vector<char> P = pack_strided(hp.data(), sizeof(DevParams), k, (size_t)bstride * 8);
  return run(device, {rd(P.data(), (int64_t)P.size(), 1), rd(X, x_len), io(K, k_len, precision / 8)}, [&](const Dev &d) {
    set_batch(k, bstride);
    if (precision == 64)
      launch_gram_lower_split(0, 0, d.as<DevParams>(0), ndim, d[1], n, npad, d[2], ld, wcols, ev != 0);
    else
      launch_gram_lower_split(0, 0, d.as<DevParams>(0), ndim, d[1], n, npad, d.f32(2), ld, wcols, ev != 0);
  });
}

extern "C" int gogp_test_gram_local(int device, int precision, const gogp_test_kparams *kparams, int ev, const double *X,
                                    int64_t x_len, int64_t n, int64_t npad, int64_t mrows, int64_t ncols, int nb_shift, int pr,
                                    int Pr, int pc, int Pc, void *K, int64_t k_len, int64_t ld) {
  if (!kparams || !X || !K || !prec_ok(precision)) return GOGP_EARG;
  if (!gram_args_ok(kparams, 1, 0, ev) || !pad_ok(npad) || !pad_ok(mrows) || !pad_ok(ncols) || n < 1 || n > npad || ld < ncols)
    return GOGP_EARG;
  if (nb_shift < 6 || nb_shift > 14 || Pr < 1 || Pc < 1 || pr < 0 || pr >= Pr || pc < 0 || pc >= Pc) return GOGP_EARG;
  BlockMap map;
  map.nb_shift = nb_shift;
  map.pr = pr;
  map.Pr = Pr;
  map.pc = pc;
  map.Pc = Pc;
  // the last local row / column must be a global one inside the padded matrix (the kernel reads X there)
  if (map.grow(mrows - 1) >= npad || map.gcol(ncols - 1) >= npad) return GOGP_EARG;
  const int ndim = kparams->ndim;
  if (x_len < npad * ndim + GOGP_MAX_NDIM || !covers(k_len, 0, ld, mrows, ncols, 1, 0)) return GOGP_EARG;
  const DevParams hp = to_dev(*kparams);
  return run(device, {rd(&hp, 1, sizeof hp), rd(X, x_len), io(K, k_len, precision / 8)}, [&](const Dev &d) {
    if (precision == 64)
      launch_gram_local(0, d.as<DevParams>(0), ndim, d[1], n, mrows, ncols, map, d[2], ld, ev != 0);
    else
      launch_gram_local(0, d.as<DevParams>(0), ndim, d[1], n, mrows, ncols, map, d.f32(2), ld, ev != 0);
  });
}

extern "C" int gogp_test_cross(int device, int precision, const gogp_test_kparams *kparams, int ev, const double *X,
                               int64_t x_len, int64_t n, int64_t npad, const double *Z, int64_t z_len, int64_t m, int64_t mpad,
                               void *KsT, int64_t k_len, int64_t ld) {
  if (!kparams || !X || !Z || !KsT || !prec_ok(precision)) return GOGP_EARG;
  if (!gram_args_ok(kparams, 1, 0, ev) || !pad_ok(npad) || !pad_ok(mpad) || n < 1 || n > npad || m < 1 || m > mpad || ld < npad)
    return GOGP_EARG;
  const int ndim = kparams->ndim;
  if (x_len < npad * ndim + GOGP_MAX_NDIM || z_len < mpad * ndim || !covers(k_len, 0, ld, mpad, npad, 1, 0)) return GOGP_EARG;
  const DevParams hp = to_dev(*kparams);
  return run(device, {rd(&hp, 1, sizeof hp), rd(X, x_len), rd(Z, z_len), io(KsT, k_len, precision / 8)}, [&](const Dev &d) {
    if (precision == 64)
      launch_cross(0, d.as<DevParams>(0), ndim, d[1], n, npad, d[2], m, mpad, d[3], ld, ev != 0);
    else
      launch_cross(0, d.as<DevParams>(0), ndim, d[1], n, npad, d[2], m, mpad, d.f32(3), ld, ev != 0);
  });
}

extern "C" int gogp_test_prior(int device, const gogp_test_kparams *kparams, const double *Z, int64_t z_len, int64_t m,
                               double *prior, int64_t prior_len) {
  if (!kparams || !Z || !prior || !gram_args_ok(kparams, 1, 0, 0)) return GOGP_EARG;
  if (m < 1 || m > SH_COUNT_MAX || z_len < m * kparams->ndim || prior_len < m) return GOGP_EARG;
  const DevParams hp = to_dev(*kparams);
  return run(device, {rd(&hp, 1, sizeof hp), rd(Z, z_len), io(prior, prior_len)},
             [&](const Dev &d) { launch_prior(0, d.as<DevParams>(0), d[1], m, d[2]); });
}

extern "C" int gogp_test_kmatvec(int device, const gogp_test_kparams *kparams, int radial1, int ev, const double *X,
                                 int64_t x_len, int64_t n, int64_t npad, const double *v, int64_t v_len, const double *y,
                                 int64_t y_len, int part_idx, int nparts, int nslab, double *part, int64_t part_len,
                                 double *out, int64_t out_len) {
  if (!kparams || !X || !v || !part || !out || !gram_args_ok(kparams, 1, radial1, ev)) return GOGP_EARG;
  if (!pad_ok(npad) || n < 1 || n > npad || nslab < 1 || nslab > 64 || nparts < 1 || nparts > 64 || part_idx < 0 ||
      part_idx >= nparts)
    return GOGP_EARG;
  if (y ? (nparts != 1 || y_len < n) : y_len != 0) return GOGP_EARG;  // launch_residual takes every column
  const int ndim = kparams->ndim;
  if (x_len < npad * ndim + GOGP_MAX_NDIM || v_len < npad || part_len < (int64_t)nslab * npad || out_len < npad) return GOGP_EARG;
  const DevParams hp = to_dev(*kparams);
  return run(device, {rd(&hp, 1, sizeof hp), rd(X, x_len), rd(v, v_len), rd(y, y_len), io(part, part_len), io(out, out_len)},
             [&](const Dev &d) {
               if (y)
                 launch_residual(0, d.as<DevParams>(0), ndim, d[1], n, npad, d[2], d[3], d[4], nslab, d[5], radial1 != 0,
                                 ev != 0);
               else
                 launch_kmatvec_share(0, d.as<DevParams>(0), ndim, d[1], n, npad, d[2], part_idx, nparts, d[4], nslab, d[5],
                                      radial1 != 0, ev != 0);
             });
}

extern "C" int gogp_test_pgrad_slabs(int64_t npad, int64_t m, int *tiles_per_slab) {
  if (npad <= 0 || npad % 64 || npad > TH_NPAD_MAX || m < 1 || m > SH_COUNT_MAX) return -1;
  return pgrad_slabs(npad, m, tiles_per_slab);
}

extern "C" int gogp_test_pgrad(int device, const gogp_test_kparams *kparams, int ev, const double *X, int64_t x_len, int64_t n,
                               int64_t npad, const double *Z, int64_t z_len, int64_t m, const double *alpha, int64_t alpha_len,
                               const double *Wt, int64_t wt_len, int64_t ld, const double *sigma, int64_t sigma_len,
                               double *part, int64_t part_len, double *dmu, int64_t dmu_len, double *dsigma,
                               int64_t dsigma_len) {
  if (!kparams || !X || !Z || !alpha || !Wt || !sigma || !part || !dmu || !dsigma) return GOGP_EARG;
  if (!gram_args_ok(kparams, 1, 0, ev) || !pad_ok(npad) || n < 1 || n > npad || m < 1 || m > (1 << 16) || ld < npad)
    return GOGP_EARG;
  const int ndim = kparams->ndim;
  const int64_t md = m * ndim, nslab = pgrad_slabs(npad, m, nullptr);
  if (x_len < npad * ndim || z_len < md || alpha_len < npad || !covers(wt_len, 0, ld, m, npad, 1, 0) || sigma_len < m ||
      part_len < 2 * nslab * md || dmu_len < md || dsigma_len < md)
    return GOGP_EARG;
  const DevParams hp = to_dev(*kparams);
  return run(device, {rd(&hp, 1, sizeof hp), rd(X, x_len), rd(Z, z_len), rd(alpha, alpha_len), rd(Wt, wt_len),
                      rd(sigma, sigma_len), io(part, part_len), io(dmu, dmu_len), io(dsigma, dsigma_len)},
             [&](const Dev &d) {
               launch_pgrad(0, d.as<DevParams>(0), ndim, d[1], n, npad, d[2], m, d[3], d[4], ld, d[5], d[6], d[7], d[8],
                            ev != 0);
             });
}

// ---- the kernels of cg.hip (the iterative exact GP), through their product launchers (tests/test_cg_kernels.py).  The
// kernels guard every access by the sizes given, so the hooks hold the arrays to exactly those: a block of T vectors
// needs (T - 1) * ld + n elements, the per-column state CG_SC_ROWS / CG_ST_ROWS rows of GOGP_CG_MAX_RHS.
namespace {
bool cg_block_ok(int64_t len, int64_t ld, int64_t n, int T) { return covers(len, 0, ld, T, n, 1, 0); }
bool cg_dims_ok(int64_t ld, int64_t n, int T) { return n >= 1 && n <= SH_COUNT_MAX && ld >= n && T >= 1 && T <= CG_MAX_T; }
bool cg_state_ok(int64_t sc_len, int64_t st_len) { return sc_len >= CG_SC_ROWS * CG_MAX_T && st_len >= CG_ST_ROWS * CG_MAX_T; }
}  // namespace

extern "C" int gogp_test_kmm_slabs(int64_t rows, int64_t cols) {
  if (rows < 1 || cols < 1) return -1;
  return kmm_slabs(rows, cols);
}

extern "C" int gogp_test_cg_dot_blocks(int64_t n) { return n < 1 ? -1 : cg_dot_blocks(n); }

// B == NULL (b_len 0): the square product, columns = rows = the rows of A; diag only then
extern "C" int gogp_test_kmm(int device, const gogp_test_kparams *kparams, const double *A, int64_t a_len, int64_t rows,
                             const double *B, int64_t b_len, int64_t cols, const double *V, int64_t v_len, int64_t ldv, int T,
                             const double *diag, int64_t diag_len, int nslab, int max_blocks, double *part, int64_t part_len,
                             double *Out, int64_t out_len, int64_t ldo) {
  if (!kparams || !A || !V || !part || !Out || !gram_args_ok(kparams, 1, 0, 0)) return GOGP_EARG;
  if (kparams->nevents != 0) return GOGP_EARG;  // the product has no instance with event discounts
  if (rows < 1 || rows > GR_NPAD_MAX || cols < 1 || cols > GR_NPAD_MAX || T < 1 || T > CG_MAX_T) return GOGP_EARG;
  if (nslab < 1 || nslab > KMM_SLABS_MAX || max_blocks < 0) return GOGP_EARG;
  const int ndim = kparams->ndim;
  if (B ? b_len < cols * ndim : (b_len != 0 || cols != rows)) return GOGP_EARG;
  if (diag ? (B != nullptr || diag_len < rows) : diag_len != 0) return GOGP_EARG;
  const int64_t rpad = (rows + 63) / 64 * 64;
  if (a_len < rows * ndim || !cg_block_ok(v_len, ldv, cols, T) || part_len < (int64_t)nslab * T * rpad || ldo < rows ||
      out_len < (int64_t)T * ldo)
    return GOGP_EARG;
  const DevParams hp = to_dev(*kparams);
  return run(device, {rd(&hp, 1, sizeof hp), rd(A, a_len), opt(rd(B, b_len)), rd(V, v_len), opt(rd(diag, diag_len)),
                      io(part, part_len), io(Out, out_len)},
             [&](const Dev &d) {
               launch_kmm(0, d.as<DevParams>(0), ndim, d[1], rows, B ? d[2] : d[1], cols, d[3], ldv, T, d[4], nslab,
                          max_blocks, d[5], d[6], ldo);
             });
}

// out may be NULL (length 0) except in mode CG_DOT_PLAIN; st holds 32-bit integers
extern "C" int gogp_test_cg_dots(int device, const double *A, int64_t a_len, const double *B, int64_t b_len, int64_t ld,
                                 int64_t n, int T, int mode, int it, double tol, double *part, int64_t part_len, double *out,
                                 int64_t out_len, double *sc, int64_t sc_len, int32_t *st, int64_t st_len) {
  if (!A || !B || !part || !sc || !st || !cg_dims_ok(ld, n, T) || mode < CG_DOT_PLAIN || mode > CG_DOT_BETA) return GOGP_EARG;
  if (!cg_block_ok(a_len, ld, n, T) || !cg_block_ok(b_len, ld, n, T) || part_len < (int64_t)T * cg_dot_blocks(n) ||
      !cg_state_ok(sc_len, st_len))
    return GOGP_EARG;
  if (out ? out_len < T : (out_len != 0 || mode == CG_DOT_PLAIN)) return GOGP_EARG;
  return run(device, {rd(A, a_len), rd(B, b_len), io(part, part_len), opt(io(out, out_len)), io(sc, sc_len), io(st, st_len, 4)},
             [&](const Dev &d) {
               launch_cg_dots(0, d[0], d[1], ld, n, T, mode, it, tol, d[2], d[3], CgState{d[4], d.as<int>(5)});
             });
}

extern "C" int gogp_test_cg_update_xr(int device, double *x, int64_t x_len, double *r, int64_t r_len, const double *p,
                                      int64_t p_len, const double *q, int64_t q_len, int64_t ld, int64_t n, int T,
                                      const double *sc, int64_t sc_len, const int32_t *st, int64_t st_len) {
  if (!x || !r || !p || !q || !sc || !st || !cg_dims_ok(ld, n, T) || !cg_state_ok(sc_len, st_len)) return GOGP_EARG;
  if (!cg_block_ok(x_len, ld, n, T) || !cg_block_ok(r_len, ld, n, T) || !cg_block_ok(p_len, ld, n, T) ||
      !cg_block_ok(q_len, ld, n, T))
    return GOGP_EARG;
  return run(device, {io(x, x_len), io(r, r_len), rd(p, p_len), rd(q, q_len), rd(sc, sc_len), rd(st, st_len, 4)},
             [&](const Dev &d) {
               launch_cg_update_xr(0, d[0], d[1], d[2], d[3], ld, n, T, CgState{d[4], d.as<int>(5)});
             });
}

extern "C" int gogp_test_cg_update_p(int device, double *p, int64_t p_len, const double *z, int64_t z_len, int64_t ld,
                                     int64_t n, int T, const double *sc, int64_t sc_len, const int32_t *st, int64_t st_len) {
  if (!p || !z || !sc || !st || !cg_dims_ok(ld, n, T) || !cg_state_ok(sc_len, st_len)) return GOGP_EARG;
  if (!cg_block_ok(p_len, ld, n, T) || !cg_block_ok(z_len, ld, n, T)) return GOGP_EARG;
  return run(device, {io(p, p_len), rd(z, z_len), rd(sc, sc_len), rd(st, st_len, 4)},
             [&](const Dev &d) { launch_cg_update_p(0, d[0], d[1], ld, n, T, CgState{d[2], d.as<int>(3)}); });
}

// w (n entries) and sub (a block) may be NULL with length 0
extern "C" int gogp_test_cg_scale(int device, const double *in, int64_t in_len, const double *w, int64_t w_len,
                                  const double *sub, int64_t sub_len, int64_t ld, int64_t n, int T, double *out,
                                  int64_t out_len) {
  if (!in || !out || !cg_dims_ok(ld, n, T) || !cg_block_ok(in_len, ld, n, T) || !cg_block_ok(out_len, ld, n, T))
    return GOGP_EARG;
  if (w ? w_len < n : w_len != 0) return GOGP_EARG;
  if (sub ? !cg_block_ok(sub_len, ld, n, T) : sub_len != 0) return GOGP_EARG;
  return run(device, {rd(in, in_len), opt(rd(w, w_len)), opt(rd(sub, sub_len)), io(out, out_len)},
             [&](const Dev &d) { launch_cg_scale(0, d[0], d[1], d[2], ld, n, T, d[3]); });
}

extern "C" int gogp_test_cg_status(int device, int T, int32_t *st, int64_t st_len) {
  if (!st || T < 1 || T > CG_MAX_T || st_len < CG_ST_ROWS * CG_MAX_T) return GOGP_EARG;
  return run(device, {io(st, st_len, 4)}, [&](const Dev &d) { launch_cg_status(0, T, CgState{nullptr, d.as<int>(0)}); });
}

// The preconditioner's application on a given scaled factor: Z = P^-1 R with Ls (r columns of ldn doubles, column-major),
// dis (n) and Cinv (rp x rp, rp = r rounded up to 16; r == 0: Jacobi, Ls and Cinv NULL).  Runs launch_cg_lst,
// launch_cg_small_mm and launch_cg_precond; C (rp x rp, may be NULL) receives launch_cg_capacitance's I + Ls^T Ls.
extern "C" int gogp_test_cg_precond(int device, const double *Ls, int64_t ls_len, int64_t ldn, int64_t n, int r,
                                    const double *dis, int64_t dis_len, const double *Cinv, int64_t cinv_len, const double *R,
                                    int64_t r_len, int64_t ld, int T, double *Z, int64_t z_len, double *C, int64_t c_len) {
  if (!dis || !R || !Z || !cg_dims_ok(ld, n, T) || r < 0 || r > GOGP_CG_MAX_RANK || dis_len < n) return GOGP_EARG;
  if (!cg_block_ok(r_len, ld, n, T) || !cg_block_ok(z_len, ld, n, T)) return GOGP_EARG;
  const int rp = (r + 15) / 16 * 16;
  if (r > 0 ? (!Ls || !Cinv || ldn < n || !covers(ls_len, 0, ldn, r, n, 1, 0) || cinv_len < (int64_t)rp * rp)
            : (Ls || Cinv || ls_len != 0 || cinv_len != 0))
    return GOGP_EARG;
  if (C ? (r < 1 || c_len < (int64_t)rp * rp) : c_len != 0) return GOGP_EARG;
  const int rr = rp > 16 ? rp : 16;
  const size_t wy = (size_t)CG_MAX_T * rr * sizeof(double);
  const size_t pb = (size_t)cg_lst_slabs(n) * (size_t)((T + 15) / 16 * 16) * rr * sizeof(double);
  return run(device, {opt(rd(Ls, ls_len)), rd(dis, dis_len), opt(rd(Cinv, cinv_len)), rd(R, r_len), io(Z, z_len),
                      opt(io(C, c_len)), scratch(wy), scratch(wy), scratch(pb)},
             [&](const Dev &d) {
               if (C) launch_cg_capacitance(0, d[0], ldn, n, r, rp, d[5]);
               if (r > 0) {
                 launch_cg_lst(0, d[0], ldn, n, r, rp, d[1], d[3], ld, T, d[8], d[6]);
                 launch_cg_small_mm(0, d[2], r, rp, d[6], T, d[7]);
               }
               launch_cg_precond(0, d[0], ldn, n, r, rp, d[1], d[3], d[7], ld, T, d[4]);
             });
}

// ---- the kernels of gogp_cg_lml_gradient: the pair reduction, the probes, the host's quadrature
extern "C" int gogp_test_cg_grad(int device, const gogp_test_kparams *kparams, const double *X, int64_t x_len, int64_t n,
                                 const double *A, int64_t a_len, const double *B, int64_t b_len, int64_t ld, int S,
                                 double scale, int accumulate, double *out /* GOGP_TEST_NACC */) {
  if (!kparams || !X || !A || !B || !out) return GOGP_EARG;
  if (!kparams_ok(kparams, 1, ard_dims_of(kparams), 0, 1, 0) || kparams->nevents != 0) return GOGP_EARG;
  if (n < 1 || n > (1 << 16) || ld < n || S < 1 || S > 4 * CG_MAX_T || !std::isfinite(scale)) return GOGP_EARG;
  if (x_len < n * kparams->ndim || !covers(a_len, 0, ld, S, n, 1, 0) || !covers(b_len, 0, ld, S, n, 1, 0)) return GOGP_EARG;
  const DevParams hp = to_dev(*kparams);
  return run(device, {rd(&hp, 1, sizeof hp), rd(X, x_len), rd(A, a_len), rd(B, b_len), io(out, NACC),
                      scratch((size_t)cg_grad_blocks(n) * NACC * sizeof(double))},
             [&](const Dev &d) {
               launch_cg_grad(0, d.as<DevParams>(0), kparams->ndim, ard_dims_of(kparams), d[1], n, d[2], d[3], ld, S, scale,
                              d[5], d[4], accumulate != 0);
             });
}

extern "C" int gogp_test_cg_probes(int device, const double *Ls, int64_t ls_len, int64_t ldn, int64_t n, int r,
                                   const double *dd, int64_t d_len, const double *Xi, int64_t xi_len, int64_t ldxi,
                                   int64_t ld, int T, double *Z, int64_t z_len) {
  if (!dd || !Xi || !Z || !cg_dims_ok(ld, n, T) || r < 0 || r > GOGP_CG_MAX_RANK || d_len < n) return GOGP_EARG;
  if (ldxi < n + r || !covers(xi_len, 0, ldxi, T, n + r, 1, 0) || !cg_block_ok(z_len, ld, n, T)) return GOGP_EARG;
  if (r > 0 ? (!Ls || ldn < n || !covers(ls_len, 0, ldn, r, n, 1, 0)) : (Ls || ls_len != 0)) return GOGP_EARG;
  return run(device, {opt(rd(Ls, ls_len)), rd(dd, d_len), rd(Xi, xi_len), io(Z, z_len)},
             [&](const Dev &d) { launch_cg_probes(0, d[0], ldn, n, r, d[1], d[2], ldxi, ld, T, d[3]); });
}

extern "C" int gogp_test_cg_quadrature(const double *a, const double *beta, int64_t m, double rho0, double *out) {
  if (!out || m < 0 || m > (1 << 20) || (m > 0 && (!a || !beta))) return GOGP_EARG;
  *out = cg_lanczos_quadrature(a, beta, 1, (int)m, rho0);
  return GOGP_OK;
}

// ---- vecchia.hip ---------------------------------------------------------------------------------------------------------
extern "C" int gogp_test_vecchia_blocks(int64_t targets, int max_blocks) {
  return targets < 1 || max_blocks < 0 ? -1 : vecchia_blocks(targets, max_blocks);
}

extern "C" int gogp_test_vecchia(int device, const gogp_test_kparams *kparams, int produce, int grad, const double *X,
                                 int64_t x_len, const double *y, int64_t y_len, const double *v, int64_t v_len, int64_t n,
                                 const double *Z, int64_t z_len, int64_t targets, const int32_t *nbr, int64_t nbr_len, int m,
                                 double *terms, int64_t terms_len, double *partials, int64_t partials_len, double *vpart,
                                 int64_t vpart_len, double *value, int64_t *info, int max_blocks) {
  if (!kparams || !value || !info || max_blocks < 0) return GOGP_EARG;
  if (!kparams_ok(kparams, 1, ard_dims_of(kparams), 0, 1, 0) || kparams->nevents != 0) return GOGP_EARG;
  const int D = kparams->ndim;
  if (n < 1 || n > (1 << 20) || targets < 1 || targets > (1 << 20) || m < 0 || m > GOGP_VECCHIA_MAX_M) return GOGP_EARG;
  if (!produce && targets != n) return GOGP_EARG;
  if (x_len < n * D || y_len < n || (v ? v_len < n : v_len != 0)) return GOGP_EARG;
  if (m > 0 ? (!nbr || nbr_len < targets * m) : (nbr || nbr_len != 0)) return GOGP_EARG;
  if (gogp_vecchia_check(nbr, targets, m, n, produce ? 0 : 1) != GOGP_OK) return GOGP_EARG;
  const int blocks = vecchia_blocks(targets, max_blocks);
  const bool want_grad = !produce && grad != 0;
  if (produce ? (!Z || z_len < targets * D || !terms || terms_len < 2 * targets || partials || vpart)
              : (Z || z_len != 0 || (terms ? terms_len < 3 * n : terms_len != 0) || !vpart || vpart_len < blocks))
    return GOGP_EARG;
  if (want_grad ? (!partials || partials_len < (int64_t)blocks * NACC) : (partials || partials_len != 0)) return GOGP_EARG;
  const DevParams hp = to_dev(*kparams);
  const std::vector<Arr> arrs = {rd(&hp, 1, sizeof hp), rd(X, x_len), rd(y, y_len), opt(rd(v, v_len)), opt(rd(Z, z_len)),
                                 opt(rd(nbr, nbr_len, 4)), opt(io(terms, terms_len)), opt(io(partials, partials_len)),
                                 opt(io(vpart, vpart_len)), io(value, 1), io(info, 1),
                                 scratch((size_t)blocks * sizeof(long long)), scratch(NACC * sizeof(double))};
  if (!have(arrs)) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    if (produce)
      launch_vecchia_produce(0, d.as<DevParams>(0), D, d[1], d[2], d[3], d[4], targets, d.as<int>(5), m, d[6],
                             d[6] + targets, d.as<long long>(11), d.as<long long>(10), max_blocks);
    else
      launch_vecchia_observe(0, d.as<DevParams>(0), D, ard_dims_of(kparams), d[1], d[2], d[3], n, d.as<int>(5), m, d[6], d[7],
                             d[8], d.as<long long>(11), d[12], d[9], d.as<long long>(10), max_blocks);
  });
}

// ---- vecchia_knn.hip ------------------------------------------------------------------------------------------------------
extern "C" int gogp_test_vecchia_knn_plan(int64_t targets, int64_t n, int m, int64_t out[3]) {
  if (!out || targets < 1 || n < 1 || m < 0 || m > GOGP_VECCHIA_MAX_M) return GOGP_EARG;
  const VknnPlan p = vknn_plan(targets, n, m);
  out[0] = p.tile, out[1] = p.slabs, out[2] = (int64_t)p.ws_bytes;
  return GOGP_OK;
}

extern "C" int gogp_test_vecchia_knn(int device, const double *X, int64_t x_len, int64_t n, int ndim, const double *Z,
                                     int64_t z_len, int64_t targets, const double *lengths, int m, int slabs, int tile_cap,
                                     int32_t *nbr, int64_t nbr_len, double *d2, int64_t d2_len, double *xs, int64_t xs_len) {
  if (!X || !xs || ndim < 1 || ndim > GOGP_MAX_NDIM || m < 0 || m > GOGP_VECCHIA_MAX_M) return GOGP_EARG;
  if (slabs < 0 || slabs > 256 || tile_cap < 0) return GOGP_EARG;
  if (n < 1 || n > (1 << 20) || targets < 1 || targets > (1 << 20)) return GOGP_EARG;
  if (Z ? z_len < targets * ndim : (z_len != 0 || targets != n)) return GOGP_EARG;
  if (x_len < n * ndim || xs_len < n * ndim) return GOGP_EARG;
  if (m > 0 && (!nbr || !d2 || nbr_len < targets * m || d2_len < targets * m)) return GOGP_EARG;
  if (lengths)
    for (int d = 0; d < ndim; ++d)
      if (!(lengths[d] > 0.0) || !std::isfinite(lengths[d])) return GOGP_EARG;
  const VknnPlan p = vknn_plan(targets, n, m, slabs);
  if (p.ws_bytes > ((size_t)1 << 28)) return GOGP_EARG;
  const std::vector<Arr> arrs = {rd(X, x_len), opt(rd(Z, z_len)), opt(rd(lengths, lengths ? ndim : 0)),
                                 opt(io(nbr, nbr_len, 4)), opt(io(d2, d2_len)), io(xs, xs_len), scratch(p.ws_bytes),
                                 scratch(Z ? (size_t)targets * ndim * sizeof(double) : 0)};
  if (!have(arrs)) return GOGP_EARG;
  return run(device, arrs, [&](const Dev &d) {
    launch_vknn_scale(0, d[0], n, ndim, d[2], d[5]);
    if (Z) launch_vknn_scale(0, d[1], targets, ndim, d[2], d[7]);
    launch_vknn(0, d[5], n, Z ? d[7] : nullptr, targets, ndim, m, slabs, tile_cap, d.as<void>(6), d.as<int>(3), d[4]);
  });
}
