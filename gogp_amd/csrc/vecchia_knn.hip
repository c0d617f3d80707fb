// vecchia_knn.hip -- neighbour tables of Vecchia's approximation built on the device (gogp_vecchia_neighbours,
// gogp_vecchia_set_data_nearest, gogp_vecchia_reneighbour, gogp_vecchia_produce_nearest; vecchia_api.hip orchestrates).
//
// The definition is that of gogp_amd/vecchia.py (nearest / nearest_to), and the table is the host's integer for integer:
//     xs = x / lengths per dimension (a plain IEEE fp64 division; lengths == nullptr: xs = x),
//     d2(a, b) = sum_d (a_d - b_d)^2, from the DIFFERENCES, in index order of d, every product rounded before it is added
//                (no fused multiply-add: vknn_d2 switches contraction off, the Makefile's -ffp-contract=on notwithstanding),
//     row i of the causal table: the m smallest keys (d2(xs_i, xs_j), j) over j < i;  row z of the query table: over all j < n.
// Keys are ordered by value, then by index; a row lists them nearest first, then -1; a distance that is not finite (an
// overflow, a NaN) is never taken.  The key is a strict total order, so the m smallest keys are one set in one sequence:
// the result cannot depend on the grid or on how the candidates are cut into slabs, and merging partial lists by key is exact.
//
// One lane owns one target, one wave (= one workgroup) a tile of VKNN_TILE = 64 targets.  The lane keeps its scaled row in
// registers (DT = ndim <= 8: an instance per dimension count) or in LDS at stride ndim | 1 (DT == 0), and its sorted list of at
// most m (d2, j) entries in LDS laid out [entry][lane]: the lanes of a wave that touch the same entry index touch 64
// consecutive words.  CAP = 32 or 64 entries per lane (m <= 31 / m <= 63): 24 or 48 KiB a wave, so six or three waves share a
// CU's LDS.  The candidate is the same address for the whole wave: a uniform load, 3 fp64 VALU instructions per dimension
// and one compare against the lane's worst entry; the insertion is a divergent shift that becomes rare once the lists
// have warmed up.  Within one scan the candidates come in ascending j, so `d2 < worst` is the whole test and an entry moves
// only past strictly larger distances.
//
// A work unit is (tile of targets) x (slab of candidates); unit u = tile_rank * S + slab, and the causal form ranks the
// tiles in DESCENDING order of their scan length so that the triangle balances over the CUs.  S == 1: the unit writes the
// table's rows.  S > 1 (few targets): it writes a partial list per (target, slab) to a transient workspace, and
// vknn_merge_kernel inserts the partial lists of a target in slab order into one list -- slabs ascend in j, so the same
// insertion applies.  vknn_plan gives S and the workspace as a function of (targets, n, m) alone, never of the device.
// No atomics, no spin-waits, vector stores only.
#include <algorithm>

#include "common.h"

namespace gogp {

constexpr int VKNN_UNITS = 512;    // work units a launch of few targets aims for
constexpr int VKNN_SLAB_MIN = 256;  // candidates a slab holds at least

// squared distance of the lane's row to a candidate, unfused: one multiply and two adds per dimension
template <class A, class B>
__device__ __forceinline__ double vknn_d2(A &&a, B &&b, int D) {
#pragma clang fp contract(off)
  const double t0 = a(0) - b(0);
  double s = t0 * t0;  // 0 + u is u in every bit: a square is never -0
  for (int d = 1; d < D; ++d) {
    const double t = a(d) - b(d);
    const double u = t * t;
    s = s + u;
  }
  return s;
}

// the lane's sorted list in LDS: entry e of lane l at e * 64 + l
struct VknnList {
  double *d2;
  int *idx;
  int lane, m, cnt;
  double worst;  // d2 of the last entry of a full list; +inf while there is room (then every finite distance is taken)
  __device__ __forceinline__ void init(double *d2s, int *idxs, int l, int mm) {
    d2 = d2s, idx = idxs, lane = l, m = mm, cnt = 0;
    worst = mm > 0 ? INFINITY : -INFINITY;
  }
  // candidates arrive so that an entry already listed with the same distance has the lower index
  __device__ __forceinline__ void offer(double v, int j) {
    if (!(v < worst)) return;
    int p = cnt < m ? cnt : m - 1;
    while (p > 0) {
      const double w = d2[(p - 1) * 64 + lane];
      if (!(w > v)) break;
      d2[p * 64 + lane] = w;
      idx[p * 64 + lane] = idx[(p - 1) * 64 + lane];
      --p;
    }
    d2[p * 64 + lane] = v;
    idx[p * 64 + lane] = j;
    if (cnt < m) ++cnt;
    if (cnt == m) worst = d2[(m - 1) * 64 + lane];
  }
  // m entries at out (and outd unless nullptr): the list, then -1 (0.0)
  __device__ __forceinline__ void store(int *out, double *outd) const {
    for (int e = 0; e < m; ++e) {
      out[e] = e < cnt ? idx[e * 64 + lane] : -1;
      if (outd) outd[e] = e < cnt ? d2[e * 64 + lane] : 0.0;
    }
  }
};

// xs[i] = x[i] / lengths[i % D] (lengths == nullptr: a copy)
__global__ __launch_bounds__(256) void vknn_scale_kernel(const double *__restrict__ x, long count, int D,
                                                         const double *__restrict__ lengths, double *__restrict__ xs) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256)
    xs[i] = lengths ? x[i] / lengths[i % D] : x[i];
}

// Xs: n scaled rows (the candidates).  Zs == nullptr: the causal form, target i = row i of Xs against j < i (targets == n);
// else the targets are the rows of Zs against all j < n.  S == 1: nbr (targets x m) and, unless nullptr, d2out; S > 1: the
// partial lists wsi / wsd ((target * S + slab) * m entries each).
template <int CAP, int DT>
__global__ __launch_bounds__(64) void vknn_kernel(const double *__restrict__ Xs, long n, const double *__restrict__ Zs,
                                                  long targets, int D, int m, int S, long slab_len,
                                                  int *__restrict__ nbr, double *__restrict__ d2out,
                                                  int *__restrict__ wsi, double *__restrict__ wsd) {
  extern __shared__ double sm[];
  double *d2s = sm;                                       // [CAP][64]
  int *idxs = reinterpret_cast<int *>(d2s + CAP * 64);    // [CAP][64]
  double *rowsm = reinterpret_cast<double *>(idxs + CAP * 64);  // DT == 0: [64][D | 1]
  const int lane = threadIdx.x;
  const bool causal = Zs == nullptr;
  const long tiles = (targets + 63) / 64, units = tiles * S;
  const int rs = D | 1;

  for (long u = blockIdx.x; u < units; u += gridDim.x) {
    const long rank = u / S;
    const int slab = (int)(u - rank * S);
    const long tile = causal ? tiles - 1 - rank : rank;
    const long t0 = tile * 64, t1 = t0 + 64 < targets ? t0 + 64 : targets;
    const long i = t0 + lane;
    const bool live = i < t1;
    // the candidates of this unit: the slab, cut at the last earlier row of the tile's last target
    const long c0 = (long)slab * slab_len;
    long c1 = c0 + slab_len < n ? c0 + slab_len : n;
    if (causal && c1 > t1 - 1) c1 = t1 - 1;
    const long lim = causal ? i : n;  // this lane takes j < lim

    const double *mine = (causal ? Xs : Zs) + (live ? i : t0) * D;
    double xr[DT > 0 ? DT : 1];
    if (DT > 0) {
#pragma unroll
      for (int d = 0; d < DT; ++d) xr[d] = mine[d];
    } else {
      __syncthreads();  // the previous unit's readers are done
      for (int d = 0; d < D; ++d) rowsm[lane * rs + d] = mine[d];
      __syncthreads();
    }
    const double *myrow = rowsm + lane * rs;
    auto dist = [&](long j) {
      const double *c = Xs + j * D;  // uniform over the wave
      if (DT > 0)
        return vknn_d2([&](int d) { return xr[d]; }, [&](int d) { return c[d]; }, DT);
      return vknn_d2([&](int d) { return myrow[d]; }, [&](int d) { return c[d]; }, D);
    };

    VknnList L;
    L.init(d2s, idxs, lane, live ? m : 0);
    long j = c0;
    // U independent distances, then the offers in order; a candidate row is ndim pairs of scalar registers, so U is what
    // keeps U rows within them
    constexpr int U = DT >= 1 && DT <= 4 ? 4 : 2;
    for (; j + U <= c1; j += U) {
      double v[U];
#pragma unroll
      for (int k = 0; k < U; ++k) v[k] = dist(j + k);
#pragma unroll
      for (int k = 0; k < U; ++k)
        if (j + k < lim) L.offer(v[k], (int)(j + k));
    }
    for (; j < c1; ++j) {
      const double v = dist(j);
      if (j < lim) L.offer(v, (int)j);
    }
    if (live) {
      if (S == 1) L.store(nbr + i * m, d2out ? d2out + i * m : nullptr);
      else L.store(wsi + (i * S + slab) * m, wsd + (i * S + slab) * m);
    }
  }
}

// one lane per target: the S partial lists of a target, in slab order, into one list
template <int CAP>
__global__ __launch_bounds__(64) void vknn_merge_kernel(const int *__restrict__ wsi, const double *__restrict__ wsd,
                                                        long targets, int m, int S, int *__restrict__ nbr,
                                                        double *__restrict__ d2out) {
  extern __shared__ double sm[];
  double *d2s = sm;
  int *idxs = reinterpret_cast<int *>(d2s + CAP * 64);
  const int lane = threadIdx.x;
  for (long t0 = (long)blockIdx.x * 64; t0 < targets; t0 += (long)gridDim.x * 64) {
    const long i = t0 + lane;
    if (i >= targets) continue;
    VknnList L;
    L.init(d2s, idxs, lane, m);
    for (int s = 0; s < S; ++s) {
      const int *pi = wsi + (i * S + s) * m;
      const double *pd = wsd + (i * S + s) * m;
      for (int e = 0; e < m; ++e) {
        const int j = pi[e];
        const double v = pd[e];
        if (j < 0 || !(v < L.worst)) break;  // a partial list ascends: nothing behind this entry can be taken either
        L.offer(v, j);
      }
    }
    L.store(nbr + i * m, d2out ? d2out + i * m : nullptr);
  }
}

// The split of a search of `targets` targets over n candidates: tiles of VKNN_TILE targets; S slabs of
// ceil(n / S) candidates (slab s: [s L, min(n, (s + 1) L))), S == 1 from VKNN_UNITS / 2 tiles on, else the fewest
// that give VKNN_UNITS work units while a slab keeps VKNN_SLAB_MIN candidates.  tiles * S < VKNN_UNITS + VKNN_UNITS / 2
// wherever S > 1, so the workspace of 12 bytes per (target, slab, entry) stays under VKNN_WS_MAX.
VknnPlan vknn_plan(int64_t targets, int64_t n, int m, int slabs) {
  VknnPlan p;
  p.tile = VKNN_TILE;
  const int64_t tiles = (std::max<int64_t>(targets, 1) + VKNN_TILE - 1) / VKNN_TILE;
  int64_t S = 1;
  if (slabs > 0) {
    S = slabs;
  } else if (tiles < VKNN_UNITS / 2) {
    S = (VKNN_UNITS + tiles - 1) / tiles;
    S = std::min<int64_t>(S, std::max<int64_t>(n / VKNN_SLAB_MIN, 1));
  }
  p.slabs = (int)S;
  p.slab_len = std::max<int64_t>((std::max<int64_t>(n, 1) + S - 1) / S, 1);
  p.ws_bytes = S > 1 && m > 0 ? (size_t)tiles * VKNN_TILE * (size_t)S * (size_t)m * 12 : 0;
  return p;
}

void launch_vknn_scale(hipStream_t s, const double *x, int64_t rows, int ndim, const double *lengths, double *xs) {
  const int64_t count = rows * ndim;
  if (count <= 0) return;
  const int blocks = (int)std::min<int64_t>((count + 255) / 256, 4096);
  GOGP_KLAUNCH(vknn_scale_kernel, dim3(blocks), dim3(256), 0, s, x, (long)count, ndim, lengths, xs);
}

static size_t vknn_lds_bytes(int cap, int dt, int ndim) {
  return (size_t)cap * 64 * 12 + (dt > 0 ? 0 : (size_t)64 * (ndim | 1) * sizeof(double));
}

template <int CAP, int DT>
static void vknn_launch1(hipStream_t s, int blocks, const double *Xs, int64_t n, const double *Zs, int64_t targets, int ndim,
                         int m, const VknnPlan &p, int *nbr, double *d2out, int *wsi, double *wsd) {
  const size_t lds = vknn_lds_bytes(CAP, DT, ndim);
  if (lds > 64 * 1024)  // CAP = 64 with the rows in LDS beyond ndim = 31: raised per launch, as vecchia.hip's vc_launch does
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&vknn_kernel<CAP, DT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)vknn_lds_bytes(CAP, DT, GOGP_MAX_NDIM));
  GOGP_KLAUNCH((vknn_kernel<CAP, DT>), dim3(blocks), dim3(64), lds, s, Xs, (long)n, Zs, (long)targets, ndim, m, p.slabs,
               (long)p.slab_len, nbr, d2out, wsi, wsd);
}

template <int CAP>
static void vknn_launch(hipStream_t s, int blocks, const double *Xs, int64_t n, const double *Zs, int64_t targets, int ndim,
                        int m, const VknnPlan &p, int *nbr, double *d2out, int *wsi, double *wsd) {
#define GOGP_VKNN_CASE(DT) \
  case DT: vknn_launch1<CAP, DT>(s, blocks, Xs, n, Zs, targets, ndim, m, p, nbr, d2out, wsi, wsd); break
  switch (ndim <= 8 ? ndim : 0) {
    GOGP_VKNN_CASE(1);
    GOGP_VKNN_CASE(2);
    GOGP_VKNN_CASE(3);
    GOGP_VKNN_CASE(4);
    GOGP_VKNN_CASE(5);
    GOGP_VKNN_CASE(6);
    GOGP_VKNN_CASE(7);
    GOGP_VKNN_CASE(8);
    default: vknn_launch1<CAP, 0>(s, blocks, Xs, n, Zs, targets, ndim, m, p, nbr, d2out, wsi, wsd); break;
  }
#undef GOGP_VKNN_CASE
}

void launch_vknn(hipStream_t s, const double *Xs, int64_t n, const double *Zs, int64_t targets, int ndim, int m, int slabs,
                 int tile_cap, void *ws, int *nbr, double *d2out) {
  if (targets <= 0 || m <= 0) return;
  const VknnPlan p = vknn_plan(targets, n, m, slabs);
  const int64_t tiles = (targets + VKNN_TILE - 1) / VKNN_TILE, units = tiles * p.slabs;
  const int blocks = (int)std::min<int64_t>(units, tile_cap > 0 ? tile_cap : INT32_MAX);
  // the workspace: the distances of every (target, slab, entry), then the indices
  double *wsd = p.slabs > 1 ? static_cast<double *>(ws) : nullptr;
  int *wsi = p.slabs > 1 ? reinterpret_cast<int *>(wsd + (size_t)tiles * VKNN_TILE * p.slabs * m) : nullptr;
  int *out = p.slabs > 1 ? nullptr : nbr;
  double *outd = p.slabs > 1 ? nullptr : d2out;
  if (m < 32) vknn_launch<32>(s, blocks, Xs, n, Zs, targets, ndim, m, p, out, outd, wsi, wsd);
  else vknn_launch<64>(s, blocks, Xs, n, Zs, targets, ndim, m, p, out, outd, wsi, wsd);
  if (p.slabs == 1) return;
  const int mblocks = (int)std::min<int64_t>(tiles, tile_cap > 0 ? tile_cap : INT32_MAX);
  if (m < 32)
    GOGP_KLAUNCH((vknn_merge_kernel<32>), dim3(mblocks), dim3(64), (size_t)32 * 64 * 12, s, (const int *)wsi, (const double *)wsd,
                 (long)targets, m, p.slabs, nbr, d2out);
  else
    GOGP_KLAUNCH((vknn_merge_kernel<64>), dim3(mblocks), dim3(64), (size_t)64 * 64 * 12, s, (const int *)wsi, (const double *)wsd,
                 (long)targets, m, p.slabs, nbr, d2out);
}

}  // namespace gogp
