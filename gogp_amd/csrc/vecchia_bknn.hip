// vecchia_bknn.hip -- the tables of Vecchia's block family built on the device (gogp_vecchia_blocks_nearest,
// gogp_vecchia_blocks_set_data_nearest, gogp_vecchia_blocks_reneighbour, gogp_vecchia_blocks_produce_nearest; vecchia_api.hip
// orchestrates).
//
// The definition is that of gogp_amd/vecchia.py (block_nearest / group_nearest_to), and the table is the host's integer for
// integer.  A query is the centroid of a block of t consecutive scaled rows,
//     cen_k = (xs_s + xs_{s+1} + ... + xs_{e-1}) / (e - s),  summed in index order, one IEEE add per row and one IEEE division
//             by the count (a block of one row is the row itself, undivided),
// and its list the min(c, .) smallest keys (d2(cen_k, xs_j), j) over j < s_k = k t (the causal form) or over all j < n (the
// query form), with xs, d2 and the order of the keys as vecchia_knn.hip states them: differences, index order of d, every
// product rounded before it is added, value then index, nearest first, then -1, a distance that is not finite never taken.
//
// This is the opposite corner of vecchia_knn.hip: few queries (n / t), each over many candidates and each with a long list
// (up to 128 entries).  So the lanes own CANDIDATES, not queries:
//   * a workgroup of 256 lanes takes a work unit: a tile of QT <= 8 consecutive queries x a slab of candidates.  The QT
//     centroids sit in LDS and are read as broadcasts; lane l reads the candidate rows c0 + l, c0 + l + 256, ... (a wave's
//     rows are consecutive in memory; the next row is in flight while this one is measured), and one candidate load serves QT
//     distances.  The causal tile scans up to the cut-off of its last query, every query masks j < s_k for itself.
//   * per query LDS holds 2 CAP keys: [0, c) the best keys so far, sorted; [c, 2 CAP) pending keys.  A lane whose key beats
//     the query's threshold -- the c-th best at the last sort -- appends it.  The slot is pending + (keys of the waves
//     before mine, from the waves' ballot counts exchanged through LDS, taken in wave order) + (population count of my wave's
//     ballot below my lane).  No atomics, no spin-waits.  A wave's chunk is at most 64 keys and the pending part at least
//     CAP >= 64, so a chunk that does not fit waits for one sort.
//   * the sort: all 256 lanes, a bitonic network over the 2 CAP keys in LDS, ordered by (d2, j); the first c stay and the
//     threshold drops.  The key is a strict total order, so the kept set and its sequence depend on nothing but the keys
//     offered: not on the arrival order, the grid, QT or the slabs, and merging partial lists by key is exact.
//   * CAP = 64 (c <= 64) or 128; the candidate row in DT = ndim <= 8 registers (an instance per dimension count) or read
//     dimension by dimension with QT running sums (DT == 0).
// unit u = tile_rank * S + slab; the causal form ranks the tiles in DESCENDING order of their scan length.  S == 1: the unit
// writes the lists.  S > 1 (few queries): it writes a partial sorted list per (query, slab) to a transient workspace and
// bknn_merge_kernel, one workgroup per query, offers them to the same buffer.  bknn_plan gives QT, S and the workspace
// as a function of (queries, n, c) alone, never of the device.  bknn_pack_kernel writes the table the block kernels read.
// Vector stores only.
#include <algorithm>
#include <climits>

#include "common.h"

namespace gogp {

constexpr int BKNN_UNITS = 512;     // work units a launch of few queries aims for
constexpr int BKNN_SLAB_MIN = 256;  // candidates a slab holds at least
constexpr int BKNN_WG = 256, BKNN_WAVES = BKNN_WG / 64;

// s + (a - b)^2, unfused
__device__ __forceinline__ double bknn_acc(double s, double a, double b) {
#pragma clang fp contract(off)
  const double t = a - b;
  const double u = t * t;
  return s + u;  // 0 + u is u in every bit: a square is never -0
}

__device__ __forceinline__ bool bknn_less(double ad, int aj, double bd, int bj) { return ad < bd || (ad == bd && aj < bj); }

__device__ __forceinline__ int bknn_rank(unsigned long long ballot) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

// cen[k][d] of the blocks k of t consecutive rows of xs (the last one shorter)
__global__ __launch_bounds__(256) void bknn_centroid_kernel(const double *__restrict__ xs, long rows, int D, long t, long blocks,
                                                            double *__restrict__ cen) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;  // a workgroup: 256 / D blocks
  if (p >= blocks * D) return;
  const long k = p / D;
  const int d = (int)(p - k * D);
  const long s = k * t, e = s + t < rows ? s + t : rows;
  double a = xs[s * D + d];
  for (long i = s + 1; i < e; ++i) a = a + xs[i * D + d];
  cen[p] = e - s > 1 ? a / (double)(e - s) : a;
}

// One query's key buffer in LDS and the copies of its state that every wave keeps for itself (they are computed alike by
// all lanes; a wave reads and writes its own copy only, so no wave waits for another's).
template <int CAP>
struct BknnBuf {
  static constexpr int N2 = 2 * CAP;
  double *kd;  // [N2]
  int *kj;     // [N2]
  int *pend;   // [BKNN_WAVES] pending keys
  double *thrd;  // [BKNN_WAVES] the threshold: key c - 1 at the last sort
  int *thrj;     // [BKNN_WAVES]

  __device__ __forceinline__ void reset(int tid) {
    if (tid < N2) kd[tid] = INFINITY, kj[tid] = INT_MAX;
    if (tid < BKNN_WAVES) pend[tid] = 0, thrd[tid] = INFINITY, thrj[tid] = INT_MAX;
  }
  // all lanes: [0, c + pending) sorted by key, the rest padding; the threshold follows.  Ends behind a barrier.
  __device__ __forceinline__ void sort(int c, int filled, int tid) {
    if (tid < N2 && tid >= filled) kd[tid] = INFINITY, kj[tid] = INT_MAX;
    __syncthreads();
    for (int k = 2; k <= N2; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        const int p = tid ^ j;
        if (tid < N2 && p > tid) {
          const double a = kd[tid], b = kd[p];
          const int aj = kj[tid], bj = kj[p];
          if (bknn_less(b, bj, a, aj) == ((tid & k) == 0)) kd[tid] = b, kd[p] = a, kj[tid] = bj, kj[p] = aj;
        }
        __syncthreads();
      }
    if ((tid & 63) == 0) {
      const int w = tid >> 6;
      thrd[w] = kd[c - 1], thrj[w] = kj[c - 1], pend[w] = 0;
    }
  }
  // all lanes, behind the barrier that published cnt (the waves' counts of `pred`): the keys offered go to the pending
  // part in wave order
  __device__ __forceinline__ void place(const int *cnt, int c, bool pred, double d, int j, int tid) {
    const int w = tid >> 6;
    int pn = __builtin_amdgcn_readfirstlane(pend[w]);
    const int rank = bknn_rank(__ballot(pred));
    for (int v = 0; v < BKNN_WAVES; ++v) {
      const int cv = __builtin_amdgcn_readfirstlane(cnt[v]);
      if (cv == 0) continue;
      if (pn + cv > N2 - c) {
        sort(c, c + pn, tid);
        pn = 0;
      }
      if (pred && v == w) kd[c + pn + rank] = d, kj[c + pn + rank] = j;
      pn += cv;
    }
    if ((tid & 63) == 0) pend[w] = pn;
  }
  // all lanes: the final sort, then c entries at out / outd (the list, then -1 / 0.0) and the count at *outc (nullptr: none)
  __device__ __forceinline__ void finish(int c, int tid, int *out, double *outd, int *outc) {
    sort(c, c + __builtin_amdgcn_readfirstlane(pend[tid >> 6]), tid);
    if (tid < c) {
      const int j = kj[tid];
      const bool have = j != INT_MAX;
      out[tid] = have ? j : -1;
      if (outd) outd[tid] = have ? kd[tid] : 0.0;
      if (outc) {
        if (have && (tid == c - 1 || kj[tid + 1] == INT_MAX)) *outc = tid + 1;
        if (!have && tid == 0) *outc = 0;
      }
    }
  }
};

// LDS of the selection: QT key buffers, the wave copies of their state, the limits, two sets of ballot counts, the centroids
template <int CAP>
struct BknnSmem {
  double *kd, *thrd, *cen;
  int *kj, *pend, *thrj, *lim, *cnt;
  __device__ __host__ static size_t bytes(int qt, int D) {
    return (size_t)qt * (2 * CAP * 12 + BKNN_WAVES * 16 + 4 + 2 * BKNN_WAVES * 4 + (size_t)D * 8) + 64;
  }
  __device__ __forceinline__ BknnSmem(double *base, int qt, int D) {
    kd = base;
    thrd = kd + (size_t)qt * 2 * CAP;
    cen = thrd + qt * BKNN_WAVES;
    kj = reinterpret_cast<int *>(cen + (size_t)qt * D);
    pend = kj + (size_t)qt * 2 * CAP;
    thrj = pend + qt * BKNN_WAVES;
    lim = thrj + qt * BKNN_WAVES;
    cnt = lim + qt;  // [2][qt][BKNN_WAVES]
  }
  __device__ __forceinline__ BknnBuf<CAP> buf(int q) const {
    return {kd + (size_t)q * 2 * CAP, kj + (size_t)q * 2 * CAP, pend + q * BKNN_WAVES, thrd + q * BKNN_WAVES, thrj + q * BKNN_WAVES};
  }
};

constexpr int BKNN_QT_MAX = 8;

// Xs: n scaled rows (the candidates); Cen: nq centroids.  t > 0: the causal form, query k takes j < min(k t, n); t == 0: all
// j < n.  S == 1: nbr (nq x c), cntout (nq) and, unless nullptr, d2out; S > 1: the partial lists wsi / wsd ((query * S + slab)
// * c entries each).  1 <= c <= CAP, 1 <= QT <= BKNN_QT_MAX, gridDim.x = ceil(nq / QT) * S.
template <int CAP, int DT>
__global__ __launch_bounds__(BKNN_WG) void bknn_select_kernel(const double *__restrict__ Xs, long n, const double *__restrict__ Cen,
                                                              long nq, long t, int D, int c, int QT, int S, long slab_len,
                                                              int *__restrict__ nbr, int *__restrict__ cntout,
                                                              double *__restrict__ d2out, int *__restrict__ wsi,
                                                              double *__restrict__ wsd) {
  extern __shared__ double sm[];
  const int DD = DT > 0 ? DT : D;
  const BknnSmem<CAP> L(sm, QT, DD);
  const int tid = threadIdx.x, wave = tid >> 6;
  const long tiles = (nq + QT - 1) / QT;
  const long rank = blockIdx.x / S;
  const int slab = (int)(blockIdx.x - rank * S);
  const long tile = t > 0 ? tiles - 1 - rank : rank;
  const long q0 = tile * QT;
  const int live = (int)(nq - q0 < QT ? nq - q0 : QT);  // queries of this tile

  for (int q = 0; q < QT; ++q) L.buf(q).reset(tid);
  if (tid < QT) {
    long lim = 0;
    if (tid < live) lim = t > 0 ? ((q0 + tid) * t < n ? (q0 + tid) * t : n) : n;
    L.lim[tid] = (int)lim;
  }
  for (int i = tid; i < QT * DD; i += BKNN_WG) L.cen[i] = i < live * DD ? Cen[q0 * DD + i] : 0.0;
  // the candidates of this unit: the slab, cut at the limit of the tile's last query
  const long c0 = (long)slab * slab_len;
  long c1 = c0 + slab_len < n ? c0 + slab_len : n;
  {
    const long last = t > 0 ? ((q0 + live - 1) * t < n ? (q0 + live - 1) * t : n) : n;
    if (c1 > last) c1 = last;
  }
  __syncthreads();

  double xr[DT > 0 ? DT : 1], xn[DT > 0 ? DT : 1];
  auto load = [&](long j, double *x) {  // row j, j < c1
    if (DT > 0 && DT % 2 == 0) {
      const double2 *p = reinterpret_cast<const double2 *>(Xs + j * DT);
#pragma unroll
      for (int d = 0; d < DT / 2; ++d) {
        const double2 v = p[d];
        x[2 * d] = v.x, x[2 * d + 1] = v.y;
      }
    } else {
#pragma unroll
      for (int d = 0; d < DT; ++d) x[d] = Xs[j * DT + d];
    }
  };
  if (DT > 0 && c0 < c1) load(c0 + tid < c1 ? c0 + tid : c1 - 1, xn);

  int par = 0;
  for (long base = c0; base < c1; base += BKNN_WG, par ^= 1) {
    const long j = base + tid;
    const bool inb = j < c1;
    const long jr = inb ? j : c1 - 1;
    double dq[BKNN_QT_MAX];
    if (DT > 0) {
#pragma unroll
      for (int d = 0; d < DT; ++d) xr[d] = xn[d];
      if (base + BKNN_WG < c1) load(j + BKNN_WG < c1 ? j + BKNN_WG : c1 - 1, xn);
#pragma unroll
      for (int q = 0; q < BKNN_QT_MAX; ++q) {
        dq[q] = 0.0;
        if (q < QT) {
#pragma unroll
          for (int d = 0; d < DT; ++d) dq[q] = bknn_acc(dq[q], L.cen[q * DT + d], xr[d]);
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < BKNN_QT_MAX; ++q) dq[q] = 0.0;
      const double *row = Xs + jr * D;
      for (int d = 0; d < D; ++d) {
        const double x = row[d];
#pragma unroll
        for (int q = 0; q < BKNN_QT_MAX; ++q)
          if (q < QT) dq[q] = bknn_acc(dq[q], L.cen[q * D + d], x);
      }
    }
    unsigned mask = 0;
    int *cnt = L.cnt + par * QT * BKNN_WAVES;
#pragma unroll
    for (int q = 0; q < BKNN_QT_MAX; ++q) {
      if (q < QT) {
        const bool pred = inb && j < L.lim[q] && dq[q] <= 1.7976931348623157e308 &&
                          bknn_less(dq[q], (int)j, L.thrd[q * BKNN_WAVES + wave], L.thrj[q * BKNN_WAVES + wave]);
        const unsigned long long b = __ballot(pred);
        if ((tid & 63) == 0) cnt[q * BKNN_WAVES + wave] = __popcll(b);
        mask |= (unsigned)pred << q;
      }
    }
    __syncthreads();
    for (int q = 0; q < QT; ++q) {
      const int *cq = cnt + q * BKNN_WAVES;
      if (__builtin_amdgcn_readfirstlane(cq[0] | cq[1] | cq[2] | cq[3]) == 0) continue;
      double d = dq[0];
#pragma unroll
      for (int k = 1; k < BKNN_QT_MAX; ++k) d = q == k ? dq[k] : d;
      L.buf(q).place(cq, c, (mask >> q) & 1u, d, (int)j, tid);
    }
  }
  __syncthreads();
  for (int q = 0; q < live; ++q) {
    const long g = q0 + q;
    if (S == 1) L.buf(q).finish(c, tid, nbr + g * c, d2out ? d2out + g * c : nullptr, cntout + g);
    else L.buf(q).finish(c, tid, wsi + (g * S + slab) * c, wsd + (g * S + slab) * c, nullptr);
  }
}

// one workgroup per query: its S partial lists offered to one buffer
template <int CAP>
__global__ __launch_bounds__(BKNN_WG) void bknn_merge_kernel(const int *__restrict__ wsi, const double *__restrict__ wsd, long nq,
                                                             int c, int S, int *__restrict__ nbr, int *__restrict__ cntout,
                                                             double *__restrict__ d2out) {
  extern __shared__ double sm[];
  const BknnSmem<CAP> L(sm, 1, 0);
  const int tid = threadIdx.x, wave = tid >> 6;
  const long g = blockIdx.x;
  if (g >= nq) return;
  BknnBuf<CAP> B = L.buf(0);
  B.reset(tid);
  __syncthreads();
  int par = 0;
  for (int s = 0; s < S; ++s, par ^= 1) {
    int j = -1;
    double d = 0.0;
    if (tid < c) j = wsi[(g * S + s) * c + tid], d = wsd[(g * S + s) * c + tid];
    const bool pred = j >= 0 && bknn_less(d, j, B.thrd[wave], B.thrj[wave]);
    const unsigned long long b = __ballot(pred);
    int *cnt = L.cnt + par * BKNN_WAVES;
    if ((tid & 63) == 0) cnt[wave] = __popcll(b);
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane(cnt[0] | cnt[1] | cnt[2] | cnt[3]) != 0) B.place(cnt, c, pred, d, j, tid);
  }
  __syncthreads();
  B.finish(c, tid, nbr + g * c, d2out ? d2out + g * c : nullptr, cntout + g);
}

// The table of the block kernels from the lists: row k of nb x (t + c) holds the nc_k = cnt[k] entries of sel (nb x c; nullptr
// with c == 0), then the targets k t .. min(k t + t, n) - 1, then -1
__global__ __launch_bounds__(256) void bknn_pack_kernel(const int *__restrict__ sel, const int *__restrict__ cnt, long nb, long n,
                                                        int t, int c, int *__restrict__ tbl, int *__restrict__ nc,
                                                        int *__restrict__ nt) {
  const int w = t + c;
  const long total = nb * w;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
    const long k = p / w;
    const int a = (int)(p - k * w);
    const int ck = c > 0 ? cnt[k] : 0;
    const long s = k * t;
    const int tk = (int)(s + t < n ? t : n - s);
    tbl[p] = a < ck ? sel[k * c + a] : a < ck + tk ? (int)(s + a - ck) : -1;
    if (a == 0) nc[k] = ck, nt[k] = tk;
  }
}

// The split of a search of `queries` centroids over n candidates: tiles of qt = min(8, queries) consecutive queries; S slabs
// of ceil(n / S) candidates (slab s: [s L, min(n, (s + 1) L))), S == 1 from BKNN_UNITS / 2 tiles on, else the fewest that give
// BKNN_UNITS work units while a slab keeps BKNN_SLAB_MIN candidates.  tiles * S < BKNN_UNITS + BKNN_UNITS / 2 wherever S > 1,
// so the workspace of 12 bytes per (query of a tile, slab, entry) stays under BKNN_WS_MAX.
BknnPlan bknn_plan(int64_t queries, int64_t n, int c, int qt, int slabs) {
  BknnPlan p;
  queries = std::max<int64_t>(queries, 1);
  p.qt = qt > 0 ? qt : (int)std::min<int64_t>(BKNN_QT_MAX, queries);
  const int64_t tiles = (queries + p.qt - 1) / p.qt;
  int64_t S = 1;
  if (slabs > 0) {
    S = slabs;
  } else if (tiles < BKNN_UNITS / 2) {
    S = (BKNN_UNITS + tiles - 1) / tiles;
    S = std::min<int64_t>(S, std::max<int64_t>(n / BKNN_SLAB_MIN, 1));
  }
  p.slabs = (int)S;
  p.slab_len = std::max<int64_t>((std::max<int64_t>(n, 1) + S - 1) / S, 1);
  p.ws_bytes = S > 1 && c > 0 ? (size_t)tiles * p.qt * (size_t)S * (size_t)c * 12 : 0;
  return p;
}

void launch_bknn_centroids(hipStream_t s, const double *xs, int64_t rows, int ndim, int64_t t, double *cen) {
  if (rows <= 0) return;
  const int64_t blocks = (rows + t - 1) / t, count = blocks * ndim;
  GOGP_KLAUNCH(bknn_centroid_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, xs, (long)rows, ndim, (long)t,
               (long)blocks, cen);
}

template <int CAP, int DT>
static void bknn_launch1(hipStream_t s, const double *Xs, int64_t n, const double *Cen, int64_t nq, int64_t t, int ndim, int c,
                         const BknnPlan &p, int *nbr, int *cnt, double *d2out, int *wsi, double *wsd) {
  const size_t lds = BknnSmem<CAP>::bytes(p.qt, ndim);  // under 30 KiB at QT = 8, CAP = 128, ndim = 64
  const int64_t tiles = (nq + p.qt - 1) / p.qt;
  GOGP_KLAUNCH((bknn_select_kernel<CAP, DT>), dim3((unsigned)(tiles * p.slabs)), dim3(BKNN_WG), lds, s, Xs, (long)n, Cen, (long)nq,
               (long)t, ndim, c, p.qt, p.slabs, (long)p.slab_len, nbr, cnt, d2out, wsi, wsd);
}

template <int CAP>
static void bknn_launch(hipStream_t s, const double *Xs, int64_t n, const double *Cen, int64_t nq, int64_t t, int ndim, int c,
                        const BknnPlan &p, int *nbr, int *cnt, double *d2out, int *wsi, double *wsd) {
#define GOGP_BKNN_CASE(DT) \
  case DT: bknn_launch1<CAP, DT>(s, Xs, n, Cen, nq, t, ndim, c, p, nbr, cnt, d2out, wsi, wsd); break
  switch (ndim <= 8 ? ndim : 0) {
    GOGP_BKNN_CASE(1);
    GOGP_BKNN_CASE(2);
    GOGP_BKNN_CASE(3);
    GOGP_BKNN_CASE(4);
    GOGP_BKNN_CASE(5);
    GOGP_BKNN_CASE(6);
    GOGP_BKNN_CASE(7);
    GOGP_BKNN_CASE(8);
    default: bknn_launch1<CAP, 0>(s, Xs, n, Cen, nq, t, ndim, c, p, nbr, cnt, d2out, wsi, wsd); break;
  }
#undef GOGP_BKNN_CASE
}

void launch_bknn(hipStream_t s, const double *Xs, int64_t n, const double *Cen, int64_t nq, int64_t t, int ndim, int c, int qt,
                 int slabs, void *ws, int *nbr, int *cnt, double *d2out) {
  if (nq <= 0 || c <= 0) return;
  const BknnPlan p = bknn_plan(nq, n, c, qt, slabs);
  const int64_t tiles = (nq + p.qt - 1) / p.qt;
  // the workspace: the distances of every (query, slab, entry), then the indices
  double *wsd = p.slabs > 1 ? static_cast<double *>(ws) : nullptr;
  int *wsi = p.slabs > 1 ? reinterpret_cast<int *>(wsd + (size_t)tiles * p.qt * p.slabs * c) : nullptr;
  if (c <= 64) bknn_launch<64>(s, Xs, n, Cen, nq, t, ndim, c, p, nbr, cnt, d2out, wsi, wsd);
  else bknn_launch<128>(s, Xs, n, Cen, nq, t, ndim, c, p, nbr, cnt, d2out, wsi, wsd);
  if (p.slabs == 1) return;
  if (c <= 64)
    GOGP_KLAUNCH((bknn_merge_kernel<64>), dim3((unsigned)nq), dim3(BKNN_WG), BknnSmem<64>::bytes(1, 0), s, (const int *)wsi,
                 (const double *)wsd, (long)nq, c, p.slabs, nbr, cnt, d2out);
  else
    GOGP_KLAUNCH((bknn_merge_kernel<128>), dim3((unsigned)nq), dim3(BKNN_WG), BknnSmem<128>::bytes(1, 0), s, (const int *)wsi,
                 (const double *)wsd, (long)nq, c, p.slabs, nbr, cnt, d2out);
}

void launch_bknn_pack(hipStream_t s, const int *sel, const int *cnt, int64_t nb, int64_t n, int t, int c, int *tbl, int *nc,
                      int *nt) {
  if (nb <= 0) return;
  const int64_t total = nb * (t + c);
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
  GOGP_KLAUNCH(bknn_pack_kernel, dim3(blocks), dim3(256), 0, s, sel, cnt, (long)nb, (long)n, t, c, tbl, nc, nt);
}

}  // namespace gogp
