// gemm_tile.h -- what the fp64 (dgemm.hip) and the fp32 (sgemm.hip) tile kernel share: everything that does not depend
// on the MFMA instruction.  The kernel arguments, the XCD remap and the RECT tile assignment at the top of the kernel,
// the device-builtin wrappers and the one launcher, which launches what the plan says (gemm_plan.h).
// Each .hip file keeps its staging / fragment maps, k-loop and epilogue and names its kernel through TileKernel<T>.
#pragma once
#include <type_traits>

#include <hip/hip_ext.h>

#include "common.h"
#include "gemm_plan.h"

namespace gogp {

// The kernel arguments.  Tile counts and tile indices are in tiles of the launched instance (64 or 128 wide).
template <class T>
struct GemmArgsCommon {
  const T *A;
  const T *B;
  T *C;
  long lda, ldb, ldc;
  int mt, nt;
  int nkt;  // K / K-step
  T alpha, beta;
  // GEMM_LAUUM only: the K range of tile (ti,tj) is [ti*BT, kend)
  int kend;
  int trap;  // GEMM_TRAP: skip tiles of strictly upper 256-blocks
  // Tile filter of a sharded (2-D block-cyclic) evaluation, GEMM_RECT only; rule 0: none.
  // The launch covers LOCAL tiles; local tile (ti, tj) lies in the distribution block
  //   global row block  gI = (rblk0 + (ti >> tpb_shift)) * Pr + pr,
  //   global col block  gJ = (cblk0 + (tj >> tpb_shift)) * Pc + pc      (common.h: GemmGrid)
  // rule 1/2: keep the tile iff it belongs to the lower triangle of the GLOBAL matrix (gI > gJ,
  // or gI == gJ and the tile is on/below the diagonal of that block); rule 2 additionally
  // overwrites (beta = 0) the tiles of row block gI == beta0 and accumulates into the others.
  int rule, tpb_shift, rblk0, cblk0, pr, Pr, pc, Pc, beta0;
  int new_row0;  // GEMM_LOWER: tile rows >= new_row0 overwrite C (common.h: GemmGrid); INT_MAX: none
  int ktri;      // GEMM_RECT: B lower triangular, tile column tj sums k < (tj + 1) * BT only
  int prio;      // chain launch: s_setprio 3 (common.h: GemmGrid)
  int krag0;     // RECT / LOWER: tile rows ti >= krag0 start at k = (ti - krag0) * BT (common.h: GemmGrid); INT_MAX: none
};
template <class T>
struct GemmArgs : GemmArgsCommon<T> {};
// What only the fp64 kernel has: its fp32 twin carries none of these (and no code that reads them).
template <>
struct GemmArgs<double> : GemmArgsCommon<double> {
  int kbeg0;     // GEMM_LAUUM: second of two launches (common.h: GemmGrid)
  long bstride;  // candidate batching: byte offset of A, B, C per blockIdx.z (common.h: Batch)
#ifdef GOGP_WGSTAMP
  unsigned long long *stamps;  // probe build: this launch's slice of the stamp buffer (common.h), or nullptr
#endif
};

// device-only builtins behind helpers: in the host pass of hipcc the unknown builtin
// silently suppresses the kernel's host stub (undefined __device_stub__ at load time)
template <class T>
__device__ __forceinline__ void load16_to_lds(const T *gsrc, T *lds_wave_base) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_global_load_lds(gsrc, lds_wave_base, 16, 0, 0);
#endif
}
__device__ __forceinline__ void raise_wave_priority() {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_s_setprio(3);
#endif
}
__device__ __forceinline__ void wait_vmcnt0() {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), lgkmcnt / expcnt untouched
#endif
}

// XCD-aware remap (blocks b and b+8 share an XCD/L2): give each XCD a
// contiguous chunk of the tile list; bijective for any grid size.
__device__ __forceinline__ int xcd_chunk(int t) {
  const int nwg = gridDim.x;
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = t & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (t >> 3);
}

// GEMM_RECT: the tile of workgroup blockIdx.x, (ti, tj) in tiles of BT, the beta of that tile and its K range, nkt
// steps of BK elements from kbeg.  false: the workgroup has no tile (whole-workgroup exit).  Every result is
// workgroup-uniform.  The triangular modes keep their assignment in the kernels: handed out of a shared function (through
// the references or from locals) it moved the register counts of the LOWER instances of both kernels and of the fp32
// LAUUM one (fp64 LOWER 48 -> 54 / 58 / 54 SGPRs), and the issue that folded the two files holds those figures fixed.
template <int BT, int BK, class T>
__device__ __forceinline__ bool rect_tile_assignment(const GemmArgs<T> &g, int &ti_out, int &tj_out, T &beta_out,
                                                     int &kbeg_out, int &nkt_out) {
  int t = blockIdx.x;
  if (!g.rule) t = xcd_chunk(t);
  int ti, tj;
  if (g.rule) {
    // Filtered launch of the sharded path: the kept tiles form a staircase (global lower
    // triangle), so contiguous chunks per XCD would be badly unbalanced.  Deal the tile ROWS
    // cyclically instead: the XCD group b & 7 takes rows x, x + 8, ... (a row's tiles share the
    // A panel in that XCD's L2).  The grid is 8 * ceil(mt / 8) * nt workgroups.
    const int x = t & 7, slot = t >> 3;
    const int rr = slot / g.nt;
    ti = x + 8 * rr;
    tj = slot - rr * g.nt;
    if (ti >= g.mt) return false;
  } else {
    ti = t / g.nt;
    tj = t - ti * g.nt;
    if (g.trap && (tj * BT) / PANEL > (ti * BT) / PANEL) return false;
  }
  T beta = g.beta;
  if (g.rule) {  // tiles of the global upper triangle
    const int gI = (g.rblk0 + (ti >> g.tpb_shift)) * g.Pr + g.pr;
    const int gJ = (g.cblk0 + (tj >> g.tpb_shift)) * g.Pc + g.pc;
    const int msk = (1 << g.tpb_shift) - 1;
    if (gI < gJ || (gI == gJ && (ti & msk) < (tj & msk))) return false;
    if (g.rule == 2) beta = (gI == g.beta0) ? T(0) : T(1);
  }
  int kbeg = 0, nkt = g.nkt;
  if (g.ktri) nkt = min(nkt, (tj + 1) * BT / BK);
  if (ti > g.krag0) {  // the rows of A below krag0 are zero left of their own diagonal tile
    kbeg = (ti - g.krag0) * BT;
    nkt -= kbeg / BK;
  }
  ti_out = ti, tj_out = tj, beta_out = beta, kbeg_out = kbeg, nkt_out = nkt;
  return true;
}

// ---- the launcher ----------------------------------------------------------------------------------------------------
// Each .hip file names its kernel: TileKernel<T>::get<MODE, BT, NW>() is the instance's address.
template <class T>
struct TileKernel;

template <class T>
void launch_tile_gemm(hipStream_t s, GemmMode mode, int mt, int nt, int64_t K, double alpha, const T *A, int64_t lda,
                      const T *B, int64_t ldb, double beta, T *C, int64_t ldc, GemmProfile *prof, const GemmGrid *grid) {
  if (mt <= 0 || nt <= 0 || K <= 0) return;
  constexpr bool F64 = std::is_same_v<T, double>;
  const GemmPlan p = gemm_plan(mode, mt, nt, K, grid, tl_batch.k, F64 ? GEMM_F64 : GEMM_F32);
  GemmArgs<T> g;
  g.A = A;
  g.B = B;
  g.C = C;
  g.lda = lda;
  g.ldb = ldb;
  g.ldc = ldc;
  g.alpha = (T)alpha;
  g.beta = (T)beta;
  g.mt = p.mt, g.nt = p.nt, g.nkt = p.nkt, g.kend = p.kend, g.trap = p.trap;
  g.rule = p.rule, g.tpb_shift = p.tpb_shift, g.rblk0 = p.rblk0, g.cblk0 = p.cblk0, g.beta0 = p.beta0;
  g.pr = p.pr, g.Pr = p.Pr, g.pc = p.pc, g.Pc = p.Pc;
  g.new_row0 = p.new_row0, g.ktri = p.ktri, g.prio = p.prio, g.krag0 = p.krag0;
  if constexpr (F64) {
    g.kbeg0 = p.kbeg0;
    g.bstride = tl_batch.stride;
#ifdef GOGP_WGSTAMP
    const int shape = p.tile == 64 ? 1 : (p.waves == 8 ? 3 : 2);
    g.stamps = stamp_reserve((long long)p.gridx * p.gridz, 10000000000LL * shape + p.tag, s);
#endif
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (prof && prof->on) {
    if (prof->used + 2 > prof->pool.size()) {
      size_t old = prof->pool.size();
      prof->pool.resize(old + 1024);
      for (size_t i = old; i < prof->pool.size(); ++i) (void)hipEventCreate(&prof->pool[i]);
    }
    e0 = prof->pool[prof->used++];
    e1 = prof->pool[prof->used++];
    prof->flops += p.flops;
    prof->launches += 1;
    prof->lflops.push_back(p.flops);
    prof->ltag.push_back(p.tag);
  }
  using K_ = TileKernel<T>;
  void (*kernel)(GemmArgs<T>);
  if (p.tile == 64)
    kernel = p.mode == GEMM_RECT ? K_::template get<GEMM_RECT, 64, 4>() : K_::template get<GEMM_LOWER, 64, 4>();
  else if (p.waves == 4)
    kernel = p.mode == GEMM_RECT ? K_::template get<GEMM_RECT, 128, 4>() : K_::template get<GEMM_LOWER, 128, 4>();
  else
    kernel = p.mode == GEMM_RECT    ? K_::template get<GEMM_RECT, 128, 8>()
             : p.mode == GEMM_LOWER ? K_::template get<GEMM_LOWER, 128, 8>()
                                    : K_::template get<GEMM_LAUUM, 128, 8>();
  const dim3 gridd(p.gridx, 1, p.gridz), block(p.waves * 64);
  // With profiling on, the two events ride on the kernel's own dispatch packet
  // (hipExtLaunchKernelGGL: start / stop timestamps of exactly this dispatch) instead of two
  // extra barrier packets in the queue -- the instrumented run keeps the un-instrumented timing.
  if (e0)
    hipExtLaunchKernelGGL(kernel, gridd, block, 0, s, e0, e1, 0, g);
  else
    GOGP_KLAUNCH(kernel, gridd, block, 0, s, g);
}

}  // namespace gogp
