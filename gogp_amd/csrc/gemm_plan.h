// gemm_plan.h -- the launch plan of the tile kernels (dgemm.hip, sgemm.hip): a pure host function with no HIP call.
// From the launcher's arguments alone it says which instance runs, on which grid, with which tile-counted arguments,
// and how many flops it does.  gemm_tile.h launches from it; the test hook gogp_test_gemm_plan returns it.
#pragma once
#include <algorithm>

#include "common.h"

namespace gogp {

// What differs between the precisions in the plan, by name.
struct GemmPrecision {
  int kstep;         // elements per K-step: one 128-B line per row
  // Launches of 513 .. 768 tiles use 64 x 64 tiles: 128 x 128 tiles have 512 places on the chip (two per CU), so such a
  // launch runs a second, almost empty round at the full per-round price (528 tiles at K = 512, the last fused K^-1
  // update of an N = 4096 evaluation: 203 us); as 64 x 64 tiles it is two rounds of a quarter of the work each
  // (one N = 4096 evaluation 3.54-3.59 -> 3.48-3.50 ms; N = 16384 and 8 candidates at N = 4096 unchanged).  The same
  // window in the fp32 kernel measured slower at N = 65536 and is not applied there.
  bool band_513_768;
  // The kernel has the candidate batch on gridDim.z: a batched launch counts the tiles of all its candidates (together
  // they fill the chip).  Without it the plan takes one candidate.
  bool cand_batch;
  // The kernel has the two-launch LAUUM (GemmGrid::kbeg0).  Without it the plan ignores kbeg0.
  bool lauum_kbeg0;
};
constexpr int SGEMM_BK = 32;  // floats per K-step of the fp32 kernel
constexpr GemmPrecision GEMM_F64 = {GEMM_BK, true, true, true}, GEMM_F32 = {SGEMM_BK, false, false, false};

struct GemmPlan {
  // the mode-independent fields of GemmArgs under their names there, counted in tiles of the chosen instance
  int mt, nt, nkt, kend, trap, rule, tpb_shift, rblk0, cblk0, pr, Pr, pc, Pc, beta0, new_row0, ktri, prio, krag0;
  int kbeg0;       // fp64 only
  GemmMode mode;   // the kernel's MODE: GEMM_TRAP runs as GEMM_RECT with trap
  int ntiles;      // 128-tiles of one candidate, skipped ones included
  double flops;    // of the whole launch
  int64_t tag;     // GemmProfile::ltag
  int tile, waves;  // the instance: 64 x 4, 128 x 4 or 128 x 8
  unsigned gridx, gridz;
};

// No HIP call: what launch_tile_gemm launches for `ncand` candidates, from the launcher's arguments alone.
inline GemmPlan gemm_plan(GemmMode mode, int mt, int nt, int64_t K, const GemmGrid *grid, int ncand, GemmPrecision prec) {
  constexpr int NONE = 0x7fffffff;
  GemmPlan p{};
  if (!prec.cand_batch) ncand = 1;
  p.mt = mt;
  p.nt = nt;
  p.nkt = (int)(K / prec.kstep);
  p.kend = (int)K;
  p.trap = mode == GEMM_TRAP;
  p.rule = p.tpb_shift = p.rblk0 = p.cblk0 = p.pr = p.pc = p.beta0 = 0;
  p.Pr = p.Pc = 1;
  p.new_row0 = (mode == GEMM_LOWER && grid && grid->new_row0 >= 0) ? grid->new_row0 : NONE;
  p.ktri = (mode == GEMM_RECT && grid && grid->ktri) ? 1 : 0;
  p.prio = grid ? grid->prio : 0;
  p.krag0 = (mode != GEMM_LAUUM && mode != GEMM_TRAP && grid && grid->krag0 >= 0 && !p.ktri) ? grid->krag0 : NONE;
  p.kbeg0 = (mode == GEMM_LAUUM && grid && prec.lauum_kbeg0) ? grid->kbeg0 : 0;
  if (grid && grid->rule) {
    p.rule = grid->rule;
    p.tpb_shift = grid->tpb_shift;
    p.rblk0 = grid->rblk0;
    p.cblk0 = grid->cblk0;
    p.pr = grid->pr;
    p.Pr = grid->Pr;
    p.pc = grid->pc;
    p.Pc = grid->Pc;
    p.beta0 = grid->beta0;
  }
  int ntiles;
  double flops;
  if (mode == GEMM_TRAP) {  // rectangular enumeration, upper 256-blocks skipped in the kernel
    mode = GEMM_RECT;
    ntiles = mt * nt;
    const int nb = nt / 2;  // 256-blocks across; block column b skips b block rows of 2 x 2 tiles
    flops = 2.0 * TILE * TILE * (double)K * ((double)mt * nt - 4.0 * nb * (nb - 1) / 2.0);
  } else if (mode == GEMM_RECT) {
    ntiles = mt * nt;
    flops = 2.0 * (double)mt * TILE * (double)nt * TILE * (double)K;
    if (p.ktri) {
      flops = 0;
      for (int j = 0; j < nt; ++j)
        flops += 2.0 * (double)mt * TILE * TILE * (double)std::min<int64_t>(K, (int64_t)(j + 1) * TILE);
    }
    if (p.krag0 != NONE) {
      flops = 0;
      for (int i = 0; i < mt; ++i)
        flops += 2.0 * (double)nt * TILE * TILE * (double)(K - (int64_t)std::max(0, i - p.krag0) * TILE);
    }
    if (p.rule) {  // count the tiles the filter keeps
      const int tpb = 1 << p.tpb_shift;
      long kept = 0;
      for (int bi = 0; bi < mt / tpb; ++bi)
        for (int bj = 0; bj < nt / tpb; ++bj) {
          const int gI = (p.rblk0 + bi) * p.Pr + p.pr, gJ = (p.cblk0 + bj) * p.Pc + p.pc;
          kept += gI > gJ ? (long)tpb * tpb : (gI == gJ ? (long)tpb * (tpb + 1) / 2 : 0);
        }
      flops = 2.0 * (double)kept * TILE * TILE * (double)K;
    }
  } else {
    ntiles = mt * (mt + 1) / 2;
    if (mode == GEMM_LOWER && p.krag0 != NONE) {
      flops = 0;
      for (int i = 0; i < mt; ++i)
        flops += 2.0 * (double)(i + 1) * TILE * TILE * (double)(K - (int64_t)std::max(0, i - p.krag0) * TILE);
    } else if (mode == GEMM_LOWER) {
      flops = 2.0 * (double)ntiles * TILE * TILE * (double)K;
    } else {
      flops = 0;
      for (int i = 0; i < mt; ++i)
        flops += 2.0 * (double)(i + 1) * TILE * TILE * (double)(K - std::max<int64_t>((int64_t)i * TILE, p.kbeg0));
    }
  }
  p.mode = mode;
  p.ntiles = ntiles;
  p.flops = flops * ncand;
  p.tag = (int64_t)mode * 100000000LL + (int64_t)(K / 16) * 100000LL + (int64_t)std::min(ntiles, 99999);
  // Small launches (the skinny GEMMs of the panel chain) use 64x64 tiles: 4x the
  // workgroups and a quarter of the per-tile latency.  LAUUM keeps 128 (its K
  // ranges are cut at 128-row granularity).  Launches of >= 3072 tiles and LAUUM use the
  // 8-wave shape of the 128x128 tile (measured 4-9 % faster in fp64; the shape matters less in
  // fp32: N = 32768 314.1 -> 312.5 ms), the rest the 4-wave one.
  const long total_tiles = (long)ntiles * ncand;
  const bool small = (mode != GEMM_LAUUM) && (total_tiles < (grid ? grid->small_below : 384) ||
                                              (prec.band_513_768 && total_tiles > 512 && total_tiles <= 768));
  // chain_prio = 1: only the skinny launches (64x64 tiles) raise their priority; 2: every chain launch
  if (p.prio == 1 && !small) p.prio = 0;
  p.tile = small ? 64 : TILE;
  p.waves = (mode == GEMM_LAUUM || (!small && total_tiles >= 3072)) ? 8 : 4;
  p.gridx = p.rule ? 8 * ((mt + 7) / 8) * nt : ntiles;
  p.gridz = (unsigned)ncand;
  if (small) {
    p.mt = mt * 2;
    p.nt = nt * 2;
    p.tpb_shift += 1;  // distribution blocks counted in 64-wide tiles
    if (p.new_row0 != NONE) p.new_row0 *= 2;
    if (p.krag0 != NONE) p.krag0 *= 2;  // counted in 64-wide tiles (and 64-column steps of the K start)
    p.gridx = (mode == GEMM_RECT) ? (p.rule ? 8 * ((p.mt + 7) / 8) * p.nt : p.mt * p.nt) : p.mt * (p.mt + 1) / 2;
  }
  return p;
}

}  // namespace gogp
