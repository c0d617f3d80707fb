// sgemm.hip -- the tile kernel of the fp32 path (BASELINE config 5): NT GEMM / SYRK / LAUUM on
// v_mfma_f32_32x32x2_f32 (gfx950: exact f32 in / f32 accumulate, 64 FLOP/clk/SIMD = 157 TFLOP/s).
//
//   C(128x128 tile) = beta*C + alpha * A(128xK) * B(128xK)^T      (row-major, f32)
//
// Same roles and modes as dgemm.hip (trailing update, panel solve through the block inverse,
// triangular inverse, K^-1 = Y Y^T); reference counterpart: gonum's Dpotrf / Dpotri / Dgemm
// behind mat.Cholesky (call sites gp/gp.go:228,338,454,480), here in single precision with the
// diagonal blocks factored in fp64 (diag256.hip) -- see DESIGN.md "fp32 path".
//
// Structure: 128x128 tile, 256 threads = 2x2 waves of 64x64 outputs = 2x2 MFMA 32x32 tiles
// (64 accumulator VGPRs).  K is walked in steps of 32 floats -- one 128-B line per row, the same
// LDS image as the fp64 kernel: operands go global -> LDS directly (global_load_lds_dwordx4),
// double-buffered, 16-B chunks XOR-swizzled with (row >> 1) & 7 (applied on the global side).
// Fragment reads are ds_read_b128: a lane takes FOUR consecutive k of its row at once and feeds
// them to four consecutive MFMAs; lane half h = lane >> 5 reads chunk 2c + h, so MFMA j of chunk
// pair c multiplies k = 8c + 4h + j on BOTH operands (the k order inside a K-step is
// permuted identically for A and B; a sum over k does not care).  16 distinct rows mod 16 per
// ds_read_b128 lane group x the swizzle = 64 distinct banks: conflict-free.
#include "gemm_tile.h"

namespace gogp {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// BT = workgroup tile (128 or 64).  NW = 4: 2x2 waves, each (BT/2)x(BT/2) outputs = MT x MT MFMA 32x32
// tiles, MT = BT/64.  NW = 8 (BT = 128): 2x4 waves, each 64x32 outputs = 2 x 1 MFMA tiles: half the
// accumulators per wave, four waves per SIMD with two workgroups per CU (the shape of the fp64 kernel's
// large launches, dgemm.hip).
template <int MODE, int BT, int NW>
__global__ __launch_bounds__(NW * 64, NW / 2) void sgemm_nt_kernel(GemmArgs<float> g) {
  constexpr int MT = BT / 64;                          // MFMA tiles per wave, rows
  constexpr int NTW = (NW == 8) ? 1 : BT / 64;         // MFMA tiles per wave, columns
  constexpr int WT = BT / 2;                           // rows per wave
  constexpr int WTN = (NW == 8) ? BT / 4 : BT / 2;     // columns per wave
  constexpr int NQ = BT * 8 / (NW * 64);               // staging loads per thread per operand
  constexpr int SROWS = NW * 8;                        // rows one staging pass covers
  __shared__ __attribute__((aligned(16))) float lds[2][2][BT * SGEMM_BK];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (g.prio) raise_wave_priority();

  // ---- tile assignment: RECT from gemm_tile.h; the triangular modes here (see there) ----
  int ti, tj, kbeg, nkt;
  float beta;
  if constexpr (MODE == GEMM_RECT) {
    if (!rect_tile_assignment<BT, SGEMM_BK>(g, ti, tj, beta, kbeg, nkt)) return;  // whole-workgroup exit (tile-uniform)
  } else {
    int t = blockIdx.x;
    if (MODE != GEMM_LAUUM) t = xcd_chunk(t);
    ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (ti * (ti + 1) / 2 > t) --ti;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    tj = t - ti * (ti + 1) / 2;
    beta = g.beta;
    if (MODE == GEMM_LOWER && ti >= g.new_row0) beta = 0.0f;
    kbeg = 0, nkt = g.nkt;
    if (MODE != GEMM_LAUUM && ti > g.krag0) {  // the rows of A below krag0 are zero left of their own diagonal tile
      kbeg = (ti - g.krag0) * BT;
      nkt -= kbeg / SGEMM_BK;
    }
    if (MODE == GEMM_LAUUM) {
      kbeg = ti * BT;
      nkt = (g.kend - kbeg) / SGEMM_BK;
      if (nkt <= 0) return;  // whole-workgroup exit (tile-uniform)
    }
  }
  const float *Ag = g.A + (long)ti * BT * g.lda + kbeg;
  const float *Bg = g.B + (long)tj * BT * g.ldb + kbeg;

  // staging: thread -> (row, 16-B chunk); chunk swizzled on the global side
  const int srow = tid >> 3;
  const int schunk = tid & 7;
  const int gchunk = schunk ^ ((srow >> 1) & 7);  // SROWS*q (multiples of 32) never change the swizzle: srow < SROWS, and (srow + SROWS * q) >> 1 & 7 == srow >> 1 & 7 for SROWS = 32 or 64
  const float *Ap = Ag + (long)srow * g.lda + gchunk * 4;
  const float *Bp = Bg + (long)srow * g.ldb + gchunk * 4;
  const long a_step = (long)SROWS * g.lda, b_step = (long)SROWS * g.ldb;

  // fragments: lane -> row (lane & 31) of its MFMA tile, k-half (lane >> 5)
  const int wr = (NW == 8) ? wid >> 2 : wid >> 1;
  const int wc = (NW == 8) ? wid & 3 : wid & 1;
  const int frow = lane & 31, fh = lane >> 5;
  const int abase = (wr * WT + frow) * SGEMM_BK;
  const int bbase = (wc * WTN + frow) * SGEMM_BK;
  int xc[4];  // LDS float offset of chunk 2c + fh of this lane's row (swizzle depends on frow only:
              // wave / MFMA-tile row offsets are multiples of 32)
#pragma unroll
  for (int c = 0; c < 4; ++c) xc[c] = ((2 * c + fh) ^ ((frow >> 1) & 7)) << 2;

  // C fragment of v_mfma_f32_32x32x2_f32: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  float *Cg = g.C + (long)(ti * BT + wr * WT) * g.ldc + tj * BT + wc * WTN;
  const int coff = (4 * fh) * (int)g.ldc + frow;
  const float alpha = g.alpha;

#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    load16_to_lds(Ap + q * a_step, &lds[0][0][(wid * 8 + SROWS * q) * SGEMM_BK]);
    load16_to_lds(Bp + q * b_step, &lds[0][1][(wid * 8 + SROWS * q) * SGEMM_BK]);
  }
  f32x16 acc[MT][NTW];
  if (beta != 0.0f) {
    const float sc = beta / alpha;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int n = 0; n < NTW; ++n)
#pragma unroll
        for (int v = 0; v < 16; ++v)
          acc[m][n][v] = sc * (Cg + (long)(m * 32 + (v & 3) + 8 * (v >> 2)) * g.ldc)[coff + n * 32];
  } else {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int n = 0; n < NTW; ++n)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[m][n][v] = 0.0f;
  }
  wait_vmcnt0();
  __syncthreads();

  int cur = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    const bool more = (kt + 1 < nkt);
    if (more) {
      const float *ap = Ap + (long)(kt + 1) * SGEMM_BK;
      const float *bp = Bp + (long)(kt + 1) * SGEMM_BK;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        load16_to_lds(ap + q * a_step, &lds[cur ^ 1][0][(wid * 8 + SROWS * q) * SGEMM_BK]);
        load16_to_lds(bp + q * b_step, &lds[cur ^ 1][1][(wid * 8 + SROWS * q) * SGEMM_BK]);
      }
    }
    const float *la = lds[cur][0];
    const float *lb = lds[cur][1];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 a[MT], b[NTW];
#pragma unroll
      for (int m = 0; m < MT; ++m) a[m] = *reinterpret_cast<const f32x4 *>(la + abase + m * 32 * SGEMM_BK + xc[c]);
#pragma unroll
      for (int n = 0; n < NTW; ++n) b[n] = *reinterpret_cast<const f32x4 *>(lb + bbase + n * 32 * SGEMM_BK + xc[c]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int n = 0; n < NTW; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m][j], b[n][j], acc[m][n], 0, 0, 0);
    }
    if (more) wait_vmcnt0();
    __syncthreads();
    cur ^= 1;
  }

#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NTW; ++n)
#pragma unroll
      for (int v = 0; v < 16; ++v)
        (Cg + (long)(m * 32 + (v & 3) + 8 * (v >> 2)) * g.ldc)[coff + n * 32] = alpha * acc[m][n][v];
}

template <>
struct TileKernel<float> {
  template <int MODE, int BT, int NW>
  static auto get() {
    return &sgemm_nt_kernel<MODE, BT, NW>;
  }
};

void launch_gemm_nt(hipStream_t s, GemmMode mode, int mt, int nt, int64_t K, double alpha, const float *A,
                    int64_t lda, const float *B, int64_t ldb, double beta, float *C, int64_t ldc,
                    GemmProfile *prof, const GemmGrid *grid) {
  launch_tile_gemm<float>(s, mode, mt, nt, K, alpha, A, lda, B, ldb, beta, C, ldc, prof, grid);
}

// the fp64 kernel under the same overloaded name (orchestration code is written once for both)
void launch_gemm_nt(hipStream_t s, GemmMode mode, int mt, int nt, int64_t K, double alpha, const double *A,
                    int64_t lda, const double *B, int64_t ldb, double beta, double *C, int64_t ldc,
                    GemmProfile *prof, const GemmGrid *grid) {
  launch_dgemm_nt(s, mode, mt, nt, K, alpha, A, lda, B, ldb, beta, C, ldc, prof, grid);
}

}  // namespace gogp
