// dgemm.hip -- the dominant kernel: fp64 NT GEMM/SYRK tile kernel on
// v_mfma_f64_16x16x4_f64 (gfx950).
//
//   C(128x128 tile) = beta*C + alpha * A(128xK) * B(128xK)^T      (row-major)
//
// One kernel shape serves every O(N^3) step of the hot path:
//   Cholesky trailing update   A22 -= L21 L21^T        GEMM_LOWER, A == B
//   panel TRSM via the inverse L21  = A21 inv(L11)^T   GEMM_RECT
//   triangular inverse (Y=L^-T) R  -= Y_m L_m^T        GEMM_RECT
//   K^-1 = Y Y^T               ragged K range per tile GEMM_LAUUM
//   Produce: V^T solve         same two RECT forms
//
// Reference counterpart: gonum's Dpotrf/Dpotri/Dtrsm/Dgemm behind
// mat.Cholesky.Factorize / SolveTo (call sites gp/gp.go:228,338,454,480).
//
// Structure (CDNA4): a 128x128 tile per workgroup in two wave shapes.  Large launches
// use 512 threads = 8 waves of 64x32 outputs (4x2 MFMA 16x16 accumulators, 64 acc
// VGPRs, <= 128 VGPRs in all): two workgroups per CU put FOUR waves on every SIMD,
// which hides the barrier / prologue / epilogue bubbles of any one of them.  Mid-size
// launches use 256 threads = 4 waves of 64x64 (128 acc VGPRs, two waves per SIMD), and
// the skinny GEMMs of the panel chain a 64x64 tile.  K is walked in steps of 16:
// both operand tiles (128 rows x 16 doubles = one 128-B line per row) go
// global -> LDS directly (global_load_lds_dwordx4), double-buffered, one barrier per step.
// LDS rows are 128 B; the 16-B chunk index is XOR-swizzled with (row>>1)&7 so
// that the MFMA fragment reads (16 rows x 2 k per 32-lane group, ds_read_b64)
// hit 32 distinct 8-B bank pairs: conflict-free.  The fragment reads are inline-assembly
// ds_read_b64 with explicit lgkmcnt waits, software-pipelined one k-group (4 columns) ahead
// of the MFMAs that consume them (round 3: +2.6 % over the same reads waited for at once).
#include "gemm_tile.h"

namespace gogp {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

#ifdef GOGP_WGSTAMP
unsigned long long *g_stamp_buf = nullptr;
long long g_stamp_cap = 0, g_stamp_used = 0, g_stamp_nrec = 0;
StampRec g_stamp_rec[1 << 16];
unsigned long long *stamp_reserve(long long nwg, long long tag, hipStream_t s) {
  if (!g_stamp_buf || g_stamp_used + nwg > g_stamp_cap || g_stamp_nrec >= (1 << 16)) return nullptr;
  unsigned long long *p = g_stamp_buf + STAMP_SLOTS * g_stamp_used;
  g_stamp_rec[g_stamp_nrec++] = {g_stamp_used, nwg, tag, (long long)(size_t)s};
  g_stamp_used += nwg;
  return p;
}
#define GOGP_STAMP_WG(k)                                                                                            \
  do {                                                                                                              \
    if (g.stamps && threadIdx.x == 0)                                                                               \
      g.stamps[((long)blockIdx.x + (long)gridDim.x * blockIdx.z) * STAMP_SLOTS + (k)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define GOGP_STAMP_WG(k) \
  do {                   \
  } while (0)
#endif

__device__ __forceinline__ int lds_off(int row, int chunk) {
  // doubles; chunk = 16-B chunk index 0..7 within the 128-B row
  return row * GEMM_BK + ((chunk ^ ((row >> 1) & 7)) << 1);
}

// Fragment reads as explicit ds_read_b64.  hipcc fuses the `double` loads of two MFMA tiles into
// ds_read2st64_b64, which the LDS serves in four 16-lane groups over a 32-bank modulus: the rows r and
// r ^ 1 of the XOR swizzle (designed for ds_read_b64: two 32-lane groups, 64 banks) then share a bank,
// SQ_LDS_BANK_CONFLICT = half of SQ_LDS_IDX_ACTIVE, 16 LDS cycles per pair against 2 x 2 (round-3 PMC).
// The compiler does not count an inline-asm read in lgkmcnt, so the waits are explicit too
// (lds_wait<N>) and every fragment is pinned behind its wait by an asm operand.
template <int OFF>
__device__ __forceinline__ double lds_read_b64(unsigned addr) {
  double v;
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
  return v;
}
template <int I, int N>
__device__ __forceinline__ void read_frags(double (&f)[N], unsigned addr) {
  if constexpr (I < N) {
    f[I] = lds_read_b64<I * 16 * GEMM_BK * 8>(addr);
    read_frags<I + 1, N>(f, addr);
  }
}
// wait until at most PENDING LDS reads are outstanding, then pin the fragments behind the wait
template <int PENDING, int NA, int NB>
__device__ __forceinline__ void lds_wait(double (&fa)[NA], double (&fb)[NB]) {
  asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(fa[0]) : "i"(PENDING));
#pragma unroll
  for (int i = 1; i < NA; ++i) asm volatile("" : "+v"(fa[i]));
#pragma unroll
  for (int i = 0; i < NB; ++i) asm volatile("" : "+v"(fb[i]));
}
__device__ __forceinline__ unsigned lds_byte_address(const double *p) {
  return (unsigned)(size_t)(__attribute__((address_space(3))) const double *)p;
}

__device__ __forceinline__ void sched_fence() {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_sched_barrier(0);
#endif
}

// BT = workgroup tile (128 or 64).  NW = 4: 2x2 waves, each (BT/2)x(BT/2) outputs =
// MT x MT MFMA tiles, MT = BT/32.  NW = 8 (BT = 128): 2x4 waves, each 64x32 outputs:
// half the accumulators per wave (<= 128 VGPRs), so four waves fit on a SIMD.
// Operand tiles go global -> LDS with global_load_lds_dwordx4 (no VGPR staging, no
// ds_write): a wave's 64 lanes x 16 B land on 1 KB of consecutive LDS = 8 rows of the tile,
// so the XOR swizzle is applied on the GLOBAL side (lane (row, pos) fetches chunk pos ^ swz(row)).
template <int MODE, int BT, int NW>
__global__ __launch_bounds__(NW * 64, NW / 2) void dgemm_nt_kernel(GemmArgs<double> g) {
  constexpr int MT = BT / 32;                          // MFMA tiles per wave, rows
  constexpr int NTW = (NW == 8) ? BT / 64 : BT / 32;   // MFMA tiles per wave, columns
  constexpr int WT = BT / 2;                           // rows per wave
  constexpr int WTN = (NW == 8) ? BT / 4 : BT / 2;     // columns per wave
  constexpr int NQ = BT * 8 / (NW * 64);               // staging loads per thread per operand
  constexpr int SROWS = NW * 8;                        // rows one staging pass covers
  __shared__ __attribute__((aligned(16))) double lds[2][2][BT * GEMM_BK];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: tile bases stay in SGPRs
  if (g.prio) raise_wave_priority();
  GOGP_STAMP_WG(0);
#ifdef GOGP_WGSTAMP
  if (g.stamps && threadIdx.x == 0) {
    unsigned long long *st = g.stamps + ((long)blockIdx.x + (long)gridDim.x * blockIdx.z) * STAMP_SLOTS;
    st[4] = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));   // HW_REG_HW_ID, 32 bits
    st[5] = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11));  // HW_REG_XCC_ID
  }
#endif

  // ---- tile assignment: RECT from gemm_tile.h; the triangular modes here (see there) ----
  int ti, tj, kbeg, nkt;
  double beta;
  if constexpr (MODE == GEMM_RECT) {
    if (!rect_tile_assignment<BT, GEMM_BK>(g, ti, tj, beta, kbeg, nkt)) return;  // whole-workgroup exit (tile-uniform)
  } else {
    int t = blockIdx.x;
    if (MODE != GEMM_LAUUM) t = xcd_chunk(t);
    ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (ti * (ti + 1) / 2 > t) --ti;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    tj = t - ti * (ti + 1) / 2;
    beta = g.beta;
    if (MODE == GEMM_LOWER && ti >= g.new_row0) beta = 0.0;
    kbeg = 0, nkt = g.nkt;
    if (MODE != GEMM_LAUUM && ti > g.krag0) {  // the rows of A below krag0 are zero left of their own diagonal tile
      kbeg = (ti - g.krag0) * BT;
      nkt -= kbeg / GEMM_BK;
    }
    if (MODE == GEMM_LAUUM) {
      kbeg = ti * BT;
      if (kbeg < g.kbeg0) {  // the first launch summed k < kbeg0 into this tile
        kbeg = g.kbeg0;
        beta = 1.0;
      }
      nkt = (g.kend - kbeg) / GEMM_BK;
      if (nkt <= 0) return;  // whole-workgroup exit (tile-uniform)
    }
  }

  const double *Ag = cand(g.A, g.bstride) + (long)ti * BT * g.lda + kbeg;
  const double *Bg = cand(g.B, g.bstride) + (long)tj * BT * g.ldb + kbeg;

  // ---- staging map: thread -> (row, 16-B chunk), NQ rows per operand --------
  const int srow = tid >> 3;  // 0..SROWS-1, +SROWS*q
  const int schunk = tid & 7;
  const int gchunk = schunk ^ ((srow >> 1) & 7);  // SROWS*q never changes swz
  const double *Ap = Ag + (long)srow * g.lda + gchunk * 2;
  const double *Bp = Bg + (long)srow * g.ldb + gchunk * 2;
  const long a_step = (long)SROWS * g.lda, b_step = (long)SROWS * g.ldb;

  // ---- fragment map --------------------------------------------------------
  const int wr = (NW == 8) ? wid >> 2 : wid >> 1;
  const int wc = (NW == 8) ? wid & 3 : wid & 1;
  const int frow = lane & 15;
  const int fk = lane >> 4;      // k within an MFMA step: 0..3
  const int fchunk = fk >> 1;    // + 2*kk
  const int fhalf = fk & 1;
  // LDS offset of fragment (m, kk) = base + m * (16 rows) + xk[kk]: the swizzle term
  // (row >> 1) & 7 only depends on frow (wave and MFMA-tile row offsets are multiples
  // of 16), so the m / n steps are immediate offsets of the ds_read
  const int abase = (wr * WT + frow) * GEMM_BK;
  const int bbase = (wc * WTN + frow) * GEMM_BK;
  // LDS byte addresses of the A / B fragment (m = 0 / n = 0) of k-group kk in buffer 0
  unsigned afrag[4], bfrag[4];
  {
    const unsigned lds0 = lds_byte_address(&lds[0][0][0]);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int xk = (((kk * 2 + fchunk) ^ ((frow >> 1) & 7)) << 1) + fhalf;
      afrag[kk] = lds0 + 8u * (unsigned)(abase + xk);
      bfrag[kk] = lds0 + 8u * (unsigned)(BT * GEMM_BK + bbase + xk);
    }
  }
  constexpr unsigned BUF_BYTES = 2u * BT * GEMM_BK * 8u;  // one double-buffer half: A tile + B tile

  // C fragment of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
  double *Cg = cand(g.C, g.bstride) + (long)(ti * BT + wr * WT) * g.ldc + tj * BT + wc * WTN;
  // address = wave-uniform row base (SGPRs) + ONE 32-bit per-lane offset + immediate: per-lane
  // 64-bit row pointers kept across the k loop spill, and a spill reload in the epilogue
  // waits (vmcnt counts stores too) for every C store issued before it
  const int coff = (lane >> 4) * (int)g.ldc + (lane & 15);
  const double alpha = g.alpha;

  // prologue loads of k-tile 0 go out first, the C tile right behind them: the
  // accumulators start at (beta/alpha) C, so the epilogue is stores only and the
  // C read latency overlaps the operand pipeline fill
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    load16_to_lds(Ap + q * a_step, &lds[0][0][(wid * 8 + SROWS * q) * GEMM_BK]);
    load16_to_lds(Bp + q * b_step, &lds[0][1][(wid * 8 + SROWS * q) * GEMM_BK]);
  }
  f64x4 acc[MT][NTW];
  if (beta != 0.0) {
    const double sc = beta / alpha;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int n = 0; n < NTW; ++n)
#pragma unroll
        for (int v = 0; v < 4; ++v)
          acc[m][n][v] = sc * (Cg + (long)(m * 16 + 4 * v) * g.ldc)[coff + n * 16];
  } else {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int n = 0; n < NTW; ++n) acc[m][n] = (f64x4){0.0, 0.0, 0.0, 0.0};
  }
  wait_vmcnt0();  // the tile is in LDS
  __syncthreads();
  GOGP_STAMP_WG(1);

  int cur = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    const bool more = (kt + 1 < nkt);
    // fragments of k-group kk + 1 are in flight while the MFMAs of kk issue (two register sets); the
    // first two groups are requested right behind the barrier, the next tile's global -> LDS loads go
    // out behind the first group's MFMAs (issued before the fragment reads instead: K = 16384 72.24
    // against 72.86 TFLOP/s, N = 16384 evaluation +0.3 ms)
    const unsigned curoff = (unsigned)cur * BUF_BYTES;
    double a[2][MT], b[2][NTW];
    read_frags<0, MT>(a[0], afrag[0] + curoff);
    read_frags<0, NTW>(b[0], bfrag[0] + curoff);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      if (kk < 3) {
        read_frags<0, MT>(a[(kk + 1) & 1], afrag[kk + 1] + curoff);
        read_frags<0, NTW>(b[(kk + 1) & 1], bfrag[kk + 1] + curoff);
        lds_wait<MT + NTW>(a[kk & 1], b[kk & 1]);
      } else {
        lds_wait<0>(a[kk & 1], b[kk & 1]);
      }
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NTW; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk & 1][m], b[kk & 1][n], acc[m][n], 0, 0, 0);
      sched_fence();  // or the MFMAs of kk sink below the wait of kk + 1
      if (kk == 0 && more) {
        // buffer cur^1 was last read in step kt-1; every wave has passed that step's barrier
        const double *ap = Ap + (long)(kt + 1) * GEMM_BK;
        const double *bp = Bp + (long)(kt + 1) * GEMM_BK;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          load16_to_lds(ap + q * a_step, &lds[cur ^ 1][0][(wid * 8 + SROWS * q) * GEMM_BK]);
          load16_to_lds(bp + q * b_step, &lds[cur ^ 1][1][(wid * 8 + SROWS * q) * GEMM_BK]);
        }
        sched_fence();
      }
    }
    if (more) wait_vmcnt0();
    __syncthreads();
    cur ^= 1;
  }

  GOGP_STAMP_WG(2);
  // ---- epilogue: stores only
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NTW; ++n)
#pragma unroll
      for (int v = 0; v < 4; ++v)
        (Cg + (long)(m * 16 + 4 * v) * g.ldc)[coff + n * 16] = alpha * acc[m][n][v];
#ifdef GOGP_WGSTAMP
  if (g.stamps) {
    wait_vmcnt0();  // probe build: the stores have left
    GOGP_STAMP_WG(3);
  }
#endif
}

template <>
struct TileKernel<double> {
  template <int MODE, int BT, int NW>
  static auto get() {
    return &dgemm_nt_kernel<MODE, BT, NW>;
  }
};

void launch_dgemm_nt(hipStream_t s, GemmMode mode, int mt, int nt, int64_t K, double alpha,
                     const double *A, int64_t lda, const double *B, int64_t ldb,
                     double beta, double *C, int64_t ldc, GemmProfile *prof, const GemmGrid *grid) {
  launch_tile_gemm<double>(s, mode, mt, nt, K, alpha, A, lda, B, ldb, beta, C, ldc, prof, grid);
}

}  // namespace gogp
