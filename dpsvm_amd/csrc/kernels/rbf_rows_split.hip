// The working-set row GEMM on split operands (rbf_rows_indexed_split): the
// kernel rows of a ws-cache round's misses, lines[out_rows[i]][j] =
// K(X[a_rows[i]], B_j), on the split rows, k blocks and epilogue of the Gram
// kernels (rbf_gemm_split.hip, split_mma.hpp), so a cached row holds the bits
// of the Gram's row.  Three kernels: up to 2 k blocks the persistent small-K
// kernel; else the LDS-DMA rows kernel, persistent over the column tiles where
// the misses are one tile row (the usual round), a tile per workgroup
// otherwise (and for the stamps diagnostics).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

#include "dpsvm/common.hpp"
#include "device_util.hpp"
#include "kernels.hpp"
#include "split_mma.hpp"
#include "../runtime/hip_check.hpp"

namespace dpsvm {
namespace dev {

// ---------------------------------------------------------------------------
// LDS-DMA ROWS GEMM: a working-set round's cache misses (up to 192 indexed A
// rows, a_rows[0 .. *m_dev)) against all of this rank's B rows, K written to
// the misses' cache lines.  The register-staged form of it (the Gram's tile
// kernel with indexed rows, since removed) waited for each 32-k stage's loads
// before the next could start, so on synthetic-2m (K = 1024, 2M B rows: the
// 8 GB split X panel per round) it ran at 2.3 TB/s of B bytes and 3.5 ms per
// round (profiles/r4_big_inputs).  Here the operands of
// a 192 x 128 tile go through three 32-k LDS buffers by global_load_lds_dwordx4
// (40 KiB each; the row data after them in the same array), the next block's
// DMA in flight while a block is multiplied; the waves (6 x 2, 32 x 64 each)
// run the tile kernel's MFMA sequence and epilogue per element, so the rows are
// bit-identical to the Gram kernels'.  Ten waves issue the DMA: 40
// wave instructions of 8 rows x 128 B per block, 4 per wave.
// ---------------------------------------------------------------------------
constexpr int kRowsGldsThreads = 768;
// kRowsBAux: cache policy of the B operand's DMA (2 = nt: streamed once per
// round, kept from evicting the A rows every tile re-reads from L2)
// NBR: B ring depth.  A and B have separate rings: A three deep (block kb + 2
// issued at block kb), B NBR deep (block kb + NBR - 1 issued at kb); the waves
// that stage A (0-5) and B (6-9) wait on their own DMA counts.  Measured at the
// synthetic-2m round shape (bench/rows_probe.py, profiles/r6_rows_kernel.txt):
// a B ring 5 deep does not beat 3, B read from L2 instead of HBM saves only
// ~10%, and the operand reads one MFMA group ahead (the Gram's read-ahead)
// change nothing — the k loop runs at ~46% MFMA with the chip at ~1.57 GHz.
// ST: diagnostics build with per-workgroup stamps (entry, first block landed,
// k loop done, stores issued, stores done; s_memrealtime at entry / end) at
// stamps[8 (blockIdx.y gridDim.x + blockIdx.x) ..] (bench/rows_probe.py --stamps)
constexpr int kRowsBAux = 2;
template <bool ST>
__global__ __launch_bounds__(kRowsGldsThreads, 1) void rbf_rows_split_glds_kernel(
    const u4* __restrict__ A, const int32_t* __restrict__ Ash, const float* __restrict__ Asq,
    const int32_t* __restrict__ a_rows, const int32_t* __restrict__ m_dev, const u4* __restrict__ B,
    const int32_t* __restrict__ Bsh, const float* __restrict__ Bsq, int64_t N, int nkb, float gamma,
    float* __restrict__ out, int64_t ldo, const int32_t* __restrict__ out_rows, uint64_t* __restrict__ stamps) {
  uint64_t st[5] = {0, 0, 0, 0, 0}, rt0 = 0;
  if constexpr (ST) {
    st[0] = __builtin_amdgcn_s_memtime();
    rt0 = __builtin_amdgcn_s_memrealtime();
  }
  constexpr int WN = 2, TM = 192, TN = 128, CPR = 8, NA = 3, NBR = 3;
  constexpr int BUFA = TM * CPR, BUFB = TN * CPR;
  constexpr int DMA_WAVES = (TM + TN) / 32;  // 10: each fills 32 rows (4 instructions of 8 rows)
  static_assert(NA * BUFA * 16 + NBR * BUFB * 16 + (3 * TM + 2 * TN) * 4 <= 160 * 1024, "LDS");
  int64_t tx, ty;
  xcd_tile(tx, ty);
  const int M = *m_dev;
  if (tx * TM >= M) return;  // uniform: no barrier reached
  __shared__ u4 lds[NA * BUFA + NBR * BUFB + (3 * TM + 2 * TN) / 4];
  u4* const ldsA = lds;
  u4* const ldsB = lds + NA * BUFA;
  float* s_asq = (float*)(lds + NA * BUFA + NBR * BUFB);
  int32_t* s_ash = (int32_t*)(s_asq + TM);
  int32_t* s_orow = s_ash + TM;
  float* s_bsq = (float*)(s_orow + TM);
  int32_t* s_bsh = (int32_t*)(s_bsq + TN);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN, hl = lane >> 5;
  const int64_t m0 = tx * TM, n0 = ty * TN;
  const int64_t rstride = (int64_t)nkb * 8;  // u4 per split row
  if (tid < TM) {
    const int64_t row = m0 + tid;
    const int64_t ar = a_rows[min(row, (int64_t)M - 1)];
    s_asq[tid] = Asq[ar];
    s_ash[tid] = Ash[ar];
    s_orow[tid] = row < M ? out_rows[row] : -1;
  } else if (tid < TM + TN) {
    const int64_t cc = min(n0 + (tid - TM), N - 1);
    s_bsq[tid - TM] = Bsq[cc];
    s_bsh[tid - TM] = Bsh[cc];
  }
  // DMA sources: wave w < 10 fills stage rows 32 w + 8 i + (lane >> 3) (rows
  // >= TM: B row r - TM of its own ring); lane position p = lane & 7 takes
  // global chunk p ^ ((row >> 1) & 7) (the read swizzle; TM is a multiple of
  // 16, so B rows keep it re-based at 0); A rows past M re-read a valid row
  // (never stored)
  const u4* src[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = min(32 * wave + 8 * i + (lane >> 3), TM + TN - 1);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    const int64_t grow = r < TM ? (int64_t)a_rows[min(m0 + r, (int64_t)M - 1)] : n0 + (r - TM);
    src[i] = (r < TM ? A : B) + grow * rstride + c;
  }
  const bool dma_wave = wave < DMA_WAVES;
  const bool b_wave = 32 * wave >= TM;  // waves 6 .. 9 stage B rows only (TM = 192 = 6 x 32)
  auto dma = [&](int kb) {
    if (b_wave) {
      u4* dst = ldsB + (kb % NBR) * BUFB + (32 * wave - TM) * CPR;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        lds_dma16<kRowsBAux>(src[i] + (int64_t)kb * 8, dst + 8 * i * CPR);
    } else {
      u4* dst = ldsA + (kb % NA) * BUFA + 32 * wave * CPR;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        lds_dma16(src[i] + (int64_t)kb * 8, dst + 8 * i * CPR);
    }
  };
  const int ahead = b_wave ? NBR - 1 : NA - 1;  // blocks a staging wave keeps issued past the current one
  __syncthreads();  // row data written (no DMA in flight yet)
  if (dma_wave) {
    for (int b = 0; b < ahead && b < nkb; ++b) dma(b);
  }

  f16v H[2], P[2], Q[2];
  zero_acc(H, P, Q);
  const int sw = ((lane & 31) >> 1) & 7;
  const int ra = (wm * 32 + (lane & 31)) * CPR;
  const int rb0 = (wn * 64 + (lane & 31)) * CPR, rb1 = rb0 + 32 * CPR;
  const bool live = m0 + wm * 32 < M;  // a wave whose rows all lie past M only stages
  for (int kb = 0; kb < nkb; ++kb) {
    // retire block kb's DMA: a staging wave's younger blocks kb + 1 .. (4
    // pieces each) may stay in flight (uniform per wave)
    const int younger = min(ahead - 1, nkb - 1 - kb);
    if (younger >= 4) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else if (younger == 3) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if (younger == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (younger == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ring_barrier();
    if constexpr (ST) {
      if (kb == 0) st[1] = __builtin_amdgcn_s_memtime();
    }
    // block kb + ahead into its ring's buffer of block kb - 1 (every wave is past it)
    if (dma_wave && kb + ahead < nkb) dma(kb + ahead);
    if (live) {
      w32_kblock(H, P, Q, ldsA + (kb % NA) * BUFA, ldsB + (kb % NBR) * BUFB, ra, rb0, rb1, hl, sw);
    }
  }
  if (!live) return;
  if constexpr (ST) st[2] = __builtin_amdgcn_s_memtime();

  // ---- epilogue: K = exp(-g max(|a|^2 + |b|^2 - 2 dot, 0)) ----
  // (w32_values written out, here and in the persistent kernel below: through
  // the helper the same values come out of a differently scheduled kernel, the
  // k loop's waits included, and these two are the round's hot kernels)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int cb = wn * 64 + 32 * j + (lane & 31);
    const float bsq = s_bsq[cb];
    const int bsh = s_bsh[cb];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int lr = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * hl;
      const float dot = ldexpf(H[j][r] + (P[j][r] + Q[j][r]), -(s_ash[lr] + bsh));
      H[j][r] = rbf_split_value(s_asq[lr], bsq, dot, gamma);
    }
  }
  const bool interior = n0 + TN <= N;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int32_t orow = s_orow[wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * hl];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t col = n0 + wn * 64 + 32 * j + (lane & 31);
      if (orow >= 0 && (interior || col < N)) out[(int64_t)orow * ldo + col] = H[j][r];
    }
  }
  if constexpr (ST) {
    st[3] = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    st[4] = __builtin_amdgcn_s_memtime();
    const uint64_t rt1 = __builtin_amdgcn_s_memrealtime();
    if (tid == 0) write_stamps(stamps + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 8, st, rt0, rt1, 0, 0);
  }
}

// ---------------------------------------------------------------------------
// Persistent LDS-DMA ROWS GEMM (the default for one tile row, M <= 192, and
// nkb >= 3: a one-block ws-cache round's misses against all of this rank's B
// rows — synthetic-2m's round).  The tile-per-workgroup kernel above spends
// ~8% of a tile in its prologue (the miss rows' data and DMA sources, the
// first blocks' latency) and the device runs ~239 of 256 workgroups at a time
// (stamps, profiles/r6_rows_kernel.txt).  Here one workgroup per CU walks
// column tiles ty = b, b + G, ...: the A side (the misses' |x|^2, shifts,
// output lines and DMA sources) is set up once, and the DMA rings run on
// across tiles — during a tile's last two k blocks the prefetch slots load
// blocks 0 and 1 of the next (A's are the same blocks, B's the next tile's
// rows), the next tile's B row data is loaded into registers during the k
// loop and stored into the other parity of a row-data area after it.  Every
// DMA wave issues 4 pieces every k block (the last tile re-loads its own
// blocks 0 / 1 into dead buffers), so one uniform vmcnt(4) retires a block;
// each epilogue ends with vmcnt(0).  Same MFMA sequence and epilogue per tile:
// bit-identical to the kernel above.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kRowsGldsThreads, 1) void rbf_rows_split_glds_persist_kernel(
    const u4* __restrict__ A, const int32_t* __restrict__ Ash, const float* __restrict__ Asq,
    const int32_t* __restrict__ a_rows, const int32_t* __restrict__ m_dev, const u4* __restrict__ B,
    const int32_t* __restrict__ Bsh, const float* __restrict__ Bsq, int64_t N, int nkb, float gamma,
    float* __restrict__ out, int64_t ldo, const int32_t* __restrict__ out_rows, int ntiles) {
  constexpr int WN = 2, TM = 192, TN = 128, CPR = 8, NBUF = 3;
  constexpr int BUFA = TM * CPR, BUFB = TN * CPR;
  constexpr int DMA_WAVES = (TM + TN) / 32;  // 10: waves 0-5 stage A rows, 6-9 B rows (4 pieces of 8 rows each)
  __shared__ u4 lds[NBUF * BUFA + NBUF * BUFB + (3 * TM + 4 * TN) / 4];
  u4* const ldsA = lds;
  u4* const ldsB = lds + NBUF * BUFA;
  float* const s_asq = (float*)(lds + NBUF * (BUFA + BUFB));
  int32_t* const s_ash = (int32_t*)(s_asq + TM);
  int32_t* const s_orow = s_ash + TM;
  float* const s_bsq = (float*)(s_orow + TM);    // [2][TN] by parity
  int32_t* const s_bsh = (int32_t*)(s_bsq + 2 * TN);  // [2][TN]
  const int M = *m_dev;
  const int G = gridDim.x;
  int ty = blockIdx.x;
  if (ty >= ntiles || M <= 0) return;  // uniform
  // (the wave index in an SGPR: the epilogue's row addresses stay scalar
  // instead of 16 VGPRs hoisted across the tile loop)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN, hl = lane >> 5;
  const int64_t rstride = (int64_t)nkb * 8;  // u4 per split row
  if (tid < TM) {
    const int64_t ar = a_rows[min(tid, M - 1)];
    s_asq[tid] = Asq[ar];
    s_ash[tid] = Ash[ar];
    s_orow[tid] = tid < M ? out_rows[tid] : -1;
  } else if (tid < TM + TN) {
    const int64_t cc = min((int64_t)ty * TN + (tid - TM), N - 1);
    s_bsq[tid - TM] = Bsq[cc];
    s_bsh[tid - TM] = Bsh[cc];
  }
  // DMA sources: the kernel above's geometry; A's fixed for the launch, B's as
  // a per-lane offset from the tile's first row (a uniform base per tile)
  const bool dma_wave = wave < DMA_WAVES;
  const bool b_wave = 32 * wave >= TM;
  // (32-bit u4 offsets: launcher, (N + 512) x nkb x 8 < 2^32; registers are
  // what the 96 accumulators leave at three waves per SIMD)
  uint32_t off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = min(32 * wave + 8 * i + (lane >> 3), TM + TN - 1);
    const uint32_t c = (uint32_t)((lane & 7) ^ ((r >> 1) & 7));
    off[i] = r < TM ? (uint32_t)a_rows[min(r, M - 1)] * (uint32_t)rstride + c : (uint32_t)(r - TM) * (uint32_t)rstride + c;
  }
  // piece set of global block g (kb of tile tt): into ring buffer g % 3
  auto dma = [&](uint32_t g, int kb, int tt) {
    const u4* base = b_wave ? B + (int64_t)tt * TN * rstride + (int64_t)kb * 8 : A + (int64_t)kb * 8;  // uniform
    u4* dst = b_wave ? ldsB + (g % NBUF) * BUFB + (32 * wave - TM) * CPR : ldsA + (g % NBUF) * BUFA + 32 * wave * CPR;
    if (b_wave) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        lds_dma16<kRowsBAux>(base + off[i], dst + 8 * i * CPR);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        lds_dma16(base + off[i], dst + 8 * i * CPR);
    }
  };
  __syncthreads();  // row data written (no DMA in flight yet)
  uint32_t g = 0;   // k blocks started over all of this workgroup's tiles
  if (dma_wave) {
    dma(0, 0, ty);
    dma(1, 1, ty);  // (launcher: nkb >= 3)
  }
  const int sw = ((lane & 31) >> 1) & 7;
  const int ra = (wm * 32 + (lane & 31)) * CPR;
  const int rb0 = (wn * 64 + (lane & 31)) * CPR, rb1 = rb0 + 32 * CPR;
  const bool live = wm * 32 < M;  // a wave whose rows all lie past M only stages
  int par = 0;
  while (true) {
    const int tn_next = ty + G;
    const bool has_next = tn_next < ntiles;  // uniform
    const int tp = has_next ? tn_next : ty;  // the last tile prefetches itself into dead buffers
    // the next tile's B row data, in flight across the k loop
    float nbsq = 0.f;
    int32_t nbsh = 0;
    if (has_next && tid >= TM && tid < TM + TN) {
      const int64_t cc = min((int64_t)tn_next * TN + (tid - TM), N - 1);
      nbsq = Bsq[cc];
      nbsh = Bsh[cc];
    }
    f16v H[2], P[2], Q[2];
    zero_acc(H, P, Q);
    for (int kb = 0; kb < nkb; ++kb) {
      // block kb landed: only block kb + 1's 4 pieces may stay in flight
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      ring_barrier();
      // block kb + 2 of this tile, or block kb + 2 - nkb of the next, into the
      // buffer of block g - 1 (every wave is past it)
      if (dma_wave) {
        const bool own = kb + 2 < nkb;
        dma(g + 2, own ? kb + 2 : kb + 2 - nkb, own ? ty : tp);
      }
      if (live) {
        w32_kblock(H, P, Q, ldsA + (g % NBUF) * BUFA, ldsB + (g % NBUF) * BUFB, ra, rb0, rb1, hl, sw);
      }
      ++g;
    }
    // the next tile's B row data into the other parity (last read by the
    // previous tile's epilogue, before this tile's first barrier)
    if (has_next && tid >= TM && tid < TM + TN) {
      s_bsq[(par ^ 1) * TN + (tid - TM)] = nbsq;
      s_bsh[(par ^ 1) * TN + (tid - TM)] = nbsh;
    }
    if (live) {
      // ---- epilogue (the kernel above's, written out for the same reason) ----
      // (per-lane addresses from a laundered lane id: hoisted out of the tile
      // loop they would hold registers across the k loop and spill)
      int el = lane;
      asm volatile("" : "+v"(el));
      const int ehl = el >> 5;
      const int64_t n0 = (int64_t)ty * TN;
      const float* bq = s_bsq + par * TN;
      const int32_t* bs = s_bsh + par * TN;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int cb = wn * 64 + 32 * j + (el & 31);
        const float bsq = bq[cb];
        const int bsh = bs[cb];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int lr = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * ehl;
          const float dot = ldexpf(H[j][r] + (P[j][r] + Q[j][r]), -(s_ash[lr] + bsh));
          H[j][r] = rbf_split_value(s_asq[lr], bsq, dot, gamma);
        }
      }
      const bool interior = n0 + TN <= N;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int32_t orow = s_orow[wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * ehl];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int64_t col = n0 + wn * 64 + 32 * j + (el & 31);
          if (orow >= 0 && (interior || col < N)) out[(int64_t)orow * ldo + col] = H[j][r];
        }
      }
    }
    // the stores and the next tile's blocks 0 / 1 retired: the loop's uniform
    // vmcnt(4) holds at the next tile's first block (and no DMA is in flight
    // when the kernel ends)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (!has_next) break;
    ty = tn_next;
    par ^= 1;
  }
}

// ---------------------------------------------------------------------------
// Persistent small-K ROWS GEMM (nkb <= 2 k blocks: d <= 64, covtype's 54
// features).  There a tile is two k blocks of MFMA work against 24-98 KiB of
// operand and store traffic, so a tile-per-workgroup grid is a chain of
// latencies (load, multiply, store) per tile.  Here one 768-thread workgroup
// per CU walks the tiles of its grid stride (64 x 192 up to 192 x 64 by the
// miss count): the A rows of its tile row (<= 48 KiB) are staged into LDS
// once, the B column tiles (and their |x|^2 / shifts) stream through two LDS buffers by LDS-DMA, the next
// tile's DMA issued before this tile's multiply, so its latency hides under
// the multiply, the epilogue and the stores; a wave then waits with vmcnt(16)
// (its 16 stores of the tile before are younger than that DMA), so the stores
// drain under the next tile instead of being waited for (every live lane
// stores exactly 16 values: rows past M and columns past N go to a scratch
// line).  MFMA sequence and epilogue as the rows kernels above: bit-identical rows.
// ---------------------------------------------------------------------------
constexpr int kRowsPersistThreads = 768;
template <int NKB>
__global__ __launch_bounds__(kRowsPersistThreads, 1) void rbf_rows_split_persist_kernel(
    const u4* __restrict__ A, const int32_t* __restrict__ Ash, const float* __restrict__ Asq,
    const int32_t* __restrict__ a_rows, const int32_t* __restrict__ m_dev, const u4* __restrict__ B,
    const int32_t* __restrict__ Bsh, const float* __restrict__ Bsq, int64_t N, float gamma,
    float* __restrict__ out, int64_t ldo, const int32_t* __restrict__ out_rows, float* __restrict__ trash) {
  // 12 waves of 32 x 32 (one MFMA tile, three accumulators each), laid out by
  // the round's miss count M: WM x WN = 2 x 6 (64 x 192 tiles) up to 64
  // misses, 4 x 3 (128 x 96) up to 128, else 6 x 2 (192 x 64) — the fewest,
  // widest tiles that cover the live rows (a tile's cost is mostly latency)
  constexpr int CPR = 8, TMX = 192, TNX = 192;
  constexpr int ABUF = TMX * NKB * CPR, BBUF = TNX * NKB * CPR;  // u4
  const int M = *m_dev;
  const int WM = M <= 64 ? 2 : M <= 128 ? 4 : 6, WN = 12 / WM, TM = 32 * WM, TN = 32 * WN;
  const int tn = (int)((N + TN - 1) / TN), tm = (M + TM - 1) / TM, total = tm * tn;
  int L = blockIdx.x;
  if (L >= total) return;  // uniform
  __shared__ u4 lds[ABUF + 2 * BBUF + (2 * 2 * TNX) / 4 + (3 * TMX) / 4];
  u4* s_a = lds;                                          // [NKB][TM rows][CPR]
  u4* s_b = lds + ABUF;                                   // [2][NKB][TN rows][CPR]
  float* s_bsq = (float*)(lds + ABUF + 2 * BBUF);         // [2][TNX], then s_bsh [2][TNX]
  int32_t* s_bsh = (int32_t*)(s_bsq + 2 * TNX);
  float* s_asq = (float*)(s_bsh + 2 * TNX);
  int32_t* s_ash = (int32_t*)(s_asq + TMX);
  int32_t* s_orow = s_ash + TMX;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN, hl = lane >> 5;
  constexpr int64_t rstride = (int64_t)NKB * 8;
  const int nb = TN * NKB / 8, nv = (TN + 63) / 64;  // B-row DMA instructions; |x|^2 (and shift) ones per tile
  // B DMA of column tile ty into buffer b: instruction i (8 k-rows x 128 B) by
  // wave i % 12, then the |x|^2 / shift dwords by the waves after
  auto dma = [&](int ty, int b) {
    const int64_t n0 = (int64_t)ty * TN;
    for (int i = wave; i < nb + 2 * nv; i += 12) {
      if (i < nb) {
        const int q = 8 * i + (lane >> 3), kb = q / TN, r = q % TN;
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        lds_dma16(B + (n0 + r) * rstride + kb * 8 + c, s_b + b * BBUF + 8 * i * CPR);
      } else {
        const int v = i - nb, part = v % nv;
        const int64_t cc = min(n0 + 64 * part + lane, N - 1);
        if (v < nv) lds_dma4(Bsq + cc, s_bsq + b * TNX + 64 * part);
        else lds_dma4(Bsh + cc, s_bsh + b * TNX + 64 * part);
      }
    }
  };
  dma(L % tn, 0);
  int ltx = -1, buf = 0;
  bool stored = false;  // this wave's 16 stores of the previous tile are younger than the pending DMA
  const int sw = ((lane & 31) >> 1) & 7;
  for (; L < total; L += gridDim.x) {
    const int tx = L / tn, ty = L % tn;
    const int64_t m0 = (int64_t)tx * TM, n0 = (int64_t)ty * TN;
    if (tx != ltx) {
      // the A rows of this tile row (plain loads: the first tile, or a new tile
      // row of a multi-block round's misses); every wave is past the old rows
      __syncthreads();
      for (int id = tid; id < TM * NKB * CPR; id += kRowsPersistThreads) {
        const int kb = id / (TM * CPR), r = (id / CPR) % TM, c = id % CPR;
        const int64_t ar = a_rows[min(m0 + r, (int64_t)M - 1)];
        s_a[(kb * TM + r) * CPR + (c ^ ((r >> 1) & 7))] = A[ar * rstride + kb * 8 + c];
      }
      if (tid < TM) {
        const int64_t row = m0 + tid;
        const int64_t ar = a_rows[min(row, (int64_t)M - 1)];
        s_asq[tid] = Asq[ar];
        s_ash[tid] = Ash[ar];
        s_orow[tid] = row < M ? out_rows[row] : -1;
      }
      ltx = tx;
      stored = false;  // those loads were waited for: nothing older is outstanding
    }
    const bool live = m0 + wm * 32 < M;
    // this tile's DMA has landed; the previous tile's stores may still drain
    if (stored) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ring_barrier();
    if (L + (int)gridDim.x < total) dma((L + gridDim.x) % tn, buf ^ 1);  // every wave is past buffer buf ^ 1
    if (live) {
      f16v H, P, Q;
#pragma unroll
      for (int r = 0; r < 16; ++r) H[r] = P[r] = Q[r] = 0.f;
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        const int ra = ((kb * TM) + wm * 32 + (lane & 31)) * CPR;
        const int rb = (buf * BBUF) + (kb * TN + wn * 32 + (lane & 31)) * CPR;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const int ch = (2 * ks + hl) ^ sw, cl = (4 + 2 * ks + hl) ^ sw;
          const h8 ah = __builtin_bit_cast(h8, s_a[ra + ch]);
          const h8 al = __builtin_bit_cast(h8, s_a[ra + cl]);
          const h8 bh = __builtin_bit_cast(h8, s_b[rb + ch]);
          const h8 bl = __builtin_bit_cast(h8, s_b[rb + cl]);
          H = mfma32_f16(ah, bh, H);
          P = mfma32_f16(ah, bl, P);
          Q = mfma32_f16(al, bh, Q);
        }
      }
      const int cb = wn * 32 + (lane & 31);
      const float bsq = s_bsq[buf * TNX + cb];
      const int bsh = s_bsh[buf * TNX + cb];
      const int64_t col = n0 + cb;
      const bool ok = col < N;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int lr = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * hl;
        const float v = w32_value(H[r], P[r], Q[r], s_ash[lr], bsh, s_asq[lr], bsq, gamma);
        const int32_t orow = s_orow[lr];
        // exactly 16 stores per lane (the vmcnt(16) above): rows past M and
        // columns past N go to the scratch line
        float* dst = (orow >= 0 && ok) ? out + (int64_t)orow * ldo + col : trash + lane;
        *dst = v;
      }
    }
    stored = live;
    buf ^= 1;
  }
}

}  // namespace dev

namespace launch {

// diagnostics: non-null = the LDS-DMA rows kernel writes per-workgroup stamps here
uint64_t* g_rows_stamps = nullptr;
void set_rows_stamps(uint64_t* p) { g_rows_stamps = p; }

void rbf_rows_indexed_split(const void* X, const int32_t* Xsh, const float* Xsq, const int32_t* a_rows,
                            const int32_t* m_dev, int64_t M_max, const void* B, const int32_t* Bsh, const float* Bsq,
                            int64_t N, int dp, float gamma, float* lines, const int32_t* out_rows, int64_t ldl,
                            hipStream_t s) {
  if (M_max <= 0 || N <= 0) return;
  // 192 x 128 tiles (12 waves): a one-block round's misses (<= 192 rows) are
  // one tile row, so every column panel of B — all of this rank's rows, the
  // bytes that bound this GEMM — is read from HBM once per round (64-row
  // tiles read it once per 64 misses)
  const int64_t tm = (M_max + 191) / 192, tn = (N + 127) / 128;
  DPSVM_CHECK(tn < 65536, "rbf_rows_indexed_split: N too large for grid.y");
  const int nkb = (dp + 31) / 32;
  if (nkb <= 2) {  // persistent small-K kernel
    // the scratch line of the fixed-count stores (64 floats, never read), one per device
    static std::mutex trash_mu;
    static float* trash_of[kMaxDevices] = {};
    float* trash = nullptr;
    {
      const int device = current_device();
      std::lock_guard<std::mutex> lk(trash_mu);
      if (!trash_of[device]) HIP_CHECK(hipMalloc((void**)&trash_of[device], 64 * sizeof(float)));
      trash = trash_of[device];
    }
    const int64_t grid = std::min<int64_t>(tm * tn, persistent_grid_limit());
    auto k = nkb == 1 ? dev::rbf_rows_split_persist_kernel<1> : dev::rbf_rows_split_persist_kernel<2>;
    k<<<dim3((unsigned)grid), dev::kRowsPersistThreads, 0, s>>>((const dev::u4*)X, Xsh, Xsq, a_rows, m_dev,
                                                                (const dev::u4*)B, Bsh, Bsq, N, gamma, lines, ldl,
                                                                out_rows, trash);
  } else if (tm == 1 && !g_rows_stamps && (N + 512) * (int64_t)nkb * 8 < (1ll << 32)) {
    // persistent over the column tiles (one tile row; 32-bit u4 offsets into B)
    const int64_t grid = std::min<int64_t>(tn, persistent_grid_limit());
    dev::rbf_rows_split_glds_persist_kernel<<<dim3((unsigned)grid), dev::kRowsGldsThreads, 0, s>>>(
        (const dev::u4*)X, Xsh, Xsq, a_rows, m_dev, (const dev::u4*)B, Bsh, Bsq, N, nkb, gamma, lines, ldl, out_rows,
        (int)tn);
  } else {
    auto k = g_rows_stamps ? dev::rbf_rows_split_glds_kernel<true> : dev::rbf_rows_split_glds_kernel<false>;
    k<<<dim3((unsigned)tm, (unsigned)tn), dev::kRowsGldsThreads, 0, s>>>((const dev::u4*)X, Xsh, Xsq, a_rows, m_dev,
                                                                        (const dev::u4*)B, Bsh, Bsq, N, nkb, gamma,
                                                                        lines, ldl, out_rows, g_rows_stamps);
  }
  post_launch("rbf_rows_indexed_split", s);
}

}  // namespace launch
}  // namespace dpsvm
