// RBF GEMM on fp16 MFMA with split operands (v_mfma_f32_32x32x16_f16): the
// fp32 dot products of the Gram at fp32 accuracy for 3/16 of the f32-MFMA time.
//
// Why: the f32-input MFMA (rbf_gemm.hip) runs at 1/16 of the f16 rate, and the
// Gram GEMM is half of the headline solve.  Every X row is scaled by a power of
// two (its largest |x| to [2^14, 2^15)) and split into two fp16 planes,
//     x * 2^s = h + l,   h = fp16(x 2^s),  l = fp16(x 2^s - h)      (22 bits)
// and a . b = 2^-(s_a + s_b) (h_a.h_b + (h_a.l_b + l_a.h_b)), the l_a.l_b term
// (2^-22 relative) dropped.  Each fp16 product is exact in fp32 and the MFMA
// accumulates in fp32, so the error vs fp64 is that of an f32 GEMM
// (tests/test_split_gemm_gpu.py and profiles/r3_split_gemm_*: max relative
// error per sum |a_k b_k| within 1.5x of the f32 MFMA kernel's on MNIST-shape,
// Gaussian and covtype-shape data).
//
// Symmetry: the three products go to three accumulators H = sum h_a h_b,
// P = sum h_a l_b, Q = sum l_a h_b and the result is H + (P + Q).  Swapping the
// operands swaps P and Q bit for bit (the same products in the same k order)
// and leaves H unchanged, so K(i, j) computed with i as the A row equals K(j, i)
// computed with j as the A row, bit for bit.  The symmetric Gram (upper tiles
// mirrored), the sharded Gram (every rank's columns, A = all rows) and the
// working-set cache's indexed rows therefore hold identical values, as the
// f32 kernels do.
//
// Operand layout ("split rows", split_rows_f16 below): row i is dp32/32 blocks
// of 128 B, each 32 h values then the 32 l values of k = 32 b .. 32 b + 31, so
// one 128-B line per row per k-stage (a whole line per load group of 8 lanes).
//
// Tiling of the first kernel (rbf_gemm_split_kernel, now the tests' reference):
// 8 waves, each 32 rows x 64 columns (2 MFMA 32x32 tiles, three accumulators
// each: 96 accumulator registers), 4 x 2 = 128 x 128 block tiles, LDS double
// buffered through registers; LDS rows are the row blocks with the 16-B chunk
// index XORed so that every ds_read_b128 lane group of the operand reads (16
// rows, one chunk) hits 16 distinct bank quads.  The kernels after it keep its
// per-element MFMA sequence (bit-identical values) and stage by LDS-DMA.
//
// Which kernel a Gram runs: launch::split_gram_path (kernels.hpp), first
// eligible of
//   Adaptive    h1 one-product pass + w64p over the hot tiles: cold_tau > 0,
//               >= 5 k blocks, ldo < 2^21, rows / tile tables in 32 bits (the
//               solver's resident Gram and its slabs)
//   W64Persist  w64p: the same without cold_tau, and M ldo, N ldo < 2^32
//   W64Grid     w64, a tile per workgroup: >= 5 k blocks, ldo < 2^21 (three-
//               product Grams of more than 2^32 elements)
//   Glds        128 x 128 LDS-DMA tiles, 64-bit indexing: everything else
//   Tile        forced only
// Variants that lost their A/B are not compiled; their measurements are in
// profiles/.
//
// This file: the operand prep (split rows, h planes, log2 norms), the STORE
// GEMMs (tile, glds, w64, w64p, h1) and their launch plan.  The working-set
// row GEMM is in rbf_rows_split.hip, the decision GEMM in
// rbf_predict_split.hip; the k blocks and epilogues all of them share are in
// split_mma.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "dpsvm/common.hpp"
#include "device_util.hpp"
#include "kernels.hpp"
#include "gram_tile_order.hpp"
#include "split_mma.hpp"
#include "../runtime/hip_check.hpp"

namespace dpsvm {
namespace dev {

constexpr int kSplitThreads = 512;
constexpr int kSplitShiftTarget = 15;  // largest |x| scaled into [2^14, 2^15)

// One wave per row: shift[r] and the h / l planes of row r (columns past dp
// are zero).  Lane q owns the 8-value chunks q, q + 64, ... (chunk q = columns
// 8 q .. 8 q + 7 = block q / 4, chunk q % 4 of both planes): the row is read
// once, as 16-B loads all in flight, the row max taken from the registers —
// 143 us for the headline's 60000 x 784 as a two-pass kernel with 4-B loads.
constexpr int kSplitRowChunks = 4;  // chunks per lane held in registers (dp <= 2048); longer rows loop
__global__ __launch_bounds__(256) void split_rows_kernel(const float* __restrict__ x, int64_t rows, int dp, int ldx,
                                                         u4* __restrict__ out, int32_t* __restrict__ shift,
                                                         int nkb) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* xr = x + r * (int64_t)ldx;
  const int nq = nkb * 4;  // chunks of the padded row
  const bool vec = ((ldx & 3) == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0);
  auto load = [&](int q, f4& lo, f4& hi) {
    const int k0 = 8 * q;
    if (vec && k0 + 8 <= dp) {
      lo = *(const f4*)(xr + k0);
      hi = *(const f4*)(xr + k0 + 4);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        lo[j] = k0 + j < dp ? xr[k0 + j] : 0.f;
        hi[j] = k0 + 4 + j < dp ? xr[k0 + 4 + j] : 0.f;
      }
    }
  };
  auto emit = [&](int q, const f4& lo, const f4& hi, int s) {
    const int b = q >> 2, c = q & 3;
    h8 hv, lv;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = ldexpf(j < 4 ? lo[j] : hi[j - 4], s);
      const _Float16 h = (_Float16)v;
      hv[j] = h;
      lv[j] = (_Float16)(v - (float)h);
    }
    u4* orow = out + r * (int64_t)nkb * 8;
    orow[8 * b + c] = __builtin_bit_cast(u4, hv);
    orow[8 * b + 4 + c] = __builtin_bit_cast(u4, lv);
  };
  f4 vl[kSplitRowChunks], vh[kSplitRowChunks];
  float m = 0.f;  // largest |x| of the row (the wave's max; order-free, exact)
#pragma unroll
  for (int i = 0; i < kSplitRowChunks; ++i) {
    const int q = lane + 64 * i;
    if (q < nq) {
      load(q, vl[i], vh[i]);
#pragma unroll
      for (int j = 0; j < 4; ++j) m = fmaxf(m, fmaxf(fabsf(vl[i][j]), fabsf(vh[i][j])));
    }
  }
  for (int q = lane + 64 * kSplitRowChunks; q < nq; q += 64) {  // rows past 2048 columns
    f4 lo, hi;
    load(q, lo, hi);
#pragma unroll
    for (int j = 0; j < 4; ++j) m = fmaxf(m, fmaxf(fabsf(lo[j]), fabsf(hi[j])));
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  int e = 0;
  if (m > 0.f && isfinite(m)) (void)frexpf(m, &e);  // m = f 2^e, f in [0.5, 1)
  const int s = m > 0.f && isfinite(m) ? kSplitShiftTarget - e : 0;
  if (lane == 0) shift[r] = s;
#pragma unroll
  for (int i = 0; i < kSplitRowChunks; ++i) {
    const int q = lane + 64 * i;
    if (q < nq) emit(q, vl[i], vh[i], s);
  }
  for (int q = lane + 64 * kSplitRowChunks; q < nq; q += 64) {
    f4 lo, hi;
    load(q, lo, hi);
    emit(q, lo, hi, s);
  }
}

// The register-staged tile kernel: the first split STORE GEMM, kept as the
// tests' bit-identity reference for the LDS-DMA kernels below (GramPath::Tile,
// forced only).  WM x WN = 4 x 2 waves, a 128 x 128 workgroup tile; KB = 2
// 32-wide k blocks per LDS stage (256-B LDS rows, chunk index XOR row & 15:
// every ds_read_b128 lane group of the operand reads on 16 distinct bank quads).
__global__ __launch_bounds__(kSplitThreads, 1) void rbf_gemm_split_kernel(
    const u4* __restrict__ A, const int32_t* __restrict__ Ash, const float* __restrict__ Asq, int64_t M,
    const u4* __restrict__ B, const int32_t* __restrict__ Bsh, const float* __restrict__ Bsq, int64_t N, int nkb,
    float gamma, float* __restrict__ out, int64_t ldo, int sym) {
  constexpr int WM = 4, WN = 2, KB = 2;
  constexpr int THREADS = 64 * WM * WN, TM = 32 * WM, TN = 64 * WN, ROWS = TM + TN;
  constexpr int CPR = 8 * KB;                    // 16-B chunks per row and stage
  constexpr int CH = ROWS * CPR;                 // chunks per stage
  constexpr int NL = (CH + THREADS - 1) / THREADS;  // chunks per thread (the last one: a spare LDS slot)
  static_assert(THREADS == kSplitThreads && THREADS >= TM, "stage geometry");
  int64_t tx, ty;
  xcd_tile(tx, ty);
  if (sym && ty < tx) return;
  __shared__ u4 lds[2][CH + 1];  // + a spare slot for the staging remainder
  __shared__ float s_asq[TM];
  __shared__ int32_t s_ash[TM];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int64_t m0 = tx * TM, n0 = ty * TN;
  const int64_t rstride = (int64_t)nkb * 8;  // u4 per split row
  const int nst = (nkb + KB - 1) / KB;       // stages

  if (tid < TM) {
    const int64_t ar = min(m0 + tid, M - 1);
    s_asq[tid] = Asq[ar];
    s_ash[tid] = Ash[ar];
  }

  // staging: chunk id = tid + THREADS i -> stage row id / CPR (A rows, then B
  // rows), chunk id % CPR; ids past the stage load a valid chunk into the spare slot
  const u4* src[NL];
  int dst[NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int idr = tid + THREADS * i, spare = idr >= CH, id = spare ? 0 : idr, r = id / CPR, c = id % CPR;
    int64_t grow;
    const u4* base;
    if (r < TM) {
      grow = m0 + r;  // rows past M: read a valid row (never stored)
      base = A;
    } else {
      grow = n0 + (r - TM);
      base = B;
    }
    src[i] = base + grow * rstride + c;
    dst[i] = spare ? CH : r * CPR + (c ^ (r & 15));
  }
  // chunk i of a stage belongs to k block (i % CPR) / 8 of it: the last stage
  // of an odd block count computes its first block only, and its chunks of the
  // missing block re-read the block before (an address select, not a branch
  // around the load: hipcc would wait vmcnt(0) at every such branch)
  auto load = [&](u4* st, int kt) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int blk = ((tid + THREADS * i) % CPR) >> 3;
      const int64_t o = (int64_t)kt * CPR - (kt * KB + blk >= nkb ? 8 : 0);
      st[i] = src[i][o];
    }
  };
  u4 st[NL];
  load(st, 0);
#pragma unroll
  for (int i = 0; i < NL; ++i) lds[0][dst[i]] = st[i];
  __syncthreads();

  f16v H[2], P[2], Q[2];
  zero_acc(H, P, Q);

  // operand rows of this lane: A row wm*32 + (lane&31), B rows TM + wn*64 + 32 j + (lane&31)
  const int sw = lane & 15, hl = lane >> 5;
  const int ra = (wm * 32 + (lane & 31)) * CPR;
  const int rb0 = (TM + wn * 64 + (lane & 31)) * CPR, rb1 = rb0 + 32 * CPR;
  int cur = 0;
  for (int kt = 0; kt < nst; ++kt) {
    const bool more = kt + 1 < nst;
    if (more) load(st, kt + 1);
#pragma unroll
    for (int blk = 0; blk < KB; ++blk) {
      if (kt * KB + blk >= nkb) break;  // uniform
      w32_kblock(H, P, Q, lds[cur], lds[cur], ra, rb0, rb1, hl, sw, 8 * blk);
    }
    if (more) {
#pragma unroll
      for (int i = 0; i < NL; ++i) lds[cur ^ 1][dst[i]] = st[i];
    }
    __syncthreads();
    cur ^= 1;
  }

  // ---- epilogue: K = exp(-g max(|a|^2 + |b|^2 - 2 dot, 0)), dot = 2^-(sa+sb) (H + (P + Q)) ----
  // (all values first, into H; then the stores: unpredicated for interior tiles.  The A rows' data goes
  // through registers ahead of the B columns' global loads, so this loop is w32_values written out)
  float asq_r[16];
  int ash_r[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int lr = wm * 32 + mfma32_row(r) + 4 * hl;
    asq_r[r] = s_asq[lr];
    ash_r[r] = s_ash[lr];
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t col = n0 + wn * 64 + 32 * j + (lane & 31);
    const int64_t cc = col < N ? col : N - 1;
    const float bsq = Bsq[cc];
    const int bsh = Bsh[cc];
#pragma unroll
    for (int r = 0; r < 16; ++r) H[j][r] = w32_value(H[j][r], P[j][r], Q[j][r], ash_r[r], bsh, asq_r[r], bsq, gamma);
  }
  w32_store_tile(H, out, ldo, m0 + wm * 32, n0 + wn * 64, hl, lane, M, N, m0 + TM <= M && n0 + TN <= N,
                 sym && ty != tx);
}

// ---------------------------------------------------------------------------
// LDS-DMA STORE GEMM: the tile kernel's MFMA sequence (128 x 128 tile, 8 waves
// of 32 x 64, k blocks in order: bit-identical Gram) with the operands staged
// by global_load_lds_dwordx4 into FOUR 32-k buffers, three blocks in flight
// ahead of the one being multiplied.  Per k block: a counted vmcnt retires the
// block's own DMA (never vmcnt(0) inside the loop), one raw s_barrier (the DMA
// has landed everywhere, and every wave is done with the buffer the next DMA
// overwrites), the DMA of block kb + 3, then 2 k16 steps of 6 MFMAs.  The
// register-staged kernels above wait for each stage's loads before the next
// stage can start (one stage of prefetch: a 0.3-0.6 us stage against a 1-2 us
// L2-miss latency).  An LDS-DMA wave instruction writes 1 KiB lane-linearly (8
// rows x 128 B): the bank swizzle of the operand reads (chunk c of row r at
// position c ^ ((r >> 1) & 7)) moves to the per-lane SOURCE address.  All LDS
// in one array (row data after the buffers): a second __shared__ object makes
// hipcc wait vmcnt(0) before the operand reads.
// ---------------------------------------------------------------------------
constexpr int kGldsThreads = 512;
__global__ __launch_bounds__(kGldsThreads, 1) void rbf_gemm_split_glds_kernel(
    const u4* __restrict__ A, const int32_t* __restrict__ Ash, const float* __restrict__ Asq, int64_t M,
    const u4* __restrict__ B, const int32_t* __restrict__ Bsh, const float* __restrict__ Bsq, int64_t N, int nkb,
    float gamma, float* __restrict__ out, int64_t ldo, int sym) {
  constexpr int WN = 2, TM = 128, TN = 128, ROWS = TM + TN, CPR = 8, BUF = ROWS * CPR, NB = 4;
  int64_t tx, ty;
  xcd_tile(tx, ty);
  if (sym && ty < tx) return;
  __shared__ u4 lds[NB * BUF + 2 * ROWS / 4];  // 4 operand buffers, then |x|^2 [ROWS] and shifts [ROWS]
  float* s_sq = (float*)(lds + NB * BUF);
  int32_t* s_sh = (int32_t*)(lds + NB * BUF) + ROWS;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN, hl = lane >> 5;
  const int64_t m0 = tx * TM, n0 = ty * TN;
  const int64_t rstride = (int64_t)nkb * 8;  // u4 per split row

  if (tid < ROWS) {
    const int64_t ri = tid < TM ? min(m0 + tid, M - 1) : min(n0 + (tid - TM), N - 1);
    s_sq[tid] = tid < TM ? Asq[ri] : Bsq[ri];
    s_sh[tid] = tid < TM ? Ash[ri] : Bsh[ri];
  }
  // DMA sources: wave w fills rows 32 w + 8 i + (lane >> 3), i = 0..3 (waves 0-3: A rows,
  // 4-7: B rows); lane position p = lane & 7 takes global chunk p ^ ((row >> 1) & 7)
  const u4* src[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = 32 * wave + 8 * i + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    src[i] = r < TM ? A + (m0 + r) * rstride + c : B + (n0 + (r - TM)) * rstride + c;
  }
  auto dma = [&](int kb) {
    u4* dst = lds + (kb & (NB - 1)) * BUF + 32 * wave * CPR;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      lds_dma16(src[i] + (int64_t)kb * 8, dst + 8 * i * CPR);
  };
  __syncthreads();  // row data written (no DMA in flight yet)
  dma(0);
  if (nkb > 1) dma(1);
  if (nkb > 2) dma(2);

  f16v H[2], P[2], Q[2];
  zero_acc(H, P, Q);
  const int sw = ((lane & 31) >> 1) & 7;
  const int ra = (wm * 32 + (lane & 31)) * CPR;
  const int rb0 = (TM + wn * 64 + (lane & 31)) * CPR, rb1 = rb0 + 32 * CPR;
  for (int kb = 0; kb < nkb; ++kb) {
    // retire block kb's DMA: the blocks after it (up to 2) may stay in flight
    const int ahead = min(2, nkb - 1 - kb);
    if (ahead == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (ahead == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ring_barrier();
    if (kb + 3 < nkb) dma(kb + 3);  // into the buffer of block kb - 1 (every wave is past it)
    const u4* buf = lds + (kb & (NB - 1)) * BUF;
    w32_kblock(H, P, Q, buf, buf, ra, rb0, rb1, hl, sw);
  }

  // ---- epilogue (as the tile kernel) ----
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int cb = TM + wn * 64 + 32 * j + (lane & 31);
    w32_values(H[j], P[j], Q[j], s_sq + wm * 32 + 4 * hl, s_sh + wm * 32 + 4 * hl, s_sq[cb], s_sh[cb], gamma);
  }
  w32_store_tile(H, out, ldo, m0 + wm * 32, n0 + wn * 64, hl, lane, M, N, m0 + TM <= M && n0 + TN <= N,
                 sym && ty != tx);
}

// The w64 kernels' epilogue: the values two at a time in
// packed f32 (v_pk_add / v_pk_mul; the same IEEE operations per value, so the
// same bits as rbf_split_value), stores through buffer descriptors: a lane
// outside the tile's columns gets an out-of-range offset and rows past M fall
// beyond the descriptor's size, so the hardware drops them — one address add
// per store and no exec-mask branch.  The scalar epilogue was ~20 VALU and ~13
// SALU per value, VALU-issue-bound: 13.4k -> 10.0k cycles a tile
// (profiles/r6_gram_lds_readahead_ab.json).  Host (split_gram_path): a tile's
// 256 x ldo floats < 2^31 bytes.  lane: the caller's (laundered) lane id.
// AD: the adaptive Gram's hot-tile pass — every element takes the one-product
// value where split_cold allows it (R = log2 |x| from Ar / Br, global loads:
// this pass runs only the few tiles the one-product pass reported).
// The stores are h1_store_block's (below), written here per group of four
// rows between the groups' values: built as values plus h1_store_block calls
// the five w64 / w64p kernels come out 57-88 instructions longer with other
// waits and six more branches (no spill), so the two stay separate — a change
// to the packed stores is made in both.
template <bool AD = false>
__device__ __forceinline__ void w64_epilogue_pe(f16v (&H)[2][2], const f16v (&P)[2][2], const f16v (&Q)[2][2],
                                                const float* s_sq, const int32_t* s_sh, int lane, int wm, int wn,
                                                bool mirror, float* out, int64_t m0, int64_t n0, int64_t M, int64_t N,
                                                int64_t ldo, float gamma, const float* Ar = nullptr,
                                                const float* Br = nullptr, float c0 = 0.f, float c1 = 0.f) {
  constexpr int TM = 256, TN = 128;
  const int hl = lane >> 5;
  float* const ob = out + m0 * ldo + n0;  // direct block
  float* const mb = out + n0 * ldo + m0;  // mirrored block (symmetric: M == N)
  const uint32_t ld = (uint32_t)ldo;
  const int rlim = (int)min<int64_t>(M - m0, TM);  // tile rows inside [0, M)
  const int clim = (int)min<int64_t>(N - n0, TN);  // tile columns inside [0, N)
  constexpr uint32_t OOB = 0x80000000u;
  const int64_t ob_bytes = min<int64_t>((M - m0) * ldo * 4 - n0 * 4, (int64_t)OOB);
  const int64_t mb_bytes = min<int64_t>((N - n0) * ldo * 4 - m0 * 4, (int64_t)OOB);
  const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(ob, 0, (int)ob_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_m = __builtin_amdgcn_make_buffer_rsrc(mb, 0, (int)mb_bytes, 0x00020000);
  const float ng = -gamma, l2e = 1.4426950408889634f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int cl = wn * 64 + 32 * j + (lane & 31);
    const bool okc = cl < clim;
    const float bsq = s_sq[TM + cl];
    const int nbsh = -s_sh[TM + cl];
    const float rb = AD ? Br[min<int64_t>(n0 + cl, N - 1)] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int lr0 = wm * 64 + 32 * i + 4 * hl;  // value r sits on row lr0 + 8 (r >> 2) + (r & 3)
      const uint32_t vo = okc ? ((uint32_t)lr0 * ld + (uint32_t)cl) * 4u : OOB;  // value 0's byte offset
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f4 asq = *(const f4*)(s_sq + lr0 + 8 * g);
        const i4v ash = *(const i4v*)(s_sh + lr0 + 8 * g);
        f4 ar = {0.f, 0.f, 0.f, 0.f};
        if constexpr (AD) {
#pragma unroll
          for (int c = 0; c < 4; ++c) ar[c] = Ar[min<int64_t>(m0 + lr0 + 8 * g + c, M - 1)];
        }
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          const int r = 4 * g + e;
          f2 h, pp, qq;
          h.x = H[i][j][r];
          h.y = H[i][j][r + 1];
          pp.x = P[i][j][r];
          pp.y = P[i][j][r + 1];
          qq.x = Q[i][j][r];
          qq.y = Q[i][j][r + 1];
          f2 dot, sq, d2, t;
          {
#pragma clang fp contract(off)
            const f2 sum = h + (pp + qq);
            dot.x = ldexpf(sum.x, nbsh - ash[e]);
            dot.y = ldexpf(sum.y, nbsh - ash[e + 1]);
            sq.x = asq[e];
            sq.y = asq[e + 1];
            d2 = (sq + bsq) - (dot + dot);  // |a|^2 + |b|^2 - 2 dot (rbf_split_value)
            d2.x = d2.x > 0.f ? d2.x : 0.f;
            d2.y = d2.y > 0.f ? d2.y : 0.f;
            t = (ng * d2) * l2e;  // __expf(-gamma d2) = exp2((-gamma d2) log2 e)
            if constexpr (AD) {  // the one-product pass's value where it is within tau (split_cold)
              f2 dot1, d21, t1;
              dot1.x = ldexpf(h.x, nbsh - ash[e]);
              dot1.y = ldexpf(h.y, nbsh - ash[e + 1]);
              d21 = (sq + bsq) - (dot1 + dot1);
              d21.x = d21.x > 0.f ? d21.x : 0.f;
              d21.y = d21.y > 0.f ? d21.y : 0.f;
              t1 = (ng * d21) * l2e;
              if (split_cold(t1.x, ar[e] + rb, c0, c1)) t.x = t1.x;
              if (split_cold(t1.y, ar[e + 1] + rb, c0, c1)) t.y = t1.y;
            }
          }
          H[i][j][r] = __builtin_amdgcn_exp2f(t.x);
          H[i][j][r + 1] = __builtin_amdgcn_exp2f(t.y);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          // (a float local first: __builtin_bit_cast of a vector element
          // subscript reads element 0 in this hipcc)
          const float hv = H[i][j][r];
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(hv), rs_o, (int)(vo + (uint32_t)(8 * g + e) * ld * 4u),
                                                0, 0);
        }
      }
      if (mirror) {
        // transposed: lane (column cl) writes rows lr .. lr + 3 of mirrored row cl
        const uint32_t vm = okc ? ((uint32_t)cl * ld + (uint32_t)lr0) * 4u : OOB;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int lr = lr0 + 8 * q;
          f4 v;
          v.x = H[i][j][4 * q + 0];
          v.y = H[i][j][4 * q + 1];
          v.z = H[i][j][4 * q + 2];
          v.w = H[i][j][4 * q + 3];
          const uint32_t o = lr + 3 < rlim ? vm + 32u * q : OOB;
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i4v, v), rs_m, (int)o, 0, 0);
          if (rlim < TM) {  // uniform: the last row tile — the values of a partial quad one at a time
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const uint32_t oc = (lr + 3 >= rlim && lr + c < rlim) ? vm + 32u * q + 4u * c : OOB;
              const float vc = v[c];
              __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(vc), rs_m, (int)oc, 0, 0);
            }
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Wide-wave LDS-DMA STORE GEMM (variant 11): 256 x 128 tiles, 8 waves of
// 64 x 64 (2 x 2 MFMA tiles, three accumulators each: 192 accumulator
// registers at two waves per SIMD).  The 32 x 64 waves of the kernels above
// read 6 KiB of LDS operands per 6 MFMAs; with the DMA's 32 KiB of LDS writes
// per k block the LDS port needs ~167 B/clk per CU against 128 (PMC: ~35% MFMA
// busy).  A 64 x 64 wave reads 8 KiB per 12 MFMAs: ~114 B/clk with the DMA, so
// the MFMA pipe, not the LDS port, sets the pace.  Same per-element k order
// (H, P, Q over the k blocks in order): bit-identical to the other kernels.
// Symmetric mode: tile (tx, ty) covers 128-row blocks 2 tx and 2 tx + 1 of
// column block ty; computed when ty >= 2 tx, each block above the diagonal
// also stored transposed (the diagonal-straddling tile's lower block is
// written twice with the same bits).  Three 48 KiB buffers of 32 k, one block
// in flight while one is multiplied.
// ---------------------------------------------------------------------------
constexpr int kW64Threads = 512;
// ST: diagnostics only — per-workgroup s_memtime stamps
// (entry, first k block landed, k loop done, stores issued, stores done) and
// s_memrealtime at entry / end into stamps[8 blockIdx.x ..] (bench/gram_stamps.py)
// tiles: nullptr = the whole tm x tn grid in the XCD order; else a compact
// table of the tiles to compute (the symmetric Gram's upper tiles, host-built
// in the XCD order: no workgroup is launched only to exit)
// Spread: the next-but-one block's six LDS-DMA pieces are issued one after each
// group of four MFMAs instead of all six right after the k-block barrier (all
// eight waves then stall on the load path at once while the MFMA pipe idles).
// Read-ahead: the operand fragments are read from LDS one MFMA group
// ahead with counted lgkmcnt waits, so only the block's first group waits on
// LDS latency (k loop 63.8k -> 59.1k cycles a tile, bench/gram_stamps.py)
template <bool ST>
__global__ __launch_bounds__(kW64Threads, 1) void rbf_gemm_split_w64_kernel(
    const u4* __restrict__ A, const int32_t* __restrict__ Ash, const float* __restrict__ Asq, int64_t M,
    const u4* __restrict__ B, const int32_t* __restrict__ Bsh, const float* __restrict__ Bsq, int64_t N, int nkb,
    float gamma, float* __restrict__ out, int64_t ldo, int sym, const uint32_t* __restrict__ tiles,
    uint64_t* __restrict__ stamps) {
  constexpr int WN = 2, TM = 256, TN = 128, ROWS = TM + TN, CPR = 8, BUF = ROWS * CPR, NB = 3;
  uint64_t st[5] = {0, 0, 0, 0, 0}, rt0 = 0;
  if constexpr (ST) {
    st[0] = __builtin_amdgcn_s_memtime();
    rt0 = __builtin_amdgcn_s_memrealtime();
  }
  int64_t tx, ty;
  if (tiles) {
    const uint32_t t = tiles[blockIdx.x];  // (tx << 16) | ty
    tx = t >> 16;
    ty = t & 0xffffu;
  } else {
    xcd_tile(tx, ty);
  }
  if (sym && ty < 2 * tx) return;  // uniform: both 128-row blocks below the diagonal
  __shared__ u4 lds[NB * BUF + 2 * ROWS / 4];  // 3 operand buffers, then |x|^2 [ROWS] and shifts [ROWS]
  float* s_sq = (float*)(lds + NB * BUF);
  int32_t* s_sh = (int32_t*)(lds + NB * BUF) + ROWS;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN, hl = lane >> 5;
  const int64_t m0 = tx * TM, n0 = ty * TN;
  const int64_t rstride = (int64_t)nkb * 8;  // u4 per split row
  if (tid < ROWS) {
    const int64_t ri = tid < TM ? min(m0 + tid, M - 1) : min(n0 + (tid - TM), N - 1);
    s_sq[tid] = tid < TM ? Asq[ri] : Bsq[ri];
    s_sh[tid] = tid < TM ? Ash[ri] : Bsh[ri];
  }
  // DMA: wave w fills stage rows 48 w + 8 i + (lane >> 3), i = 0..5; lane
  // position p = lane & 7 takes global chunk p ^ ((row >> 1) & 7).  An 8-row
  // group is all A or all B rows: a wave-uniform base (SGPRs) plus a 32-bit
  // lane offset keeps the addressing out of the 256 registers the 192
  // accumulators leave room in
  const u4* base[6];
  uint32_t off[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int g = __builtin_amdgcn_readfirstlane(48 * wave + 8 * i);  // first row of the group (uniform)
    const int r = g + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    base[i] = g < TM ? A + (m0 + g) * rstride : B + (n0 + (g - TM)) * rstride;
    off[i] = (uint32_t)((lane >> 3) * rstride + c);
  }
  auto dma_piece = [&](int kb, int i) {
    u4* dst = lds + (kb % NB) * BUF + 48 * wave * CPR;
    lds_dma16(base[i] + (int64_t)kb * 8 + off[i], dst + 8 * i * CPR);
  };
  auto dma = [&](int kb) {
#pragma unroll
    for (int i = 0; i < 6; ++i) dma_piece(kb, i);
  };
  __syncthreads();  // row data written (no DMA in flight yet)
  dma(0);
  if (nkb > 1) dma(1);

  f16v H[2][2], P[2][2], Q[2][2];
  zero_acc(H, P, Q);
  const int sw = ((lane & 31) >> 1) & 7;
  const int ra0 = (wm * 64 + (lane & 31)) * CPR;
  const int rb0 = (TM + wn * 64 + (lane & 31)) * CPR;
  for (int kb = 0; kb < nkb; ++kb) {
    // retire block kb's DMA (block kb + 1 may stay in flight)
    if (kb + 1 < nkb) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ring_barrier();
    if constexpr (ST) {
      if (kb == 0) st[1] = __builtin_amdgcn_s_memtime();
    }
    // block kb + 2 goes into the buffer of block kb - 1 (every wave is past it)
    const bool spread = kb + 2 < nkb;  // uniform
    auto piece = [&](int i) {
      if (spread) {
        __builtin_amdgcn_sched_barrier(0);
        dma_piece(kb + 2, i);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    w64_kblock(H, P, Q, lds + (kb % NB) * BUF, ra0, rb0, hl, sw, piece);
  }

  if constexpr (ST) st[2] = __builtin_amdgcn_s_memtime();
  // ---- epilogue, one 32 x 32 MFMA tile at a time: values, direct stores,
  // transposed stores.  ONE code path for interior and edge tiles: a second,
  // interior-only copy (round 4) made the compiler spill 396 B of the live
  // accumulators to scratch (175 scratch instructions) ----
  const bool mirror = sym && ty > 2 * tx + (wm >> 1);  // this wave's 64 rows lie in 128-row block 2 tx + (wm >> 1)
  w64_epilogue_pe(H, P, Q, s_sq, s_sh, lane, wm, wn, mirror, out, m0, n0, M, N, ldo, gamma);
  if constexpr (ST) {
    st[3] = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    st[4] = __builtin_amdgcn_s_memtime();
    const uint64_t rt1 = __builtin_amdgcn_s_memrealtime();
    if (tid == 0) write_stamps(stamps + (size_t)blockIdx.x * 8, st, rt0, rt1, tx, ty);
  }
}

// ---------------------------------------------------------------------------
// Persistent wide-wave STORE GEMM (the default; variant 12): the w64 kernel's
// tile, k loop and epilogue, one workgroup per CU walking tiles L = b, b + G, ... of the
// same table.  The w64 kernel's stamps put ~12% of a tile in its prologue (row
// data, then the first LDS-DMA block's latency) with the MFMA pipe idle, and
// ~7% of the CU time between workgroups (237.5 of 256 in flight).  Here the
// LDS-DMA ring runs on across tiles: during the last two k blocks of tile t
// the prefetch slots load blocks 0 and 1 of tile t + 1 (a block counter g
// over all tiles picks the buffer, g mod 3), and the next tile's |x|^2 and
// shifts arrive by LDS-DMA into the other parity of a row-data area (issued
// after tile t's k loop); every epilogue ends with vmcnt(0), so the loop's one
// uniform wait holds at the next tile's first block.  With the packed
// epilogue: 8.86 vs 9.01 ms symmetric, 2.30 vs 2.47 ms for the P = 8 slab
// against the w64 kernel (profiles/r6_gram_lds_readahead_ab.json).  Same MFMA
// sequence per output: bit-identical to the w64 kernel.
// ST: per-tile stamps (first wait, first block landed, k loop done, stores
// issued) and s_memrealtime at the tile's start / end into stamps[8 L ..].
// ---------------------------------------------------------------------------
// LDS-DMA piece of a k block into ring buffer buf.  The persistent kernel
// gives every wave four pieces of A rows (wave w: rows 32 w + 8 i) and two of B
// rows (rows 256 + 16 w + 8 i): six pieces a wave as in the w64 kernel (one
// uniform vmcnt), with two fixed source pointers and row bases, so a piece is
// one scalar add and two vector ops (u: the k block's row offset, uniform).
// Lane position p = lane & 7 takes global chunk p ^ ((row >> 1) & 7), the w64
// kernel's swizzle; for these rows that is p ^ (((lane >> 4) + 4 (i & 1)) & 7):
// two lane offsets for all pieces (off_e / off_o).
// The address is a uniform base plus the lane's byte offset (laundered by the
// caller, so it is not re-derived per piece): the saddr form of the DMA, no
// vector math per piece.
__device__ __forceinline__ void w64p_piece(const u4* __restrict__ src, u4* lds, uint32_t u, uint32_t step,
                                           int dst_row8, uint32_t off_e, uint32_t off_o, int buf, int i) {
  constexpr int BUF = 384 * 8;
  u4* dst = lds + buf * BUF + dst_row8 + i * 64;
  const char* base = (const char*)(src + (u + (uint32_t)i * step));  // uniform
  lds_dma16(base + ((i & 1) ? off_o : off_e), dst);
}

// a tile's |x|^2 and shifts into row-data parity par: dwords d = 64 (2 wave +
// i) + lane (two 4-B LDS-DMA instructions a wave, every wave: a uniform count
// for the waits; ROWS = 384 and TM = 256 are multiples of 64, so the array an
// instruction reads is wave-uniform); rows past M / N clamp as the w64 kernel's
// loads do
__device__ __forceinline__ void w64p_row_dma(const float* __restrict__ Asq, const float* __restrict__ Bsq,
                                             const int32_t* __restrict__ Ash, const int32_t* __restrict__ Bsh, int M,
                                             int N, uint32_t* s_rows, int wave, int lane, int m0, int n0, int par) {
  constexpr int TM = 256, ROWS = 384, RD = 1024;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int d0 = __builtin_amdgcn_readfirstlane(64 * (2 * wave + i));
    const int r0 = d0 < ROWS ? d0 : d0 - ROWS;    // uniform
    const bool a_rows = r0 < TM, sq = d0 < ROWS;  // uniform
    const uint32_t* arr = sq ? (a_rows ? (const uint32_t*)Asq : (const uint32_t*)Bsq)
                             : (a_rows ? (const uint32_t*)Ash : (const uint32_t*)Bsh);
    const int r = r0 + lane;
    const int ri = a_rows ? min(m0 + r, M - 1) : min(n0 + (r - TM), N - 1);
    const uint32_t* src = d0 >= 2 * ROWS ? arr : arr + ri;  // padding: any valid address
    lds_dma4(src, s_rows + par * RD + d0);
  }
}

// AD: the adaptive Gram's hot-tile pass — the tile count is read from
// ntiles_dev (written by the one-product pass) and the epilogue applies
// split_cold with Ar / Br, c0, c1.
template <bool ST, bool AD = false>
__global__ __launch_bounds__(kW64Threads, 1) void rbf_gemm_split_w64p_kernel(
    const u4* __restrict__ A, const int32_t* __restrict__ Ash, const float* __restrict__ Asq, int M,
    const u4* __restrict__ B, const int32_t* __restrict__ Bsh, const float* __restrict__ Bsq, int N, int nkb,
    float gamma, float* __restrict__ out, int ldo, int sym, const uint32_t* __restrict__ tiles, int ntiles,
    int tm, int tn, uint64_t* __restrict__ stamps, const float* __restrict__ Ar = nullptr,
    const float* __restrict__ Br = nullptr, float c0 = 0.f, float c1 = 0.f,
    const uint32_t* __restrict__ ntiles_dev = nullptr) {
  // 32-bit indices throughout (launcher: M, N, ldo and (M + 512) x nkb x 8 < 2^31):
  // the loop-carried tile state must fit the scalar registers beside the
  // k loop's, or the 192 accumulators spill
  constexpr int WN = 2, TM = 256, TN = 128, ROWS = TM + TN, CPR = 8, BUF = ROWS * CPR, NB = 3;
  constexpr int RD = 1024;  // row-data dwords per parity: |x|^2 [ROWS], shifts [ROWS], DMA padding
  __shared__ u4 lds[NB * BUF + 2 * RD / 4];  // 3 operand buffers, then row data [2][RD]
  uint32_t* const s_rows = (uint32_t*)(lds + NB * BUF);
  const int G = gridDim.x;
  int L = blockIdx.x;
  if constexpr (AD) ntiles = (int)__builtin_amdgcn_readfirstlane(*ntiles_dev);
  if (L >= ntiles) return;  // uniform: no barrier reached
  uint32_t t = tiles[L];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN, hl = lane >> 5;
  const uint32_t rs = (uint32_t)nkb * 8;  // u4 per split row
  // every wave: 4 pieces of A rows, 2 of B rows a k block (w64p_piece)
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  const uint32_t step = 8 * rs;
  // the lanes' byte offsets within a piece (even / odd pieces)
  uint32_t off_e = 16u * ((uint32_t)(lane >> 3) * rs + (uint32_t)((lane & 7) ^ (lane >> 4)));
  uint32_t off_o = 16u * ((uint32_t)(lane >> 3) * rs + (uint32_t)((lane & 7) ^ ((lane >> 4) + 4)));
  asm volatile("" : "+v"(off_e), "+v"(off_o));
  const int dstA = 32 * wv * 8, dstB = (TM + 16 * wv) * 8;
#define PIECE_A(uA_, buf_, i_) w64p_piece(A, lds, uA_, step, dstA, off_e, off_o, buf_, i_)
#define PIECE_B(uB_, buf_, i_) w64p_piece(B, lds, uB_, step, dstB, off_e, off_o, buf_, i_)
#define ROW_DMA(m0_, n0_, par_) w64p_row_dma(Asq, Bsq, Ash, Bsh, M, N, s_rows, wave, lane, m0_, n0_, par_)
  int Ln = L + G;
  uint32_t tn_next = Ln < ntiles ? tiles[Ln] : 0u;
  int par = 0;
  uint32_t g = 0;  // k blocks started over all of this workgroup's tiles: ring buffer g % NB
  {
    const int m0 = (int)(t >> 16) * TM, n0 = (int)(t & 0xffffu) * TN;
    ROW_DMA(m0, n0, 0);
#pragma unroll
    for (int b = 0; b < 2; ++b) {  // blocks 0 and 1 (launcher: nkb >= 3)
      const uint32_t uA = (uint32_t)(m0 + 32 * wv) * rs + (uint32_t)b * 8;
      const uint32_t uB = (uint32_t)(n0 + 16 * wv) * rs + (uint32_t)b * 8;
#pragma unroll
      for (int i = 0; i < 4; ++i) PIECE_A(uA, b, i);
#pragma unroll
      for (int i = 0; i < 2; ++i) PIECE_B(uB, b, i);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the loop's first wait counts 6 younger: tile 0 starts landed
  }
  const int sw = ((lane & 31) >> 1) & 7;
  const int ra0 = (wm * 64 + (lane & 31)) * CPR;
  const int rb0 = (TM + wn * 64 + (lane & 31)) * CPR;
  while (true) {
    uint64_t st[4] = {0, 0, 0, 0}, rt0 = 0;
    if constexpr (ST) {
      st[0] = __builtin_amdgcn_s_memtime();
      rt0 = __builtin_amdgcn_s_memrealtime();
    }
    const bool has_next = Ln < ntiles;  // uniform
    const int tx = (int)(t >> 16), ty = (int)(t & 0xffffu);
    const int m0 = tx * TM, n0 = ty * TN;
    // (the last tile prefetches its own blocks 0 / 1 into dead buffers: no branch in the loop)
    const uint32_t tp = has_next ? tn_next : t;
    const int nm0 = (int)(tp >> 16) * TM, nn0 = (int)(tp & 0xffffu) * TN;
    f16v H[2][2], P[2][2], Q[2][2];
    // (written out, not zero_acc: that form costs the k loop's entry a wait state)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) H[i][j][r] = P[i][j][r] = Q[i][j][r] = 0.f;
#pragma clang loop unroll(disable)
    for (int kb = 0; kb < nkb; ++kb) {
      // retire block kb's DMA: block kb + 1 (6 pieces a wave) may stay in flight.
      // Every k block prefetches (the last tile's last two re-load blocks 0 / 1
      // of itself into dead buffers) and every epilogue ends with vmcnt(0): one
      // wait, no branch (a taken branch a piece cost ~10% of the loop)
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      ring_barrier();
      if constexpr (ST) {
        if (kb == 0) st[1] = __builtin_amdgcn_s_memtime();
      }
      // the prefetch slot: block kb + 2 of this tile, or block kb + 2 - nkb of
      // the next one, into the buffer of block g - 1 (every wave is past it)
      const bool own = kb + 2 < nkb;
      const int pkb = own ? kb + 2 : kb + 2 - nkb;
      const uint32_t uA = (uint32_t)((own ? m0 : nm0) + 32 * wv) * rs + (uint32_t)pkb * 8;
      const uint32_t uB = (uint32_t)((own ? n0 : nn0) + 16 * wv) * rs + (uint32_t)pkb * 8;
      const int pbuf = (int)((g + 2) % NB);
      // after MFMA group j (0..5) of the block: A0, A1, B0, A2, A3, B1
      auto piece = [&](int j) {
        __builtin_amdgcn_sched_barrier(0);
        if (j == 2 || j == 5) PIECE_B(uB, pbuf, j == 2 ? 0 : 1);
        else PIECE_A(uA, pbuf, j < 2 ? j : j - 1);
        __builtin_amdgcn_sched_barrier(0);
      };
      w64_kblock(H, P, Q, lds + (g % NB) * BUF, ra0, rb0, hl, sw, piece);
      ++g;
    }
    if constexpr (ST) st[2] = __builtin_amdgcn_s_memtime();
    // the next tile's row data into the other parity (last read by the previous
    // tile's epilogue, before this tile's first barrier)
    if (has_next) ROW_DMA(nm0, nn0, par ^ 1);

    // ---- epilogue of the w64 kernel (row data from parity `par`) ----
    // (the per-lane epilogue addresses are recomputed per tile from a
    // laundered lane id: hoisted out of the tile loop they would hold ~64
    // registers across the k loop)
    int el = lane;
    asm volatile("" : "+v"(el));
    w64_epilogue_pe<AD>(H, P, Q, (const float*)(s_rows + par * RD), (const int32_t*)(s_rows + par * RD + ROWS), el,
                        wm, wn, sym && ty > 2 * tx + (wm >> 1), out, m0, n0, M, N, ldo, gamma, Ar, Br, c0, c1);
    // the stores, the next tile's blocks 0 / 1 and its row data retired here:
    // the loop's uniform vmcnt(6) then holds at the next tile's first block (and
    // no DMA is in flight when the kernel ends)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (ST) {
      st[3] = __builtin_amdgcn_s_memtime();
      const uint64_t rt1 = __builtin_amdgcn_s_memrealtime();
      if (tid == 0) {
        uint64_t* o = stamps + (size_t)L * 8;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = st[i];
        o[4] = st[3];
        o[5] = rt0;
        o[6] = rt1;
        o[7] = t;
      }
    }
    if (!has_next) break;
    L = Ln;
    t = tn_next;
    par ^= 1;
    Ln = L + G;
    if (Ln < ntiles) tn_next = tiles[Ln];
  }
}
#undef PIECE_A
#undef PIECE_B
#undef ROW_DMA

// ---------------------------------------------------------------------------
// Adaptive split Gram, pass 1: the one-product (h_a . h_b) Gram with per-tile
// hot reports (docs/DESIGN.md §13).  Where the kernel is far from the identity
// only near the diagonal (the headline: every off-diagonal K < 3e-6), the two
// correction products change no stored value by more than tau = 2^-22 — 45x
// below the three-product Gram's own error vs float64 — and split_cold proves
// it element by element.  This pass multiplies the h planes only (1/3 of the
// MFMAs, half the operand bytes), stores K1 everywhere and appends every tile
// holding an element split_cold rejects to a list; pass 2 (w64p, AD) recomputes
// those tiles with all three products.  The H accumulator's MFMA sequence is
// the three-product kernels' (same k order), so K1 and the rule's inputs are
// the same bits in both passes.
// The operands are h planes (split_hplane_kernel, stage-major); the tile is
// 256 x 256, the pair of 256 x 128 tiles the hot-tile pass counts in: 832 KB of
// operands through the CU per 256 KB of stores instead of 1,248 KB (the kernel
// is bound by the bytes through the CU's one memory pipeline, not by MFMAs or
// latency: profiles/gram_overlap/).  The kernel is described at its definition
// below.  Measured and dropped on the way (256 x 128 tiles,
// profiles/r6_gram_adapt/h1_ablation_kernels.txt, profiles/gram_overlap/): the
// split rows' h halves as operands (half of every fetched line unused: 7.32
// ms), deferring a tile's stores into the next tile's ring (spills, 10.3 ms),
// two workgroups per CU of 128 x 64 waves over 32-k stages (8.5 ms),
// staggered workgroup starts (no change); DMA waves apart from the compute
// waves were worth 3.5% there (6.32 -> 6.10 ms) and have no room beside the
// 16 compute waves of this tile.
// ---------------------------------------------------------------------------
// the one-product epilogue's math for one 32 x 32 MFMA block (i, j) of a wave:
// v becomes K1 = exp2(t1) in place; returns (per lane) whether one of the
// lane's elements is hot.  One block at a time, each followed by its stores
// (h1_store_block): the wave's first stores enter the memory pipeline after one
// block's values, not after all four
__device__ __forceinline__ bool h1_block_values(f16v& v, int i, int j, const float* s_sq, const int32_t* s_sh,
                                                const float* s_r, int lane, int wm, int wn, float gamma, float c0,
                                                float c1) {
  constexpr int TM = 256;
  const int hl = lane >> 5;
  const float ng = -gamma, l2e = 1.4426950408889634f;
  bool hot = false;
  const int cl = wn * 64 + 32 * j + (lane & 31);
  const float bsq = s_sq[TM + cl];
  const int nbsh = -s_sh[TM + cl];
  const float rb = s_r[TM + cl];
  const int lr0 = wm * 64 + 32 * i + 4 * hl;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f4 asq = *(const f4*)(s_sq + lr0 + 8 * g);
    const i4v ash = *(const i4v*)(s_sh + lr0 + 8 * g);
    const f4 ar = *(const f4*)(s_r + lr0 + 8 * g);
#pragma unroll
    for (int e = 0; e < 4; e += 2) {
      const int r = 4 * g + e;
      f2 h, dot, sq, d2, t;
      h.x = v[r];
      h.y = v[r + 1];
      {
#pragma clang fp contract(off)
        dot.x = ldexpf(h.x, nbsh - ash[e]);
        dot.y = ldexpf(h.y, nbsh - ash[e + 1]);
        sq.x = asq[e];
        sq.y = asq[e + 1];
        d2 = (sq + bsq) - (dot + dot);
        d2.x = d2.x > 0.f ? d2.x : 0.f;
        d2.y = d2.y > 0.f ? d2.y : 0.f;
        t = (ng * d2) * l2e;
        hot |= !split_cold(t.x, ar[e] + rb, c0, c1);
        hot |= !split_cold(t.y, ar[e + 1] + rb, c0, c1);
      }
      v[r] = __builtin_amdgcn_exp2f(t.x);
      v[r + 1] = __builtin_amdgcn_exp2f(t.y);
    }
  }
  return hot;
}

// the stores of one 32 x 32 MFMA block (i, j) of a wave's values v: 16 direct
// 4-B stores per lane, and for a mirroring wave 4 transposed 16-B ones (plus,
// on the last row tile, a partial quad's values one at a time); out-of-range
// offsets where a value has no place (the hardware drops those).  The same
// stores as w64_epilogue_pe's (above), which keeps its own copy: see there.
__device__ __forceinline__ void h1_store_block(const f16v& v, int i, int j, int lane, int wm, int wn, bool mirror,
                                               bool valid, float* out, int m0, int n0, int M, int N, int ldo) {
  constexpr int TM = 256, TN = 256;
  constexpr uint32_t OOB = 0x80000000u;
  const int hl = lane >> 5;
  float* const ob = out + ((int64_t)m0 * ldo + n0);
  float* const mb = out + ((int64_t)n0 * ldo + m0);
  const uint32_t ld = (uint32_t)ldo;
  const int rlim = min(M - m0, TM);
  const int clim = min(N - n0, TN);
  const int64_t ob_bytes = min<int64_t>((int64_t)(M - m0) * ldo * 4 - (int64_t)n0 * 4, (int64_t)OOB);
  const int64_t mb_bytes = min<int64_t>((int64_t)(N - n0) * ldo * 4 - (int64_t)m0 * 4, (int64_t)OOB);
  const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(ob, 0, (int)ob_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_m = __builtin_amdgcn_make_buffer_rsrc(mb, 0, (int)mb_bytes, 0x00020000);
  const int cl = wn * 64 + 32 * j + (lane & 31);
  const bool okc = valid && cl < clim;
  constexpr int CP = 0;  // buffer-store cache policy (non-temporal measured slower: profiles/r6_late)
  const int lr0 = wm * 64 + 32 * i + 4 * hl;
  const uint32_t vo = okc ? ((uint32_t)lr0 * ld + (uint32_t)cl) * 4u : OOB;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float hv = v[r];
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(hv), rs_o,
                                          (int)(vo + (uint32_t)(8 * (r >> 2) + (r & 3)) * ld * 4u), 0, CP);
  }
  if (!(mirror && valid)) return;  // uniform
  const bool okm = okc;
  const uint32_t vm = okm ? ((uint32_t)cl * ld + (uint32_t)lr0) * 4u : OOB;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int lr = lr0 + 8 * q;
    f4 w;
    w.x = v[4 * q + 0];
    w.y = v[4 * q + 1];
    w.z = v[4 * q + 2];
    w.w = v[4 * q + 3];
    const uint32_t o = lr + 3 < rlim && okm ? vm + 32u * q : OOB;
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i4v, w), rs_m, (int)o, 0, CP);
    if (rlim < TM) {  // uniform: the last row tile — a partial quad's values one at a time
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t oc = (okm && lr + 3 >= rlim && lr + c < rlim) ? vm + 32u * q + 4u * c : OOB;
        const float vc = w[c];
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(vc), rs_m, (int)oc, 0, CP);
      }
    }
  }
}

template <class T>
__device__ __forceinline__ T pick(bool c, T a, T b) {  // c ? a : b of two values
  return c ? a : b;
}

constexpr int kH1Threads = 1024;  // 16 waves of 64 x 64: 4 x 4 over a 256 x 256 tile
// The one-product pass: 256 x 256 tiles (the pair of 256 x 128 tiles (tx, 2 u), (tx, 2 u + 1) in one), one
// persistent workgroup a CU.  Operands are the stage-major h planes (split_hplane_kernel): a ring stage is 32 k of
// the tile's 256 A rows and 256 B rows, two contiguous 16-KiB blocks of whole lines; FOUR 32-KiB buffers, three
// stages in flight (96 KiB), the ring running on across tiles as in the w64p kernel.  Every wave issues two of a
// stage's 32 LDS-DMA pieces (waves 0-7: A rows 32 w + 16 i, waves 8-15: B rows), multiplies its 64 x 64 block
// (two k16 steps a stage: the H accumulator's MFMA sequence of every other kernel) and stores it; every epilogue
// ends with vmcnt(0), so the loop's one counted wait holds at the next tile's first stage.  LDS rows are 64 B:
// chunk c of stage row r sits at position c ^ ((r >> 2) & 3), so the 16 rows of a ds_read_b128 lane group hit 16
// distinct bank quads; the swizzle is in the lanes' source offsets, which are the same for every piece.
// Epilogue: one 32 x 32 block at a time, its values then its stores (h1_block_values / h1_store_block).
// Symmetric: tile (tx, u) is computed iff u >= tx; a tile right of the diagonal is also stored transposed, a
// diagonal tile computes both triangles and stores directly only.  Hot reports are per 256 x 128 half, as the
// hot-tile pass and gram_adapt_last count: half (tx, 2 u + h) is appended once iff one of its elements fails
// split_cold (half_hot [2 ntiles], zeroed: the per-half report counts; hot[0] the list's length, hot[1 ..] its
// entries).  tn: the Gram's count of 128-column tiles (an odd count: the last tile has a left half only — its
// right half's stores fall to the buffer range check, its row data indices clamp, and it is never reported).
// RA / RB: the rows of the A / B planes (multiples of 256).
__global__ __launch_bounds__(kH1Threads, 1) void rbf_gemm_split_h1_kernel(
    const u4* __restrict__ A, const int32_t* __restrict__ Ash, const float* __restrict__ Asq,
    const float* __restrict__ Ar, int M, int RA, const u4* __restrict__ B, const int32_t* __restrict__ Bsh,
    const float* __restrict__ Bsq, const float* __restrict__ Br, int N, int RB, int nst, float gamma, float c0,
    float c1, float* __restrict__ out, int ldo, int sym, const uint32_t* __restrict__ tiles, int ntiles, int tn,
    uint32_t* __restrict__ half_hot, uint32_t* __restrict__ hot) {
  constexpr int WN = 4, TM = 256, TN = 256, ROWS = TM + TN, CPR = 4, BUF = ROWS * CPR, NB = 4, RD = 2048;
  __shared__ u4 lds[NB * BUF + 2 * RD / 4];  // 4 operand buffers, then row data [2][RD]: |x|^2, shifts, log2 |x| [ROWS]
  uint32_t* const s_rows = (uint32_t*)(lds + NB * BUF);
  const int G = gridDim.x;
  int L = blockIdx.x;
  if (L >= ntiles) return;  // uniform: no barrier reached
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  const int wm = wave / WN, wn = wave % WN, hl = lane >> 5;
  // this wave's pieces of a stage: rows 32 wv + 16 i of the stage's 512 (A rows, then B rows)
  const bool a_wave = wv < 8;  // uniform
  const u4* const P = pick(a_wave, A, B);
  const int64_t R = pick(a_wave, RA, RB);
  const int prow = a_wave ? 32 * wv : 32 * (wv - 8);
  uint32_t loff = 16u * (uint32_t)((lane >> 2) * 4 + ((lane & 3) ^ ((lane >> 4) & 3)));  // bytes within a piece
  asm volatile("" : "+v"(loff));
  auto stage_dma = [&](int m0_, int n0_, int st, int buf) {
    const char* src = (const char*)(P + ((int64_t)st * R + pick(a_wave, m0_, n0_) + prow) * CPR);  // uniform
    u4* dst = lds + buf * BUF + 32 * wv * CPR;
    lds_dma16(src + loff, dst);
    lds_dma16(src + 1024 + loff, dst + 16 * CPR);
  };
  // a tile's row data into parity par_: 32 instructions of 64 dwords, two a wave; q = wv + 16 i < 24: array q / 8
  // (|x|^2, shifts, log2 |x|), rows 64 (q % 8) .. (A rows below 256); the rest load a valid word into the padding
  auto rowdata = [&](int m0_, int n0_, int par_) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = wv + 16 * i, ch = q & 7;  // uniform
      const bool a_rows = ch < 4, pad = q >= 24;
      // (pick: by value — a conditional on two captured pointers is an lvalue, and its address select keeps
      // the captures in scratch)
      const float* const fa = pick(q < 8 || pad, Asq, Ar);
      const float* const fb = pick(pad, Asq, pick(q < 8, Bsq, Br));
      const uint32_t* base = pick(q >= 8 && q < 16, (const uint32_t*)pick(a_rows, Ash, Bsh),
                                  (const uint32_t*)pick(a_rows, fa, fb));
      const int r = 64 * (ch & 3) + lane;
      const int ri = pad ? min(lane, M - 1) : a_rows ? min(m0_ + r, M - 1) : min(n0_ + r, N - 1);
      lds_dma4(base + ri, s_rows + par_ * RD + 64 * q);
    }
  };
  uint32_t t = tiles[L];
  int Ln = L + G;
  uint32_t tn_next = Ln < ntiles ? tiles[Ln] : 0u;
  uint32_t g = 0;  // stages started over all of this workgroup's tiles: ring buffer g % NB
  {
    const int m0 = (int)(t >> 16) * TM, n0 = (int)(t & 0xffffu) * TN;
    rowdata(m0, n0, 0);
    stage_dma(m0, n0, 0, 0);  // (launcher: nst >= 5)
    stage_dma(m0, n0, 1, 1);
    stage_dma(m0, n0, 2, 2);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the loop's first wait counts 4 younger: tile 0 starts landed
  }
  const int sw = (lane >> 2) & 3;
  const uint32_t ra0 = (uint32_t)(wm * 64 + (lane & 31)) * 64u, rb0 = (uint32_t)(TM + wn * 64 + (lane & 31)) * 64u;
  const uint32_t ck0 = 16u * (uint32_t)(hl ^ sw), ck1 = 16u * (uint32_t)((2 + hl) ^ sw);  // k16 steps 0 / 1
  int par = 0;
  while (true) {
    const bool has_next = Ln < ntiles;  // uniform
    const int tx = (int)(t >> 16), tu = (int)(t & 0xffffu);
    const int m0 = tx * TM, n0 = tu * TN;
    // (the last tile prefetches its own stages 0-2 into dead buffers: no branch in the loop)
    const uint32_t tp = has_next ? tn_next : t;
    const int nm0 = (int)(tp >> 16) * TM, nn0 = (int)(tp & 0xffffu) * TN;
    f16v H[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) H[i][j][r] = 0.f;
#pragma clang loop unroll(disable)
    for (int s = 0; s < nst; ++s) {
      // retire stage s's DMA: stages s + 1 and s + 2 (two pieces a wave each) may stay in flight
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      ring_barrier();
      // stage s + 3 of this tile, or stage s + 3 - nst of the next, into the buffer of stage g - 1
      const bool own = s + 3 < nst;
      stage_dma(own ? m0 : nm0, own ? n0 : nn0, own ? s + 3 : s + 3 - nst, (int)((g + 3) % NB));
      const uint32_t bb = lds_addr(lds + (g % NB) * BUF);
      const uint32_t pa = bb + ra0, pb = bb + rb0;
      auto rd = [&](uint32_t c, h8& a0, h8& a1, h8& b0, h8& b1) {
        const uint32_t qa = pa + c, qb = pb + c;
        asm volatile("ds_read_b128 %0, %1" : "=v"(a0) : "v"(qa) : "memory");
        asm volatile("ds_read_b128 %0, %1 offset:2048" : "=v"(a1) : "v"(qa) : "memory");  // + 32 rows
        asm volatile("ds_read_b128 %0, %1" : "=v"(b0) : "v"(qb) : "memory");
        asm volatile("ds_read_b128 %0, %1 offset:2048" : "=v"(b1) : "v"(qb) : "memory");
      };
      h8 x0, x1, x2, x3, y0, y1, y2, y3;
      rd(ck0, x0, x1, x2, x3);
      rd(ck1, y0, y1, y2, y3);
      asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3));
      H[0][0] = mfma32_f16(x0, x2, H[0][0]);
      H[0][1] = mfma32_f16(x0, x3, H[0][1]);
      H[1][0] = mfma32_f16(x1, x2, H[1][0]);
      H[1][1] = mfma32_f16(x1, x3, H[1][1]);
      __builtin_amdgcn_sched_barrier(0);  // (the second wait would otherwise move above the first step's MFMAs)
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(y0), "+v"(y1), "+v"(y2), "+v"(y3));
      H[0][0] = mfma32_f16(y0, y2, H[0][0]);
      H[0][1] = mfma32_f16(y0, y3, H[0][1]);
      H[1][0] = mfma32_f16(y1, y2, H[1][0]);
      H[1][1] = mfma32_f16(y1, y3, H[1][1]);
      ++g;
    }
    // the next tile's row data into the other parity (last read by the previous tile's epilogue)
    if (has_next) rowdata(nm0, nn0, par ^ 1);
    int el = lane;
    asm volatile("" : "+v"(el));
    const float* rows = (const float*)(s_rows + par * RD);
    const bool mirror = sym && tu > tx;
    // one 32 x 32 block at a time: its values, then its stores, so the waves feed the memory pipeline after
    // the first block's values.  The hot flag is reduced to a wave-uniform bit per block: one per-lane flag over
    // the four blocks lets the compiler sink every block's split_cold to the tile's end, its inputs live
    // across the stores
    bool hotw = false;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        __builtin_amdgcn_sched_barrier(0);
        hotw |= __builtin_amdgcn_ballot_w64(h1_block_values(H[i][j], i, j, rows, (const int32_t*)(rows + ROWS),
                                                            rows + 2 * ROWS, el, wm, wn, gamma, c0, c1)) != 0;
        __builtin_amdgcn_sched_barrier(0);
        h1_store_block(H[i][j], i, j, el, wm, wn, mirror, true, out, m0, n0, M, N, ldo);
      }
    const int half = wn >> 1, ty = 2 * tu + half;  // the wave's 256 x 128 half
    if (hotw && ty < tn && lane == 0) {  // the half's first report appends it to the list
      if (atomicAdd(half_hot + 2 * L + half, 1u) == 0u) {
        const uint32_t k = atomicAdd(hot, 1u);
        hot[1 + k] = ((uint32_t)tx << 16) | (uint32_t)ty;
      }
    }
    // the stores, the next tile's stages 0-2 and its row data retired here: the loop's uniform vmcnt(4) then
    // holds at the next tile's first stage (and no DMA is in flight when the kernel ends)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (!has_next) break;
    L = Ln;
    t = tn_next;
    par ^= 1;
    Ln = L + G;
    if (Ln < ntiles) tn_next = tiles[Ln];
  }
}

// h planes of split rows (the one-product pass's operands), stage-major: [k block][row][32 halfs] — a tile's
// 256-row panel of one ring stage is one contiguous 16-KiB block of whole 128-B lines
__global__ __launch_bounds__(256) void split_hplane_kernel(const u4* __restrict__ src, int64_t rows, int nkb,
                                                          u4* __restrict__ dst) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * nkb * 4) return;
  const int64_t b = e / (rows * 4), q = e - b * rows * 4, r = q >> 2;
  const int c = (int)(q & 3);
  dst[e] = src[r * nkb * 8 + b * 8 + c];
}

// R = log2 |x| = split_log2norm(|x|^2) of n rows (the adaptive Gram's rule input)
__global__ __launch_bounds__(256) void split_log2norm_kernel(const float* __restrict__ sq, int n,
                                                             float* __restrict__ r) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) r[i] = split_log2norm(sq[i]);
}

}  // namespace dev

namespace launch {

namespace {
int g_split_variant = -1;
}

int split_gemm_variant() {
  if (g_split_variant < 0) {
    const char* e = std::getenv("DPSVM_SPLIT_GEMM");  // test hook: the values of split_gram_path's `variant`
    g_split_variant = e ? atoi(e) : 0;
  }
  return g_split_variant;
}

void set_split_gemm_variant(int v) { g_split_variant = v; }

// The split STORE GEMM's launch plan, the one place its shape conditions live
// (rbf_gemm_store_split, the solver's setup and gram_adapt_prep all ask here).
// First eligible of Adaptive, W64Persist, W64Grid, Glds; a forced variant only
// removes candidates, so a shape it cannot take falls through to the next.
GramPath split_gram_path(const GramShape& g, int variant) {
  if (variant == 1) return GramPath::Tile;
  const bool any = variant != 3 && variant != 11 && variant != 12;  // 0 and unknown numbers: auto
  const int64_t nkb = (g.dp + 31) / 32, tm2 = (g.M + 255) / 256, tn = (g.N + 127) / 128;
  // The wide-wave kernels' packed epilogue (w64_epilogue_pe, h1_store_block)
  // stores through a buffer descriptor of at most 2^31 bytes at 32-bit byte
  // offsets from the tile's first element: the last of a tile's 256 rows starts
  // 255 ldo floats in, so 256 x ldo x 4 B < 2^31, ldo < 2^21.  (Beyond that the
  // hardware range check drops the late rows' stores without an error.)
  const bool wide = (any || variant == 11 || variant == 12) && nkb >= 5 && g.ldo < (1ll << 21);
  if (!wide) return GramPath::Glds;
  // persistent kernels: split operand rows ((rows + 512) x nkb x 8 u4) and tile tables in 32 bits
  const bool persist_ok = (any || variant == 12) && (g.M + 512) * nkb * 8 < (1ll << 31) &&
                          (g.N + 512) * nkb * 8 < (1ll << 31) && tm2 < 65536 && tn < 65536;
  if (persist_ok && g.cold) return GramPath::Adaptive;  // 64-bit tile bases: also Grams of more than 2^32 elements
  if (persist_ok && g.M * g.ldo < (1ll << 32) && g.N * g.ldo < (1ll << 32)) return GramPath::W64Persist;
  return GramPath::W64Grid;
}

const char* gram_path_name(GramPath p) {
  switch (p) {
    case GramPath::Tile: return "Tile";
    case GramPath::Glds: return "Glds";
    case GramPath::W64Grid: return "W64Grid";
    case GramPath::W64Persist: return "W64Persist";
    case GramPath::Adaptive: return "Adaptive";
  }
  return "?";
}

// diagnostics: non-null = the wide-wave Gram kernel writes per-workgroup stamps here
uint64_t* g_gram_stamps = nullptr;

void set_gram_stamps(uint64_t* p) { g_gram_stamps = p; }

int64_t split_row_u4(int dp) { return (int64_t)((dp + 31) / 32) * 8; }

int64_t split_pad_rows(int64_t rows) { return (rows + 255) / 256 * 256 + 256; }

int persistent_grid_limit() {
  int n = 0;
  HIP_CHECK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, current_device()));
  return std::max(8, n);
}

void split_rows_f16(const float* x, int64_t rows, int dp, int ldx, void* out, int32_t* shift, hipStream_t s) {
  if (rows <= 0) return;
  const int nkb = (dp + 31) / 32;
  dev::split_rows_kernel<<<dim3((unsigned)((rows + 3) / 4)), 256, 0, s>>>(x, rows, dp, ldx, (dev::u4*)out, shift,
                                                                          nkb);
  post_launch("split_rows_f16", s);
}

namespace {
// The symmetric Gram's upper tiles of the 256 x 128 wide-wave kernel (tile
// (tx, ty) is needed when ty >= 2 tx) as a compact table in an XCD order
// (chunks of CH tiles of GM tile rows dealt round-robin to the 8 XCDs, as
// xcd_tile_of does with 64 / 8): built once per shape on the host, kept on the device.  The full grid
// launched tm x tn workgroups of which half exited at once (55k of 110k on
// the headline).
struct TileTable {
  uint32_t* dev = nullptr;
  int64_t count = 0;
};
// Keyed by (device, tm, tn, sym, one_product): the table lives in the memory of the device that
// launches the GEMM (svmTrain -p N: one rank per device, threads of one process).
const TileTable& sym_tile_table(int64_t tm, int64_t tn, hipStream_t s, bool sym = true, bool one_product = false) {
  static std::mutex mu;
  static std::map<std::tuple<int, int64_t, int64_t, bool, bool>, TileTable> cache;
  const int device = current_device();
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find({device, tm, tn, sym, one_product});
  if (it != cache.end()) return it->second;
  // the needed tiles in groups of GM tile rows, column by column, rows inside a
  // column; chunks of CH consecutive tiles dealt round-robin to the 8 XCDs.
  // Three-product kernels: GM 4 / CH 32 (an XCD's chunk: 4 A panels x 8 B
  // panels), 9.34-9.45 ms vs 9.47-9.50 for GM 8 / CH 64
  // (profiles/r5_gram_tile_order_ab.txt; bit-identical output).  The one-product
  // pass has its own table of 256 x 256 tiles (gram_tile_order.hpp)
  std::vector<uint32_t> tab;
  if (one_product) {
    tab = gram_tile_order(tm, tn, sym);  // 256 x 256 tiles (gram_tile_order.hpp)
  } else {
    std::vector<uint32_t> order;
    const int64_t GM = 4, CH = 32;
    for (int64_t g0 = 0; g0 < tm; g0 += GM) {
      const int64_t gm = std::min(GM, tm - g0);
      for (int64_t ty = 0; ty < tn; ++ty)
        for (int64_t tx = g0; tx < g0 + gm; ++tx)
          if (!sym || ty >= 2 * tx) order.push_back((uint32_t)((tx << 16) | ty));
    }
    tab = xcd_deal(order, CH);
  }
  const int64_t total = (int64_t)tab.size();
  TileTable t;
  t.count = total;
  HIP_CHECK(hipMalloc((void**)&t.dev, (size_t)total * sizeof(uint32_t)));
  HIP_CHECK(hipMemcpyAsync(t.dev, tab.data(), (size_t)total * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return cache.emplace(std::make_tuple(device, tm, tn, sym, one_product), t).first->second;
}
}  // namespace

// split_cold's constants: E = e |a| |b| with e = 4.5 2^-11 gamma bounds gamma times the one- vs
// three-product d^2 difference; cold iff R_i + R_j <= c1 (E <= 1) and t1 <= c0 - (R_i + R_j)
// (1.72 K1 E <= tau, e^E - 1 <= 1.72 E for E <= 1), c0 with a 0.01 (0.7%) margin in log2
void split_cold_consts(float gamma, float tau, float* c0, float* c1) {
  const double e = 4.5 * std::ldexp(1.0, -11) * (double)gamma;
  *c1 = (float)(-std::log2(e));
  *c0 = (float)(std::log2((double)tau) - std::log2(1.72 * e) - 0.01);
}

namespace {
// the calling thread's last adaptive Gram (svmTrain -p N: one rank per thread)
thread_local int64_t t_adapt_tiles = -1;
thread_local uint32_t* t_adapt_hot = nullptr;  // pinned: the hot-tile count, copied after pass 1
}  // namespace

void gram_adapt_last(int64_t* tiles, int64_t* hot) {
  *tiles = t_adapt_tiles;
  *hot = t_adapt_tiles >= 0 && t_adapt_hot ? (int64_t)*(volatile uint32_t*)t_adapt_hot : -1;
}

void gram_adapt_prep(const void* A, const float* Asq, int64_t M, int dp, int64_t ldo, hipStream_t s,
                     GramAdaptPrep* prep) {
  *prep = GramAdaptPrep{};
  DPSVM_CHECK(M > 0 && split_gram_path(GramShape{M, M, ldo, dp, true, true}, split_gemm_variant()) ==
                           GramPath::Adaptive,
              "gram_adapt_prep: this Gram's plan is not adaptive");
  const int nkb = (dp + 31) / 32;
  const int64_t tm2 = (M + 255) / 256, tn = (M + 127) / 128;
  const int64_t ntiles = sym_tile_table(tm2, tn, s, true).count;
  const int64_t nt256 = sym_tile_table(tm2, tn, s, true, true).count;
  const int64_t ra = tm2 * 256, np = ra * nkb * 4;  // stage-major planes: [nkb][ra] rows of 4 u4
  const size_t pb = (size_t)np * 16, rb = (size_t)M * 4, hb = (size_t)(2 * nt256 + 1 + ntiles) * 4;
  HIP_CHECK(hipMalloc(&prep->planes, pb));
  HIP_CHECK(hipMalloc((void**)&prep->r, rb));
  HIP_CHECK(hipMalloc((void**)&prep->hot, hb));
  prep->bytes = pb + rb + hb;
  dev::split_hplane_kernel<<<dim3((unsigned)((np + 255) / 256)), 256, 0, s>>>((const dev::u4*)A, ra, nkb,
                                                                             (dev::u4*)prep->planes);
  post_launch("split_hplane", s);
  dev::split_log2norm_kernel<<<dim3((unsigned)((M + 255) / 256)), 256, 0, s>>>(Asq, (int)M, prep->r);
  post_launch("split_log2norm", s);
  prep->A = A;
  prep->M = M;
  prep->dp = dp;
  prep->ntiles = ntiles;
}

void gram_adapt_prep_free(GramAdaptPrep* prep) {
  if (prep->planes) (void)hipFree(prep->planes);
  if (prep->r) (void)hipFree(prep->r);
  if (prep->hot) (void)hipFree(prep->hot);
  *prep = GramAdaptPrep{};
}

namespace {
// One launch function per GramPath (rbf_gemm_store_split switches over split_gram_path's answer).
struct GramArgs {
  const void* A;
  const int32_t* Ash;
  const float* Asq;
  int64_t M;
  const void* B;
  const int32_t* Bsh;
  const float* Bsq;
  int64_t N;
  int dp, nkb;
  float gamma;
  float* out;
  int64_t ldo;
  bool symmetric;
  hipStream_t s;
};

void launch_gram_tile(const GramArgs& g) {
  const int64_t tm = (g.M + 127) / 128, tn = (g.N + 127) / 128;
  dev::rbf_gemm_split_kernel<<<dim3((unsigned)tm, (unsigned)tn), dev::kSplitThreads, 0, g.s>>>(
      (const dev::u4*)g.A, g.Ash, g.Asq, g.M, (const dev::u4*)g.B, g.Bsh, g.Bsq, g.N, g.nkb, g.gamma, g.out, g.ldo,
      g.symmetric ? 1 : 0);
  post_launch("rbf_gemm_store_split", g.s);
}

void launch_gram_glds(const GramArgs& g) {  // LDS-DMA, three k blocks in flight
  const int64_t tm = (g.M + 127) / 128, tn = (g.N + 127) / 128;
  dev::rbf_gemm_split_glds_kernel<<<dim3((unsigned)tm, (unsigned)tn), dev::kGldsThreads, 0, g.s>>>(
      (const dev::u4*)g.A, g.Ash, g.Asq, g.M, (const dev::u4*)g.B, g.Bsh, g.Bsq, g.N, g.nkb, g.gamma, g.out, g.ldo,
      g.symmetric ? 1 : 0);
  post_launch("rbf_gemm_split_glds", g.s);
}

// wide-wave, a tile per workgroup: the symmetric Gram's upper tiles from the compact table where it can
// index them (16-bit tile coordinates), else the whole grid
void launch_gram_w64_grid(const GramArgs& g) {
  const int64_t tm2 = (g.M + 255) / 256, tn = (g.N + 127) / 128;
  auto kern = g_gram_stamps ? dev::rbf_gemm_split_w64_kernel<true> : dev::rbf_gemm_split_w64_kernel<false>;
  if (g.symmetric && tm2 < 65536 && tn < 65536) {
    const auto& tab = sym_tile_table(tm2, tn, g.s);
    kern<<<dim3((unsigned)tab.count), dev::kW64Threads, 0, g.s>>>(
        (const dev::u4*)g.A, g.Ash, g.Asq, g.M, (const dev::u4*)g.B, g.Bsh, g.Bsq, g.N, g.nkb, g.gamma, g.out, g.ldo,
        1, tab.dev, g_gram_stamps);
  } else {
    kern<<<dim3((unsigned)tm2, (unsigned)tn), dev::kW64Threads, 0, g.s>>>(
        (const dev::u4*)g.A, g.Ash, g.Asq, g.M, (const dev::u4*)g.B, g.Bsh, g.Bsq, g.N, g.nkb, g.gamma, g.out, g.ldo,
        g.symmetric ? 1 : 0, nullptr, g_gram_stamps);
  }
  post_launch("rbf_gemm_split_w64", g.s);
}

// persistent over the tiles: one workgroup per CU, the LDS-DMA ring running on across tiles
// (non-symmetric: every tile, same XCD order)
void launch_gram_w64_persist(const GramArgs& g) {
  const int64_t tm2 = (g.M + 255) / 256, tn = (g.N + 127) / 128;
  const auto& t = sym_tile_table(tm2, tn, g.s, g.symmetric);
  const int64_t grid = std::min<int64_t>(t.count, persistent_grid_limit());
  auto pk = g_gram_stamps ? dev::rbf_gemm_split_w64p_kernel<true> : dev::rbf_gemm_split_w64p_kernel<false>;
  pk<<<dim3((unsigned)grid), dev::kW64Threads, 0, g.s>>>(
      (const dev::u4*)g.A, g.Ash, g.Asq, (int)g.M, (const dev::u4*)g.B, g.Bsh, g.Bsq, (int)g.N, g.nkb, g.gamma, g.out,
      (int)g.ldo, g.symmetric ? 1 : 0, t.dev, (int)t.count, (int)tm2, (int)tn, g_gram_stamps, nullptr, nullptr, 0.f,
      0.f, nullptr);
  post_launch("rbf_gemm_split_w64p", g.s);
}

// adaptive: pass 1 one-product over every tile, pass 2 three products over the reported ones.  Its kernels
// (h1, w64p with AD) index a tile's stores from 64-bit tile bases with 32-bit offsets and the operand rows
// in 32 bits: they also take Grams of more than 2^32 elements (200k rows: 160 GB)
void launch_gram_adaptive(const GramArgs& g, float cold_tau, const GramAdaptPrep* prep) {
  const int64_t tm2 = (g.M + 255) / 256, tn = (g.N + 127) / 128;
  const int64_t ntiles = sym_tile_table(tm2, tn, g.s, g.symmetric).count;  // in 256 x 128 units
  const auto& t1 = sym_tile_table(tm2, tn, g.s, g.symmetric, true);       // the one-product pass's 256 x 256 tiles
  const int64_t nt256 = t1.count;
  const int64_t grid1 = std::min<int64_t>(nt256, persistent_grid_limit());
  const int64_t grid2 = std::min<int64_t>(ntiles, persistent_grid_limit());
  float c0 = 0.f, c1 = 0.f;
  split_cold_consts(g.gamma, cold_tau, &c0, &c1);
  // a solver's prep of these very rows: the h planes and R are there, the hot buffer is re-zeroed
  const bool pre = prep && g.symmetric && prep->planes && prep->A == g.A && prep->M == g.M && prep->dp == g.dp &&
                   prep->ntiles == ntiles;
  const int64_t nr = g.symmetric ? g.M : g.M + g.N;
  float* r = pre ? prep->r : nullptr;
  // [2 nt256] per-half report counts, then the hot list: its length and its entries (at most ntiles)
  uint32_t* hb = pre ? prep->hot : nullptr;
  if (!pre) {
    HIP_CHECK(hipMallocAsync((void**)&r, (size_t)nr * 4, g.s));
    HIP_CHECK(hipMallocAsync((void**)&hb, (size_t)(2 * nt256 + 1 + ntiles) * 4, g.s));
  }
  HIP_CHECK(hipMemsetAsync(hb, 0, (size_t)(2 * nt256 + 1) * 4, g.s));
  uint32_t* const hot = hb + 2 * nt256;
  float* br = r;
  if (!pre) {
    dev::split_log2norm_kernel<<<dim3((unsigned)((g.M + 255) / 256)), 256, 0, g.s>>>(g.Asq, (int)g.M, r);
    if (!g.symmetric) {
      br = r + g.M;
      dev::split_log2norm_kernel<<<dim3((unsigned)((g.N + 255) / 256)), 256, 0, g.s>>>(g.Bsq, (int)g.N, br);
    }
    post_launch("split_log2norm", g.s);
  }
  // the stage-major h planes of the rows the tiles read (whole 256-row panels of A and of B)
  const int64_t ra = tm2 * 256, rb = g.symmetric ? ra : (g.N + 255) / 256 * 256;
  const dev::u4 *hA = nullptr, *hB = nullptr;
  dev::u4* planes = nullptr;
  if (pre) {
    hA = hB = (const dev::u4*)prep->planes;
  } else {
    const int64_t npa = ra * g.nkb * 4, npb = g.symmetric ? 0 : rb * g.nkb * 4;
    HIP_CHECK(hipMallocAsync((void**)&planes, (size_t)(npa + npb) * 16, g.s));
    dev::split_hplane_kernel<<<dim3((unsigned)((npa + 255) / 256)), 256, 0, g.s>>>((const dev::u4*)g.A, ra, g.nkb,
                                                                                  planes);
    hA = hB = planes;
    if (!g.symmetric) {
      dev::split_hplane_kernel<<<dim3((unsigned)((npb + 255) / 256)), 256, 0, g.s>>>((const dev::u4*)g.B, rb, g.nkb,
                                                                                    planes + npa);
      hB = planes + npa;
    }
    post_launch("split_hplane", g.s);
  }
  dev::rbf_gemm_split_h1_kernel<<<dim3((unsigned)grid1), dev::kH1Threads, 0, g.s>>>(
      hA, g.Ash, g.Asq, r, (int)g.M, (int)ra, hB, g.Bsh, g.Bsq, br, (int)g.N, (int)rb, g.nkb, g.gamma, c0, c1, g.out,
      (int)g.ldo, g.symmetric ? 1 : 0, t1.dev, (int)nt256, (int)tn, hb, hot);
  if (planes) HIP_CHECK(hipFreeAsync(planes, g.s));
  post_launch("rbf_gemm_split_h1", g.s);
  dev::rbf_gemm_split_w64p_kernel<false, true><<<dim3((unsigned)grid2), dev::kW64Threads, 0, g.s>>>(
      (const dev::u4*)g.A, g.Ash, g.Asq, (int)g.M, (const dev::u4*)g.B, g.Bsh, g.Bsq, (int)g.N, g.nkb, g.gamma, g.out,
      (int)g.ldo, g.symmetric ? 1 : 0, hot + 1, 0, (int)tm2, (int)tn, nullptr, r, br, c0, c1, hot);
  post_launch("rbf_gemm_split_w64p_hot", g.s);
  if (!t_adapt_hot) HIP_CHECK(hipHostMalloc((void**)&t_adapt_hot, 4, hipHostMallocDefault));
  HIP_CHECK(hipMemcpyAsync(t_adapt_hot, hot, 4, hipMemcpyDeviceToHost, g.s));
  t_adapt_tiles = ntiles;
  if (!pre) {
    HIP_CHECK(hipFreeAsync(r, g.s));
    HIP_CHECK(hipFreeAsync(hb, g.s));
  }
}
}  // namespace

void rbf_gemm_store_split(const void* A, const int32_t* Ash, const float* Asq, int64_t M, const void* B,
                          const int32_t* Bsh, const float* Bsq, int64_t N, int dp, float gamma, float* out,
                          int64_t ldo, hipStream_t s, bool symmetric, float cold_tau, const GramAdaptPrep* prep) {
  t_adapt_tiles = -1;
  if (M <= 0 || N <= 0) return;
  DPSVM_CHECK(!symmetric || (A == B && Asq == Bsq && Ash == Bsh && M == N && ldo % 4 == 0),
              "rbf_gemm_store_split: symmetric mode needs B == A, N == M");
  DPSVM_CHECK((N + 127) / 128 < 65536, "rbf_gemm_store_split: N too large for grid.y");
  const GramArgs g{A, Ash, Asq, M, B, Bsh, Bsq, N, dp, (dp + 31) / 32, gamma, out, ldo, symmetric, s};
  const bool cold = cold_tau > 0.f && gamma > 0.f;
  switch (split_gram_path(GramShape{M, N, ldo, dp, symmetric, cold}, split_gemm_variant())) {
    case GramPath::Tile: return launch_gram_tile(g);
    case GramPath::Glds: return launch_gram_glds(g);
    case GramPath::W64Grid: return launch_gram_w64_grid(g);
    case GramPath::W64Persist: return launch_gram_w64_persist(g);
    case GramPath::Adaptive: return launch_gram_adaptive(g, cold_tau, prep);
  }
}


}  // namespace launch
}  // namespace dpsvm
