// The wave-level pieces every split-operand GEMM kernel is built from
// (rbf_gemm_split.hip, rbf_rows_split.hip, rbf_predict_split.hip): the LDS-DMA
// call, the two k blocks (32 x 64 and 64 x 64 waves), the scalar epilogue and
// the 32 x 64 wave tile's stores.  Every kernel multiplies a k block and turns
// H, P, Q into K through THESE functions, so the Gram, its slabs, the cached
// rows and the decision values hold the same bits by construction.  No helper
// carries state.
#pragma once

#include "split_util.hpp"

namespace dpsvm {
namespace dev {

// One LDS-DMA wave instruction (global_load_lds): 16 or 4 bytes per lane,
// written lane-linearly from dst on.  AUX: the cache policy, an immediate (0,
// or 2 = nt)
template <int AUX = 0>
__device__ __forceinline__ void lds_dma16(const void* src, void* dst) {
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)dst, 16, 0, AUX);
}
__device__ __forceinline__ void lds_dma4(const void* src, void* dst) {
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)dst, 4, 0, 0);
}

// a ring stage's hand-over: this wave's LDS reads retired, then every wave at
// the barrier (the stage's DMA, waited for by the caller's vmcnt, has landed
// everywhere, and every wave is done with the buffer the next DMA overwrites)
__device__ __forceinline__ void ring_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// a wave's three accumulators (32 x 64 waves: [2], 64 x 64 waves: [2][2]) to zero
__device__ __forceinline__ void zero_acc(f16v (&H)[2], f16v (&P)[2], f16v (&Q)[2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) H[j][r] = P[j][r] = Q[j][r] = 0.f;
}
__device__ __forceinline__ void zero_acc(f16v (&H)[2][2], f16v (&P)[2][2], f16v (&Q)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) zero_acc(H[i], P[i], Q[i]);
}

// The k block of a 32 x 64 wave (one A fragment row, two B): 2 k16 steps of 6
// LDS fragment reads and 6 MFMAs.  bufa / bufb: the block's A / B rows in LDS
// (128-B rows of 8 chunks: 4 of h, then 4 of l); ra, rb0, rb1: this lane's
// rows, in chunks; chunk c of a row sits at c ^ sw.  c0: the block's first
// chunk in a row that holds more than one block.
__device__ __forceinline__ void w32_kblock(f16v (&H)[2], f16v (&P)[2], f16v (&Q)[2], const u4* bufa, const u4* bufb,
                                           int ra, int rb0, int rb1, int hl, int sw, int c0 = 0) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int ch = (c0 + 2 * ks + hl) ^ sw, cl = (c0 + 4 + 2 * ks + hl) ^ sw;
    const h8 ah = __builtin_bit_cast(h8, bufa[ra + ch]);
    const h8 al = __builtin_bit_cast(h8, bufa[ra + cl]);
    const h8 bh0 = __builtin_bit_cast(h8, bufb[rb0 + ch]);
    const h8 bl0 = __builtin_bit_cast(h8, bufb[rb0 + cl]);
    const h8 bh1 = __builtin_bit_cast(h8, bufb[rb1 + ch]);
    const h8 bl1 = __builtin_bit_cast(h8, bufb[rb1 + cl]);
    H[0] = mfma32_f16(ah, bh0, H[0]);
    H[1] = mfma32_f16(ah, bh1, H[1]);
    P[0] = mfma32_f16(ah, bl0, P[0]);
    P[1] = mfma32_f16(ah, bl1, P[1]);
    Q[0] = mfma32_f16(al, bh0, Q[0]);
    Q[1] = mfma32_f16(al, bh1, Q[1]);
  }
}

// The k block of a 64 x 64 wave (2 x 2 MFMA tiles): 6 groups of 4 MFMAs, the
// same k order per element as w32_kblock.  buf: the block's rows in LDS (A and
// B in one buffer), ra0 / rb0 this lane's first A / B row, in chunks; the
// second fragment of each is 32 rows (4096 B) on.  The operand fragments are
// read from LDS one MFMA group ahead, in asm with counted waits (the compiler
// drains lgkmcnt to 0 around the LDS-DMA): a group's fragments land while the
// previous group's MFMAs run, except the block's first.  Eight fragments live
// at most.  A wait names the fragments it retires ("+v"), so no MFMA can move
// above it.  piece(i) runs after MFMA group i = 0 .. 5: the caller's LDS-DMA
// of a later block, spread over the block.
template <class Piece>
__device__ __forceinline__ void w64_kblock(f16v (&H)[2][2], f16v (&P)[2][2], f16v (&Q)[2][2], const u4* buf, int ra0,
                                           int rb0, int hl, int sw, Piece&& piece) {
  const uint32_t abase = lds_addr(buf + ra0), bbase = lds_addr(buf + rb0);
  auto rd2 = [&](uint32_t base, int c, h8& x0, h8& x1) {
    const uint32_t a0 = base + 16u * (uint32_t)c;
    asm volatile("ds_read_b128 %0, %1" : "=v"(x0) : "v"(a0) : "memory");
    asm volatile("ds_read_b128 %0, %1 offset:4096" : "=v"(x1) : "v"(a0) : "memory");  // + 32 rows
  };
  const int ch0 = hl ^ sw, cl0 = (4 + hl) ^ sw, ch1 = (2 + hl) ^ sw, cl1 = (6 + hl) ^ sw;
  h8 ah0, ah1, bh0, bh1, bl0, bl1, al0, al1, bh0n, bh1n;
  rd2(abase, ch0, ah0, ah1);
  rd2(bbase, ch0, bh0, bh1);
  rd2(bbase, cl0, bl0, bl1);
  asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(ah0), "+v"(ah1), "+v"(bh0), "+v"(bh1));
  H[0][0] = mfma32_f16(ah0, bh0, H[0][0]);
  H[0][1] = mfma32_f16(ah0, bh1, H[0][1]);
  H[1][0] = mfma32_f16(ah1, bh0, H[1][0]);
  H[1][1] = mfma32_f16(ah1, bh1, H[1][1]);
  piece(0);
  rd2(abase, cl0, al0, al1);
  asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(bl0), "+v"(bl1));
  P[0][0] = mfma32_f16(ah0, bl0, P[0][0]);
  P[0][1] = mfma32_f16(ah0, bl1, P[0][1]);
  P[1][0] = mfma32_f16(ah1, bl0, P[1][0]);
  P[1][1] = mfma32_f16(ah1, bl1, P[1][1]);
  piece(1);
  rd2(abase, ch1, ah0, ah1);  // k step 1 (A hi of step 0 is dead)
  rd2(bbase, ch1, bh0n, bh1n);
  asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(al0), "+v"(al1));
  Q[0][0] = mfma32_f16(al0, bh0, Q[0][0]);
  Q[0][1] = mfma32_f16(al0, bh1, Q[0][1]);
  Q[1][0] = mfma32_f16(al1, bh0, Q[1][0]);
  Q[1][1] = mfma32_f16(al1, bh1, Q[1][1]);
  piece(2);
  rd2(bbase, cl1, bl0, bl1);
  asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(ah0), "+v"(ah1), "+v"(bh0n), "+v"(bh1n));
  H[0][0] = mfma32_f16(ah0, bh0n, H[0][0]);
  H[0][1] = mfma32_f16(ah0, bh1n, H[0][1]);
  H[1][0] = mfma32_f16(ah1, bh0n, H[1][0]);
  H[1][1] = mfma32_f16(ah1, bh1n, H[1][1]);
  piece(3);
  rd2(abase, cl1, al0, al1);
  asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(bl0), "+v"(bl1));
  P[0][0] = mfma32_f16(ah0, bl0, P[0][0]);
  P[0][1] = mfma32_f16(ah0, bl1, P[0][1]);
  P[1][0] = mfma32_f16(ah1, bl0, P[1][0]);
  P[1][1] = mfma32_f16(ah1, bl1, P[1][1]);
  piece(4);
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(al0), "+v"(al1));
  Q[0][0] = mfma32_f16(al0, bh0n, Q[0][0]);
  Q[0][1] = mfma32_f16(al0, bh1n, Q[0][1]);
  Q[1][0] = mfma32_f16(al1, bh0n, Q[1][0]);
  Q[1][1] = mfma32_f16(al1, bh1n, Q[1][1]);
  piece(5);
}

// The scalar epilogue: K = exp(-g max(|a|^2 + |b|^2 - 2 dot, 0)) with dot =
// 2^-(sa + sb) (H + (P + Q)), from the A row's and the B row's shift and |x|^2.
// (The A row's come by reference, the shifts first: the order in which the
// kernels' own epilogues read them before this function held the formula.)
__device__ __forceinline__ float w32_value(float h, float p, float q, const int32_t& ash, int bsh, const float& asq,
                                           float bsq, float gamma) {
  const float sum = h + (p + q);
  const float dot = ldexpf(sum, -(ash + bsh));
  return rbf_split_value(asq, bsq, dot, gamma);
}

// row of accumulator value r of a 32 x 32 MFMA tile, from the lane group's first (4 hl)
__device__ __forceinline__ constexpr int mfma32_row(int r) { return (r & 3) + 8 * (r >> 2); }

// The scalar epilogue of one MFMA tile's 16 values, into H.  asq / ash: the
// row data of this lane group's first row (value r belongs to row
// mfma32_row(r) after it); bsq / bsh: this lane's column
__device__ __forceinline__ void w32_values(f16v& H, const f16v& P, const f16v& Q, const float* asq, const int32_t* ash,
                                           float bsq, int bsh, float gamma) {
#pragma unroll
  for (int r = 0; r < 16; ++r)
    H[r] = w32_value(H[r], P[r], Q[r], ash[mfma32_row(r)], bsh, asq[mfma32_row(r)], bsq, gamma);
}

// The stores of a 32 x 64 wave tile of a 128 x 128 STORE tile whose first
// element is (row0, col0): value (j, r) to out[row0 + 4 hl + mfma32_row(r)]
// [col0 + 32 j + (lane & 31)], and with `mirror` (the symmetric Gram's tiles
// above the diagonal: M == N) also transposed — a lane holds 4 consecutive rows
// per group, so 16-B stores out[col][row .. row + 3].  interior: the whole
// 128 x 128 tile lies inside M x N (unpredicated stores).
__device__ __forceinline__ void w32_store_tile(const f16v (&H)[2], float* out, int64_t ldo, int64_t row0, int64_t col0,
                                               int hl, int lane, int64_t M, int64_t N, bool interior, bool mirror) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = row0 + mfma32_row(r) + 4 * hl;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t col = col0 + 32 * j + (lane & 31);
      if (interior || (row < M && col < N)) out[row * ldo + col] = H[j][r];
    }
  }
  if (!mirror) return;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t col = col0 + 32 * j + (lane & 31);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t row = row0 + 8 * q + 4 * hl;
      float* dst = out + col * ldo + row;
      f4 v;
      v.x = H[j][4 * q + 0];
      v.y = H[j][4 * q + 1];
      v.z = H[j][4 * q + 2];
      v.w = H[j][4 * q + 3];
      if (interior) {
        *(f4*)dst = v;
      } else if (col < M) {
        if (row + 3 < N) {
          *(f4*)dst = v;
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (row + c < N) dst[c] = v[c];
        }
      }
    }
  }
}

// The diagnostics builds' 8-word stamp record: five s_memtime stamps, s_memrealtime at entry / end, the tile
__device__ __forceinline__ void write_stamps(uint64_t* o, const uint64_t (&st)[5], uint64_t rt0, uint64_t rt1,
                                             int64_t tx, int64_t ty) {
#pragma unroll
  for (int i = 0; i < 5; ++i) o[i] = st[i];
  o[5] = rt0;
  o[6] = rt1;
  o[7] = ((uint64_t)tx << 32) | (uint64_t)ty;
}

}  // namespace dev
}  // namespace dpsvm
