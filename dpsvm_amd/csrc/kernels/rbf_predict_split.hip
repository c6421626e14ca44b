// The decision GEMM on split operands (rbf_predict_split): dec_i = sum_j
// coef_j K(A_i, B_j) on the split rows, k block and epilogue of the Gram
// kernels (rbf_gemm_split.hip, split_mma.hpp), the kernel block folded into
// per-row sums instead of stored; and its multi-output sibling (rbf_predict_multi:
// k coefficient columns on one SV set, the kernel block folded into k sums a row).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dpsvm/common.hpp"
#include "device_util.hpp"
#include "kernels.hpp"
#include "split_mma.hpp"
#include "../runtime/hip_check.hpp"

namespace dpsvm {
namespace dev {

constexpr int kPredictThreads = 512;

// ---------------------------------------------------------------------------
// Decision GEMM on split operands (predict: training accuracy, GpuPredictor,
// svmTest, the shrinking phases' gradient update): dec_i = sum_j coef_j K(A_i,
// B_j) with A = query rows, B = support vectors.  A workgroup owns 128 query
// rows and a range of SV tiles; the (SV tile, k block) sequence is ONE LDS-DMA
// pipeline (the Gram's LDS-DMA STORE kernel's staging, rbf_gemm_split_glds_kernel: four 32-k buffers, three blocks
// in flight across tile boundaries — the query panel is the same for every SV
// tile), and each SV tile's 128 x 128 kernel block is folded into per-row sums
// in registers (no store).  Partial sums per SV split: partial[split][row].
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kPredictThreads, 1) void rbf_predict_split_kernel(
    const u4* __restrict__ A, const int32_t* __restrict__ Ash, const float* __restrict__ Asq, int64_t M,
    const u4* __restrict__ B, const int32_t* __restrict__ Bsh, const float* __restrict__ Bsq,
    const float* __restrict__ coef, int64_t N, int nkb, float gamma, float* __restrict__ partial, int64_t ldp,
    int per) {
  constexpr int WN = 2, TM = 128, TN = 128, ROWS = TM + TN, CPR = 8, BUF = ROWS * CPR, NB = 4;
  __shared__ u4 lds[NB * BUF + 2 * TM / 4];
  float* s_asq = (float*)(lds + NB * BUF);
  int32_t* s_ash = (int32_t*)(lds + NB * BUF) + TM;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN, hl = lane >> 5;
  const int64_t m0 = (int64_t)blockIdx.x * TM;
  const int64_t tn_all = (N + TN - 1) / TN;
  const int64_t t0 = (int64_t)blockIdx.y * per, t1 = min(t0 + per, tn_all);
  float* out = partial + (int64_t)blockIdx.y * ldp + m0;
  if (t0 >= t1) {  // uniform: an empty split contributes zeros
    if (tid < TM) out[tid] = 0.f;
    return;
  }
  const int64_t rstride = (int64_t)nkb * 8;
  if (tid < TM) {
    const int64_t ri = min(m0 + tid, M - 1);
    s_asq[tid] = Asq[ri];
    s_ash[tid] = Ash[ri];
  }
  const u4* src[4];
  bool isb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = 32 * wave + 8 * i + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    isb[i] = r >= TM;
    src[i] = r < TM ? A + (m0 + r) * rstride + c : B + (t0 * TN + (r - TM)) * rstride + c;
  }
  const int64_t nblk = (t1 - t0) * nkb;
  auto dma = [&](int64_t g) {
    const int64_t t = g / nkb, kb = g - t * nkb;
    u4* dst = lds + (g & (NB - 1)) * BUF + 32 * wave * CPR;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      lds_dma16(src[i] + (isb[i] ? t * TN * rstride : 0) + kb * 8, dst + 8 * i * CPR);
  };
  __syncthreads();
  dma(0);
  if (nblk > 1) dma(1);
  if (nblk > 2) dma(2);

  f16v H[2], P[2], Q[2];
  zero_acc(H, P, Q);
  float acc[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int sw = ((lane & 31) >> 1) & 7;
  const int ra = (wm * 32 + (lane & 31)) * CPR;
  const int rb0 = (TM + wn * 64 + (lane & 31)) * CPR, rb1 = rb0 + 32 * CPR;
  int kb = 0;
  int64_t t = t0;
  for (int64_t g = 0; g < nblk; ++g) {
    const int64_t ahead = min((int64_t)2, nblk - 1 - g);
    if (ahead == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (ahead == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ring_barrier();
    if (g + 3 < nblk) dma(g + 3);
    const u4* buf = lds + (g & (NB - 1)) * BUF;
    w32_kblock(H, P, Q, buf, buf, ra, rb0, rb1, hl, sw);
    if (++kb == nkb) {  // the SV tile is complete: fold its kernel block into the row sums
      const int64_t n0 = t * TN;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int64_t col = n0 + wn * 64 + 32 * j + (lane & 31);
        const int64_t cc = col < N ? col : N - 1;
        const float cf = col < N ? coef[cc] : 0.f;
        const float bsq = Bsq[cc];
        const int bsh = Bsh[cc];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int lr = wm * 32 + mfma32_row(r) + 4 * hl;
          // (w32_value written out: through the helper this loop's reads are issued in another
          // order and the k loop around it is scheduled with two more waits)
          const float dot = ldexpf(H[j][r] + (P[j][r] + Q[j][r]), -(s_ash[lr] + bsh));
          acc[r] += cf * rbf_split_value(s_asq[lr], bsq, dot, gamma);
          H[j][r] = P[j][r] = Q[j][r] = 0.f;
        }
      }
      kb = 0;
      ++t;
    }
  }
  // the 32 columns of a lane group, then the two column waves through LDS
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float v = acc[r];
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 16, 64);
    acc[r] = v;
  }
  __syncthreads();  // every wave is past its last operand read (no DMA in flight)
  float* red = (float*)lds;  // [WN][TM]
  if ((lane & 31) == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wn * TM + wm * 32 + mfma32_row(r) + 4 * hl] = acc[r];
  }
  __syncthreads();
  if (tid < TM) out[tid] = red[tid] + red[TM + tid];
}

// ---------------------------------------------------------------------------
// The multi-output decision GEMM (one-vs-rest prediction): out[i][c] = sum_j
// coef[j][c] K(A_i, B_j) for kPredictCols = 32 columns a pass (blockIdx.z).
// rbf_predict_split_kernel's pipeline (the same staging, ring and w32_kblock
// sequence) with the first GEMM's operand roles swapped: a wave multiplies 32
// SVs (its A fragment) by 64 queries (two B fragments), so a lane owns a query
// and accumulator value r of half-wave hl belongs to SV mfma32_row(r) + 4 hl.
// The split GEMM holds the same bits under the swap (H and P + Q commute), and
// rbf_split_value gets the single-output kernel's arguments, so every kernel
// value is the one that kernel forms.  The kernel block is then folded by
// v_mfma_f32_32x32x2_f32 with no data movement: value r is that instruction's A
// operand as it stands (queries x 2 SVs, one per half-wave), its B operand
// coef[that SV][lane & 31]; 16 f32 MFMAs fold a 32 x 32 block into 32 columns
// (exact f32 products and sums, D[j] = queries x columns, 32 registers for 64
// queries).  The four SV waves' sums meet in LDS at the end.
// coefp: [passes][Npad][32], zero beyond N and beyond column k (Npad = 128 x
// the SV tiles: no bound test on the load); partial: [pass][split][32][ldp],
// rows contiguous for the store here and for the reduce, columns >= k untouched.
// ---------------------------------------------------------------------------
constexpr int kPredictCols = 32;

__global__ __launch_bounds__(kPredictThreads, 1) void rbf_predict_multi_kernel(
    const u4* __restrict__ A, const int32_t* __restrict__ Ash, const float* __restrict__ Asq, int64_t M,
    const u4* __restrict__ B, const int32_t* __restrict__ Bsh, const float* __restrict__ Bsq,
    const float* __restrict__ coefp, int64_t N, int64_t Npad, int k, int nkb, float gamma,
    float* __restrict__ partial, int64_t ldp, int per) {
  constexpr int WN = 2, TM = 128, TN = 128, ROWS = TM + TN, CPR = 8, BUF = ROWS * CPR, NB = 4, KC = kPredictCols;
  constexpr int LDR = TM + 1;  // the end reduce's row of one (SV wave, column): conflict-free by column and by row
  static_assert(4 * KC * LDR * 4 <= NB * BUF * 16, "the end reduce fits the operand ring");
  __shared__ u4 lds[NB * BUF];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN, hl = lane >> 5;
  const int64_t m0 = (int64_t)blockIdx.x * TM;
  const int64_t tn_all = (N + TN - 1) / TN;
  const int64_t t0 = (int64_t)blockIdx.y * per, t1 = min(t0 + per, tn_all);
  const int kc = min(KC, k - (int)blockIdx.z * KC);  // this pass's columns
  float* out = partial + (((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * KC) * ldp + m0;
  if (t0 >= t1) {  // uniform: an empty split contributes zeros
    for (int e = tid; e < kc * TM; e += kPredictThreads) out[(int64_t)(e / TM) * ldp + e % TM] = 0.f;
    return;
  }
  const float* cp = coefp + (int64_t)blockIdx.z * Npad * KC + (lane & 31);
  const int64_t rstride = (int64_t)nkb * 8;
  // this lane's two queries (B fragments j = 0, 1)
  float qsq[2];
  int32_t qsh[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t qi = min(m0 + wn * 64 + 32 * j + (lane & 31), M - 1);
    qsq[j] = Asq[qi];
    qsh[j] = Ash[qi];
  }
  const u4* src[4];
  bool isb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = 32 * wave + 8 * i + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    isb[i] = r >= TM;
    src[i] = r < TM ? A + (m0 + r) * rstride + c : B + (t0 * TN + (r - TM)) * rstride + c;
  }
  const int64_t nblk = (t1 - t0) * nkb;
  auto dma = [&](int64_t g) {
    const int64_t t = g / nkb, kb = g - t * nkb;
    u4* dst = lds + (g & (NB - 1)) * BUF + 32 * wave * CPR;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      lds_dma16(src[i] + (isb[i] ? t * TN * rstride : 0) + kb * 8, dst + 8 * i * CPR);
  };
  dma(0);
  if (nblk > 1) dma(1);
  if (nblk > 2) dma(2);

  f16v H[2], P[2], Q[2], D[2];
  zero_acc(H, P, Q);
#pragma unroll
  for (int r = 0; r < 16; ++r) D[0][r] = D[1][r] = 0.f;
  const int sw = ((lane & 31) >> 1) & 7;
  // rows in the ring's buffers: queries 0 .. 127, SVs 128 .. 255; the SVs are this GEMM's A rows
  const int ra = (TM + wm * 32 + (lane & 31)) * CPR;
  const int rb0 = (wn * 64 + (lane & 31)) * CPR, rb1 = rb0 + 32 * CPR;
  int kb = 0;
  int64_t t = t0;
  for (int64_t g = 0; g < nblk; ++g) {
    const int64_t ahead = min((int64_t)2, nblk - 1 - g);
    if (ahead == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (ahead == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ring_barrier();
    if (g + 3 < nblk) dma(g + 3);
    const u4* buf = lds + (g & (NB - 1)) * BUF;
    w32_kblock(H, P, Q, buf, buf, ra, rb0, rb1, hl, sw);
    if (++kb == nkb) {  // the SV tile is complete: fold this wave's 32 SVs x 64 queries into the queries' columns
      const int64_t n0 = t * TN + wm * 32;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t sv = n0 + mfma32_row(r) + 4 * hl;  // < Npad
        const int64_t sc = sv < N ? sv : N - 1;
        const float cf = cp[sv * KC];
        const float bsq = Bsq[sc];
        const int bsh = Bsh[sc];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float dot = ldexpf(H[j][r] + (P[j][r] + Q[j][r]), -(qsh[j] + bsh));
          D[j] = mfma32(rbf_split_value(qsq[j], bsq, dot, gamma), cf, D[j]);
          H[j][r] = P[j][r] = Q[j][r] = 0.f;
        }
      }
      kb = 0;
      ++t;
    }
  }
  __syncthreads();  // every wave is past its last operand read (no DMA in flight)
  float* red = (float*)lds;  // [4 SV waves][KC][LDR]
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      red[(wm * KC + (lane & 31)) * LDR + wn * 64 + 32 * j + mfma32_row(r) + 4 * hl] = D[j][r];
  __syncthreads();
  for (int e = tid; e < kc * TM; e += kPredictThreads) {
    const int c = e / TM, row = e % TM;
    const float* p = red + c * LDR + row;
    out[(int64_t)c * ldp + row] = ((p[0] + p[KC * LDR]) + p[2 * KC * LDR]) + p[3 * KC * LDR];
  }
}

// coefp[pass][j][c] = coef[j][pass * kPredictCols + c] (0 beyond N rows / k columns)
__global__ void predict_pack_coef_kernel(const float* __restrict__ coef, int64_t N, int ldc, int k, int64_t Npad,
                                         int passes, float* __restrict__ coefp) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)passes * Npad * kPredictCols) return;
  const int c = (int)(e % kPredictCols);
  const int64_t j = e / kPredictCols % Npad;
  const int col = (int)(e / (kPredictCols * Npad)) * kPredictCols + c;
  coefp[e] = (j < N && col < k) ? coef[j * ldc + col] : 0.f;
}

// predict_reduce_kernel's k-column twin: dec[i][c] = sum over splits of partial[pass][split][column][i] - b[c]
// (thread = (row, column), rows fastest: contiguous reads; the splits in index order like the single-output reduce)
__global__ void predict_reduce_multi_kernel(const float* __restrict__ partial, int64_t M, int64_t ldp, int splits,
                                            const float* __restrict__ b, float* __restrict__ dec, int64_t ldd) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int c = blockIdx.y;
  if (i >= M) return;
  const int pass = c / kPredictCols, cc = c % kPredictCols;
  const float* p = partial + (((int64_t)pass * splits) * kPredictCols + cc) * ldp + i;
  float s = 0.f;
  for (int q = 0; q < splits; ++q) s += p[(int64_t)q * kPredictCols * ldp];
  dec[i * ldd + c] = s - b[c];
}

// column c of a row-major [rows][ld] matrix into a contiguous vector, or back (the dp < 128 loop of
// single-output launches)
__global__ void predict_column_kernel(const float* __restrict__ src, int64_t rows, int64_t ld_src,
                                      float* __restrict__ dst, int64_t ld_dst, const float* __restrict__ sub) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows) dst[i * ld_dst] = sub ? src[i * ld_src] - sub[0] : src[i * ld_src];
}

}  // namespace dev

namespace launch {

namespace {
// both operands of a decision GEMM split into stream-ordered scratch (rows padded: the kernels read whole
// 128-row tiles)
struct PredictOperands {
  void *a_pl = nullptr, *b_pl = nullptr;
  int32_t *a_sh = nullptr, *b_sh = nullptr;
  PredictOperands(const float* A, int64_t M, int lda, const float* B, int64_t N, int ldb, int dp, hipStream_t s) {
    const int64_t pa = split_pad_rows(M), pb = split_pad_rows(N), ru = split_row_u4(dp) * 16;
    HIP_CHECK(hipMallocAsync(&a_pl, (size_t)(pa * ru), s));
    HIP_CHECK(hipMallocAsync(&b_pl, (size_t)(pb * ru), s));
    HIP_CHECK(hipMallocAsync((void**)&a_sh, (size_t)pa * 4, s));
    HIP_CHECK(hipMallocAsync((void**)&b_sh, (size_t)pb * 4, s));
    HIP_CHECK(hipMemsetAsync(a_pl, 0, (size_t)(pa * ru), s));
    HIP_CHECK(hipMemsetAsync(b_pl, 0, (size_t)(pb * ru), s));
    HIP_CHECK(hipMemsetAsync(a_sh, 0, (size_t)pa * 4, s));
    HIP_CHECK(hipMemsetAsync(b_sh, 0, (size_t)pb * 4, s));
    split_rows_f16(A, M, dp, lda, a_pl, a_sh, s);
    split_rows_f16(B, N, dp, ldb, b_pl, b_sh, s);
  }
  void release(hipStream_t s) {
    HIP_CHECK(hipFreeAsync(a_pl, s));
    HIP_CHECK(hipFreeAsync(b_pl, s));
    HIP_CHECK(hipFreeAsync(a_sh, s));
    HIP_CHECK(hipFreeAsync(b_sh, s));
  }
};

// SV splits of a decision GEMM of tm x tn tiles: ~2 workgroups per CU of a 256-CU device
int64_t split_count(int64_t tm, int64_t tn, int64_t max_splits) {
  return std::max<int64_t>(1, std::min<int64_t>({max_splits, tn, (512 + tm - 1) / tm}));
}

int64_t round_up128(int64_t v) { return (v + 127) / 128 * 128; }
}  // namespace

void rbf_predict_split(const float* A, const float* Asq, int64_t M, int lda, const float* B, const float* Bsq,
                       const float* coef, int64_t N, int ldb, int dp, float gamma, float* partial, int64_t ldp,
                       int max_splits, hipStream_t s) {
  const int nkb = (dp + 31) / 32;
  PredictOperands op(A, M, lda, B, N, ldb, dp, s);
  const int64_t tm = (M + 127) / 128, tn = (N + 127) / 128;
  // at most the scratch's splits
  int64_t splits = split_count(tm, tn, max_splits);
  const int per = (int)((tn + splits - 1) / splits);
  splits = (tn + per - 1) / per;
  dev::rbf_predict_split_kernel<<<dim3((unsigned)tm, (unsigned)splits), dev::kPredictThreads, 0, s>>>(
      (const dev::u4*)op.a_pl, op.a_sh, Asq, M, (const dev::u4*)op.b_pl, op.b_sh, Bsq, coef, N, nkb, gamma, partial,
      ldp, per);
  post_launch("rbf_predict_split", s);
  // zero the splits the reduce reads beyond the launched ones
  if (splits < max_splits)
    HIP_CHECK(hipMemsetAsync(partial + splits * ldp, 0, (size_t)(max_splits - splits) * ldp * 4, s));
  op.release(s);
}

// scratch of rbf_predict_multi: [packed coefficients | partial sums] of the multi-output kernel, or the
// single-output launches' [scratch | one coefficient column | one output column] — the larger of the two
int64_t predict_multi_scratch_floats(int64_t M, int64_t N, int k) {
  M = std::max<int64_t>(M, 1), N = std::max<int64_t>(N, 1), k = std::max(k, 1);
  const int64_t ldp = round_up128(M), npad = round_up128(N);
  const int64_t passes = (k + dev::kPredictCols - 1) / dev::kPredictCols;
  const int64_t splits = split_count(ldp / 128, npad / 128, INT32_MAX);
  const int64_t multi = passes * dev::kPredictCols * (npad + splits * ldp);
  const int64_t loop = predict_scratch_floats(M, N) + (npad + 128) + ldp;
  return std::max(multi, loop);
}

void rbf_predict_multi(const float* A, const float* Asq, int64_t M, int lda, const float* B, const float* Bsq,
                       const float* coef, int ldc, int k, int64_t N, int ldb, int dp, float gamma, const float* b,
                       float* scratch, float* dec, int64_t ldd, hipStream_t s, int precision) {
  if (M <= 0 || k <= 0) return;
  DPSVM_CHECK(dp % 16 == 0, "rbf_predict_multi: dp must be a multiple of 16");
  DPSVM_CHECK(ldc >= k && ldd >= k, "rbf_predict_multi: coef / dec rows hold k columns");
  const int64_t ldp = round_up128(M), npad = round_up128(std::max<int64_t>(N, 1));
  const bool split = precision == 2 || (precision == 0 && predict_uses_split(dp));
  if (!split || k == 1) {
    // no f32 twin, and one column is the single-output kernel's own job: k launches of rbf_predict, column c's
    // coefficients gathered into a vector (zero on the padding rows), its values scattered into dec's column
    float* part = scratch;
    float* ccol = part + predict_scratch_floats(M, std::max<int64_t>(N, 1));
    float* dcol = ccol + npad + 128;
    HIP_CHECK(hipMemsetAsync(ccol, 0, (size_t)(npad + 128) * 4, s));
    for (int c = 0; c < k; ++c) {
      if (N > 0)
        dev::predict_column_kernel<<<dim3((unsigned)((N + 255) / 256)), 256, 0, s>>>(coef + c, N, ldc, ccol, 1,
                                                                                   nullptr);
      rbf_predict(A, Asq, M, lda, B, Bsq, ccol, N, ldb, dp, gamma, 0.f, part, dcol, nullptr, nullptr, s, precision);
      dev::predict_column_kernel<<<dim3((unsigned)((M + 255) / 256)), 256, 0, s>>>(dcol, M, 1, dec + c, ldd, b + c);
      post_launch("predict_column", s);
    }
    return;
  }
  const int passes = (k + dev::kPredictCols - 1) / dev::kPredictCols;
  DPSVM_CHECK(passes < 65536, "rbf_predict_multi: too many columns for grid.z");
  float* coefp = scratch;
  float* partial = coefp + (int64_t)passes * dev::kPredictCols * npad;
  int64_t splits = 0;
  if (N > 0) {
    const int nkb = (dp + 31) / 32;
    const int64_t tm = ldp / 128, tn = npad / 128;
    splits = split_count(tm, tn, INT32_MAX);
    const int per = (int)((tn + splits - 1) / splits);
    splits = (tn + per - 1) / per;
    DPSVM_CHECK(splits < 65536, "rbf_predict_multi: too many SV splits for grid.y");
    const int64_t ne = (int64_t)passes * dev::kPredictCols * npad;
    dev::predict_pack_coef_kernel<<<dim3((unsigned)((ne + 255) / 256)), 256, 0, s>>>(coef, N, ldc, k, npad, passes,
                                                                                    coefp);
    post_launch("predict_pack_coef", s);
    PredictOperands op(A, M, lda, B, N, ldb, dp, s);
    dev::rbf_predict_multi_kernel<<<dim3((unsigned)tm, (unsigned)splits, (unsigned)passes), dev::kPredictThreads, 0,
                                    s>>>((const dev::u4*)op.a_pl, op.a_sh, Asq, M, (const dev::u4*)op.b_pl, op.b_sh,
                                         Bsq, coefp, N, npad, k, nkb, gamma, partial, ldp, per);
    post_launch("rbf_predict_multi", s);
    op.release(s);
  }
  // no SVs: zero splits, every value -b[c]
  dev::predict_reduce_multi_kernel<<<dim3((unsigned)((M + 255) / 256), (unsigned)k), 256, 0, s>>>(
      partial, M, ldp, (int)splits, b, dec, ldd);
  post_launch("predict_reduce_multi", s);
}

}  // namespace launch
}  // namespace dpsvm
