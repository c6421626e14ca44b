// gram_rows_dot: decision values from a rectangular Gram K(test, train) — the
// prediction of a model trained on a precomputed kernel (docs/DESIGN.md §20):
//
//   out[i ldo + c] = float(sum_{j < n} double(Kt[i ld + j]) double(coef[c ldc + j]) - double(b[c])),  i < nt, c < k
//
// The row-reduction counterpart of gram_rows_wsum (gram_wsum.hip sums rows into
// columns; here every row needs its own dot products).  Kt is in HBM and read
// once for a group of kDotGroup machines, whose coefficient rows (k x n, a few
// hundred KiB) stay in L2; more machines are further passes (blockIdx.y).  One
// workgroup of 256 threads owns one row (k = 1) or kDotRows adjacent rows (a
// machine's coefficient unit is then loaded from L2 once for all of them: with
// a row a workgroup the L2 traffic is k times Kt's): thread t takes the 16-B
// units t, t + 256, .. of a row in that order (several in flight), adds each
// unit's four products in column order into one double per row and machine (a
// product of two floats is exact in double), the units' tail (n % 4 columns) by
// elements; then a fixed xor butterfly per wave and the four waves in order.
// Rows that do not allow 16-B loads (a base or a stride off 16 bytes) take the
// same units by four element loads each.  No atomics and no occupancy query:
// the summation order is a function of n alone, so results are bit-equal run
// to run, device to device and whatever the strides.  Columns >= n of a row
// (ld > n) are never read.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dpsvm/common.hpp"
#include "device_util.hpp"
#include "kernels.hpp"
#include "../runtime/hip_check.hpp"

namespace dpsvm {
namespace dev {

constexpr int kDotThreads = 256;
constexpr int kDotLoads = 4;  // 16-B loads in flight per thread and row (one row a workgroup)
constexpr int kDotRows = 4;   // rows a workgroup of the multi-machine kernel (two loads in flight a row)

// four adjacent floats: one 16-B load (VEC: the address is 16-B aligned), else by elements
template <bool VEC, bool NT>
__device__ __forceinline__ f4 dot_load4(const float* p) {
  if constexpr (VEC) {
    if constexpr (NT) return __builtin_nontemporal_load((const f4*)p);
    else return *(const f4*)p;
  } else {
    if constexpr (NT)
      return f4{__builtin_nontemporal_load(p), __builtin_nontemporal_load(p + 1), __builtin_nontemporal_load(p + 2),
                __builtin_nontemporal_load(p + 3)};
    else return f4{p[0], p[1], p[2], p[3]};
  }
}

// VEC: Kt / coef rows are 16-B aligned (base pointers, ld % 4 == 0, ldc % 4 == 0); else loads by elements.
// R rows a workgroup (rows past nt - 1 read row nt - 1 again and store nothing), U units in flight a row: neither
// changes the order in which a row's products are added.
template <bool NT, bool VEC, int KG, int R, int U>
__global__ __launch_bounds__(kDotThreads) void gram_dot_kernel(const float* __restrict__ Kt, int64_t nt, int64_t ld,
                                                               int64_t n, const float* __restrict__ coef, int64_t ldc,
                                                               int k, const float* __restrict__ b,
                                                               float* __restrict__ out, int64_t ldo) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * R;
  const int c0 = (int)blockIdx.y * KG;
  const int kg = min(KG, k - c0);  // >= 1 by the grid
  const float* row[R];
#pragma unroll
  for (int r = 0; r < R; ++r) row[r] = Kt + min((long long)(i0 + r), (long long)(nt - 1)) * ld;
  const float* cf = coef + (int64_t)c0 * ldc;
  double acc[R][KG];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int c = 0; c < KG; ++c) acc[r][c] = 0.0;
  const int64_t n4 = n >> 2;  // whole 4-column units of a row
  for (int64_t g0 = tid; g0 < n4; g0 += (int64_t)U * kDotThreads) {
    f4 kv[U][R];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t g = min((long long)(g0 + (int64_t)u * kDotThreads), (long long)(n4 - 1));
#pragma unroll
      for (int r = 0; r < R; ++r) kv[u][r] = dot_load4<VEC, NT>(row[r] + 4 * g);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t g = g0 + (int64_t)u * kDotThreads;
      if (g < n4) {
#pragma unroll
        for (int c = 0; c < KG; ++c) {
          if (c < kg) {
            const f4 cv = dot_load4<VEC, false>(cf + (int64_t)c * ldc + 4 * g);
            const double cx = (double)cv.x, cy = (double)cv.y, cz = (double)cv.z, cw = (double)cv.w;
#pragma unroll
            for (int r = 0; r < R; ++r) {
              acc[r][c] = fma((double)kv[u][r].x, cx, acc[r][c]);
              acc[r][c] = fma((double)kv[u][r].y, cy, acc[r][c]);
              acc[r][c] = fma((double)kv[u][r].z, cz, acc[r][c]);
              acc[r][c] = fma((double)kv[u][r].w, cw, acc[r][c]);
            }
          }
        }
      }
    }
  }
  // by elements: the tail of a row (< 4 columns)
  for (int64_t j = 4 * n4 + tid; j < n; j += kDotThreads) {
#pragma unroll
    for (int c = 0; c < KG; ++c) {
      if (c < kg) {
        const double cj = (double)cf[(int64_t)c * ldc + j];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r][c] = fma((double)row[r][j], cj, acc[r][c]);
      }
    }
  }
  __shared__ double red[kDotThreads / 64][R][KG];
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int c = 0; c < KG; ++c) {
      double v = acc[r][c];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
      if (lane == 0) red[wave][r][c] = v;
    }
  }
  __syncthreads();
  if (tid < R * KG) {
    const int r = tid / KG, c = tid - r * KG;
    if (c < kg && i0 + r < nt) {
      const double s = ((red[0][r][c] + red[1][r][c]) + red[2][r][c]) + red[3][r][c];
      out[(i0 + r) * ldo + c0 + c] = (float)(s - (double)b[c0 + c]);
    }
  }
}

}  // namespace dev

namespace launch {

void gram_rows_dot(const float* Kt, int64_t nt, int64_t ld, int64_t n, const float* coef, int64_t ldc, int k,
                   const float* b, float* out, int64_t ldo, hipStream_t s) {
  DPSVM_CHECK(nt >= 0 && n >= 0 && k >= 0, "gram_rows_dot: negative size");
  DPSVM_CHECK(ld >= n && ldc >= n && ldo >= k, "gram_rows_dot: ld >= n, ldc >= n, ldo >= k");
  DPSVM_CHECK(nt < ((int64_t)1 << 31), "gram_rows_dot: at most 2^31 - 1 rows a launch");
  if (nt == 0 || k == 0) return;
  DPSVM_CHECK(Kt && coef && b && out, "gram_rows_dot: null Kt / coef / b / out");
  constexpr int KG = kDotGroup;
  const bool one = k == 1;
  const int passes = one ? 1 : (k + KG - 1) / KG;
  DPSVM_CHECK(passes <= 65535, "gram_rows_dot: too many machines");
  const bool vec = (((uintptr_t)Kt | (uintptr_t)coef) % 16 == 0) && ld % 4 == 0 && ldc % 4 == 0;
  // as gram_rows_wsum: a matrix far beyond the last-level cache is read with non-temporal loads
  const bool nt_loads = nt * ld * (int64_t)sizeof(float) > (int64_t(1) << 30);
  constexpr int R = dev::kDotRows;
  const dim3 grid1((unsigned)nt, 1), gridk((unsigned)((nt + R - 1) / R), (unsigned)passes), threads(dev::kDotThreads);
#define DPSVM_DOT(NT, VEC)                                                                                        \
  do {                                                                                                            \
    if (one)                                                                                                      \
      dev::gram_dot_kernel<NT, VEC, 1, 1, dev::kDotLoads><<<grid1, threads, 0, s>>>(Kt, nt, ld, n, coef, ldc, k, b, \
                                                                                   out, ldo);                    \
    else                                                                                                          \
      dev::gram_dot_kernel<NT, VEC, KG, R, 2><<<gridk, threads, 0, s>>>(Kt, nt, ld, n, coef, ldc, k, b, out, ldo); \
  } while (0)
  if (nt_loads && vec) DPSVM_DOT(true, true);
  else if (nt_loads) DPSVM_DOT(true, false);
  else if (vec) DPSVM_DOT(false, true);
  else DPSVM_DOT(false, false);
#undef DPSVM_DOT
  post_launch("gram_rows_dot", s);
}

}  // namespace launch
}  // namespace dpsvm
