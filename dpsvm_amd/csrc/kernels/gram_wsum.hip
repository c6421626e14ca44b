// gram_rows_wsum: a weighted sum of resident Gram rows, accumulated in fp64 and
// rounded to fp32 once (docs/DESIGN.md §18):
//
//   out[j] = float(sum_{r < m} double(coef[r]) double(G[line(r) ldg + j]) + (base ? double(base[j]) : 0)),  j < n
//
// line(r) = lines[r], or r when lines == nullptr (a contiguous prefix of the
// Gram: the one-class start f = K alpha of alpha = [1 .. 1, frac, 0 .. 0]).
// The values are in HBM already, so the kernel is a stream read of m rows:
// 16-B loads, several rows in flight per thread, no LDS.  Two launches and no
// atomics, so the result is a function of the inputs alone:
//
//   stage 1  grid = ceil(n / 1024) column groups x S row slices.  A workgroup
//            of 256 threads owns 1024 columns (4 adjacent ones per thread, as
//            ws_pass1_v4_kernel) and a contiguous slice of the list, which it
//            adds in list order into four doubles per thread: part[s][j].
//   stage 2  sums the S partials in the order s = 0, 1, .., adds base, rounds
//            once and stores (16-B stores; the tail of a row by elements, so
//            columns >= n of a padded out stay as they are).
//
// S = gram_wsum_slices(n, m) depends on the shape only (no occupancy query):
// bit-equal results run to run and device to device.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dpsvm/common.hpp"
#include "dpsvm/device_state.hpp"
#include "device_util.hpp"
#include "kernels.hpp"
#include "../runtime/hip_check.hpp"

namespace dpsvm {
namespace dev {

typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int kWsumThreads = kWsPass1Cols / 4;  // 4 adjacent columns a thread
constexpr int kWsumRows = 12;  // rows x 16 B in flight per thread (ws_pass1_v4_kernel's depth, 8 / 16 rejected there)

// part: [S][n4] doubles, n4 = round_up(n, 4).  The columns [n, n4) of a row are
// read (ldg >= n4: ldg % 4 == 0) and summed like the others; stage 2 drops them.
template <bool NT, bool IDENT>
__global__ __launch_bounds__(kWsumThreads) void gram_wsum_stage1_kernel(const float* __restrict__ gram, int64_t ldg,
                                                                        int64_t n, int64_t n4,
                                                                        const int32_t* __restrict__ lines,
                                                                        const float* __restrict__ coef, int64_t m,
                                                                        int S, double* __restrict__ part) {
  const int grp = (int)(blockIdx.x), s = (int)blockIdx.y;
  const int64_t j0 = (int64_t)grp * kWsPass1Cols + 4 * (int64_t)threadIdx.x;
  if (j0 >= n) return;  // no barrier below
  const int64_t per = (m + S - 1) / S;
  const int64_t k_lo = min((long long)m, (long long)s * per), k_hi = min((long long)m, (long long)(k_lo + per));
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int64_t k0 = k_lo; k0 < k_hi; k0 += kWsumRows) {
    f4 kv[kWsumRows];
#pragma unroll
    for (int u = 0; u < kWsumRows; ++u) {
      const int64_t kk = min((long long)(k0 + u), (long long)(k_hi - 1));
      const int64_t line = IDENT ? kk : (int64_t)lines[kk];  // uniform: a scalar load
      const f4* src = (const f4*)(gram + line * ldg + j0);
      if constexpr (NT) kv[u] = __builtin_nontemporal_load(src);
      else kv[u] = *src;
    }
#pragma unroll
    for (int u = 0; u < kWsumRows; ++u) {
      if (k0 + u < k_hi) {
        // a product of two floats is exact in double: one rounding per term, in the add
        const double cc = (double)coef[k0 + u];
        a0 = fma(cc, (double)kv[u].x, a0);
        a1 = fma(cc, (double)kv[u].y, a1);
        a2 = fma(cc, (double)kv[u].z, a2);
        a3 = fma(cc, (double)kv[u].w, a3);
      }
    }
  }
  d2* dst = (d2*)(part + (int64_t)s * n4 + j0);
  dst[0] = d2{a0, a1};
  dst[1] = d2{a2, a3};
}

__global__ __launch_bounds__(256) void gram_wsum_stage2_kernel(const double* __restrict__ part, int S, int64_t n,
                                                               int64_t n4, const float* __restrict__ base,
                                                               float* __restrict__ out) {
  const int64_t j0 = 4 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
  if (j0 >= n) return;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int s = 0; s < S; ++s) {
    const d2* src = (const d2*)(part + (int64_t)s * n4 + j0);
    const d2 lo = src[0], hi = src[1];
    a0 += lo.x;
    a1 += lo.y;
    a2 += hi.x;
    a3 += hi.y;
  }
  if (j0 + 4 <= n) {
    if (base) {
      const f4 b = *(const f4*)(base + j0);
      a0 += (double)b.x;
      a1 += (double)b.y;
      a2 += (double)b.z;
      a3 += (double)b.w;
    }
    *(f4*)(out + j0) = f4{(float)a0, (float)a1, (float)a2, (float)a3};
  } else {
    const double a[4] = {a0, a1, a2, a3};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (j0 + e < n) out[j0 + e] = (float)(a[e] + (base ? (double)base[j0 + e] : 0.0));
  }
}

}  // namespace dev

namespace launch {

int gram_wsum_slices(int64_t n, int64_t m) {
  if (n <= 0 || m <= 0) return 0;
  // about 4 workgroups a CU (256 CUs) when the list allows it, at least 2 loads' depth of rows a slice
  const int64_t groups = (n + kWsPass1Cols - 1) / kWsPass1Cols;
  const int64_t want = (1024 + groups - 1) / groups;
  const int64_t by_rows = std::max<int64_t>(1, m / (2 * dev::kWsumRows));
  return (int)std::min<int64_t>({want, by_rows, 64});
}

int64_t gram_wsum_scratch_doubles(int64_t n) {
  // the largest S of any m at this n
  const int64_t n4 = (n + 3) / 4 * 4;
  return n4 * std::max(1, gram_wsum_slices(n, n > 0 ? (int64_t)1 << 40 : 0));
}

void gram_rows_wsum(const float* gram, int64_t L, int64_t ldg, int64_t n, const int32_t* lines, const float* coef,
                    int64_t m, const float* base, float* out, double* part, hipStream_t s) {
  DPSVM_CHECK(n >= 0 && m >= 0 && L >= 0, "gram_rows_wsum: negative size");
  DPSVM_CHECK(ldg % 4 == 0 && ldg >= n, "gram_rows_wsum: ldg must be a multiple of 4 and >= n (16-B row loads)");
  DPSVM_CHECK(lines != nullptr || m <= L, "gram_rows_wsum: identity lines need m <= the Gram's lines");
  DPSVM_CHECK(((uintptr_t)gram | (uintptr_t)out | (uintptr_t)base | (uintptr_t)part) % 16 == 0,
              "gram_rows_wsum: gram / base / out / part must be 16-B aligned");
  if (n == 0) return;
  const int64_t n4 = (n + 3) / 4 * 4;
  const int S = gram_wsum_slices(n, m);
  if (S > 0) {
    DPSVM_CHECK(gram && coef && part, "gram_rows_wsum: null gram / coef / part");
    const dim3 grid((unsigned)((n + kWsPass1Cols - 1) / kWsPass1Cols), (unsigned)S);
    // as ws_pass1_nt: a Gram far beyond the last-level cache is read with non-temporal loads
    const bool nt = L * ldg * (int64_t)sizeof(float) > (int64_t(1) << 30);
    const bool ident = lines == nullptr;
    const dim3 threads(dev::kWsumThreads);
    if (nt && ident)
      dev::gram_wsum_stage1_kernel<true, true><<<grid, threads, 0, s>>>(gram, ldg, n, n4, lines, coef, m, S, part);
    else if (nt)
      dev::gram_wsum_stage1_kernel<true, false><<<grid, threads, 0, s>>>(gram, ldg, n, n4, lines, coef, m, S, part);
    else if (ident)
      dev::gram_wsum_stage1_kernel<false, true><<<grid, threads, 0, s>>>(gram, ldg, n, n4, lines, coef, m, S, part);
    else
      dev::gram_wsum_stage1_kernel<false, false><<<grid, threads, 0, s>>>(gram, ldg, n, n4, lines, coef, m, S, part);
    post_launch("gram_wsum_stage1", s);
  }
  dev::gram_wsum_stage2_kernel<<<dim3((unsigned)((n4 / 4 + 255) / 256)), 256, 0, s>>>(part, S, n, n4, base, out);
  post_launch("gram_wsum_stage2", s);
}

}  // namespace launch
}  // namespace dpsvm
