// Probability estimates (Platt scaling; docs/DESIGN.md §16): the held-out decision
// values of a cross-validation fold read from the solver's gradient, the sigmoid
// fit P(y = +1 | d) = 1 / (1 + exp(A d + B)) on them (Lin, Lin and Weng's Newton
// method with backtracking, the one LIBSVM's sigmoid_train uses) and the
// probability epilogue of the decision GEMM.  No reference counterpart: the
// reference has signed distances only.
#include <hip/hip_runtime.h>

#include "dpsvm/common.hpp"
#include "kernels.hpp"
#include "../runtime/hip_check.hpp"

namespace dpsvm {
namespace dev {

// dec[slot n + i] = float(double(f_i) + y_i - b) for the rows i of one fold: a held-out row (C_i = 0) keeps
// alpha_i = 0 while every round's f update keeps f_i = sum_j alpha_j y_j K_ij - y_i current
__global__ __launch_bounds__(256) void holdout_decision_kernel(const float* f, const float* y, const int32_t* rows,
                                                               int64_t nr, double b, float* dec) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= nr) return;
  const int64_t i = rows[r];
  dec[i] = (float)((double)f[i] + (double)y[i] - b);
}

constexpr int kPlattThreads = 1024;
constexpr int kPlattWaves = kPlattThreads / 64;
constexpr int kPlattMaxIter = 100;   // Newton steps at most
constexpr double kPlattMinStep = 1e-10;
constexpr double kPlattSigma = 1e-12;  // Hessian ridge
constexpr double kPlattEps = 1e-5;     // stop: both gradient components below

// NV sums of one workgroup in a fixed order: per thread (the caller's strided loop), __shfl_down within the wave,
// the 16 wave partials through LDS added in wave order by every thread — all threads hold the same bits, no atomics
template <int NV>
__device__ __forceinline__ void platt_block_sum(double (&v)[NV], double* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < NV; ++k) lds[wave * NV + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    double s = lds[k];
    for (int w = 1; w < kPlattWaves; ++w) s += lds[w * NV + k];
    v[k] = s;
  }
  __syncthreads();  // the next sum writes the same words
}

// sum_i t_i x_i (x >= 0) or (t_i - 1) x_i (x < 0), plus log1p(exp(-|x_i|)), x_i = A d_i + B
__device__ __forceinline__ double platt_objective(const float* d, const float* y, int64_t n, double A, double B,
                                                  double hi, double lo, double* lds) {
  double v[1] = {0.0};
  for (int64_t i = threadIdx.x; i < n; i += kPlattThreads) {
    const double t = y[i] > 0.f ? hi : lo;
    const double x = (double)d[i] * A + B;
    v[0] += (x >= 0.0 ? t * x : (t - 1.0) * x) + log1p(exp(-fabs(x)));
  }
  platt_block_sum<1>(v, lds);
  return v[0];
}

// One workgroup per machine (grid.x): the whole fit in one launch.  Every loop is bounded (100 steps, 34
// halvings of the step from 1 down to 1e-10) and nothing is polled.  All arithmetic in fp64: with fp32 terms
// or sums the decrease test is never met near the optimum.  The decisions are streamed from memory each pass.
__global__ __launch_bounds__(kPlattThreads) void platt_fit_kernel(const float* dec, int64_t ldd, const float* yy,
                                                                  int64_t ldy, int64_t n, PlattFit* out) {
  __shared__ double lds[kPlattWaves * 5];
  const float* d = dec + (int64_t)blockIdx.x * ldd;
  const float* y = yy + (int64_t)blockIdx.x * ldy;
  double c[1] = {0.0};
  for (int64_t i = threadIdx.x; i < n; i += kPlattThreads) c[0] += y[i] > 0.f ? 1.0 : 0.0;
  platt_block_sum<1>(c, lds);
  const double np = c[0], nn = (double)n - np;
  const double hi = (np + 1.0) / (np + 2.0), lo = 1.0 / (nn + 2.0);
  double A = 0.0, B = log((nn + 1.0) / (np + 1.0));
  double fval = platt_objective(d, y, n, A, B, hi, lo, lds);
  int evals = 1, iters = 0, status = 2;
  for (; iters < kPlattMaxIter; ++iters) {
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // h11, h22, h21, g1, g2
    for (int64_t i = threadIdx.x; i < n; i += kPlattThreads) {
      const double t = y[i] > 0.f ? hi : lo;
      const double di = (double)d[i];
      const double x = di * A + B;
      const double e = exp(-fabs(x));
      const double u = 1.0 / (1.0 + e), w = e * u;
      const double p = x >= 0.0 ? w : u, q = x >= 0.0 ? u : w;
      const double d2 = p * q, d1 = t - p;
      s[0] += di * di * d2;
      s[1] += d2;
      s[2] += di * d2;
      s[3] += di * d1;
      s[4] += d1;
    }
    platt_block_sum<5>(s, lds);
    const double h11 = s[0] + kPlattSigma, h22 = s[1] + kPlattSigma, h21 = s[2], g1 = s[3], g2 = s[4];
    if (fabs(g1) < kPlattEps && fabs(g2) < kPlattEps) {
      status = 0;
      break;
    }
    const double det = h11 * h22 - h21 * h21;
    const double dA = -(h22 * g1 - h21 * g2) / det, dB = -(-h21 * g1 + h11 * g2) / det;
    const double gd = g1 * dA + g2 * dB;
    double step = 1.0;
    bool moved = false;
    while (step >= kPlattMinStep) {
      const double nA = A + step * dA, nB = B + step * dB;
      const double nf = platt_objective(d, y, n, nA, nB, hi, lo, lds);
      ++evals;
      if (nf < fval + 1e-4 * step * gd) {
        A = nA, B = nB, fval = nf;
        moved = true;
        break;
      }
      step *= 0.5;
    }
    if (!moved) {
      status = 1;
      break;
    }
  }
  if (threadIdx.x == 0) {
    PlattFit r;
    r.A = A, r.B = B, r.fval = fval;
    r.iters = iters, r.evals = evals, r.status = status;
    out[blockIdx.x] = r;
  }
}

// 1 / (1 + exp(x)) in the two-branch form
__device__ __forceinline__ double platt_sigmoid(double x) {
  if (x >= 0.0) {
    const double e = exp(-x);
    return e / (1.0 + e);
  }
  return 1.0 / (1.0 + exp(x));
}

// dec [n][k] decisions -> probabilities in place, a thread per row: p_c = sigmoid(A_c d_c + B_c); k > 2: divided
// by the row's sum (a sum of 0: 1 / k each).  fp64, rounded to float once.
__global__ __launch_bounds__(256) void proba_rows_kernel(float* dec, int64_t n, int k, const double* A,
                                                         const double* B) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float* row = dec + i * k;
  if (k <= 2) {
    for (int c = 0; c < k; ++c) row[c] = (float)platt_sigmoid((double)row[c] * A[c] + B[c]);
    return;
  }
  double sum = 0.0;
  for (int c = 0; c < k; ++c) sum += platt_sigmoid((double)row[c] * A[c] + B[c]);
  for (int c = 0; c < k; ++c)
    row[c] = sum > 0.0 ? (float)(platt_sigmoid((double)row[c] * A[c] + B[c]) / sum) : (float)(1.0 / k);
}

}  // namespace dev

namespace launch {

void holdout_decision(const float* f, const float* y, const int32_t* rows, int64_t nr, double b, float* dec,
                      hipStream_t s) {
  if (nr <= 0) return;
  dev::holdout_decision_kernel<<<dim3((unsigned)((nr + 255) / 256)), 256, 0, s>>>(f, y, rows, nr, b, dec);
  post_launch("holdout_decision", s);
}

void platt_fit(const float* dec, int64_t ldd, const float* y, int64_t ldy, int64_t n, int machines, PlattFit* out,
               hipStream_t s) {
  if (machines <= 0) return;
  dev::platt_fit_kernel<<<dim3((unsigned)machines), dev::kPlattThreads, 0, s>>>(dec, ldd, y, ldy, n, out);
  post_launch("platt_fit", s);
}

void proba_rows(float* dec, int64_t n, int k, const double* A, const double* B, hipStream_t s) {
  if (n <= 0 || k <= 0) return;
  dev::proba_rows_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, s>>>(dec, n, k, A, B);
  post_launch("proba_rows", s);
}

}  // namespace launch
}  // namespace dpsvm
