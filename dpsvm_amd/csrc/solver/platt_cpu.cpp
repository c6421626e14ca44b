// Platt scaling on the host in plain double: the twins of kernels/platt.hip for
// device="cpu" (the same targets, start, Newton step, ridge, backtracking and stop
// rules; sums in index order).  Lin, Lin and Weng's method, as LIBSVM's sigmoid_train.
#include <cmath>

#include "dpsvm/solver.hpp"

namespace dpsvm {

namespace {

double platt_objective(const float* dec, const float* y, int64_t n, double A, double B, double hi, double lo) {
  double f = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    const double t = y[i] > 0.f ? hi : lo;
    const double x = (double)dec[i] * A + B;
    f += (x >= 0.0 ? t * x : (t - 1.0) * x) + std::log1p(std::exp(-std::fabs(x)));
  }
  return f;
}

double platt_sigmoid(double x) {
  if (x >= 0.0) {
    const double e = std::exp(-x);
    return e / (1.0 + e);
  }
  return 1.0 / (1.0 + std::exp(x));
}

}  // namespace

PlattFit platt_fit_cpu(const float* dec, const float* y, int64_t n) {
  DPSVM_CHECK(n >= 1 && dec && y, "platt_fit_cpu: n >= 1 decisions and labels");
  double np = 0.0;
  for (int64_t i = 0; i < n; ++i) np += y[i] > 0.f ? 1.0 : 0.0;
  const double nn = (double)n - np;
  const double hi = (np + 1.0) / (np + 2.0), lo = 1.0 / (nn + 2.0);
  PlattFit r;
  r.A = 0.0;
  r.B = std::log((nn + 1.0) / (np + 1.0));
  r.fval = platt_objective(dec, y, n, r.A, r.B, hi, lo);
  r.evals = 1;
  r.status = 2;
  for (r.iters = 0; r.iters < 100; ++r.iters) {
    double h11 = 1e-12, h22 = 1e-12, h21 = 0.0, g1 = 0.0, g2 = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      const double t = y[i] > 0.f ? hi : lo;
      const double di = (double)dec[i];
      const double x = di * r.A + r.B;
      const double e = std::exp(-std::fabs(x));
      const double u = 1.0 / (1.0 + e), w = e * u;
      const double p = x >= 0.0 ? w : u, q = x >= 0.0 ? u : w;
      const double d2 = p * q, d1 = t - p;
      h11 += di * di * d2;
      h22 += d2;
      h21 += di * d2;
      g1 += di * d1;
      g2 += d1;
    }
    if (std::fabs(g1) < 1e-5 && std::fabs(g2) < 1e-5) {
      r.status = 0;
      break;
    }
    const double det = h11 * h22 - h21 * h21;
    const double dA = -(h22 * g1 - h21 * g2) / det, dB = -(-h21 * g1 + h11 * g2) / det;
    const double gd = g1 * dA + g2 * dB;
    double step = 1.0;
    bool moved = false;
    while (step >= 1e-10) {
      const double nA = r.A + step * dA, nB = r.B + step * dB;
      const double nf = platt_objective(dec, y, n, nA, nB, hi, lo);
      ++r.evals;
      if (nf < r.fval + 1e-4 * step * gd) {
        r.A = nA, r.B = nB, r.fval = nf;
        moved = true;
        break;
      }
      step *= 0.5;
    }
    if (!moved) {
      r.status = 1;
      break;
    }
  }
  return r;
}

std::vector<float> proba_cpu(const float* dec, int64_t n, int k, const double* A, const double* B) {
  DPSVM_CHECK(n >= 0 && k >= 1, "proba_cpu: dec [n][k], k >= 1");
  std::vector<float> out((size_t)n * k);
  std::vector<double> p((size_t)k);
  for (int64_t i = 0; i < n; ++i) {
    double sum = 0.0;
    for (int c = 0; c < k; ++c) sum += p[c] = platt_sigmoid((double)dec[i * k + c] * A[c] + B[c]);
    for (int c = 0; c < k; ++c)
      out[i * k + c] = k <= 2 ? (float)p[c] : sum > 0.0 ? (float)(p[c] / sum) : (float)(1.0 / k);
  }
  return out;
}

}  // namespace dpsvm
