// Data and model I/O.
//
// Reference behaviour:
//   CSV loader  parse.cpp:10-43        (label first, then d features; first n lines)
//   model file  svmTrainMain.cpp:386-416  ("gamma\nb\n" then "alpha,y,x1..xd" per SV)
//   seq model   seq.cpp:295-321        (legacy: same without the b line)
#pragma once

#include <cstdint>
#include <functional>
#include <string>
#include <vector>

namespace dpsvm {

struct Dataset {
  int64_t n = 0;
  int d = 0;
  std::vector<float> x;  // n*d row-major
  std::vector<float> y;  // +1 / -1
};

// Read the first `n` rows (n <= 0: all rows) of a dense CSV "label,f1,...,fd".
// d <= 0 infers the feature count from the first row.  Rows with fewer than d
// features are zero-padded; extra columns are an error (reference: no checks).
// Labels are parsed as numbers and mapped to +1 / -1 (anything > 0 -> +1).
Dataset read_csv(const std::string& path, int64_t n, int d, int threads = 0);
// Rows [row0, row0+rows) only (shard-aware loading for partitioned X).
Dataset read_csv_rows(const std::string& path, int64_t row0, int64_t rows, int d, int threads = 0);
void write_csv(const std::string& path, const Dataset& ds);

// Sparse LIBSVM text ("+1 3:1 11:1 ...") -> dense, feature k (1-based) -> column k-1.
Dataset read_libsvm(const std::string& path, int d, int64_t n = 0);

// kernel / degree / coef0 of Model and MultiModel: "rbf" (gamma; degree and coef0 unused), or a dot-product kernel
// (dpsvm/dot_kernel.hpp) "linear" | "poly" | "sigmoid" on the same gamma.  The model files carry one leading line
// "dpsvm-kernel <name> <degree> <coef0>" for a kernel other than "rbf" and nothing for "rbf" (those files are
// unchanged); a reader fails on a name it does not know.
struct Model {
  std::string kernel = "rbf";
  int degree = 0;
  float coef0 = 0.f;
  float gamma = 0.f;
  float b = 0.f;
  int d = 0;
  bool has_b = true;           // false: legacy seq format (no b line)
  std::vector<float> alpha;    // nsv
  std::vector<float> y;        // nsv
  std::vector<float> x;        // nsv*d
  int64_t nsv() const { return (int64_t)alpha.size(); }
};

// Support vectors (alpha != 0) in global index order (svmTrainMain.cpp:397).
Model make_model(const Dataset& ds, const std::vector<float>& alpha, float b, float gamma);
// precision: significant digits (reference: ostream default 6; we default to 9 = exact f32)
void write_model(const std::string& path, const Model& m, int precision = 9, bool legacy = false);
// Auto-detects the dpsvm format vs the legacy seq format (2nd line has commas).
Model read_model(const std::string& path, bool force_legacy = false);

// One-vs-rest multi-class model: k machines (machine c: classes[c] against the
// rest) with one gamma on the union of their support vectors.
//   decision[i][c] = sum_s coef[s][c] K(x_s, x_i) - b[c]
struct MultiModel {
  std::string kernel = "rbf";  // as Model's
  int degree = 0;
  float coef0 = 0.f;
  float gamma = 0.f;
  int d = 0;
  std::vector<float> classes;  // k class labels
  std::vector<float> b;        // k
  std::vector<float> coef;     // nsv*k row-major: alpha_c * y_c of the union's rows
  std::vector<float> x;        // nsv*d
  int k() const { return (int)classes.size(); }
  int64_t nsv() const { return classes.empty() ? 0 : (int64_t)(coef.size() / classes.size()); }
};
// alphas, ys: k rows of n (machine c's dual variables and its +1 / -1 labels).
// Union SVs = the rows with any alpha_c > 0, in global index order.
MultiModel make_multi_model(const Dataset& ds, const std::vector<float>& classes, const std::vector<float>& alphas,
                            const std::vector<float>& ys, const std::vector<float>& b, float gamma);
// Text: "dpsvm-ovr <k> <nsv> <d>" \n classes \n gamma \n b_0 .. b_{k-1} \n then per SV its k
// coefficients and d features; numbers comma-separated, `precision` as write_model.
void write_multi_model(const std::string& path, const MultiModel& m, int precision = 9);
MultiModel read_multi_model(const std::string& path);
// true when the file starts with the multi-class header (after a "dpsvm-kernel" line, if any)
bool is_multi_model(const std::string& path);

// Deterministic synthetic generators (identical on every rank; row-seeded so a
// rank can generate only its own rows).
enum class Synth : int {
  MnistShape = 0,   // 784-d pixel-like features in [0,1] (~19% nonzero), random +/-1 labels
  MnistParity = 1,  // 784-d digit-like prototypes + noise, label = parity of the prototype
  AdultShape = 2,   // 123-d binary one-hot features, labels from a hidden rule (~24% +1)
  CovtypeShape = 3, // 54-d: 10 continuous in [0,1] + 44 binary; nonlinear labels
  Blobs = 4,        // two isotropic gaussians, unit variance, centres +/- sep/2 on axis 0
  Uniform = 5,      // dense uniform [0,1) features, random labels
};
Synth synth_from_name(const std::string& name);
std::string synth_name(Synth s);
int synth_default_d(Synth s);
Dataset make_synthetic(Synth kind, int64_t n, int d, uint64_t seed, int64_t row0 = 0,
                       int64_t rows = -1, float sep = 2.0f, int threads = 0);

// small helpers
void parallel_for(int64_t n, int threads, const std::function<void(int64_t, int64_t)>& fn);
int default_threads();

}  // namespace dpsvm
