// SV compaction, distributed training accuracy, decision values and the stand-
// alone GpuPredictor (svmTest GPU path).  The kernel-level test entry points are
// in kernel_entry.hip / ws_kernel_entry.hip.
// Reference: test_setup / aggregate_sv / get_train_accuracy (svmTrain.cu:569-665:
// rank 0 alone, n x (Sgemv + transform_reduce)) and seq_test.cpp:187-210.
#include <hip/hip_runtime.h>

#include "gpu_impl.hpp"

namespace dpsvm {

using gpu::dmalloc;
using gpu::round_up;

namespace {

// rows of an SV buffer: whole 128-row tiles plus one of slack (the decision GEMMs read whole tiles)
int64_t sv_pad_rows(int64_t nsv) { return round_up(std::max<int64_t>(nsv, 1), 128) + 128; }

// A support-vector set on the device: rows [pad][dp], |x|^2 [pad], coefficients alpha*y [pad][k] (k = 1 for a
// binary model) and, for a multi-class predictor, the k thresholds.  Rows past the ones filled are zero:
// coef = 0 makes them inert.
struct DeviceSvs {
  int64_t nsv = 0;
  float *sv = nullptr, *svsq = nullptr, *coef = nullptr, *bk = nullptr;
  DeviceSvs() = default;
  DeviceSvs(const DeviceSvs&) = delete;
  ~DeviceSvs() {
    for (void* p : {(void*)sv, (void*)svsq, (void*)coef, (void*)bk}) if (p) (void)hipFree(p);
  }
  void alloc_zero(int64_t rows, int dp, int k, hipStream_t s) {
    nsv = rows;
    const int64_t pad = sv_pad_rows(rows);
    size_t tb = 0;
    sv = dmalloc<float>((size_t)pad * dp, &tb);
    svsq = dmalloc<float>((size_t)pad, &tb);
    coef = dmalloc<float>((size_t)pad * k, &tb);
    HIP_CHECK(hipMemsetAsync(sv, 0, (size_t)pad * dp * 4, s));
    HIP_CHECK(hipMemsetAsync(svsq, 0, pad * 4, s));
    HIP_CHECK(hipMemsetAsync(coef, 0, (size_t)pad * k * 4, s));
  }
};

// Decision values of a host matrix [nt][d] in chunks of 2^20 rows: upload (rows zero-padded to dp, whole tiles
// zeroed), |x|^2, launch(dx, dsq, rows, scratch, ddec) writes the chunk's [rows][cols] values, download.
// scratch_floats(rows) is what one launch of `rows` rows needs: its split count depends on the row count, so the
// scratch is sized for the larger of the full chunk's and the tail's.  post(ddec, rows) runs on the chunk's values
// before their download (the probability epilogue).
template <class ScratchFn, class LaunchFn, class PostFn>
std::vector<float> predict_host_chunks(const float* xh, int64_t nt, int d, int dp, int cols, hipStream_t stream,
                                       ScratchFn scratch_floats, LaunchFn launch, PostFn post) {
  std::vector<float> out((size_t)nt * cols);
  if (nt == 0) return out;
  const int64_t chunk = 1 << 20;
  const int64_t crows = std::min(nt, chunk), tail = nt % chunk, cpad = round_up(crows, 128) + 128;
  size_t tb = 0;
  float* dx = dmalloc<float>((size_t)cpad * dp, &tb);
  float* dsq = dmalloc<float>((size_t)cpad, &tb);
  float* ddec = dmalloc<float>((size_t)cpad * cols, &tb);
  const int64_t sfloats = std::max<int64_t>(scratch_floats(crows), tail ? scratch_floats(tail) : 0);
  float* scratch = dmalloc<float>((size_t)sfloats, &tb);
  for (int64_t r0 = 0; r0 < nt; r0 += chunk) {
    const int64_t rows = std::min(chunk, nt - r0);
    HIP_CHECK(hipMemsetAsync(dx, 0, (size_t)cpad * dp * 4, stream));
    HIP_CHECK(hipMemsetAsync(dsq, 0, cpad * 4, stream));
    HIP_CHECK(hipMemcpy2DAsync(dx, (size_t)dp * 4, xh + (size_t)r0 * d, (size_t)d * 4, (size_t)d * 4, (size_t)rows,
                               hipMemcpyHostToDevice, stream));
    launch::row_sqnorm(dx, rows, dp, dp, dsq, stream);
    launch(dx, dsq, rows, scratch, ddec);
    post(ddec, rows);
    HIP_CHECK(hipMemcpyAsync(out.data() + (size_t)r0 * cols, ddec, (size_t)rows * cols * 4, hipMemcpyDeviceToHost,
                             stream));
  }
  HIP_CHECK(hipStreamSynchronize(stream));
  for (void* p : {(void*)dx, (void*)dsq, (void*)ddec, (void*)scratch}) (void)hipFree(p);
  return out;
}
template <class ScratchFn, class LaunchFn>
std::vector<float> predict_host_chunks(const float* xh, int64_t nt, int d, int dp, int cols, hipStream_t stream,
                                       ScratchFn scratch_floats, LaunchFn launch) {
  return predict_host_chunks(xh, nt, d, dp, cols, stream, scratch_floats, launch, [](float*, int64_t) {});
}

}  // namespace

// The SVs (rows, |x|^2, alpha*y) of a host alpha; every rank ends with all of them (padded per-rank blocks in
// partitioned mode).
static void build_svs(GpuSolver::Impl& m, const std::vector<float>& alpha, DeviceSvs& s) {
  HIP_CHECK(hipMemcpyAsync(m.alpha, alpha.data(), m.n * 4, hipMemcpyHostToDevice, m.stream));
  size_t tb = 0;
  if (m.replicated) {
    int32_t* idx = dmalloc<int32_t>((size_t)m.n, &tb);
    int32_t* cnt = dmalloc<int32_t>(1, &tb);
    int32_t* scratch = dmalloc<int32_t>((size_t)launch::compact_scratch_ints(m.n), &tb);
    launch::compact_positive(m.alpha, m.n, idx, cnt, scratch, m.stream);
    int32_t nsv = 0;
    HIP_CHECK(hipMemcpyAsync(&nsv, cnt, 4, hipMemcpyDeviceToHost, m.stream));
    HIP_CHECK(hipStreamSynchronize(m.stream));
    s.alloc_zero(nsv, m.dp, 1, m.stream);
    launch::gather_sv(m.x, 0, m.xsq, m.alpha, m.y, idx, nsv, m.dp, s.sv, s.svsq, s.coef, m.stream);
    HIP_CHECK(hipStreamSynchronize(m.stream));
    for (void* p : {(void*)idx, (void*)cnt, (void*)scratch}) (void)hipFree(p);
    return;
  }
  // partitioned: each rank gathers its local SVs; all-gather padded blocks
  std::vector<int32_t> local_idx;
  for (int64_t j = 0; j < m.nl; ++j)
    if (alpha[m.off + j] > 0.f) local_idx.push_back((int32_t)(m.off + j));
  std::vector<double> cnts((size_t)m.world, 0.0);
  cnts[m.rank] = (double)local_idx.size();
  m.allreduce_sum_host(cnts.data(), m.world, "SV count all-reduce");
  int64_t per = 1;
  for (double c : cnts) per = std::max<int64_t>(per, (int64_t)c);
  s.alloc_zero(per * m.world, m.dp, 1, m.stream);
  int32_t* didx = dmalloc<int32_t>(std::max<size_t>(1, local_idx.size()), &tb);
  if (!local_idx.empty()) {
    HIP_CHECK(hipMemcpyAsync(didx, local_idx.data(), local_idx.size() * 4, hipMemcpyHostToDevice, m.stream));
    launch::gather_sv(m.x, m.args.x_row0, m.xsq, m.alpha, m.y, didx, (int64_t)local_idx.size(), m.dp,
                      s.sv + (size_t)m.rank * per * m.dp, s.svsq + m.rank * per, s.coef + m.rank * per, m.stream);
  }
  HIP_CHECK(hipStreamSynchronize(m.stream));
  (void)hipFree(didx);
  if (m.world == 1) return;
  // zero-padded blocks; coef = 0 on padding rows makes them inert
  auto gather = [&](float* buf, int64_t elems) {
    if (m.comm->device_memory()) {
      m.comm->allgather(buf + (size_t)m.rank * elems, buf, elems * 4, m.stream);
      sync_collective(m.comm, m.stream, "SV all-gather");
    } else {
      std::vector<float> h((size_t)elems * m.world);
      HIP_CHECK(hipMemcpy(h.data() + (size_t)m.rank * elems, buf + (size_t)m.rank * elems, elems * 4,
                          hipMemcpyDeviceToHost));
      m.comm->allgather(h.data() + (size_t)m.rank * elems, h.data(), elems * 4, nullptr);
      HIP_CHECK(hipMemcpy(buf, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    }
  };
  gather(s.sv, per * m.dp);
  gather(s.svsq, per);
  gather(s.coef, per);
}

// This rank's own rows [off, off + nl) against an SV set: their decision values sum_i coef_i K(i, j) - b into
// out_dev (or null), and / or the rows whose sign matches the label y[j] counted into *correct (or null; device).
static void predict_shard(GpuSolver::Impl& m, const DeviceSvs& s, float b, float* out_dev, const float* y,
                          int32_t* correct) {
  size_t tb = 0;
  float* part = dmalloc<float>((size_t)launch::predict_scratch_floats(m.nl, s.nsv), &tb);
  const int64_t lrow = m.off - m.args.x_row0;
  launch::rbf_predict(m.x + (size_t)lrow * m.dp, m.xsq + m.off, m.nl, m.dp, s.sv, s.svsq, s.coef, s.nsv, m.dp, m.dp,
                      m.gamma, b, part, out_dev, y, correct, m.stream);
  HIP_CHECK(hipStreamSynchronize(m.stream));
  (void)hipFree(part);
}

// f-style decision values of this rank's rows without b: out_j = sum_i alpha_i y_i K(i, j)
// for j in [off, off + nl), from a host alpha (length n).  Used to rebuild f on resume and
// by the DPSVM_VERIFY consistency check; collective in partitioned mode (SV all-gather).
void gpu_local_decision(GpuSolver::Impl& m, const std::vector<float>& alpha, float* out_dev) {
  DeviceSvs s;
  build_svs(m, alpha, s);
  predict_shard(m, s, 0.f, out_dev, nullptr, nullptr);
}

// ---------------------------------------------------------------------------
// Distributed training accuracy: every rank compacts the SVs from the
// replicated alpha, predicts its own shard rows on MFMA, one sum all-reduce.
// Reference: rank 0 alone, n x (Sgemv + transform_reduce) (svmTrain.cu:633-665).
// ---------------------------------------------------------------------------
double GpuSolver::train_accuracy(const SolveResult& r) {
  auto& m = *impl_;
  require_classifier(m.problem, "train_accuracy");
  require_x(m.kernel, "train_accuracy");
  HIP_CHECK(hipSetDevice(m.device));
  DeviceSvs s;
  build_svs(m, r.alpha, s);
  size_t tb = 0;
  int32_t* correct = dmalloc<int32_t>(1, &tb);
  HIP_CHECK(hipMemsetAsync(correct, 0, 4, m.stream));
  predict_shard(m, s, r.b, nullptr, m.y + m.off, correct);
  int32_t ok = 0;
  HIP_CHECK(hipMemcpy(&ok, correct, 4, hipMemcpyDeviceToHost));
  (void)hipFree(correct);
  double tot = ok;
  m.allreduce_sum_host(&tot, 1, "accuracy all-reduce");
  return tot / (double)m.n;
}

std::vector<float> GpuSolver::gradient() const {
  const auto& m = *impl_;
  HIP_CHECK(hipSetDevice(m.device));
  const int64_t rows = m.svr() ? m.ns : m.nl;  // epsilon-SVR: the 2n state rows (one rank)
  std::vector<float> f((size_t)rows);
  if (rows > 0) HIP_CHECK(hipMemcpy(f.data(), m.f, (size_t)rows * 4, hipMemcpyDeviceToHost));
  return f;
}

// ---------------------------------------------------------------------------
// Held-out decisions and the sigmoid fit on them (platt.hip): a fold's rows never leave the device
// ---------------------------------------------------------------------------
void GpuSolver::holdout_decisions(const int32_t* rows, int64_t nr, double b, int slot) {
  auto& m = *impl_;
  require_classifier(m.problem, "holdout_decisions");
  DPSVM_CHECK(m.engine && m.f && m.world == 1 && m.nl == m.n,
              "holdout_decisions: after setup() on one rank with all rows");
  DPSVM_CHECK(slot >= 0 && slot < (1 << 20) && nr >= 0 && nr <= m.n && (rows || nr == 0),
              "holdout_decisions: slot >= 0, at most n rows");
  for (int64_t r = 0; r < nr; ++r) DPSVM_CHECK(rows[r] >= 0 && rows[r] < m.n, "holdout_decisions: a row outside [0, n)");
  HIP_CHECK(hipSetDevice(m.device));
  if (slot >= m.holdout_slots) {  // grow: the slots written so far move over, the new ones are zero
    float* grown = dmalloc<float>((size_t)(slot + 1) * m.n, &m.bytes);
    HIP_CHECK(hipMemsetAsync(grown, 0, (size_t)(slot + 1) * m.n * 4, m.stream));
    if (m.holdout) {
      HIP_CHECK(hipMemcpyAsync(grown, m.holdout, (size_t)m.holdout_slots * m.n * 4, hipMemcpyDeviceToDevice,
                               m.stream));
      HIP_CHECK(hipStreamSynchronize(m.stream));
      HIP_CHECK(hipFree(m.holdout));
      m.bytes -= (size_t)m.holdout_slots * m.n * 4;
    }
    m.holdout = grown;
    m.holdout_slots = slot + 1;
    m.info.bytes_device = m.bytes;
  }
  if (!m.holdout_rows) {
    m.holdout_rows = dmalloc<int32_t>((size_t)m.n, &m.bytes);
    m.info.bytes_device = m.bytes;
  }
  if (nr == 0) return;
  HIP_CHECK(hipMemcpyAsync(m.holdout_rows, rows, (size_t)nr * 4, hipMemcpyHostToDevice, m.stream));
  launch::holdout_decision(m.f, m.y, m.holdout_rows, nr, b, m.holdout + (size_t)slot * m.n, m.stream);
  HIP_CHECK(hipStreamSynchronize(m.stream));  // rows is the caller's memory
}

std::vector<float> GpuSolver::holdout(int slot) const {
  const auto& m = *impl_;
  DPSVM_CHECK(slot >= 0 && slot < m.holdout_slots, "holdout: no such slot (holdout_decisions first)");
  HIP_CHECK(hipSetDevice(m.device));
  std::vector<float> out((size_t)m.n);
  HIP_CHECK(hipMemcpyAsync(out.data(), m.holdout + (size_t)slot * m.n, (size_t)m.n * 4, hipMemcpyDeviceToHost,
                           m.stream));
  HIP_CHECK(hipStreamSynchronize(m.stream));
  return out;
}

PlattFit GpuSolver::platt_fit(int slot) {
  auto& m = *impl_;
  require_classifier(m.problem, "platt_fit");
  DPSVM_CHECK(slot >= 0 && slot < m.holdout_slots, "platt_fit: no such slot (holdout_decisions first)");
  HIP_CHECK(hipSetDevice(m.device));
  if (!m.platt_out) {
    m.platt_out = dmalloc<PlattFit>(1, &m.bytes);
    m.info.bytes_device = m.bytes;
  }
  launch::platt_fit(m.holdout + (size_t)slot * m.n, m.n, m.y, m.n, m.n, 1, m.platt_out, m.stream);
  PlattFit r;
  HIP_CHECK(hipMemcpyAsync(&r, m.platt_out, sizeof(r), hipMemcpyDeviceToHost, m.stream));
  HIP_CHECK(hipStreamSynchronize(m.stream));
  return r;
}

std::vector<float> GpuSolver::decision(const SolveResult& r, const float* xh, int64_t nt, int d) {
  auto& m = *impl_;
  if (m.svr()) require_classifier(m.problem, "decision");  // (one-class: the same decision, served)
  require_x(m.kernel, "decision");
  DPSVM_CHECK(d == m.d, "feature count mismatch");
  HIP_CHECK(hipSetDevice(m.device));
  DeviceSvs s;
  build_svs(m, r.alpha, s);
  return predict_host_chunks(
      xh, nt, d, m.dp, 1, m.stream, [&](int64_t rows) { return launch::predict_scratch_floats(rows, s.nsv); },
      [&](const float* dx, const float* dsq, int64_t rows, float* part, float* ddec) {
        launch::rbf_predict(dx, dsq, rows, m.dp, s.sv, s.svsq, s.coef, s.nsv, m.dp, m.dp, m.gamma, r.b, part, ddec,
                            nullptr, nullptr, m.stream);
      });
}

// ---------------------------------------------------------------------------
// GpuPredictor (svmTest GPU path)
// ---------------------------------------------------------------------------
struct GpuPredictor::Impl {
  int device = 0;
  int d = 0, dp = 0;
  int precision = 0;  // launch::rbf_predict's: 0 auto, 1 f32, 2 split
  float gamma = 0.f, b = 0.f;
  int k = 0;  // > 0: a multi-class model (s.coef [nsv][k], s.bk its k thresholds)
  DeviceSvs s;
  hipStream_t stream = nullptr;
  ~Impl() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamDestroy(stream);
  }
  // what the two constructors share: device, stream, geometry, the zeroed SV set with the model's rows (host
  // [nsv][model_d]) and their norms.  The constructor fills coef (cols per row) and synchronizes.
  void init(int dev, int prec, int model_d, float g, int64_t nsv, const float* x, int cols) {
    DPSVM_CHECK(prec >= 0 && prec <= 2, "GpuPredictor: precision must be 0 (auto), 1 (f32) or 2 (split)");
    device = dev;
    precision = prec;
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    d = std::max(1, model_d);
    dp = pad_features(d);
    gamma = g;
    s.alloc_zero(nsv, dp, cols, stream);
    if (nsv) {
      HIP_CHECK(hipMemcpy2DAsync(s.sv, (size_t)dp * 4, x, (size_t)model_d * 4, (size_t)model_d * 4, (size_t)nsv,
                                 hipMemcpyHostToDevice, stream));
      launch::row_sqnorm(s.sv, nsv, dp, dp, s.svsq, stream);
    }
  }
};

GpuPredictor::GpuPredictor(const Model& mdl, int device, int precision) : impl_(new Impl) {
  auto& m = *impl_;
  m.init(device, precision, mdl.d, mdl.gamma, mdl.nsv(), mdl.x.data(), 1);
  m.b = mdl.b;
  std::vector<float> c((size_t)m.s.nsv);
  for (int64_t i = 0; i < m.s.nsv; ++i) c[i] = mdl.alpha[i] * mdl.y[i];
  if (m.s.nsv) HIP_CHECK(hipMemcpyAsync(m.s.coef, c.data(), m.s.nsv * 4, hipMemcpyHostToDevice, m.stream));
  HIP_CHECK(hipStreamSynchronize(m.stream));
}

GpuPredictor::GpuPredictor(const MultiModel& mdl, int device, int precision) : impl_(new Impl) {
  auto& m = *impl_;
  DPSVM_CHECK(mdl.k() >= 1 && (int)mdl.b.size() == mdl.k(), "GpuPredictor: a multi-class model needs k >= 1 classes");
  m.init(device, precision, mdl.d, mdl.gamma, mdl.nsv(), mdl.x.data(), mdl.k());
  m.k = mdl.k();
  size_t tb = 0;
  m.s.bk = dmalloc<float>((size_t)m.k, &tb);
  HIP_CHECK(hipMemcpyAsync(m.s.bk, mdl.b.data(), (size_t)m.k * 4, hipMemcpyHostToDevice, m.stream));
  if (m.s.nsv)
    HIP_CHECK(hipMemcpyAsync(m.s.coef, mdl.coef.data(), (size_t)m.s.nsv * m.k * 4, hipMemcpyHostToDevice, m.stream));
  HIP_CHECK(hipStreamSynchronize(m.stream));
}

GpuPredictor::~GpuPredictor() = default;

int GpuPredictor::k() const { return impl_->k; }

// the model's decision GEMM over a host matrix in chunks ([nt][max(k, 1)]), post(ddec, rows) before each download
template <class PostFn>
static std::vector<float> predictor_chunks(GpuPredictor::Impl& m, const float* xh, int64_t nt, int d, PostFn post) {
  DPSVM_CHECK(d == m.d || m.s.nsv == 0, "feature count mismatch between model and data");
  HIP_CHECK(hipSetDevice(m.device));
  if (m.k > 0)
    return predict_host_chunks(
        xh, nt, d, m.dp, m.k, m.stream,
        [&](int64_t rows) { return launch::predict_multi_scratch_floats(rows, m.s.nsv, m.k); },
        [&](const float* dx, const float* dsq, int64_t rows, float* scratch, float* ddec) {
          launch::rbf_predict_multi(dx, dsq, rows, m.dp, m.s.sv, m.s.svsq, m.s.coef, m.k, m.k, m.s.nsv, m.dp, m.dp,
                                    m.gamma, m.s.bk, scratch, ddec, m.k, m.stream, m.precision);
        },
        post);
  return predict_host_chunks(
      xh, nt, d, m.dp, 1, m.stream, [&](int64_t rows) { return launch::predict_scratch_floats(rows, m.s.nsv); },
      [&](const float* dx, const float* dsq, int64_t rows, float* part, float* ddec) {
        launch::rbf_predict(dx, dsq, rows, m.dp, m.s.sv, m.s.svsq, m.s.coef, m.s.nsv, m.dp, m.dp, m.gamma, m.b, part,
                            ddec, nullptr, nullptr, m.stream, m.precision);
      },
      post);
}

std::vector<float> GpuPredictor::decision_multi(const float* xh, int64_t nt, int d) {
  DPSVM_CHECK(impl_->k > 0, "decision_multi: this predictor holds a binary model");
  return predictor_chunks(*impl_, xh, nt, d, [](float*, int64_t) {});
}

std::vector<float> GpuPredictor::decision(const float* xh, int64_t nt, int d) {
  DPSVM_CHECK(impl_->k == 0, "decision: this predictor holds a multi-class model (decision_multi)");
  return predictor_chunks(*impl_, xh, nt, d, [](float*, int64_t) {});
}

std::vector<float> GpuPredictor::proba(const float* xh, int64_t nt, int d, const double* A, const double* B) {
  auto& m = *impl_;
  const int cols = std::max(m.k, 1);
  HIP_CHECK(hipSetDevice(m.device));
  size_t tb = 0;
  double* ab = dmalloc<double>((size_t)2 * cols, &tb);
  HIP_CHECK(hipMemcpyAsync(ab, A, (size_t)cols * 8, hipMemcpyHostToDevice, m.stream));
  HIP_CHECK(hipMemcpyAsync(ab + cols, B, (size_t)cols * 8, hipMemcpyHostToDevice, m.stream));
  HIP_CHECK(hipStreamSynchronize(m.stream));  // A, B are the caller's memory
  std::vector<float> out;
  try {
    out = predictor_chunks(m, xh, nt, d,
                           [&](float* ddec, int64_t rows) { launch::proba_rows(ddec, rows, cols, ab, ab + cols, m.stream); });
  } catch (...) {
    (void)hipFree(ab);
    throw;
  }
  (void)hipFree(ab);
  return out;
}

void GpuPredictor::decision_device(const float* x_dev, int64_t nt, int d, int ld, float* out_dev, void* stream) {
  auto& m = *impl_;
  DPSVM_CHECK(m.k == 0, "decision_device: this predictor holds a multi-class model");
  DPSVM_CHECK(d == m.d, "feature count mismatch");
  DPSVM_CHECK(ld % 16 == 0 && ld >= m.dp, "decision_device: ld must be a multiple of 16 >= padded d");
  hipStream_t s = (hipStream_t)stream;
  size_t tb = 0;
  const int64_t pad = round_up(nt, 128) + 128;
  float* dsq = dmalloc<float>((size_t)pad, &tb);
  float* part = dmalloc<float>((size_t)launch::predict_scratch_floats(nt, m.s.nsv), &tb);
  HIP_CHECK(hipMemsetAsync(dsq, 0, pad * 4, s));
  launch::row_sqnorm(x_dev, nt, m.dp, ld, dsq, s);
  launch::rbf_predict(x_dev, dsq, nt, ld, m.s.sv, m.s.svsq, m.s.coef, m.s.nsv, m.dp, m.dp, m.gamma, m.b, part, out_dev,
                      nullptr, nullptr, s, m.precision);
  HIP_CHECK(hipStreamSynchronize(s));
  (void)hipFree(dsq);
  (void)hipFree(part);
}

int device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

std::string device_name(int dev) {
  hipDeviceProp_t p;
  HIP_CHECK(hipGetDeviceProperties(&p, dev));
  std::string nm = p.name;
  while (!nm.empty() && nm.back() == ' ') nm.pop_back();
  return nm.empty() ? std::string(p.gcnArchName) : nm;
}

}  // namespace dpsvm
