// Kernel-level test entry points (device pointers in and out): one launcher
// each on caller-owned state, for tests/test_kernels_gpu.py and the probes under
// bench/ — the row / Gram / decision GEMMs, the pair engines' selection and X
// pass, SV compaction.  The working-set kernels' are in ws_kernel_entry.hip.
#include <hip/hip_runtime.h>

#include "gpu_impl.hpp"

namespace dpsvm {

using gpu::dmalloc;

namespace kernels {

void row_sqnorm(const float* x, int64_t n, int d, int ld, float* out, void* stream) {
  launch::row_sqnorm(x, n, d, ld, out, (hipStream_t)stream);
}

void stream_read(const void* x, int64_t bytes, float* out, int blocks, void* stream) {
  launch::stream_read(x, bytes, out, blocks, (hipStream_t)stream);
}

void rbf_rows(const float* x, const float* xsq, int64_t n, int ld, const float* w, const float* wsq, int nq,
              float gamma, float* out, int64_t out_ld, void* stream) {
  DPSVM_CHECK(nq >= 1 && nq <= kNQ, "rbf_rows: 1 <= nq <= 16");
  DPSVM_CHECK(ld % 16 == 0, "rbf_rows: ld must be a multiple of 16");
  hipStream_t s = (hipStream_t)stream;
  std::vector<float> hsq((size_t)nq);
  HIP_CHECK(hipMemcpyAsync(hsq.data(), wsq, nq * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  SmoCtrl c;
  memset(&c, 0, sizeof(c));
  c.nq = nq;
  c.n_compute = nq;  // all queries are kOpCompute (0) after the memset
  for (int q = 0; q < nq; ++q) {
    c.q_idx[q] = q;
    c.q_line[q] = q;
    c.q_sq[q] = hsq[q];
    c.q_ptr[q] = w + (size_t)q * ld;
  }
  size_t tb = 0;
  SmoCtrl* dc = dmalloc<SmoCtrl>(1, &tb);
  HIP_CHECK(hipMemcpyAsync(dc, &c, sizeof(c), hipMemcpyHostToDevice, s));
  SmoArgs a{};
  a.x = x;
  a.xsq = xsq;
  a.lines = out;
  a.ldl = out_ld;
  a.ctrl = dc;
  a.n = n;
  a.nl = n;
  a.off = 0;
  a.x_row0 = 0;
  a.dp = ld;
  a.d = ld;
  a.G = (int32_t)((n + kStepRows - 1) / kStepRows);
  a.gamma = gamma;
  gpu::need_quarantine("k_rbf_rows (smo_rows)").smo_rows(a, s);
  HIP_CHECK(hipStreamSynchronize(s));
  (void)hipFree(dc);
}

void select_partials(const float* f, const float* alpha, const float* y, int64_t n, int64_t offset, float C,
                     uint64_t* partials, int* blocks_out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  SmoCtrl c;
  memset(&c, 0, sizeof(c));
  c.line_hi = c.line_lo = -1;
  size_t tb = 0;
  SmoCtrl* dc = dmalloc<SmoCtrl>(1, &tb);
  HIP_CHECK(hipMemcpyAsync(dc, &c, sizeof(c), hipMemcpyHostToDevice, s));
  SmoArgs a{};
  a.f = const_cast<float*>(f);
  a.alpha = const_cast<float*>(alpha);
  a.y = y;
  a.ctrl = dc;
  a.partials = partials;
  a.nl = n;
  a.off = offset;
  a.C = C;
  a.G = (int32_t)((n + kStepRows - 1) / kStepRows);
  gpu::need_quarantine("k_select_partials (smo_step)").smo_step(a, s);
  HIP_CHECK(hipStreamSynchronize(s));
  (void)hipFree(dc);
  if (blocks_out) *blocks_out = a.G;
}

void predict(const float* x, const float* xsq, int64_t n, int ld, const float* sv, const float* svsq,
             const float* coef, int64_t nsv, int sv_ld, float gamma, float b, float* dec, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  DPSVM_CHECK(ld == sv_ld && ld % 16 == 0, "predict: ld == sv_ld, multiple of 16");
  size_t tb = 0;
  float* part = dmalloc<float>((size_t)launch::predict_scratch_floats(n, nsv), &tb);
  launch::rbf_predict(x, xsq, n, ld, sv, svsq, coef, nsv, sv_ld, ld, gamma, b, part, dec, nullptr, nullptr, s);
  HIP_CHECK(hipStreamSynchronize(s));
  (void)hipFree(part);
}

void predict_multi(const float* x, const float* xsq, int64_t n, int ld, const float* sv, const float* svsq,
                   const float* coef, int k, int64_t nsv, int sv_ld, float gamma, const float* b, float* dec,
                   void* stream) {
  hipStream_t s = (hipStream_t)stream;
  DPSVM_CHECK(ld == sv_ld && ld % 16 == 0 && k >= 1, "predict_multi: ld == sv_ld, multiple of 16; k >= 1");
  size_t tb = 0;
  float* scratch = dmalloc<float>((size_t)launch::predict_multi_scratch_floats(n, nsv, k), &tb);
  launch::rbf_predict_multi(x, xsq, n, ld, sv, svsq, coef, k, k, nsv, sv_ld, ld, gamma, b, scratch, dec, k, s);
  HIP_CHECK(hipStreamSynchronize(s));
  (void)hipFree(scratch);
}

std::vector<float> predict_multi_bench(const float* x, const float* xsq, int64_t n, int ld, const float* sv,
                                       const float* svsq, const float* coef, const float* coef_cols, int64_t ldcc,
                                       int k, int64_t nsv, float gamma, const float* b, float* dec, bool multi,
                                       int reps, void* stream) {
  DPSVM_CHECK(ld % 16 == 0 && k >= 1 && reps > 0, "predict_multi_bench: arguments");
  hipStream_t s = (hipStream_t)stream;
  size_t tb = 0;
  float* scratch = dmalloc<float>((size_t)launch::predict_multi_scratch_floats(n, nsv, k), &tb);
  hipEvent_t e0, e1;
  HIP_CHECK(hipEventCreate(&e0));
  HIP_CHECK(hipEventCreate(&e1));
  std::vector<float> ms;
  for (int r = 0; r < reps; ++r) {
    HIP_CHECK(hipEventRecord(e0, s));
    if (multi) {
      launch::rbf_predict_multi(x, xsq, n, ld, sv, svsq, coef, k, k, nsv, ld, ld, gamma, b, scratch, dec, k, s);
    } else {
      for (int c = 0; c < k; ++c)
        launch::rbf_predict(x, xsq, n, ld, sv, svsq, coef_cols + (size_t)c * ldcc, nsv, ld, ld, gamma, 0.f, scratch,
                            dec, nullptr, nullptr, s);
    }
    HIP_CHECK(hipEventRecord(e1, s));
    HIP_CHECK(hipEventSynchronize(e1));
    float t = 0.f;
    HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
    ms.push_back(t);
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipFree(scratch);
  return ms;
}

void rbf_gram(const float* a, const float* asq, int64_t m, const float* b, const float* bsq, int64_t n, int ld,
              float gamma, float* out, int64_t out_ld, bool symmetric, void* stream) {
  launch::rbf_gemm_store(a, asq, m, ld, b, bsq, n, ld, ld, gamma, out, out_ld, (hipStream_t)stream, symmetric);
}

namespace {
// split rows (rbf_gemm_split.hip) of `rows` fp32 rows of x, in a fresh buffer
struct SplitRows {
  void* planes = nullptr;
  int32_t* shift = nullptr;
  SplitRows(const float* x, int64_t rows, int ld, hipStream_t s) {
    const int64_t pr = launch::split_pad_rows(rows);
    const size_t bytes = (size_t)pr * launch::split_row_u4(ld) * 16;
    size_t tb = 0;
    planes = dmalloc<uint8_t>(bytes, &tb);
    shift = dmalloc<int32_t>((size_t)pr, &tb);
    HIP_CHECK(hipMemsetAsync(planes, 0, bytes, s));
    HIP_CHECK(hipMemsetAsync(shift, 0, (size_t)pr * 4, s));
    launch::split_rows_f16(x, rows, ld, ld, planes, shift, s);
  }
  ~SplitRows() {
    (void)hipFree(planes);
    (void)hipFree(shift);
  }
};
}  // namespace

void rbf_gram_split(const float* a, const float* asq, int64_t m, const float* b, const float* bsq, int64_t n, int ld,
                    float gamma, float* out, int64_t out_ld, bool symmetric, void* stream, float cold_tau) {
  hipStream_t s = (hipStream_t)stream;
  SplitRows sa(a, m, ld, s);
  if (symmetric) {
    launch::rbf_gemm_store_split(sa.planes, sa.shift, asq, m, sa.planes, sa.shift, asq, n, ld, gamma, out, out_ld, s,
                                 true, cold_tau);
    HIP_CHECK(hipStreamSynchronize(s));
    return;
  }
  SplitRows sb(b, n, ld, s);
  launch::rbf_gemm_store_split(sa.planes, sa.shift, asq, m, sb.planes, sb.shift, bsq, n, ld, gamma, out, out_ld, s,
                               false, cold_tau);
  HIP_CHECK(hipStreamSynchronize(s));
}

std::vector<float> dot_gram_split(const float* a, int64_t m, const float* b, int64_t n, int d, int lda, int ldb,
                                  const DotKernelSpec& spec, float gamma, float* out, int64_t out_ld, bool symmetric,
                                  void* stream, int reps) {
  hipStream_t s = (hipStream_t)stream;
  std::vector<float> us;
  if (m <= 0 || n <= 0) return us;
  DPSVM_CHECK(d >= 1 && lda >= d && (symmetric || ldb >= d), "dot_gram_split: rows of d >= 1 floats at stride >= d");
  const auto split = [&](const float* x, int64_t rows, int ldx, void** planes, int32_t** shift) {
    const int64_t pr = launch::split_pad_rows(rows);
    const size_t bytes = (size_t)pr * launch::split_row_u4(d) * 16;
    size_t tb = 0;
    *planes = dmalloc<uint8_t>(bytes, &tb);
    *shift = dmalloc<int32_t>((size_t)pr, &tb);
    HIP_CHECK(hipMemsetAsync(*planes, 0, bytes, s));
    HIP_CHECK(hipMemsetAsync(*shift, 0, (size_t)pr * 4, s));
    launch::split_rows_f16(x, rows, d, ldx, *planes, *shift, s);
  };
  void *pa = nullptr, *pb = nullptr;
  int32_t *sa = nullptr, *sb = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  struct Free {
    void *&pa, *&pb;
    int32_t *&sa, *&sb;
    hipEvent_t &e0, &e1;
    ~Free() {
      (void)hipFree(pa);
      (void)hipFree(pb);
      (void)hipFree(sa);
      (void)hipFree(sb);
      if (e0) (void)hipEventDestroy(e0);
      if (e1) (void)hipEventDestroy(e1);
    }
  } free_all{pa, pb, sa, sb, e0, e1};
  split(a, m, lda, &pa, &sa);
  if (!symmetric) split(b, n, ldb, &pb, &sb);
  const void* B = symmetric ? pa : pb;
  const int32_t* Bsh = symmetric ? sa : sb;
  if (reps > 0) {
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
  }
  for (int r = 0; r <= reps; ++r) {  // reps timed launches, then the returned one
    if (r < reps) HIP_CHECK(hipEventRecord(e0, s));
    launch::dot_gram_split(pa, sa, m, B, Bsh, n, d, spec, gamma, out, out_ld, symmetric, s);
    if (r < reps) {
      HIP_CHECK(hipEventRecord(e1, s));
      HIP_CHECK(hipEventSynchronize(e1));
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
      us.push_back(ms * 1e3f);
    }
  }
  HIP_CHECK(hipStreamSynchronize(s));
  return us;
}

std::pair<int64_t, int64_t> gram_adapt_last() {
  int64_t t = -1, h = -1;
  launch::gram_adapt_last(&t, &h);
  return {t, h};
}

void rbf_rows_indexed(const float* x, const float* xsq, int64_t n, int ld, const int* rows, int m, float gamma,
                      float* out, int64_t out_ld, const int* out_rows, void* stream, bool split) {
  DPSVM_CHECK(ld % 16 == 0 && m >= 0 && m <= 4096, "rbf_rows_indexed: ld multiple of 16, m <= 4096");
  hipStream_t s = (hipStream_t)stream;
  size_t tb = 0;
  int32_t* md = dmalloc<int32_t>(1, &tb);
  HIP_CHECK(hipMemcpyAsync(md, &m, 4, hipMemcpyHostToDevice, s));
  if (split) {
    SplitRows sx(x, n, ld, s);
    launch::rbf_rows_indexed_split(sx.planes, sx.shift, xsq, rows, md, m, sx.planes, sx.shift, xsq, n, ld, gamma, out,
                                   out_rows, out_ld, s);
    HIP_CHECK(hipStreamSynchronize(s));
  } else {
    launch::rbf_rows_indexed(x, xsq, rows, md, m, x, xsq, n, ld, gamma, out, out_rows, out_ld, s);
    HIP_CHECK(hipStreamSynchronize(s));
  }
  (void)hipFree(md);
}

std::vector<float> rbf_rows_indexed_split_bench(const float* x, const float* xsq, int64_t n, int ld, const int* rows,
                                                int m, float gamma, float* out, int64_t out_ld, const int* out_rows,
                                                int reps, void* stream) {
  DPSVM_CHECK(ld % 16 == 0 && m >= 0 && m <= 4096 && reps > 0, "rbf_rows_indexed_split_bench: arguments");
  hipStream_t s = (hipStream_t)stream;
  size_t tb = 0;
  int32_t* md = dmalloc<int32_t>(1, &tb);
  HIP_CHECK(hipMemcpyAsync(md, &m, 4, hipMemcpyHostToDevice, s));
  SplitRows sx(x, n, ld, s);
  hipEvent_t e0, e1;
  HIP_CHECK(hipEventCreate(&e0));
  HIP_CHECK(hipEventCreate(&e1));
  std::vector<float> ms;
  for (int r = 0; r < reps; ++r) {
    HIP_CHECK(hipEventRecord(e0, s));
    launch::rbf_rows_indexed_split(sx.planes, sx.shift, xsq, rows, md, m, sx.planes, sx.shift, xsq, n, ld, gamma, out,
                                   out_rows, out_ld, s);
    HIP_CHECK(hipEventRecord(e1, s));
    HIP_CHECK(hipEventSynchronize(e1));
    float t = 0.f;
    HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
    ms.push_back(t);
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipFree(md);
  return ms;
}

void xpass_rows(const float* x, const float* xsq, int64_t n, int ld, const int* keys, int nq, float gamma,
                float* out, int64_t out_ld, int rows_per_group, void* stream) {
  DPSVM_CHECK(ld % 16 == 0 && rows_per_group > 0 && rows_per_group % kFusedThreads == 0,
              "xpass_rows: ld multiple of 16, rows_per_group multiple of 256");
  const int64_t G = (n + rows_per_group - 1) / rows_per_group;
  DPSVM_CHECK(out_ld >= G * rows_per_group, "xpass_rows: out rows must cover every workgroup's tiles");
  SmoArgs a{};
  a.x = x;
  a.xsq = xsq;
  a.lines = out;
  a.ldl = out_ld;
  a.n = n;
  a.nl = n;
  a.off = 0;
  a.x_row0 = 0;
  a.dp = ld;
  a.d = ld;
  a.gamma = gamma;
  a.fused_rows = rows_per_group;
  a.fused_G = (int32_t)G;
  hipStream_t s = (hipStream_t)stream;
  gpu::need_quarantine("k_xpass_rows (xpass)").xpass_rows(a, keys, nq, s);
  HIP_CHECK(hipStreamSynchronize(s));
}

void fused_select(const float* f, const float* alpha, const float* y, int64_t n, float C, int rows_per_group,
                  uint64_t* keys_out, void* stream) {
  DPSVM_CHECK(rows_per_group > 0 && rows_per_group % kFusedThreads == 0, "fused_select: rows multiple of 256");
  SmoArgs a{};
  a.f = const_cast<float*>(f);
  a.alpha = const_cast<float*>(alpha);
  a.y = y;
  a.nl = n;
  a.n = n;
  a.off = 0;
  a.C = C;
  a.fused_rows = rows_per_group;
  a.fused_G = (int32_t)((n + rows_per_group - 1) / rows_per_group);
  a.xworld = 0;  // keys to memory, no exchange
  hipStream_t s = (hipStream_t)stream;
  launch::smo_fused(a, 0, nullptr, keys_out, nullptr, nullptr, s);
  HIP_CHECK(hipStreamSynchronize(s));
}

int64_t compact_nonzero(const float* alpha, int64_t n, int* idx_out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  size_t tb = 0;
  int32_t* cnt = dmalloc<int32_t>(1, &tb);
  int32_t* scratch = dmalloc<int32_t>((size_t)launch::compact_scratch_ints(n), &tb);
  launch::compact_positive(alpha, n, idx_out, cnt, scratch, s);
  int32_t h = 0;
  HIP_CHECK(hipMemcpyAsync(&h, cnt, 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  (void)hipFree(cnt);
  (void)hipFree(scratch);
  return h;
}

// ---- probability estimates (platt.hip): host vectors in and out on the null stream ----
namespace {
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t count;
  explicit DevBuf(size_t c) : count(std::max<size_t>(c, 1)) {
    size_t tb = 0;
    p = dmalloc<T>(count, &tb);
    HIP_CHECK(hipMemset(p, 0, count * sizeof(T)));
  }
  explicit DevBuf(const std::vector<T>& h) : DevBuf(h.size()) {
    if (!h.empty()) HIP_CHECK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  }
  DevBuf(const DevBuf&) = delete;
  ~DevBuf() { (void)hipFree(p); }
  std::vector<T> down(size_t c) const {
    std::vector<T> h(c);
    if (c) HIP_CHECK(hipMemcpy(h.data(), p, c * sizeof(T), hipMemcpyDeviceToHost));
    return h;
  }
};
}  // namespace

std::vector<float> holdout_decision(const std::vector<float>& f, const std::vector<float>& y,
                                    const std::vector<int32_t>& rows, double b, std::vector<float> dec, int slot) {
  const int64_t n = (int64_t)f.size();
  DPSVM_CHECK(n > 0 && (int64_t)y.size() == n, "holdout_decision: f and y of n > 0 rows");
  DPSVM_CHECK(slot >= 0 && (int64_t)dec.size() % n == 0 && (int64_t)slot < (int64_t)dec.size() / n,
              "holdout_decision: dec [slots][n] with slot < slots");
  for (int32_t r : rows) DPSVM_CHECK(r >= 0 && r < n, "holdout_decision: a row outside [0, n)");
  DevBuf<float> df(f), dy(y), dd(dec);
  DevBuf<int32_t> dr(rows);
  launch::holdout_decision(df.p, dy.p, dr.p, (int64_t)rows.size(), b, dd.p + (size_t)slot * n, nullptr);
  HIP_CHECK(hipStreamSynchronize(nullptr));
  return dd.down(dec.size());
}

std::vector<PlattFit> platt_fit(const std::vector<float>& dec, const std::vector<float>& y, int m, int64_t n) {
  DPSVM_CHECK(m >= 1 && n >= 1 && (int64_t)dec.size() == m * n && (int64_t)y.size() == m * n,
              "platt_fit: dec and y [m][n], m, n >= 1");
  DevBuf<float> dd(dec), dy(y);
  DevBuf<PlattFit> out((size_t)m);
  launch::platt_fit(dd.p, n, dy.p, n, n, m, out.p, nullptr);
  HIP_CHECK(hipStreamSynchronize(nullptr));
  return out.down((size_t)m);
}

std::vector<float> platt_fit_bench(const std::vector<float>& dec, const std::vector<float>& y, int m, int64_t n,
                                   int reps) {
  DPSVM_CHECK(m >= 1 && n >= 1 && reps > 0 && (int64_t)dec.size() == m * n && (int64_t)y.size() == m * n,
              "platt_fit_bench: dec and y [m][n], m, n >= 1, reps > 0");
  DevBuf<float> dd(dec), dy(y);
  DevBuf<PlattFit> out((size_t)m);
  hipEvent_t e0, e1;
  HIP_CHECK(hipEventCreate(&e0));
  HIP_CHECK(hipEventCreate(&e1));
  std::vector<float> ms;
  for (int r = 0; r < reps; ++r) {
    HIP_CHECK(hipEventRecord(e0, nullptr));
    launch::platt_fit(dd.p, n, dy.p, n, n, m, out.p, nullptr);
    HIP_CHECK(hipEventRecord(e1, nullptr));
    HIP_CHECK(hipEventSynchronize(e1));
    float t = 0.f;
    HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
    ms.push_back(t);
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return ms;
}

std::vector<float> proba_rows(const std::vector<float>& dec, int64_t n, int k, const std::vector<double>& A,
                              const std::vector<double>& B) {
  DPSVM_CHECK(n >= 1 && k >= 1 && (int64_t)dec.size() == n * k && (int)A.size() == k && (int)B.size() == k,
              "proba_rows: dec [n][k], A and B of k values");
  DevBuf<float> dd(dec);
  DevBuf<double> dA(A), dB(B);
  launch::proba_rows(dd.p, n, k, dA.p, dB.p, nullptr);
  HIP_CHECK(hipStreamSynchronize(nullptr));
  return dd.down(dec.size());
}

}  // namespace kernels

}  // namespace dpsvm
