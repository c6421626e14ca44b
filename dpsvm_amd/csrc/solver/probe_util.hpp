// Scaffold of the kernel probes (kernel_entry.hip, ws_kernel_entry.hip; nothing
// else includes it): the device buffers of one probe call, the event timer,
// the split-operand rows, the control record and arguments of a one-rank
// working-set launch.  A probe checks its arguments, then builds an Arena: no
// call site frees a buffer, destroys an event or reasons about the lifetime
// of a host vector it uploads.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "dpsvm/kernel_probes.hpp"
#include "gpu_impl.hpp"

namespace dpsvm {
namespace kernels {
namespace probe {

// Every device buffer of one probe call, bound to the stream the call works on:
// freed by the destructor (after the stream has drained), also on a throw.
class Arena {
 public:
  hipStream_t s = nullptr;
  // a non-blocking stream of its own (the probes on host vectors)
  Arena() : own_(true) { HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
  // the caller's stream (the entries on device pointers; nullptr: the null stream)
  explicit Arena(void* stream) : s((hipStream_t)stream) {}
  Arena(const Arena&) = delete;
  Arena& operator=(const Arena&) = delete;
  ~Arena() {
    (void)hipStreamSynchronize(s);
    for (void* p : bufs_) (void)hipFree(p);
    if (own_) (void)hipStreamDestroy(s);
  }
  // max(count, 1) zeroed elements
  template <class T>
  T* alloc(size_t count) {
    count = std::max<size_t>(count, 1);
    size_t tb = 0;
    bufs_.push_back(nullptr);
    T* d = gpu::dmalloc<T>(count, &tb);
    bufs_.back() = d;
    HIP_CHECK(hipMemsetAsync(d, 0, count * sizeof(T), s));
    return d;
  }
  // max(count, 1) zeroed elements of a peer-exchange receive buffer, allocated as GpuSolver::Impl::setup_exchange
  // allocates one: uncached device memory, plain device memory where that is refused (*uncached says which)
  template <class T>
  T* alloc_receive(size_t count, bool* uncached) {
    count = std::max<size_t>(count, 1);
    void* d = nullptr;
    bufs_.push_back(nullptr);
    *uncached = hipExtMallocWithFlags(&d, count * sizeof(T), hipDeviceMallocUncached) == hipSuccess;
    if (!*uncached) {
      (void)hipGetLastError();
      HIP_CHECK(hipMalloc(&d, count * sizeof(T)));
    }
    bufs_.back() = d;
    HIP_CHECK(hipMemset(d, 0, count * sizeof(T)));
    HIP_CHECK(hipDeviceSynchronize());
    return (T*)d;
  }
  // count elements: the first min(n, count) of h, zeros behind them.  The copy has left the (pageable) host
  // memory when up returns — it synchronises the stream — so h may be a temporary.
  // No byte is written twice: the zero fill covers only what lies behind the copy.
  template <class T>
  T* up(const T* h, size_t n, size_t count) {
    count = std::max<size_t>(count, 1);
    n = std::min(n, count);
    size_t tb = 0;
    bufs_.push_back(nullptr);
    T* d = gpu::dmalloc<T>(count, &tb);
    bufs_.back() = d;
    if (n < count) HIP_CHECK(hipMemsetAsync(d + n, 0, (count - n) * sizeof(T), s));
    if (n) HIP_CHECK(hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return d;
  }
  template <class T>
  T* up(const std::vector<T>& h, size_t count) {
    return up(h.data(), h.size(), count);
  }
  template <class T>
  T* up_one(const T& h) {
    return up(&h, 1, 1);
  }
  template <class T>
  std::vector<T> down(const T* d, size_t count) {
    std::vector<T> h(count);
    if (count) HIP_CHECK(hipMemcpyAsync(h.data(), d, count * sizeof(T), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return h;
  }

 private:
  bool own_ = false;
  std::vector<void*> bufs_;
};

// Event times of launches on a stream; the two events live as long as the timer.
class EventTimer {
 public:
  explicit EventTimer(hipStream_t s) : s_(s) {
    for (hipEvent_t& e : e_) HIP_CHECK(hipEventCreate(&e));
  }
  EventTimer(const EventTimer&) = delete;
  EventTimer& operator=(const EventTimer&) = delete;
  ~EventTimer() {
    for (hipEvent_t e : e_)
      if (e) (void)hipEventDestroy(e);
  }
  // microseconds of one repetition: record, launch, record, wait for the second event, read the elapsed time
  template <class Fn>
  double us(Fn&& launch) {
    HIP_CHECK(hipEventRecord(e_[0], s_));
    launch();
    HIP_CHECK(hipEventRecord(e_[1], s_));
    HIP_CHECK(hipEventSynchronize(e_[1]));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, e_[0], e_[1]));
    return 1e3 * (double)ms;
  }

 private:
  hipStream_t s_;
  hipEvent_t e_[2] = {nullptr, nullptr};
};

// microseconds of each of reps launches (none, and no event, for reps <= 0)
template <class Fn>
std::vector<double> time_launches(hipStream_t s, int reps, Fn&& launch) {
  std::vector<double> us;
  if (reps <= 0) return us;
  EventTimer t(s);
  for (int r = 0; r < reps; ++r) us.push_back(t.us(launch));
  return us;
}

// the times in the unit (scale 1: us, 1e-3: ms) and type an entry's Python surface returns
inline std::vector<float> to_f32(const std::vector<double>& us, double scale = 1.0) {
  std::vector<float> out;
  for (double t : us) out.push_back((float)(t * scale));
  return out;
}

// The split GEMMs' operands (split_rows_f16) of `rows` fp32 device rows of d floats at stride ldx.
struct SplitRows {
  void* planes = nullptr;
  int32_t* shift = nullptr;
  SplitRows(Arena& st, const float* x, int64_t rows, int d, int ldx) {
    const int64_t pr = launch::split_pad_rows(rows);
    planes = st.alloc<uint8_t>((size_t)pr * launch::split_row_u4(d) * 16);
    shift = st.alloc<int32_t>((size_t)pr);
    launch::split_rows_f16(x, rows, d, ldx, planes, shift, st.s);
  }
};

// a running round's control record, everything else zero
inline std::unique_ptr<WsCtrl> blank_ctrl() {
  auto c = std::make_unique<WsCtrl>();
  memset(c.get(), 0, sizeof(WsCtrl));
  c->done = kRunning;
  return c;
}

// the arguments every probe of a working-set kernel shares: one rank owning all n rows, the solver's defaults
inline WsArgs single_rank_args(int64_t n = 0) {
  WsArgs a{};
  a.n = a.nl = n;
  a.off = 0;
  a.world = 1;
  a.rank = 0;
  a.t_halve = 0.9f;
  a.clip_fallback = 1;
  return a;
}

}  // namespace probe
}  // namespace kernels
}  // namespace dpsvm
