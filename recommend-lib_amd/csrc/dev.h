// dev.h — the device-side host layer every C ABI file shares: the HIP status check, an owner of
// one device array, a handle's stream with its two timing events, and the padded-row copies.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/bprmf.h"
#include "status.h"

namespace bprmf {

#define HIPCHK(x)                                                                           \
  do {                                                                                      \
    hipError_t e_ = (x);                                                                    \
    if (e_ != hipSuccess) return bprmf::fail(BPRMF_E_HIP, "%s: %s", #x, hipGetErrorString(e_)); \
  } while (0)

template <typename T>
int dalloc(T** p, int64_t count) {
  *p = nullptr;
  if (count <= 0) return 0;
  HIPCHK(hipMalloc((void**)p, sizeof(T) * (size_t)count));
  return 0;
}

// Move-only owner of one hipMalloc'd array.  Every allocating call returns 0 or a fail() status,
// n <= 0 gives a null buffer, and after a failure the buffer is empty.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, n_ = o.n_;
      o.p_ = nullptr, o.n_ = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr, n_ = 0;
  }
  int alloc(int64_t n) {
    reset();
    if (int r = dalloc(&p_, n)) return r;
    n_ = p_ ? n : 0;
    return 0;
  }
  int zalloc(int64_t n) {
    if (int r = alloc(n)) return r;
    return p_ ? filled(hipMemset(p_, 0, bytes())) : 0;
  }
  // grow-only: the contents are dropped when it grows
  int reserve(int64_t n) { return n <= n_ ? 0 : alloc(n); }
  int upload(const T* src, int64_t n) {
    if (int r = alloc(n)) return r;
    return p_ ? filled(hipMemcpy(p_, src, bytes(), hipMemcpyHostToDevice)) : 0;
  }
  int upload(const std::vector<T>& v) { return upload(v.data(), (int64_t)v.size()); }
  int64_t size() const { return n_; }
  T* get() const { return p_; }
  operator T*() const { return p_; }

 private:
  size_t bytes() const { return sizeof(T) * (size_t)n_; }
  int filled(hipError_t e) {
    if (e == hipSuccess) return 0;
    reset();
    return fail(BPRMF_E_HIP, "filling a device buffer: %s", hipGetErrorString(e));
  }
  T* p_ = nullptr;
  int64_t n_ = 0;
};

// A handle's device, its non-blocking stream and the event pair that times a call.
struct Lane {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  Lane() = default;
  Lane(const Lane&) = delete;
  Lane& operator=(const Lane&) = delete;
  ~Lane() { close(); }
  int use() const {
    HIPCHK(hipSetDevice(device));
    return 0;
  }
  int open(int dev) {
    device = dev;
    if (int r = use()) return r;
    if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess)
      return fail(BPRMF_E_HIP, "stream/event creation failed");
    return 0;
  }
  void close() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (stream) (void)hipStreamDestroy(stream);
    ev0 = ev1 = nullptr, stream = nullptr;
  }
  int begin() {
    HIPCHK(hipEventRecord(ev0, stream));
    return 0;
  }
  int end(double* seconds) {  // waits for everything queued since begin()
    HIPCHK(hipEventRecord(ev1, stream));
    HIPCHK(hipEventSynchronize(ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
    *seconds = ms * 1e-3;
    return 0;
  }
};

// 2-D copies between dense [rows, k] host rows and padded [rows, ld] device rows
inline int copy_rows_in(float* dev, const float* host, int64_t rows, int k, int ld, hipStream_t s) {
  if (rows <= 0) return 0;
  HIPCHK(hipMemcpy2DAsync(dev, 4 * (size_t)ld, host, 4 * (size_t)k, 4 * (size_t)k, (size_t)rows,
                          hipMemcpyHostToDevice, s));
  return 0;
}
inline int copy_rows_out(float* host, const float* dev, int64_t rows, int k, int ld, hipStream_t s) {
  if (rows <= 0) return 0;
  HIPCHK(hipMemcpy2DAsync(host, 4 * (size_t)k, dev, 4 * (size_t)ld, 4 * (size_t)k, (size_t)rows,
                          hipMemcpyDeviceToHost, s));
  return 0;
}

}  // namespace bprmf
