// Move-only owners of what the API layer (ofdg_api.hip) takes from the HIP runtime: device memory, pinned host memory,
// events and streams.  Each frees what it holds when it goes out of scope; nothing here launches or waits for anything.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace ofdg {

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;     // elements
  bool view = false;  // p points into another allocation (the record arena of an uploaded batch): not ours to free
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap), view(o.view) { o.p = nullptr; o.cap = 0; o.view = false; }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); std::swap(view, o.view); return *this; }
  ~DevBuf() { release(); }
  // exactly n elements in place of what is held (pools and tables, sized once)
  hipError_t alloc(size_t n) {
    if (p && !view) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; }
    p = nullptr; cap = 0; view = false;
    hipError_t e = hipMalloc((void**)&p, n * sizeof(T));
    if (e == hipSuccess) cap = n;
    return e;
  }
  // room for n elements; what grows, grows by a quarter more (per-call workspaces)
  hipError_t reserve(size_t n) { return (n <= cap && !view) ? hipSuccess : alloc(n + n / 4 + 16); }
  // look at n elements of somebody else's memory (what we own is given up first)
  hipError_t alias(T* q, size_t n) {
    if (p && !view) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; }
    p = q; cap = n; view = true;
    return hipSuccess;
  }
  void release() { if (p && !view) (void)hipFree(p); p = nullptr; cap = 0; view = false; }
};

struct PinnedBuf {  // hipHostMalloc
  void* p = nullptr;
  size_t bytes = 0;
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
  hipError_t alloc(size_t n, unsigned flags) {
    if (p) { hipError_t e = hipHostFree(p); if (e != hipSuccess) return e; }
    p = nullptr; bytes = 0;
    hipError_t e = hipHostMalloc(&p, n, flags);
    if (e == hipSuccess) bytes = n;
    return e;
  }
};

struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
  ~Event() { if (e) (void)hipEventDestroy(e); }
  hipError_t create(unsigned flags) { return hipEventCreateWithFlags(&e, flags); }
  operator hipEvent_t() const { return e; }
};

struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
  ~Stream() { if (s) (void)hipStreamDestroy(s); }
  hipError_t create(unsigned flags) { return hipStreamCreateWithFlags(&s, flags); }
  operator hipStream_t() const { return s; }
};

}  // namespace ofdg
