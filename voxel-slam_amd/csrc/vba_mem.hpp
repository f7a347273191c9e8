// Owning device / pinned-host buffers of the context and the handle structs ("source layout").  A buffer is freed by its
// member's destructor.  No pool, no growth policy, no stream of its own: how much to ask for, when to drain the stream before a
// buffer is replaced and what an allocation counter adds stay at the call site.  It defines no kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace vba {

template <class T, bool Pinned>
struct Mem {
  T *p = nullptr;
  size_t n = 0;        // capacity, elements

  Mem() = default;
  Mem(const Mem &) = delete;
  Mem &operator=(const Mem &) = delete;
  Mem(Mem &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  Mem &operator=(Mem &&o) noexcept {
    if (this != &o) { reset(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
    return *this;
  }
  ~Mem() { reset(); }
  operator T *() const { return p; }
  T *operator->() const { return p; }

  void reset() {
    if (p) { if (Pinned) (void)hipHostFree(p); else (void)hipFree(p); }
    p = nullptr; n = 0;
  }
  // at least `want` elements, contents not kept: free, allocate exactly `want`, record.  Empty after a failed allocation.
  hipError_t ensure(size_t want) {
    if (want <= n) return hipSuccess;
    reset();
    const hipError_t e = Pinned ? hipHostMalloc((void **)&p, want * sizeof(T), hipHostMallocDefault) : hipMalloc((void **)&p, want * sizeof(T));
    if (e != hipSuccess) { p = nullptr; return e; }
    n = want;
    return hipSuccess;
  }
  // exactly `want` elements with the first `keep` of the old block copied on `stream`; synchronises before the old block is
  // freed.  After a failure the old block is intact and the new one is gone.
  hipError_t grow_keep(size_t want, size_t keep, hipStream_t stream) {
    static_assert(!Pinned, "grow_keep copies device to device");
    Mem nw;
    hipError_t e = nw.ensure(want);
    if (e == hipSuccess && p && keep) e = hipMemcpyAsync(nw.p, p, keep * sizeof(T), hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess && p) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) *this = static_cast<Mem &&>(nw);
    return e;
  }
};
template <class T> using DevMem = Mem<T, false>;
template <class T> using PinMem = Mem<T, true>;

}  // namespace vba
