// Owning device / pinned-host buffers of the context and the handle structs ("source layout").  A buffer is freed by its
// member's destructor.  No pool, no growth policy, no stream of its own: how much to ask for, when to drain the stream before a
// buffer is replaced and what an allocation counter adds stay at the call site.  It defines no kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <vector>

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

// A family of [rows][cap] device arrays that share one capacity (array i: arrs[i].rows rows of arrs[i].elem-byte elements) grows
// from oldcap to newcap columns as a whole: every new block is allocated and zero-filled and takes the first `used` columns of its
// old block at the new stride, the stream is synchronised once, then `own` holds the new blocks and the old ones are freed.  After a
// failure `own` is untouched (the stride its arrays were written with stays the one the caller records) and the new blocks are gone.
template <class Arr>
hipError_t grow_family(std::vector<DevMem<char>> &own, const std::vector<Arr> &arrs, size_t oldcap, size_t newcap, size_t used, hipStream_t stream) {
  std::vector<DevMem<char>> nw(arrs.size());
  hipError_t e = hipSuccess;
  for (size_t i = 0; e == hipSuccess && i < arrs.size(); i++) {
    const size_t elem = arrs[i].elem, bytes = elem * arrs[i].rows * newcap;
    e = nw[i].ensure(bytes);
    if (e == hipSuccess) e = hipMemsetAsync(nw[i].p, 0, bytes, stream);
    if (e == hipSuccess && i < own.size() && own[i].p && used > 0)
      e = hipMemcpy2DAsync(nw[i].p, newcap * elem, own[i].p, oldcap * elem, used * elem, arrs[i].rows, hipMemcpyDeviceToDevice, stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e == hipSuccess) own.swap(nw);
  return e;
}

}  // namespace vba
