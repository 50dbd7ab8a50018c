// device_scope.h -- what an entry point outside the training path does on the host around its kernels, each stated once (host code only):
//   DeviceBuf    owns a hipMalloc (or pinned host) allocation for the length of a call or the life of a handle;
//   read_back    brings a status word or a small array back on the stream and waits for it;
//   host_copy    a host array holding `count` elements of a device array.
// With these an entry point returns early through GSS_HIP / GSS_LAUNCH_CHECK / GSS_REQUIRE and leaks nothing.
//
// The lifetime rule: hipFree waits for the device to finish, so a DeviceBuf may leave its scope, on an early return as on the ordinary one,
// with kernels that read or write it still in flight on a stream.  That makes every early return safe; it is no reason to drop a
// hipStreamSynchronize that orders something else (a host read of a result, a caller's workspace that the next call reuses).
//
// A handle struct with DeviceBuf members (gss_paths, gss_prox, gss_ppr) is destroyed with `delete p`, and while it is being created a
// std::unique_ptr holds it.  Such a struct is declared visibility("hidden"), so that its implicit destructor is not an export of the library.
#pragma once
#include <memory>
#include <new>

#include "common.h"

namespace gss {
namespace {   // as in profile_front.h: every file that includes this has its own copy and the library exports nothing from here

template <typename T, bool kPinned = false>
struct DeviceBuf {
  T *p = nullptr;
  size_t bytes = 0;
  DeviceBuf() = default;
  DeviceBuf(const DeviceBuf &) = delete;   // nothing moves one either: handles hold them as members and live on the heap
  DeviceBuf &operator=(const DeviceBuf &) = delete;
  ~DeviceBuf() { release(); }
  void release() {
    if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    bytes = 0;
  }
  // Frees what it holds and allocates `want` bytes (contents undefined): also the way to regrow.  On failure it holds nothing, the sticky
  // HIP error is cleared, and the refusal is "<who>: hipMalloc of <want> bytes failed"
  int alloc(const char *who, size_t want) {
    release();
    if ((kPinned ? hipHostMalloc((void **)&p, want) : hipMalloc((void **)&p, want)) != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      return fail(GSS_ENOMEM, "%s: hipMalloc of %zu bytes failed", who, want);
    }
    bytes = want;
    return GSS_OK;
  }
};

// `bytes` from device to host on the stream, then waits for the stream: what the host reads next is there
inline int read_back(void *host, const void *dev, size_t bytes, hipStream_t st) {
  GSS_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
  GSS_HIP(hipStreamSynchronize(st));
  return GSS_OK;
}

// h = a host copy of dev[0 .. count), read back on the stream; without host memory the GSS_ENOMEM refusal in the caller's words (fmt, args)
template <typename T, typename... Args>
int host_copy(std::unique_ptr<T[]> &h, const T *dev, size_t count, hipStream_t st, const char *fmt, Args... args) {
  h.reset(new (std::nothrow) T[count]);
  if (!h) return fail(GSS_ENOMEM, fmt, args...);
  return read_back(h.get(), dev, count * sizeof(T), st);
}

}  // namespace
}  // namespace gss
