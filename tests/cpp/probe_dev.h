// What the kernel probes (imputer_probe.hip, latent_probe.hip) share: a device copy of a host
// array of an exact length, and the early return on a HIP error.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

// a device buffer of exactly `count` elements holding the host array's contents (no buffer for
// a null pointer or no elements); back() copies the whole of it to the host array again
template <class T>
struct Dev {
  T *ptr = nullptr;
  T *host;
  size_t bytes;
  hipError_t err = hipSuccess;
  Dev(const T *h, size_t count) : host(const_cast<T *>(h)), bytes(count * sizeof(T)) {
    if (!h || !count) return;
    err = hipMalloc((void **)&ptr, bytes);
    if (err == hipSuccess) err = hipMemcpy(ptr, h, bytes, hipMemcpyHostToDevice);
  }
  hipError_t back() { return ptr ? hipMemcpy(host, ptr, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
  ~Dev() {
    if (ptr) (void)hipFree(ptr);
  }
  Dev(const Dev &) = delete;
};

#define IP_TRY(expr)                              \
  do {                                            \
    hipError_t e__ = (expr);                      \
    if (e__ != hipSuccess) return (int)e__;       \
  } while (0)
