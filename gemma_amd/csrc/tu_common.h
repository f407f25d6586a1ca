// Host-side plumbing shared by gemma_hip.hip and the separately compiled feature units (eigh_tu, vc_tu, prdt_tu, mqs_tu, cor_tu): the owning
// device buffer, HIP error reporting into a message string, and the staging copy of a block of host rows.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/gemma_hip.h"

namespace gemma_hip {

// A device allocation that grows and never shrinks.  No destructor: the states that hold these (g_ctx, g_rg, g_pd, g_vc, g_mqs, g_cor) have
// static lifetime, and a hipFree from a static destructor would run after the runtime is gone.  Every owner releases member by
// member from its shutdown; a local that has to be freed on every return path is a ScopedBuf.
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  int reserve(size_t bytes) {
    if (bytes <= cap) return GEMMA_HIP_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    if (hipMalloc(&p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      return GEMMA_HIP_ENOMEM;
    }
    cap = bytes;
    return GEMMA_HIP_OK;
  }
  // The same with the text of the refusal ("<who>: cannot allocate <bytes> bytes of device memory") and a floor under the
  // allocation: a request of zero bytes still leaves a pointer that kernels and copies may be handed.
  int reserve(size_t bytes, const char *who, std::string &msg, size_t min_bytes = 16) {
    const int rc = reserve(std::max(bytes, min_bytes));
    if (rc) msg = std::string(who) + ": cannot allocate " + std::to_string(bytes) + " bytes of device memory";
    return rc;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T> T *as() { return reinterpret_cast<T *>(p); }
};

struct ScopedBuf : DevBuf { // scratch of one call: released on every return path
  ScopedBuf() = default;
  ScopedBuf(const ScopedBuf &) = delete;
  ScopedBuf &operator=(const ScopedBuf &) = delete;
  ~ScopedBuf() { release(); }
};

inline int hip_err(hipError_t e, const char *what, std::string &msg) {
  msg = std::string(what) + ": " + hipGetErrorString(e);
  return GEMMA_HIP_ERUNTIME;
}
// in a function that returns a GEMMA_HIP_* code and has a std::string msg in scope
#define TU_CHK(expr)                                      \
  do {                                                    \
    hipError_t e_ = (expr);                               \
    if (e_ != hipSuccess) return hip_err(e_, #expr, msg); \
  } while (0)

// A block of host rows to the device: the row_bytes leading bytes of `rows` rows of pitch pitch_bytes, packed into buf on stream s
// (only these bytes of a host row are read: the caller's last row may end there).  src and ld (in elements of elem_bytes) then
// name the device copy.  buf grows through hipFree when it has to; a caller whose earlier asynchronous work may still read buf
// on another stream waits for that before the call.
inline int stage_rows(DevBuf &buf, const void *host, size_t rows, size_t row_bytes, size_t pitch_bytes, size_t elem_bytes, hipStream_t s,
                      const char *who, std::string &msg, const void *&src, long &ld) {
  const int rc = buf.reserve(rows * row_bytes, who, msg);
  if (rc) return rc;
  TU_CHK(hipMemcpy2DAsync(buf.p, row_bytes, host, pitch_bytes, row_bytes, rows, hipMemcpyHostToDevice, s));
  src = buf.p;
  ld = (long)(row_bytes / elem_bytes);
  return GEMMA_HIP_OK;
}

} // namespace gemma_hip
