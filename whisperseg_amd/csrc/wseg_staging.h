// A host table's way to the device without waiting for the stream (wseg_measure.hip, wseg_patch.hip, wseg_pitch.hip): the table
// arrives as a host array and the call must not synchronise, so it is written into a pinned buffer the library owns and copied
// from there on the stream; an event behind the copy says when the buffer is free again.  A call takes a free buffer that is large
// enough or makes a new one; the pool — one for the whole library — lives as long as the process.
#pragma once
#include <mutex>
#include <vector>
#include "wseg_common.h"

namespace wseg {

struct Staging {
  void* host;
  size_t cap;
  hipEvent_t done;
  int device;                                        // the event's
  bool taken;
};
inline std::mutex g_staging_mutex;
inline std::vector<Staging> g_staging;

inline int staging_take(size_t bytes, int* index, void** host) {
  int device = 0;
  WSEG_HIP_CHECK(hipGetDevice(&device));
  std::lock_guard<std::mutex> lock(g_staging_mutex);
  for (size_t i = 0; i < g_staging.size(); ++i) {
    Staging& s = g_staging[i];
    if (!s.taken && s.device == device && s.cap >= bytes && hipEventQuery(s.done) == hipSuccess) {
      s.taken = true;
      *index = (int)i;
      *host = s.host;
      return WSEG_OK;
    }
  }
  (void)hipGetLastError();                           // (hipErrorNotReady of a query is no error of this call)
  Staging s;
  s.cap = align_up(bytes, (size_t)65536);
  s.taken = true;
  s.device = device;
  WSEG_HIP_CHECK(hipHostMalloc(&s.host, s.cap, hipHostMallocDefault));
  hipError_t e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
  if (e != hipSuccess) {
    (void)hipHostFree(s.host);
    set_error("hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
    return WSEG_ERR_HIP;
  }
  g_staging.push_back(s);
  *index = (int)g_staging.size() - 1;
  *host = s.host;
  return WSEG_OK;
}

// `bytes` that fill(host pointer) writes into a pinned buffer, copied to the device pointer dst on the stream -> WSEG_OK, or the
// error with the calling function's name `fn` in wseg_last_error().
template <class Fill>
inline int staging_upload(size_t bytes, void* dst, hipStream_t stream, const char* fn, Fill fill) {
  int slot = -1;
  void* host = nullptr;
  if (const int rc = staging_take(bytes, &slot, &host)) return rc;
  fill(host);
  hipError_t e = hipMemcpyAsync(dst, host, bytes, hipMemcpyHostToDevice, stream);
  {                                                  // the event behind the copy frees the buffer (no copy was started: free at once)
    std::lock_guard<std::mutex> lock(g_staging_mutex);
    if (e == hipSuccess) e = hipEventRecord(g_staging[slot].done, stream);
    g_staging[slot].taken = false;
  }
  if (e != hipSuccess) { set_error("%s: the table's copy failed: %s", fn, hipGetErrorString(e)); return WSEG_ERR_HIP; }
  return WSEG_OK;
}

// pcm (float32 [n], may be null only when n == 0), out (float32) and scratch (8-byte aligned, at least `needed` bytes) of a call
// that has segments -> WSEG_OK, or WSEG_ERR_INVALID with the argument's name.
inline int device_buffers_check(const char* fn, const float* pcm, int64_t n, const float* out, const void* scratch, size_t scratch_bytes,
                                int64_t needed) {
  if ((n > 0 && !pcm) || ((uintptr_t)pcm & 3)) { set_error("%s: pcm must be a float32 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!out || ((uintptr_t)out & 3)) { set_error("%s: out must be a float32 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!scratch || ((uintptr_t)scratch & 7) || scratch_bytes < (size_t)needed) {
    set_error("%s: scratch must be an 8-byte aligned device buffer of at least %lld bytes (got %zu)", fn, (long long)needed, scratch_bytes);
    return WSEG_ERR_INVALID;
  }
  return WSEG_OK;
}

}  // namespace wseg
