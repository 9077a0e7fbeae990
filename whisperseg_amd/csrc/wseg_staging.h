// A host table's way to the device without waiting for the stream (wseg_measure.hip, wseg_patch.hip): the table arrives as a host
// array and the call must not synchronise, so it is written into a pinned buffer the library owns and copied from there on the
// stream; an event behind the copy says when the buffer is free again.  A call takes a free buffer that is large enough or makes
// a new one; the pool — one for the whole library — lives as long as the process.
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

inline int staging_take(size_t bytes, int* index) {
  int device = 0;
  WSEG_HIP_CHECK(hipGetDevice(&device));
  std::lock_guard<std::mutex> lock(g_staging_mutex);
  for (size_t i = 0; i < g_staging.size(); ++i) {
    Staging& s = g_staging[i];
    if (!s.taken && s.device == device && s.cap >= bytes && hipEventQuery(s.done) == hipSuccess) {
      s.taken = true;
      *index = (int)i;
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
  return WSEG_OK;
}
inline void* staging_host(int index) {
  std::lock_guard<std::mutex> lock(g_staging_mutex);
  return g_staging[index].host;
}
// Records the event behind the copy (enqueued == false: no copy was started, the buffer is free at once) and gives the buffer back.
inline hipError_t staging_release(int index, hipStream_t stream, bool enqueued) {
  std::lock_guard<std::mutex> lock(g_staging_mutex);
  Staging& s = g_staging[index];
  const hipError_t e = enqueued ? hipEventRecord(s.done, stream) : hipSuccess;
  s.taken = false;
  return e;
}

}  // namespace wseg
