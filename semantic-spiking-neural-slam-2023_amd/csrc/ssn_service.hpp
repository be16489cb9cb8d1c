// ssn_service.hpp - host plumbing of the off-step-path services (ssn_decode.hip, ssn_encode.hip, ssn_bind.hip, ssn_recall.hip;
// ssn_probe.hip for the declaration): errors reported through ssn_last_error, the device kept current for a call, the device check
// at creation, and - for the three services that work on a stream of their own - the Lane they own (device, scratch area, stream,
// events), the staging of host rows and the entry check of a block of rows.  DESIGN.md 3.18; service.py is the Python half.
// Host code only.  ssn_host.hip owns the error string and keeps its own fail / HIPCHK, which add file and line.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include "../../include/ssn.h"

namespace ssn {

int probe_fail(int code, const char* what, hipError_t e);      // ssn_host.hip: sets ssn_last_error

namespace svc {

__attribute__((format(printf, 2, 3))) inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return probe_fail(code, buf, hipSuccess);
}

// returns from the calling function with the status of a failed HIP call; the message is the call's own text
#define SVC_HIP(expr)                                                                                   \
  do {                                                                                                  \
    hipError_t e__ = (expr);                                                                            \
    if (e__ != hipSuccess) return ssn::probe_fail(e__ == hipErrorOutOfMemory ? SSN_ENOMEM : SSN_EHIP, #expr, e__); \
  } while (0)

struct DevGuard {      // the service's device for the duration of a call, the caller's afterwards
  int prev = -1;
  explicit DevGuard(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; (void)hipSetDevice(dev); }
  ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// The device check of a *_create: SSN_EHIP without a usable HIP device; with `who`, SSN_EINVAL for a `device` the runtime does not
// have (who == nullptr: the device is not the caller's to choose, only the count is tested).
inline int check_device(const char* who, int device) {
  int ndev = 0;
  const hipError_t dev_err = hipGetDeviceCount(&ndev);
  if (dev_err != hipSuccess || ndev <= 0)
    return fail(SSN_EHIP, "no HIP device available (there is no CPU fallback): hipGetDeviceCount -> %s, %d devices", hipGetErrorString(dev_err), ndev);
  if (who && (device < 0 || device >= ndev)) return fail(SSN_EINVAL, "%s: device %d out of range (%d devices)", who, device, ndev);
  return SSN_OK;
}

// What a service works with beside its tables: its device, a scratch area fixed at creation, a stream and the events that time
// the kernels of a call.  ssn_decoder, ssn_encoder and ssn_binder derive from it; their own destructors free only their tables.
struct Lane {
  int device = 0;
  int64_t scratch_bytes = 0;
  char* scratch = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  int64_t launches = 0;      // of the last call

  // The tail of a *_create.  `asked` bytes of scratch, 0 for the default: 64 MB, or min_bytes when that is more.  The arguments are
  // judged before any HIP call - SSN_EINVAL for a negative size or one below min_bytes, which is one <unit_fmt, ...> ("row of d 97") -
  // then check_device, then the stream, the events and the scratch area are made.
  __attribute__((format(printf, 6, 7))) int open(const char* who, int dev, int64_t asked, int64_t min_bytes, const char* unit_fmt, ...) {
    if (asked < 0) return fail(SSN_EINVAL, "%s: negative scratch_bytes", who);
    if (asked && asked < min_bytes) {
      char unit[128];
      va_list ap;
      va_start(ap, unit_fmt);
      vsnprintf(unit, sizeof unit, unit_fmt, ap);
      va_end(ap);
      return fail(SSN_EINVAL, "%s: scratch_bytes %lld too small for one %s (%lld bytes)", who, (long long)asked, unit, (long long)min_bytes);
    }
    if (const int rc = check_device(who, dev)) return rc;
    device = dev;
    scratch_bytes = asked ? asked : (min_bytes > ((int64_t)64 << 20) ? min_bytes : (int64_t)64 << 20);
    DevGuard g(device);
    SVC_HIP(hipStreamCreate(&stream));
    for (hipEvent_t& e : ev) SVC_HIP(hipEventCreate(&e));
    SVC_HIP(hipMalloc((void**)&scratch, (size_t)scratch_bytes));
    return SSN_OK;
  }

  Lane() = default;
  Lane(const Lane&) = delete;
  Lane& operator=(const Lane&) = delete;
  ~Lane() {
    DevGuard g(device);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
    if (scratch) (void)hipFree(scratch);
  }
};

// the device milliseconds between two recorded events, complete by now, added to *acc
inline int elapsed(hipEvent_t a, hipEvent_t b, double* acc) {
  float ms = 0.0f;
  SVC_HIP(hipEventElapsedTime(&ms, a, b));
  *acc += ms;
  return SSN_OK;
}

// Host rows into a staging area on the device, on `stream`: `rows` rows of `width` elements of esz bytes, ld elements apart at
// src, dense at dst - one copy when they are dense at src too, a 2-D copy otherwise.
inline int stage_rows(hipStream_t stream, void* dst, const void* src, int64_t ld, int64_t width, size_t esz, int64_t rows) {
  if (ld == width) SVC_HIP(hipMemcpyAsync(dst, src, (size_t)rows * width * esz, hipMemcpyHostToDevice, stream));
  else SVC_HIP(hipMemcpy2DAsync(dst, (size_t)width * esz, src, (size_t)ld * esz, (size_t)width * esz, (size_t)rows, hipMemcpyHostToDevice, stream));
  return SSN_OK;
}

// The entry check of a block of rows, the argument <what>_dtype / <what>_ld of `who`: SSN_EINVAL for a dtype that is neither
// SSN_F32 nor SSN_F64 and for a leading dimension below the width.  `of` (" of the rows") and `width_name` word the second message.
inline int check_rows(const char* who, const char* what, int dtype, int64_t ld, int64_t width, const char* of = "", const char* width_name = "the width") {
  if (dtype != SSN_F32 && dtype != SSN_F64) return fail(SSN_EINVAL, "%s: unknown %s_dtype %d", who, what, dtype);
  if (ld < width) return fail(SSN_EINVAL, "%s: leading dimension %lld%s below %s %lld", who, (long long)ld, of, width_name, (long long)width);
  return SSN_OK;
}

}  // namespace svc
}  // namespace ssn
