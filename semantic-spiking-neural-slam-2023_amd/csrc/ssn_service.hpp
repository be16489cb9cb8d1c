// ssn_service.hpp - host plumbing of the off-step-path services (ssn_decode.hip, ssn_encode.hip, ssn_recall.hip; ssn_probe.hip for
// the declaration): errors reported through ssn_last_error, the device kept current for a call, the device check at creation.
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

}  // namespace svc
}  // namespace ssn
