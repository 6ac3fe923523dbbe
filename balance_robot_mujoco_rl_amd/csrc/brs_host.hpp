// brs_host.hpp -- the host-side plumbing the four translation units of libbrs_hip.so share: device guard, error slots, device
// check, and what more than one unit asks about a variant.  Host code only (no kernel, no __device__ function), so it stays
// out of the build id, which names the device code a profile was measured on.
//
// The rule for every entry point that touches the device: construct a DeviceGuard on the handle's device first, and if `!g.ok`
// return BRS_ERR_HIP with "<function>: hipSetDevice failed" -- never launch or copy on whatever device happens to be current.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/brs.h"

namespace brs::host {

// makes `dev` current for the scope and restores the caller's device afterwards
struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard&) = delete;
};

// error text of the calls of handle family H that have no handle (a failed create): one slot per family and thread
template <class H> std::string& no_handle_error() { thread_local std::string slot; return slot; }
// records `msg` in the handle (any type with a std::string err), or in its family's slot if h is null; returns `code`
template <class H> int fail(H* h, int code, const std::string& msg) { (h ? h->err : no_handle_error<H>()) = msg; return code; }
template <class H> const char* last_error(const H* h) { return (h ? h->err : no_handle_error<H>()).c_str(); }

#define BRS_HIP_TRY(h, expr)                                                                                          \
  do {                                                                                                                \
    hipError_t e_ = (expr);                                                                                           \
    if (e_ != hipSuccess) return brs::host::fail(h, BRS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// The handle-dependent half of an entry point, after the argument checks that need no handle: the null handle, what the call needs
// of its handle -- `needs(h)` returns nullptr or the text that follows "<who>: " --, the device guard, `launch()`, which enqueues on
// the caller's stream, and hipGetLastError.  The checks run in this order, which is part of the ABI.
template <class H, class Needs, class Launch> int launch_on(H* h, const char* who, Needs&& needs, Launch&& launch) {
  // (a text is put together only where a check fails: a call that succeeds allocates nothing)
  if (!h) return fail(h, BRS_ERR_ARG, std::string(who) + ": null handle");
  if (const char* why = needs(h)) return fail(h, BRS_ERR_ARG, std::string(who) + ": " + why);
  DeviceGuard g(h->device);
  if (!g.ok) return fail(h, BRS_ERR_HIP, std::string(who) + ": hipSetDevice failed");
  launch();
  BRS_HIP_TRY(h, hipGetLastError());
  return BRS_OK;
}
// a call that needs nothing of its handle but its device
inline const char* needs_nothing(const void*) { return nullptr; }
// the DDPG / TD3 calls exist at the reference widths only (h->arch: a BRS_ARCH_* of include/brs_policy.h): nullptr, or what launch_on says
#define BRS_REFERENCE_ARCH_ONLY(h) \
  ((h)->arch != BRS_ARCH_REFERENCE ? "the handle's architecture does not serve this call (DDPG and TD3 run at BRS_ARCH_REFERENCE only)" : nullptr)

// BRS_OK if `device` is an ordinal of this machine; otherwise the code to return and, in *msg, the text for `who`
inline int check_device(int device, const char* who, std::string* msg) {
  int ndev = 0;
  const hipError_t e = hipGetDeviceCount(&ndev);
  const bool none = e != hipSuccess || ndev <= 0;
  if (none) *msg = std::string(who) + ": no HIP device (" + hipGetErrorString(e) + "); there is no CPU fallback";
  else if (device < 0 || device >= ndev) *msg = std::string(who) + ": device ordinal out of range";
  else return BRS_OK;
  return none ? BRS_ERR_HIP : BRS_ERR_ARG;
}

inline bool known_variant(int variant) { return variant >= BRS_ENV01_V1 && variant <= BRS_ENV02_V1; }
// the Env03 family: a free block next to the robot (16 / 14 coordinates instead of 9 / 8; brs_sizes has the numbers)
inline bool has_block(int variant) { return variant == BRS_ENV03_V1 || variant == BRS_ENV03_V2; }

}  // namespace brs::host
