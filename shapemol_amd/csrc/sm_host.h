// The error-and-device protocol of the library's host code (host only; included by every translation unit): a failure stores
// its message as the thread's last error (shapemol_last_error) and returns non-zero; a context opens its device when it is
// created and closes it before it is deleted.  The sampling translation unit owns the error string itself (g_err and fail of
// sm_pack.h); its HIPCHK is SMCHK under the name its call sites use.  Also `put`, with which a call builds the byte image of its
// one upload.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

extern "C" void shapemol_set_error_(const char *msg);     // shapemol_hip.hip: stores the thread's last error

namespace {

// appends `count` items to the host image of an upload -> their offset, 8-aligned
template <typename T> size_t put(std::vector<unsigned char> &img, const T *src, size_t count) {
    const size_t o = (img.size() + 7) / 8 * 8;
    img.resize(o + count * sizeof(T));
    if (count) std::memcpy(img.data() + o, src, count * sizeof(T));
    return o;
}

inline int sm_fail(const std::string &m) { shapemol_set_error_(m.c_str()); return 1; }

// return from the calling function with "<the call as written>: <HIP's error string>" when a HIP call fails
#define SMCHK(expr)                                                                          \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return sm_fail(std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// a *_create function's device: one of the machine's (else "<who>: no such HIP device"), made current
inline int sm_open_device(int device, const char *who) {
    int ndev = 0;
    SMCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return sm_fail(std::string(who) + ": no such HIP device");
    SMCHK(hipSetDevice(device));
    return 0;
}

// before a *_destroy function deletes its context: nothing on the device still uses the context's memory.  A destroy function
// has nobody to report to, so errors are dropped
inline void sm_close_device(int device) {
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
}

}  // namespace
