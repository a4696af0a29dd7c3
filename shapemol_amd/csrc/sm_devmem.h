// The one place of the library that allocates and frees device memory (host only; included by every translation unit).
// Invariant: a capacity is non-zero only while every pointer of its group is valid; a failed growth leaves capacity 0 and
// null pointers; destroy frees through the same lists growth uses.  Errors come back as hipError_t for the caller's
// SMCHK (sm_host.h).  The raw operations are the four dm_* functions; a host test defines SM_DEVMEM_STUB and supplies its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <vector>

namespace {

#ifndef SM_DEVMEM_STUB
inline hipError_t dm_malloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
inline hipError_t dm_free(void *p) { return hipFree(p); }
inline hipError_t dm_zero(void *p, size_t bytes) { return hipMemset(p, 0, bytes); }
inline hipError_t dm_sync() { return hipDeviceSynchronize(); }
#endif

// one buffer of a group: the owner's pointer, its size, whether it is zero-filled
struct DevBuf { void **p; size_t bytes; bool zero; };
template <typename T> DevBuf dev_buf(T **p, size_t bytes, bool zero = false) { return {reinterpret_cast<void **>(p), bytes, zero}; }

// Owner of a group of buffers that are freed together.  It keeps the addresses of the owners' pointers: release() frees the
// buffers AND nulls those pointers, a failed alloc() releases the whole list, and a list that goes away releases
struct DevList {
    std::vector<void **> owned;       // the owners' pointers, each to a live buffer of this list
    size_t pad = 0;                   // bytes behind every buffer (allocated, and zeroed with it)
    explicit DevList(size_t pad_bytes = 0) : pad(pad_bytes) {}
    DevList(const DevList &) = delete; DevList &operator=(const DevList &) = delete;
    ~DevList() { release(); }
    // a new buffer for *b.p (null or stale on entry, and not yet in the list); on a failure the whole list is released
    hipError_t alloc(const DevBuf &b) {
        void *q = nullptr;
        hipError_t e = dm_malloc(&q, b.bytes + pad);
        if (e == hipSuccess && b.zero && (e = dm_zero(q, b.bytes + pad)) != hipSuccess) (void)dm_free(q);
        if (e != hipSuccess) { release(); return e; }
        *b.p = q;
        owned.push_back(b.p);
        return hipSuccess;
    }
    template <typename T> hipError_t alloc(T **p, size_t bytes, bool zero = false) { return alloc(dev_buf(p, bytes, zero)); }

    void release() {
        for (void **p : owned) { (void)dm_free(*p); *p = nullptr; }
        owned.clear();
    }
};

// The buffers `bufs` (all of `list`, sizes given for `need`) share the capacity `cap`: nothing when they hold `need`, else new
// ones behind a device synchronise -- a kernel in flight may still use the old.  A capacity only grows.  While the buffers are
// gone the capacity is 0 and the pointers are null, so after a failed malloc the next call grows again.  What else a growth
// invalidates (captured graphs, identities) is the caller's to drop first.
inline hipError_t grow(DevList &list, std::initializer_list<DevBuf> bufs, int64_t &cap, int64_t need) {
    if (need <= cap) return hipSuccess;
    hipError_t e = dm_sync();
    if (e != hipSuccess) return e;
    list.release();
    cap = 0;
    for (const DevBuf &b : bufs)
        if ((e = list.alloc(b)) != hipSuccess) return e;
    cap = need;
    return hipSuccess;
}

}  // namespace
