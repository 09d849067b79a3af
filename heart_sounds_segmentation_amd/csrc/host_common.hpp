// host_common.hpp -- what the host side of every unit of libhssfsst.so shares: the thread's error text and fail(), the HIP error
// macros, the device scope, the once-per-kernel LDS limit and the owners of device and pinned buffers.  No kernel here.  Everything lives in a namespace
// with hidden visibility: none of it is in the library's dynamic symbol table, and the error text is ONE variable for all units
// (an inline thread_local: hssfsst_last_error() of hssfsst.hip returns what fail() wrote in any other unit).
#pragma once

#include "../../include/hssfsst.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <new>
#include <vector>

#include "fsst_launch_shape.hpp"                          // kMaxLdsBytes (host arithmetic only)

namespace hssfsst {
namespace host __attribute__((visibility("hidden"))) {

inline thread_local char g_err[512] = "";

inline int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return ::hssfsst::host::fail(HSSFSST_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                   \
    } while (0)

// behind a kernel launch of the entry point `entry`
inline int launch_check(const char* entry, const char* what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(HSSFSST_EHIP, "%s: launch of %s failed: %s", entry, what, hipGetErrorString(e));
    return 0;
}

// Makes `device` current for the scope and restores the caller's device on every exit path (a process
// that drives several GPUs must not find its current HIP device changed by a library call).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device)
    {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) {
            err = hipSetDevice(device);
            switched = (err == hipSuccess);
        }
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define DEVICE_SCOPE(dev)                                                                      \
    ::hssfsst::host::DeviceGuard device_guard_(dev);                                           \
    if (device_guard_.err != hipSuccess)                                                       \
        return ::hssfsst::host::fail(HSSFSST_EHIP, "selecting device %d failed: %s", (dev), hipGetErrorString(device_guard_.err))

// the plan creates' device argument: a HIP device must exist (this library has no CPU path) and `device` must be one
inline int check_device(const char* what, int device)
{
    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(HSSFSST_ENODEVICE, "%s: no HIP device (%s); this library has no CPU path", what,
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    }
    if (device < 0 || device >= ndev) return fail(HSSFSST_EINVAL, "%s: device %d out of range [0,%d)", what, device, ndev);
    return 0;
}

// The dynamic-LDS limit is a property of the kernel instantiation (per device), not of a plan: raise it ONCE to
// the full 160 KiB, so that plans with different band widths sharing an instantiation cannot lower it under each
// other and the hot path makes no driver call for it.
template <class Kern>
int allow_full_lds(Kern kern, int device, std::atomic<unsigned long long>& done)
{
    const unsigned long long bit = 1ull << (device & 63);
    if (done.load(std::memory_order_acquire) & bit) return 0;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes));
    done.fetch_or(bit, std::memory_order_release);
    return 0;
}

// A plan's device buffer: capacity in elements of T; grow() frees the old block and allocates a larger one (contents are not
// kept), upload() makes a fresh block holding a host table.  Freed with its owner.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    T* get() const { return p; }
    int grow(size_t need)
    {
        if (need <= cap) return 0;
        if (p) { HIP_TRY(hipFree(p)); p = nullptr; cap = 0; }
        void* v = nullptr;
        const hipError_t e = hipMalloc(&v, need * sizeof(T));
        if (e != hipSuccess) return fail(HSSFSST_ENOMEM, "hipMalloc(%zu B): %s", need * sizeof(T), hipGetErrorString(e));
        p = static_cast<T*>(v);
        cap = need;
        return 0;
    }
    int upload(const T* host, size_t n)                 // (into an empty or smaller buffer: grow() makes it fresh)
    {
        if (int rc = grow(n)) return rc;
        HIP_TRY(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
        return 0;
    }
};

// A plan's pinned host buffer.  Mapped (the staging of small execs, the lent pool): hipHostMallocMapped with its device alias d,
// a power of two from 4096 elements; otherwise default flags, no alias, 1.5x what is needed.  Capacity in elements of es bytes.
template <class T>
struct PinnedBuf {
    T* h = nullptr;
    T* d = nullptr;
    size_t cap = 0;
    bool mapped = true;
    PinnedBuf() = default;
    explicit PinnedBuf(bool mapped_) : mapped(mapped_) {}
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { if (h) (void)hipHostFree(h); }
    int grow(size_t need, size_t es)
    {
        if (need <= cap) return 0;
        if (h) { HIP_TRY(hipHostFree(h)); h = nullptr; d = nullptr; cap = 0; }
        size_t c = need + need / 2;
        if (mapped) for (c = size_t(1) << 12; c < need; c *= 2) {}
        void* hp = nullptr;
        HIP_TRY(hipHostMalloc(&hp, c * es, mapped ? hipHostMallocMapped : hipHostMallocDefault));
        void* dp = nullptr;
        const hipError_t e = mapped ? hipHostGetDevicePointer(&dp, hp, 0) : hipSuccess;
        if (e != hipSuccess) {
            (void)hipHostFree(hp);
            return fail(HSSFSST_EHIP, "hipHostGetDevicePointer: %s", hipGetErrorString(e));
        }
        h = static_cast<T*>(hp); d = static_cast<T*>(dp); cap = c;
        return 0;
    }
};

// A table that is made on the host for a list and read on the device: a ring of kRing pinned (not mapped) host blocks, a device
// block, per host block the event of its last upload (a host block is not rewritten before that copy is done) and the key of the
// list the device block holds.
//   if (!t.same(n, key)) { t.begin(bytes, &h); ...fill h...; t.commit(stream, n, key); }     key(i): the i-th of n 64-bit words
// begin() drops the key first and commit() stores it last, behind the queued copy: whatever fails in between, the next call with
// the same list makes the table again.  A user without a key (n = 0) uploads at every call.  `what`: the entry point, for errors.
// Why a ring: with ONE host block a call whose list differs from the previous call's had to wait on the host for the previous
// upload, i.e. for everything queued on the stream before it -- a caller that walks groups of a long list (HipSegmenter.ragged
// with max_steps) behind other work stalled at its second group.  With the ring only the upload kRing list changes back is waited
// for.  The device block is one: the uploads and the kernels that read it are ordered by the plan's one stream.
struct UploadedTable {
    static constexpr int kRing = 4;
    const char* what;
    PinnedBuf<unsigned char> h[kRing];
    DevBuf<unsigned char> d;
    hipEvent_t ev[kRing] = {};
    int cur = 0;
    std::vector<int64_t> key;
    size_t bytes = 0;
    explicit UploadedTable(const char* what_) : what(what_) { for (auto& b : h) b.mapped = false; }
    UploadedTable(const UploadedTable&) = delete;
    UploadedTable& operator=(const UploadedTable&) = delete;
    ~UploadedTable() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    const unsigned char* get() const { return d.get(); }
    template <class Key>
    bool same(size_t n, Key&& at) const
    {
        if (key.empty() || key.size() != n) return false;
        for (size_t i = 0; i < n; ++i) if (key[i] != at(i)) return false;
        return true;
    }
    int begin(size_t nbytes, unsigned char** host)
    {
        key.clear();
        cur = (cur + 1) % kRing;
        if (ev[cur]) HIP_TRY(hipEventSynchronize(ev[cur]));  // (the upload kRing changes back may still read this host block)
        if (int rc = h[cur].grow(nbytes, 1)) return rc;
        if (int rc = d.grow(nbytes)) return rc;
        bytes = nbytes;
        *host = h[cur].h;
        return 0;
    }
    template <class Key>
    int commit(hipStream_t st, size_t n, Key&& at)
    {
        if (!ev[cur]) HIP_TRY(hipEventCreateWithFlags(&ev[cur], hipEventDisableTiming));
        HIP_TRY(hipMemcpyAsync(d.get(), h[cur].h, bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(ev[cur], st));
        try {
            key.resize(n);
        } catch (const std::bad_alloc&) {
            return fail(HSSFSST_ENOMEM, "%s: out of host memory", what);
        }
        for (size_t i = 0; i < n; ++i) key[i] = at(i);
        return 0;
    }
    int commit(hipStream_t st) { return commit(st, 0, [](size_t) { return int64_t(0); }); }
};

}  // namespace host
}  // namespace hssfsst
