// Host plumbing around the HIP runtime, stated once for render_host.hip, tiles.hip, denoise.hip and display.hip: the error
// check, the device scope of an entry point, the device buffer a record keeps between calls, and the per-device record
// lookup.  Host-only: it needs <hip/hip_runtime_api.h> alone, so a plain C++ compiler builds it
// against stand-in definitions of the runtime calls (tests/hip_host_driver.cpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <memory>
#include <vector>

#include "scene.hpp"

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            set_error("HIP error %d (%s) at %s:%d: %s", (int)e_, hipGetErrorString(e_), __FILE__, __LINE__, #expr); \
            return RT_ERR_HIP;                                                                \
        }                                                                                     \
    } while (0)

namespace rtmi {

// The calling thread's device for the length of a scope: the caller's device comes back on every return path.
struct DeviceScope {
    int prev = -1;
    bool restore = false;
    // makes `device` the current one (a runtime call only if it is not); `who`: "the render path", "the denoiser", ...
    int enter(int device, const char *who) {
        int ndev = 0;
        HIP_TRY(hipGetDeviceCount(&ndev));
        if (ndev <= 0) {
            set_error("no HIP device visible: %s has no CPU fallback", who);
            return RT_ERR_HIP;
        }
        if (device < 0 || device >= ndev) {
            set_error("device %d out of range (%d visible)", device, ndev);
            return RT_ERR_ARG;
        }
        HIP_TRY(hipGetDevice(&prev));
        if (prev != device) {
            HIP_TRY(hipSetDevice(device));
            restore = true;
        }
        return RT_OK;
    }
    // for code that selects several devices itself: remembers the caller's device, which the scope's end selects again
    int save() {
        HIP_TRY(hipGetDevice(&prev));
        restore = true;
        return RT_OK;
    }
    ~DeviceScope() {
        if (restore) (void)hipSetDevice(prev);
    }
};

// A device buffer kept between calls that only grows: `capacity()` elements of T on the device that was current when it
// was allocated.  It owns the memory: release() and the destructor free it with that device current and leave the caller's
// device as it was.
template <class T>
class DeviceBuffer {
    T *ptr_ = nullptr;
    size_t cap_ = 0;
    int device_ = -1;

  public:
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    DeviceBuffer(DeviceBuffer &&o) noexcept : ptr_(o.ptr_), cap_(o.cap_), device_(o.device_) { o.ptr_ = nullptr, o.cap_ = 0; }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept {
        if (this != &o) {
            release();
            ptr_ = o.ptr_, cap_ = o.cap_, device_ = o.device_;
            o.ptr_ = nullptr, o.cap_ = 0;
        }
        return *this;
    }
    ~DeviceBuffer() { release(); }

    T *get() const { return ptr_; }
    size_t capacity() const { return cap_; }

    // room for at least n elements, on the current device (the buffer's own, if it has memory already).  No runtime call when
    // the capacity suffices; otherwise the old memory is freed first and the contents are gone.  A failed allocation leaves
    // the buffer empty, and a later call tries again.
    int reserve(size_t n) {
        if (cap_ >= n) return RT_OK;
        if (ptr_) HIP_TRY(hipFree(ptr_));
        ptr_ = nullptr, cap_ = 0;
        HIP_TRY(hipGetDevice(&device_));
        T *p = nullptr;
        HIP_TRY(hipMalloc((void **)&p, n * sizeof(T)));
        ptr_ = p, cap_ = n;
        return RT_OK;
    }

    void release() {
        if (ptr_) {
            int cur = -1;
            const bool have = hipGetDevice(&cur) == hipSuccess;
            if (cur == device_ || hipSetDevice(device_) == hipSuccess) (void)hipFree(ptr_);
            if (have && cur != device_) (void)hipSetDevice(cur);
        }
        ptr_ = nullptr, cap_ = 0;
    }
};

// the record of `device` in `list` (T has an int member `device`), created at its first use; under the list's lock
template <class T>
T *device_record(std::vector<std::unique_ptr<T>> &list, int device) {
    for (auto &r : list)
        if (r->device == device) return r.get();
    list.emplace_back(new T());
    list.back()->device = device;
    return list.back().get();
}

}  // namespace rtmi
