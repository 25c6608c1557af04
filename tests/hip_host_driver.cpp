// csrc/hip_host.h under AddressSanitizer + UBSan without a GPU: this program defines the few HIP runtime calls the header
// makes as a fake with two devices (hipMalloc is malloc and remembers the device; hipFree insists on that device) and
// drives the failure paths no GPU test reaches.  Built and run by tests/test_sanitize.py; no HIP runtime is linked.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <utility>
#include <vector>

#include "../ray-tracing-in-cuda_amd/csrc/hip_host.h"

using namespace rtmi;

// ---- the fake runtime
static int f_devices = 2, f_current = 0;
static bool f_fail_malloc = false;      // the next hipMalloc fails (once)
static std::map<void *, int> f_live;    // allocation -> the device it was made on
static int f_mallocs = 0, f_frees = 0, f_sets = 0, f_calls = 0;

extern "C" {
hipError_t hipGetDeviceCount(int *n) {
    ++f_calls;
    *n = f_devices;
    return hipSuccess;
}
hipError_t hipGetDevice(int *d) {
    ++f_calls;
    *d = f_current;
    return hipSuccess;
}
hipError_t hipSetDevice(int d) {
    ++f_calls, ++f_sets;
    if (d < 0 || d >= f_devices) return hipErrorInvalidDevice;
    f_current = d;
    return hipSuccess;
}
hipError_t hipMalloc(void **p, size_t bytes) {
    ++f_calls;
    if (f_fail_malloc) {
        f_fail_malloc = false;
        return hipErrorOutOfMemory;
    }
    *p = malloc(bytes ? bytes : 1);
    f_live[*p] = f_current;
    ++f_mallocs;
    return hipSuccess;
}
hipError_t hipFree(void *p) {
    ++f_calls;
    auto it = f_live.find(p);
    if (it == f_live.end()) return hipErrorInvalidValue;  // (a double free, or a pointer that is not ours)
    if (it->second != f_current) {
        fprintf(stderr, "hipFree with device %d current of memory allocated on device %d\n", f_current, it->second);
        abort();
    }
    f_live.erase(it);
    free(p);
    ++f_frees;
    return hipSuccess;
}
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "fake HIP error"; }
}

#define CHECK(c)                                                                                \
    do {                                                                                        \
        if (!(c)) {                                                                             \
            fprintf(stderr, "CHECK failed line %d: %s (%s)\n", __LINE__, #c, get_error());      \
            return 1;                                                                           \
        }                                                                                       \
    } while (0)

static bool error_has(const char *what) { return strstr(get_error(), what) != nullptr; }

// an entry point that returns early inside its scope
static int early_return(int device, bool fail) {
    DeviceScope scope;
    int rc = scope.enter(device, "the denoiser");
    if (rc) return rc;
    if (f_current != device) return -1;
    if (fail) return RT_ERR_LIMIT;
    return RT_OK;
}

struct Record {
    int device = -1;
    DeviceBuffer<float> buf;
};

static int run() {
    // ---- the kept buffer
    {
        DeviceBuffer<float> b;
        CHECK(b.get() == nullptr && b.capacity() == 0);
        int calls = f_calls;
        CHECK(b.reserve(0) == RT_OK && f_calls == calls && b.get() == nullptr);  // nothing asked, nothing done
        CHECK(b.reserve(100) == RT_OK && b.get() && b.capacity() == 100 && f_mallocs == 1);
        b.get()[99] = 1.0f;  // (the sanitizer checks the size)
        float *p = b.get();
        calls = f_calls;
        CHECK(b.reserve(100) == RT_OK && b.reserve(7) == RT_OK && b.get() == p && b.capacity() == 100);
        CHECK(f_calls == calls);  // the steady state makes no runtime call
        CHECK(b.reserve(101) == RT_OK && b.capacity() == 101 && f_mallocs == 2 && f_frees == 1 && f_live.size() == 1);
        b.get()[100] = 1.0f;
        // a failed allocation: the buffer is empty, the message names the call, the next call tries again
        f_fail_malloc = true;
        CHECK(b.reserve(1000) == RT_ERR_HIP);
        CHECK(b.get() == nullptr && b.capacity() == 0 && f_live.empty() && f_frees == 2);
        CHECK(error_has("hipMalloc") && error_has("out of memory") && error_has("hip_host.h"));
        CHECK(b.reserve(10) == RT_OK && b.get() && b.capacity() == 10 && f_mallocs == 3);
        // release: one free; a second release and the destructor free nothing
        b.release();
        CHECK(b.get() == nullptr && b.capacity() == 0 && f_frees == 3);
        b.release();
        CHECK(f_frees == 3);
    }
    CHECK(f_frees == 3 && f_live.empty());
    // ---- freed under the allocating device, the caller's device restored
    {
        DeviceBuffer<int> on1, moved_to;
        {
            DeviceScope scope;
            CHECK(scope.enter(1, "the render path") == RT_OK && f_current == 1);
            CHECK(on1.reserve(4) == RT_OK);
        }
        CHECK(f_current == 0 && f_live.begin()->second == 1);
        int frees = f_frees;
        on1.release();  // (device 0 is current)
        CHECK(f_frees == frees + 1 && f_current == 0);
        {
            DeviceScope scope;
            CHECK(scope.enter(1, "the render path") == RT_OK);
            CHECK(on1.reserve(4) == RT_OK);
        }
        frees = f_frees;
        {
            DeviceBuffer<int> dies_here(std::move(on1));  // a moved-from buffer owns nothing
            CHECK(on1.get() == nullptr && on1.capacity() == 0 && dies_here.capacity() == 4);
            moved_to = std::move(dies_here);
            CHECK(dies_here.get() == nullptr && moved_to.capacity() == 4);
        }
        CHECK(f_frees == frees && f_live.size() == 1);
        on1.release();
        CHECK(f_frees == frees);
        {
            DeviceBuffer<int> other;
            CHECK(other.reserve(2) == RT_OK);  // on device 0
            moved_to = std::move(other);       // the assignment frees what the target held, on device 1
            CHECK(f_frees == frees + 1 && f_current == 0 && f_live.begin()->second == 0);
        }
        CHECK(f_frees == frees + 1);
    }  // moved_to's destructor: the one free left
    CHECK(f_live.empty() && f_mallocs == f_frees && f_current == 0);

    // ---- the device scope
    {
        int sets = f_sets;
        CHECK(early_return(0, false) == RT_OK && f_sets == sets);  // the current device: never selected
        CHECK(early_return(1, false) == RT_OK && f_sets == sets + 2 && f_current == 0);
        CHECK(early_return(1, true) == RT_ERR_LIMIT && f_sets == sets + 4 && f_current == 0);
        sets = f_sets;
        CHECK(early_return(-1, false) == RT_ERR_ARG && error_has("device -1 out of range (2 visible)"));
        CHECK(early_return(2, false) == RT_ERR_ARG && error_has("device 2 out of range (2 visible)"));
        CHECK(f_sets == sets && f_current == 0);
        f_devices = 0;
        CHECK(early_return(0, false) == RT_ERR_HIP);
        CHECK(strcmp(get_error(), "no HIP device visible: the denoiser has no CPU fallback") == 0);
        f_devices = 2;
        CHECK(f_sets == sets && f_current == 0);
        {  // save(): whatever the code selects, the caller's device comes back
            f_current = 1;
            {
                DeviceScope scope;
                CHECK(scope.save() == RT_OK);
                CHECK(hipSetDevice(0) == hipSuccess);
            }
            CHECK(f_current == 1);
            f_current = 0;
        }
    }

    // ---- the per-device record
    {
        std::vector<std::unique_ptr<Record>> list;
        Record *r0 = device_record(list, 0), *r1 = device_record(list, 1);
        CHECK(r0 && r1 && r0 != r1 && r0->device == 0 && r1->device == 1 && list.size() == 2);
        CHECK(device_record(list, 0) == r0 && device_record(list, 1) == r1 && list.size() == 2);
        // records that own buffers on their devices: destroying the list frees each under its own device
        for (Record *r : {r0, r1}) {
            DeviceScope scope;
            CHECK(scope.enter(r->device, "the render path") == RT_OK);
            CHECK(r->buf.reserve(16) == RT_OK);
        }
        CHECK(f_live.size() == 2);
    }
    CHECK(f_live.empty() && f_mallocs == f_frees && f_current == 0);
    return 0;
}

int main() {
    if (run()) return 1;
    printf("hip_host driver ok: %d allocations, %d frees, %d live\n", f_mallocs, f_frees, (int)f_live.size());
    return f_live.empty() ? 0 : 1;
}
