// dsi_owned.hpp -- move-only owners of the HIP resources the host layer holds: device memory, page-locked host
// memory, events and streams.  Each frees what it holds in its destructor, so an object struct of dsi_engine.cpp
// lists a resource once, as a member, and `delete obj` releases it.
//
// Host code only: nothing but the HIP runtime API and the standard library (tests/cpp/test_owned.cpp compiles this
// header with a plain host compiler against counting fakes of the eight runtime calls used below).
//
// No owner may have static or thread storage duration: its destructor would run after the HIP runtime has been torn
// down at process exit.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>

namespace dsi {

// device buffer that only ever grows
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;  // elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t reserve(size_t n)
    {
        if (n <= cap) return hipSuccess;
        if (p) {
            hipError_t e = hipFree(p);  // implicit device sync
            p = nullptr;
            cap = 0;
            if (e != hipSuccess) return e;
        }
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T));
        if (e == hipSuccess)
            cap = n;
        else
            p = nullptr;
        return e;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// one handle `h` and the runtime call that gives it back; converts to the handle, so that it goes wherever the
// runtime or a launch wrapper takes one
template <typename H, typename Arg, hipError_t (*Destroy)(Arg)>
struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    Owned(Owned&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Owned& operator=(Owned&& o) noexcept
    {
        if (this != &o) {
            release();
            h = std::exchange(o.h, nullptr);
        }
        return *this;
    }
    ~Owned() { release(); }
    void release()
    {
        if (h) (void)Destroy(h);
        h = nullptr;
    }
    operator H() const { return h; }
};

// The flags stay where the handle is made (hipEventDisableTiming, hipEventReleaseToSystem, hipStreamNonBlocking):
// these two only own.
struct Event : Owned<hipEvent_t, hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags)
    {
        release();
        hipError_t e = hipEventCreateWithFlags(&h, flags);
        if (e != hipSuccess) h = nullptr;
        return e;
    }
};

struct Stream : Owned<hipStream_t, hipStream_t, hipStreamDestroy> {
    hipError_t create(unsigned flags)
    {
        release();
        hipError_t e = hipStreamCreateWithFlags(&h, flags);
        if (e != hipSuccess) h = nullptr;
        return e;
    }
};

// page-locked host memory
template <typename T>
struct HostPinned : Owned<T*, void*, hipHostFree> {
    hipError_t alloc(size_t n, unsigned flags)
    {
        this->release();
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&this->h), n * sizeof(T), flags);
        if (e != hipSuccess) this->h = nullptr;
        return e;
    }
};

}  // namespace dsi
