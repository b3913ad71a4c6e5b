// Move-only owners of what a filter handle holds on the HIP side: device buffers, pinned blocks, events, the stream, and the "staged
// image" of the calls that do not wait for the device.  Each frees itself, so the handle needs no list of frees: deleting it (with its
// device current) releases everything, members in reverse order of declaration.  The owners convert to the raw pointer, so kernels'
// argument structs and the runtime's calls take them as they took the raw members.  What is allocated on demand goes through the one
// transaction of eqf_workspace_host.hpp; the owners only hand it their slots.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>
#include <utility>

#include "eqf_workspace_host.hpp"

namespace eqf {

namespace detail {
struct FreeDevice { static void free(void* p) { (void)hipFree(p); } };
struct FreePinned { static void free(void* p) { (void)hipHostFree(p); } };
struct FreeEvent { static void free(void* p) { (void)hipEventDestroy(static_cast<hipEvent_t>(p)); } };
struct FreeStream { static void free(void* p) { (void)hipStreamDestroy(static_cast<hipStream_t>(p)); } };

// the size of a raw pointer; P is the pointer (or handle) type
template <class P, class Free>
class Owner {
public:
    Owner() = default;
    Owner(Owner&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    Owner& operator=(Owner&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
        }
        return *this;
    }
    Owner(const Owner&) = delete;
    Owner& operator=(const Owner&) = delete;
    ~Owner() { reset(); }
    void reset() {
        if (p_) Free::free(p_);
        p_ = nullptr;
    }
    operator P() const { return p_; }
    // an untyped buffer is cast like the raw void* it stands for
    template <class U, class Q = P, class = std::enable_if_t<std::is_same<Q, void*>::value>>
    explicit operator U*() const { return static_cast<U*>(p_); }
    P get() const { return p_; }
    P* put() { return &p_; }  // (for the runtime's create calls: the owner must be empty)
    void** slot() { return reinterpret_cast<void**>(&p_); }

private:
    P p_ = nullptr;
};
}  // namespace detail

template <class T>
using DevPtr = detail::Owner<T*, detail::FreeDevice>;
using Event = detail::Owner<hipEvent_t, detail::FreeEvent>;
using Stream = detail::Owner<hipStream_t, detail::FreeStream>;
static_assert(sizeof(DevPtr<double>) == sizeof(double*) && sizeof(Event) == sizeof(hipEvent_t), "the owners are raw pointers in size");

// A pinned block; Mapped: it also keeps the device-side address of the block, for images a kernel reads directly.
template <class T, bool Mapped = false>
class PinnedPtr : public detail::Owner<T*, detail::FreePinned> {};
template <class T>
class PinnedPtr<T, true> : public detail::Owner<T*, detail::FreePinned> {
public:
    T* dev = nullptr;
    void** mapped() { return reinterpret_cast<void**>(&dev); }
};

// The operands of a call that does not wait: a pinned image the host fills, its device copy, and the event "the last upload from the
// pinned image has been read".  cap: what both images hold, in bytes.
template <bool Mapped = false>
struct StagedImage {
    PinnedPtr<char, Mapped> host;
    DevPtr<char> dev;
    Event read;
    std::size_t cap = 0;
    // wait until the pinned image may be written again
    hipError_t wait() const { return hipEventSynchronize(read); }
    hipError_t record(hipStream_t stream) const { return hipEventRecord(read, stream); }
    // upload bytes [off, off + bytes) on `stream` and record
    hipError_t upload(std::size_t bytes, hipStream_t stream, std::size_t off = 0) const {
        const hipError_t e = hipMemcpyAsync(dev.get() + off, host.get() + off, bytes, hipMemcpyHostToDevice, stream);
        return e != hipSuccess ? e : record(stream);
    }
};

}  // namespace eqf
