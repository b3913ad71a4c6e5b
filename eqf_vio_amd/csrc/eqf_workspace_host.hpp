// The one allocation transaction of a filter handle (standard library only; the HIP side -- the owners of what a handle holds and the
// backend that allocates -- is eqf_workspace.hpp / eqf_capi.hip; tests/workspace_host_main.cpp drives this header with a counting fake).
//
// A call names the slots it needs and how many bytes each must hold (Want).  reserve() keeps every slot that is there and large enough
// -- buffers only grow --, allocates everything that is missing or too small FIRST, and only then touches the handle:
//   * a failed allocation frees what this call got, clears the backend's error state and leaves every slot and capacity as it was;
//   * if a slot that already existed is being replaced, the stream is drained ONCE before anything old is freed (an earlier call that did
//     not wait may still use it); a failing drain is a failure like the others;
//   * then the old pieces are freed and the new ones installed together with their capacities.
// The result tells which wants were installed: a route that must initialise a new buffer (a zero fill) looks there.
#pragma once
#include <cstddef>

namespace eqf {
namespace workspace {

enum Piece { kDevice = 0, kPinned = 1, kEvent = 2 };

// One slot of a call.  `slot`: the raw pointer (or event handle) inside its owner.  `cap`: where the slot's capacity in bytes lives -- the
// slot is replaced when bytes > *cap; nullptr: the slot has one size for the handle's life and is allocated when it is missing.
// bytes == 0: not wanted by this call.  `mapped` (pinned only): where the device-side address of the block goes, for images a kernel reads.
struct Want {
    Piece piece;
    void** slot;
    std::size_t* cap;
    std::size_t bytes;
    void** mapped;
};
inline Want device(void** slot, std::size_t bytes, std::size_t* cap = nullptr) { return Want{kDevice, slot, cap, bytes, nullptr}; }
inline Want pinned(void** slot, std::size_t bytes, std::size_t* cap = nullptr, void** mapped = nullptr) {
    return Want{kPinned, slot, cap, bytes, mapped};
}
inline Want event(void** slot) { return Want{kEvent, slot, nullptr, 1, nullptr}; }

struct Result {
    bool ok;
    unsigned long long installed;  // bit i: want i was allocated by this call (new or replaced)
    bool has(int i) const { return (installed >> i) & 1ull; }
};

constexpr int kMaxWants = 64;

// Backend: void* allocDevice(size_t), void* allocPinned(size_t, void** mapped), void* allocEvent() (nullptr: failed);
// void freeDevice(void*), freePinned(void*), freeEvent(void*); bool drain(); void clearError().
template <class Backend>
Result reserve(Backend& be, const Want* w, int n) {
    void* fresh[kMaxWants];
    void* freshMapped[kMaxWants];
    unsigned long long need = 0;
    bool replaces = false;
    if (n > kMaxWants) return Result{false, 0};
    for (int i = 0; i < n; ++i) {
        const bool missing = w[i].cap ? w[i].bytes > *w[i].cap : (w[i].bytes > 0 && !*w[i].slot);
        if (!missing) continue;
        need |= 1ull << i;
        replaces = replaces || *w[i].slot != nullptr;
    }
    if (!need) return Result{true, 0};
    auto release = [&](Piece piece, void* p) {
        if (piece == kDevice) be.freeDevice(p);
        else if (piece == kPinned) be.freePinned(p);
        else be.freeEvent(p);
    };
    int got = 0;
    bool ok = true;
    for (; got < n && ok; ++got) {
        fresh[got] = freshMapped[got] = nullptr;
        if (!((need >> got) & 1ull)) continue;
        if (w[got].piece == kDevice) fresh[got] = be.allocDevice(w[got].bytes);
        else if (w[got].piece == kPinned) fresh[got] = be.allocPinned(w[got].bytes, w[got].mapped ? &freshMapped[got] : nullptr);
        else fresh[got] = be.allocEvent();
        ok = fresh[got] != nullptr;
    }
    if (ok && replaces) ok = be.drain();
    if (!ok) {
        for (int i = got - 1; i >= 0; --i)
            if (fresh[i]) release(w[i].piece, fresh[i]);
        be.clearError();
        return Result{false, 0};
    }
    for (int i = 0; i < n; ++i) {
        if (!((need >> i) & 1ull)) continue;
        if (*w[i].slot) release(w[i].piece, *w[i].slot);
        *w[i].slot = fresh[i];
        if (w[i].cap) *w[i].cap = w[i].bytes;
        if (w[i].mapped) *w[i].mapped = freshMapped[i];
    }
    return Result{true, need};
}
template <class Backend, int N>
Result reserve(Backend& be, const Want (&w)[N]) {
    static_assert(N <= kMaxWants, "more wants than a call may name");
    return reserve(be, w, N);
}

}  // namespace workspace
}  // namespace eqf
