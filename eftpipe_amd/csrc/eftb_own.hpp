// eftb_own.hpp -- who frees what: an ordered list of (handle, releaser) pairs.  Everything an engine acquires (device and page-locked
// memory, events, streams: eftbird.hip's helpers beside HIPCHK) is held here the moment it exists, so a failing exit needs no clean-up of
// its own and eftb_destroy names no pointer.  The engine's pointer fields only view what the ledger owns: they are swapped and aliased
// freely.  No HIP include, so a host compiler alone builds it (tests/test_own_host.py runs tests/own_host_test.cpp under the address and
// undefined-behaviour sanitizers).
#pragma once

#include <cstddef>
#include <vector>

namespace eftb {

class Ledger {
public:
    using Releaser = void (*)(void*);
    using Mark = size_t;

    Ledger() = default;
    Ledger(const Ledger&) = delete;
    Ledger& operator=(const Ledger&) = delete;
    ~Ledger() { release_to(0); }  // everything, newest first

    void hold(void* handle, Releaser releaser) { held_.push_back(Held{handle, releaser}); }

    // runs the releaser of this one handle and forgets it; a null handle or one the ledger does not hold is a no-op
    void release(void* handle) {
        if (!handle) return;
        for (size_t i = held_.size(); i-- > 0;)
            if (held_[i].handle == handle) {
                const Held h = held_[i];
                held_.erase(held_.begin() + (std::ptrdiff_t)i);
                h.releaser(h.handle);
                return;
            }
    }

    // everything held since mark(), newest first.  A mark counts what is held: it stands while nothing held before it is released
    Mark mark() const { return held_.size(); }
    void release_to(Mark mark) {
        while (held_.size() > mark) {
            const Held h = held_.back();
            held_.pop_back();
            h.releaser(h.handle);
        }
    }

private:
    struct Held { void* handle; Releaser releaser; };
    std::vector<Held> held_;
};

}  // namespace eftb
