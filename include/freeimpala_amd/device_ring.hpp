// device_ring.hpp -- C++ host side of the device entry ring (include/fi_ring.h).
//
// The reference's SharedBuffer in device memory: recording DeviceActors push their completed
// unrolls into a DeviceRing, and a learner handle on the same device steps from it -- FIFO
// (n_fresh = batch: SharedBuffer::readBatch) or with part of the batch replayed from the entries
// read before that are still resident. Failures never throw: a call returns false (step_ring: the
// status code) and last_error() / fi_last_error() holds the message. Construction throws
// std::runtime_error. One thread at a time per DeviceRing.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "device_actor.hpp"
#include "fi_ring.h"

namespace freeimpala_amd {

class DeviceRing {
public:
    DeviceRing(size_t entry_bytes, int64_t capacity, uint64_t seed = 0, int device = 0) {
        if (fi_ring_create(device, entry_bytes, capacity, seed, &h_) != FI_OK)
            throw std::runtime_error(std::string("fi_ring_create: ") + fi_last_error());
    }
    ~DeviceRing() { fi_ring_destroy(h_); }
    DeviceRing(const DeviceRing&) = delete;
    DeviceRing& operator=(const DeviceRing&) = delete;

    const std::string& last_error() const { return err_; }
    fi_ring* handle() { return h_; }

    fi_ring_state info() const {
        fi_ring_state s{};
        (void)fi_ring_info(h_, &s);
        return s;
    }
    bool seed(uint64_t seed, uint64_t draw = 0) { return ok(fi_ring_seed(h_, seed, draw)); }
    // n entries in device memory, entry_stride apart, once ready_event (hipEvent_t or null) has completed
    bool push(const void* entries_dev, size_t entry_stride, int32_t n, void* ready_event = nullptr) {
        return ok(fi_ring_push(h_, entries_dev, entry_stride, n, ready_event));
    }
    // acquire the actor's completed unroll, push it, release it: false when none waits or the ring is full
    bool push_rollout(DeviceActor& actor) { return ok(fi_ring_push_rollout(h_, actor.handle())); }
    void* pushed_event() { return fi_ring_pushed_event(h_); }
    void* stream() { return fi_ring_stream(h_); }
    bool read_slots(int64_t first_slot, int32_t n, std::vector<uint8_t>& out) {
        out.resize((size_t)(n > 0 ? n : 0) * info().entry_bytes);
        return ok(fi_ring_read_slots(h_, first_slot, n, out.data(), out.size()));
    }
    // the entry indices the last step_ring chose, column by column (batch: that learner's)
    bool last_entries(int32_t batch, std::vector<uint64_t>& out) {
        out.resize((size_t)(batch > 0 ? batch : 0));
        return ok(fi_ring_last_entries(h_, out.data(), batch));
    }

private:
    bool ok(int rc) {
        if (rc == FI_OK) return true;
        err_ = fi_last_error();
        return false;
    }

    fi_ring* h_ = nullptr;
    std::string err_;
};

// One learner step from the ring: columns [0, n_fresh) take the oldest unread entries, the others
// are replayed. The status is fi_learner_step_ring's.
inline int step_ring(fi_learner* learner, DeviceRing& ring, int32_t n_fresh, fi_step_stats* stats) {
    return fi_learner_step_ring(learner, ring.handle(), n_fresh, stats);
}

// Philox4x32-10, first word: key = seed, counter = {e low, e high, stream, 0}
inline uint32_t philox4_first(uint64_t seed, uint64_t e, uint32_t stream) {
    uint32_t c0 = (uint32_t)e, c1 = (uint32_t)(e >> 32), c2 = stream, c3 = 0u;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0;
        c1 = (uint32_t)p1;
        c2 = n2;
        c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// The batch rule on the host (include/fi_ring.h), from the ring's numbers before the step; empty
// when the step would be refused.
inline std::vector<uint64_t> ring_batch_entries(const fi_ring_state& s, int32_t batch, int32_t n_fresh) {
    const uint64_t lo = s.head > s.capacity ? s.head - s.capacity : 0, n_valid = s.tail - lo;
    if (n_fresh < 0 || n_fresh > batch || (uint64_t)n_fresh > s.head - s.tail || (n_fresh < batch && n_valid == 0)) return {};
    std::vector<uint64_t> out;
    for (int32_t c = 0; c < batch; ++c) {
        if (c < n_fresh) {
            out.push_back(s.tail + (uint64_t)c);
        } else {
            const uint64_t x = philox4_first(s.seed, s.draw * (uint64_t)batch + (uint64_t)c, 7u);
            out.push_back(lo + ((x * n_valid) >> 32));
        }
    }
    return out;
}

}  // namespace freeimpala_amd
