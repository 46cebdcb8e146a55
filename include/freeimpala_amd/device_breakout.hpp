// device_breakout.hpp -- C++ host side of the device Breakout environment (include/fi_breakout.h):
// num_envs environments whose state is in device memory, an fi_env handle like DeviceCatchEnv's
// (device_actor.hpp) with the same surface. rollout() enqueues n_steps of act -> step -> outcome on
// the actor's stream and returns at once; steps_enqueued counts the steps before a refusal.
// read_state() and set_state() move all nine fields of the rule's state. Failures never throw: the
// call returns false and last_error() holds the message. Construction throws std::runtime_error.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "fi_breakout.h"
#include "freeimpala_amd/device_actor.hpp"

namespace freeimpala_amd {

class DeviceBreakoutEnv {
public:
    using Tensors = DeviceCatchEnv::Tensors;
    // num_envs values per field; dr and dc are -1 or +1, bricks the 63-bit mask
    struct State {
        std::vector<int32_t> r, c, p, dr, dc, t, score;
        std::vector<uint32_t> k;
        std::vector<uint64_t> bricks;
    };

    DeviceBreakoutEnv(int num_envs, float gamma, uint64_t seed, int max_steps = 1000, int device = 0) : n_(num_envs) {
        if (fi_breakout_create(device, num_envs, gamma, seed, max_steps, &h_) != FI_OK)
            throw std::runtime_error(std::string("fi_breakout_create: ") + fi_last_error());
    }
    ~DeviceBreakoutEnv() { fi_env_destroy(h_); }
    DeviceBreakoutEnv(const DeviceBreakoutEnv&) = delete;
    DeviceBreakoutEnv& operator=(const DeviceBreakoutEnv&) = delete;

    int num_envs() const { return n_; }
    int max_steps() const { return fi_breakout_max_steps(h_); }
    const std::string& last_error() const { return err_; }
    bool step(const int32_t* actions_dev, void* ready_event = nullptr, void* stream = nullptr) {
        return ok(fi_env_step(h_, actions_dev, ready_event, stream));
    }
    Tensors tensors() {
        Tensors t;
        fi_env_tensors(h_, &t.planes, &t.episode_start, &t.rewards, &t.discounts);
        return t;
    }
    void* stepped_event() { return fi_env_stepped_event(h_); }
    // finished episodes and the sum of their scores
    bool stats(uint64_t& episodes, int64_t& return_sum) { return ok(fi_env_stats(h_, &episodes, &return_sum)); }
    bool rollout(DeviceActor& actor, int n_steps, int32_t* steps_enqueued = nullptr) {
        return ok(fi_env_rollout(h_, actor.handle(), n_steps, steps_enqueued));
    }
    bool read_state(State& s) {
        const size_t n = (size_t)n_;
        for (auto* v : {&s.r, &s.c, &s.p, &s.dr, &s.dc, &s.t, &s.score}) v->resize(n);
        s.k.resize(n);
        s.bricks.resize(n);
        return ok(fi_breakout_read_state(h_, s.r.data(), s.c.data(), s.p.data(), s.k.data(), s.dr.data(), s.dc.data(),
                                         s.t.data(), s.score.data(), s.bricks.data()));
    }
    // waits for the last step, writes the state and renders it; nothing of the environment may be in flight
    bool set_state(const State& s) {
        const size_t n = (size_t)n_;
        for (const auto* v : {&s.r, &s.c, &s.p, &s.dr, &s.dc, &s.t, &s.score})
            if (v->size() != n) return bad("set_state: every field must hold num_envs values");
        if (s.k.size() != n || s.bricks.size() != n) return bad("set_state: every field must hold num_envs values");
        return ok(fi_breakout_set_state(h_, s.r.data(), s.c.data(), s.p.data(), s.k.data(), s.dr.data(), s.dc.data(),
                                        s.t.data(), s.score.data(), s.bricks.data()));
    }
    fi_env* handle() { return h_; }

private:
    bool ok(int rc) {
        if (rc == FI_OK) return true;
        err_ = fi_last_error();
        return false;
    }
    bool bad(const char* msg) {
        err_ = msg;
        return false;
    }

    int n_;
    fi_env* h_ = nullptr;
    std::string err_;
};

}  // namespace freeimpala_amd
