// device_actor.hpp -- C++ host side of batched policy inference (include/fi_actor.h).
//
// What an actor process needs to turn observations into actions with the policy the learner
// publishes: a DeviceActor owns one fi_actor handle (N environments per call, one HIP stream),
// takes the published blob (DeviceLearner::publish / ModelManager's bytes) and returns actions,
// the policy's logits (the mu field of the records it writes) and values. Failures of an act call
// never throw: it returns false and last_error() holds the message, as DeviceLearner::step does.
// Construction throws std::runtime_error when the HIP library or device is unusable -- there is
// no CPU fallback. One thread at a time per DeviceActor.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "fi_actor.h"
#include "fi_env.h"
#include "fi_explore.h"
#include "fi_gather.h"
#include "fi_publish.h"
#include "fi_rollout.h"

namespace freeimpala_amd {

struct ActorConfig {
    std::string arch = "mlp";  // mlp|atari
    int num_envs = 1;          // N environments per act call
    int num_actions = 18;
    int obs_dim = 128;
    int hidden = 256;
    bool greedy = false;       // argmax instead of a draw
    uint64_t seed = 0;         // key of the action draws
    int device = 0;

    fi_actor_config abi_config() const {
        fi_actor_config c;
        fi_actor_config_init(&c);
        c.arch = arch == "atari" ? FI_ARCH_ATARI : FI_ARCH_MLP;
        c.num_envs = num_envs;
        c.num_actions = num_actions;
        c.obs_dim = obs_dim;
        c.hidden = hidden;
        c.mode = greedy ? FI_ACT_GREEDY : FI_ACT_SAMPLE;
        c.seed = seed;
        c.device = device;
        return c;
    }
};

struct ActResult {
    std::vector<int32_t> actions;  // N
    std::vector<float> logits;     // N * A
    std::vector<float> values;     // N
};

class DeviceActor {
public:
    static constexpr size_t kPlaneBytes = 84 * 84, kFrameBytes = 4 * kPlaneBytes;

    explicit DeviceActor(const ActorConfig& cfg) : cfg_(cfg) {
        if (cfg.arch != "mlp" && cfg.arch != "atari") throw std::invalid_argument("ActorConfig.arch: mlp|atari");
        const fi_actor_config c = cfg.abi_config();
        if (fi_actor_create(&c, &h_) != FI_OK) throw std::runtime_error(std::string("fi_actor_create: ") + fi_last_error());
    }
    ~DeviceActor() { fi_actor_destroy(h_); }
    DeviceActor(const DeviceActor&) = delete;
    DeviceActor& operator=(const DeviceActor&) = delete;

    const ActorConfig& config() const { return cfg_; }
    size_t param_count() const { return fi_actor_param_count(h_); }
    uint64_t version() const { return fi_actor_version(h_); }
    const std::string& last_error() const { return err_; }

    // the blob DeviceLearner::publish fills (fp32 or bf16) and its version
    bool load(const std::vector<char>& blob, uint64_t version) {
        return ok(fi_actor_set_params(h_, blob.data(), blob.size(), version));
    }
    // the learner's newest publication on the device (include/fi_publish.h: DeviceLearner::publish_dev),
    // in stream order: nothing is copied through the host and nothing waits. May be called on this
    // actor's thread while another thread drives the learner.
    bool set_params_dev(fi_learner* learner) { return ok(fi_actor_set_params_dev(h_, learner)); }
    // waits for the stream: the handle's fp32 parameters
    bool read_params(std::vector<float>& out) {
        out.resize(param_count());
        return ok(fi_actor_read_params(h_, out.data(), out.size()));
    }
    bool set_greedy(bool greedy) { return ok(fi_actor_set_mode(h_, greedy ? FI_ACT_GREEDY : FI_ACT_SAMPLE)); }
    bool seed(uint64_t seed, uint64_t draw = 0) { return ok(fi_actor_seed(h_, seed, draw)); }

    // Exploration (include/fi_explore.h): the draw gets a temperature and one epsilon per environment
    // (empty: all 0), and a recording handle writes the behaviour logits into its records' mu. Allowed
    // between any two act calls; greedy mode ignores both.
    bool set_exploration(float temperature, const std::vector<float>& epsilon = {}) {
        if (!epsilon.empty() && epsilon.size() != (size_t)cfg_.num_envs)
            return bad("set_exploration: epsilon must be empty or hold num_envs floats");
        return ok(fi_explore_set(h_, temperature, epsilon.empty() ? nullptr : epsilon.data()));
    }
    bool clear_exploration() { return ok(fi_explore_clear(h_)); }
    // the last act call's behaviour logits (N * A; waits): false unless that call explored
    bool read_behaviour(std::vector<float>& out) {
        out.resize((size_t)cfg_.num_envs * cfg_.num_actions);
        return ok(fi_explore_read_behaviour(h_, out.data(), out.size()));
    }

    // obs: N * obs_dim floats (MLP)
    bool act_obs(const std::vector<float>& obs, ActResult& out) {
        if (obs.size() != (size_t)cfg_.num_envs * cfg_.obs_dim) return bad("act_obs: obs must hold num_envs * obs_dim floats");
        size(out);
        return ok(fi_actor_act_obs(h_, obs.data(), out.actions.data(), out.logits.data(), out.values.data()));
    }
    // frames: N stacks of 84x84x4 bytes (Atari)
    bool act_frames(const std::vector<uint8_t>& frames, ActResult& out) {
        if (frames.size() != (size_t)cfg_.num_envs * kFrameBytes) return bad("act_frames: frames must hold num_envs * 28224 bytes");
        size(out);
        return ok(fi_actor_act_frames(h_, frames.data(), out.actions.data(), out.logits.data(), out.values.data()));
    }
    // planes: N newest 84x84 observations; episode_start: N flags (Atari; the stacks stay on the device)
    bool act_planes(const std::vector<uint8_t>& planes, const std::vector<uint8_t>& episode_start, ActResult& out) {
        if (planes.size() != (size_t)cfg_.num_envs * kPlaneBytes || episode_start.size() != (size_t)cfg_.num_envs)
            return bad("act_planes: planes must hold num_envs * 7056 bytes and episode_start num_envs flags");
        size(out);
        return ok(fi_actor_act_planes(h_, planes.data(), episode_start.data(), out.actions.data(), out.logits.data(),
                                      out.values.data()));
    }
    bool reset_stacks() { return ok(fi_actor_reset_stacks(h_)); }
    bool read_stacks(std::vector<uint8_t>& out) {
        out.resize((size_t)cfg_.num_envs * kFrameBytes);
        return ok(fi_actor_read_stacks(h_, out.data(), out.size()));
    }

    // Rollouts recorded on the device (include/fi_rollout.h): after begin_rollout(T) every act_planes
    // / act_obs call records its step, outcome() adds the environments' rewards and discounts, and a
    // learner handle on the same device steps from the completed unroll: fi_learner_step_rollout(
    // learner, actor.handle(), &stats).
    bool begin_rollout(int seq_len) { return ok(fi_rollout_begin(h_, seq_len)); }
    bool outcome(const std::vector<float>& rewards, const std::vector<float>& discounts) {
        if (rewards.size() != (size_t)cfg_.num_envs || discounts.size() != (size_t)cfg_.num_envs)
            return bad("outcome: rewards and discounts must hold num_envs floats each");
        return ok(fi_rollout_outcome(h_, rewards.data(), discounts.data()));
    }
    bool rollout_ready() const { return fi_rollout_ready(h_) != 0; }
    size_t rollout_entry_bytes() const { return fi_rollout_entry_bytes(h_); }
    // the completed unroll's num_envs entries, back to back; it stays unreleased
    bool read_rollout(std::vector<uint8_t>& out) {
        out.resize((size_t)cfg_.num_envs * fi_rollout_entry_bytes(h_));
        return ok(fi_rollout_read(h_, out.data(), out.size()));
    }
    bool release_rollout(void* consumed_event = nullptr) { return ok(fi_rollout_release(h_, consumed_event)); }
    bool end_rollout() { return ok(fi_rollout_end(h_)); }
    fi_actor* handle() { return h_; }

    // Device pointers in, nothing waits (include/fi_env.h): the act call and the outcome are enqueued
    // on the handle's stream behind ready_event (a hipEvent_t or nullptr) and read the caller's
    // device memory; outputs_dev() names the handle's own output tensors and the event behind the
    // last such call; sync() waits and reports the rows that held NaN / Inf logits since the last sync
    // (false, with the count, when there were any).
    struct DeviceOutputs {
        const int32_t* actions = nullptr;  // N
        const float* logits = nullptr;     // N * A
        const float* values = nullptr;     // N
        void* done_event = nullptr;
    };
    bool act_planes_dev(const uint8_t* planes_dev, const uint8_t* episode_start_dev, void* ready_event = nullptr) {
        return ok(fi_actor_act_planes_dev(h_, planes_dev, episode_start_dev, ready_event));
    }
    bool act_obs_dev(const float* obs_dev, void* ready_event = nullptr) {
        return ok(fi_actor_act_obs_dev(h_, obs_dev, ready_event));
    }
    bool outputs_dev(DeviceOutputs& out) {
        return ok(fi_actor_outputs_dev(h_, &out.actions, &out.logits, &out.values, &out.done_event));
    }
    bool outcome_dev(const float* rewards_dev, const float* discounts_dev, void* ready_event = nullptr) {
        return ok(fi_rollout_outcome_dev(h_, rewards_dev, discounts_dev, ready_event));
    }
    bool sync(int64_t* nonfinite_rows = nullptr) { return ok(fi_actor_sync(h_, nonfinite_rows)); }
    void* stream() { return fi_actor_stream(h_); }  // hipStream_t

private:
    void size(ActResult& out) const {
        out.actions.resize((size_t)cfg_.num_envs);
        out.logits.resize((size_t)cfg_.num_envs * cfg_.num_actions);
        out.values.resize((size_t)cfg_.num_envs);
    }
    bool ok(int rc) {
        if (rc == FI_OK) return true;
        err_ = fi_last_error();
        return false;
    }
    bool bad(const char* msg) {
        err_ = msg;
        return false;
    }

    ActorConfig cfg_;
    fi_actor* h_ = nullptr;
    std::string err_;
};

// The built-in device environment (include/fi_env.h: Catch on 84x84 planes, num_envs of them, their
// state in device memory). rollout() enqueues n_steps of act -> step -> outcome on the actor's
// stream and returns at once; steps_enqueued counts the steps before a refusal.
class DeviceCatchEnv {
public:
    struct Tensors {
        const uint8_t* planes = nullptr;         // N * 7056
        const uint8_t* episode_start = nullptr;  // N
        const float* rewards = nullptr;          // N
        const float* discounts = nullptr;        // N
    };

    DeviceCatchEnv(int num_envs, float gamma, uint64_t seed, int device = 0) : n_(num_envs) {
        if (fi_env_create(device, num_envs, gamma, seed, &h_) != FI_OK)
            throw std::runtime_error(std::string("fi_env_create: ") + fi_last_error());
    }
    ~DeviceCatchEnv() { fi_env_destroy(h_); }
    DeviceCatchEnv(const DeviceCatchEnv&) = delete;
    DeviceCatchEnv& operator=(const DeviceCatchEnv&) = delete;

    int num_envs() const { return n_; }
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
    bool stats(uint64_t& episodes, int64_t& return_sum) { return ok(fi_env_stats(h_, &episodes, &return_sum)); }
    bool rollout(DeviceActor& actor, int n_steps, int32_t* steps_enqueued = nullptr) {
        return ok(fi_env_rollout(h_, actor.handle(), n_steps, steps_enqueued));
    }
    fi_env* handle() { return h_; }

private:
    bool ok(int rc) {
        if (rc == FI_OK) return true;
        err_ = fi_last_error();
        return false;
    }

    int n_;
    fi_env* h_ = nullptr;
    std::string err_;
};

// Several recording actors fill one learner batch (include/fi_gather.h): actor k's completed unroll
// becomes the next num_envs columns; the num_envs sum to the learner's batch. Acquire, step,
// release in one call; the status is fi_learner_step_rollouts' (fi_last_error() has the message),
// and after a refusal every unroll still waits.
inline int step_rollouts(fi_learner* learner, const std::vector<DeviceActor*>& actors, fi_step_stats* stats) {
    std::vector<fi_actor*> handles;
    handles.reserve(actors.size());
    for (DeviceActor* a : actors) handles.push_back(a ? a->handle() : nullptr);
    return fi_learner_step_rollouts(learner, handles.data(), (int32_t)handles.size(), stats);
}

}  // namespace freeimpala_amd
