// host_rollouts_check.cpp -- two MLP actors, then two Atari actors, of different sizes and
// parameter versions record one unroll each on the device, and one learner steps from both through
// freeimpala_amd::step_rollouts (include/freeimpala_amd/device_actor.hpp over include/fi_gather.h):
// actor 0 fills the first columns of the batch, actor 1 the rest. The entries are read back once,
// and a second learner with the same parameters that steps from the concatenated host copy must
// report the same losses. Prints one line per policy; everything is seeded, so a second run prints
// the same lines.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "freeimpala_amd/device_actor.hpp"

using freeimpala_amd::ActorConfig;
using freeimpala_amd::ActResult;
using freeimpala_amd::DeviceActor;

#define CHECK(c)                                                                                       \
    do {                                                                                               \
        if (!(c)) {                                                                                    \
            std::fprintf(stderr, "CHECK failed at line %d: %s (%s)\n", __LINE__, #c, fi_last_error()); \
            return 1;                                                                                  \
        }                                                                                              \
    } while (0)

static uint64_t g_x = 0x9E3779B97F4A7C15ull;
static uint64_t next() {
    g_x ^= g_x << 13;
    g_x ^= g_x >> 7;
    g_x ^= g_x << 17;
    return g_x;
}

struct Learner {
    fi_learner* h = nullptr;
    ~Learner() { fi_learner_destroy(h); }
};

static int make_learner(int arch, int T, int B, int A, int D, Learner& out) {
    fi_learner_config c;
    fi_learner_config_init(&c);
    c.arch = arch;
    c.seq_len = T;
    c.batch = B;
    c.num_actions = A;
    c.obs_dim = D;
    c.seed = 7;
    CHECK(fi_learner_create(&c, &out.h) == FI_OK);
    if (arch == FI_ARCH_ATARI) CHECK(fi_learner_set_record_format(out.h, FI_RECORDS_PLANES) == FI_OK);
    return 0;
}

// `steps` act calls with their outcomes
static int act(DeviceActor& actor, int steps) {
    const ActorConfig& c = actor.config();
    const int N = c.num_envs;
    ActResult r;
    std::vector<float> obs((size_t)N * c.obs_dim), rew(N), disc(N);
    std::vector<uint8_t> planes((size_t)N * DeviceActor::kPlaneBytes), start(N);
    for (int t = 0; t < steps; ++t) {
        if (c.arch == "atari") {
            for (uint8_t& v : planes) v = (uint8_t)(next() >> 56);
            for (int i = 0; i < N; ++i) start[i] = t == 0 || (t == 2 && i == 1);
            CHECK(actor.act_planes(planes, start, r));
        } else {
            for (float& v : obs) v = (float)((next() >> 40) * (1.0 / 16777216.0)) * 2.f - 1.f;
            CHECK(actor.act_obs(obs, r));
        }
        for (int i = 0; i < N; ++i) {
            rew[i] = (float)(int)(next() % 3) - 1.f;
            disc[i] = next() % 5 ? 0.99f : 0.f;
        }
        CHECK(actor.outcome(rew, disc));
    }
    return 0;
}

// both actors record an unroll (actor 1 holds parameter version 3), then both learners step: `dev`
// from the two device buffers, `host` from their host copies, concatenated
static int run(const char* name, DeviceActor& a0, DeviceActor& a1, int T, Learner& dev, Learner& host) {
    std::vector<char> blob(fi_learner_param_bytes(dev.h));
    uint64_t version = 0;
    CHECK(fi_learner_get_params(dev.h, blob.data(), blob.size(), &version) == FI_OK);
    CHECK(a0.load(blob, 0) && a1.load(blob, 3));
    CHECK(a0.begin_rollout(T) && a1.begin_rollout(T));
    fi_step_stats sd{}, sh{};
    fi_batch_versions bv{};
    const std::vector<DeviceActor*> both{&a0, &a1};
    CHECK(fi_learner_batch_versions(dev.h, &bv) == FI_ERR_STATE);  // no such step yet
    if (act(a0, T + 1)) return 1;
    CHECK(a0.rollout_ready() && !a1.rollout_ready());
    CHECK(freeimpala_amd::step_rollouts(dev.h, both, &sd) == FI_ERR_STATE);  // actor 1 is not ready ...
    CHECK(a0.rollout_ready());                                                // ... and actor 0 still waits
    if (act(a1, T + 1)) return 1;
    CHECK(freeimpala_amd::step_rollouts(dev.h, {&a0, &a0}, &sd) == FI_ERR_INVALID);  // one handle twice
    CHECK(freeimpala_amd::step_rollouts(dev.h, {&a0}, &sd) == FI_ERR_INVALID);       // num_envs below the batch
    std::vector<uint8_t> e0, e1;
    CHECK(a0.read_rollout(e0) && a1.read_rollout(e1));
    CHECK(freeimpala_amd::step_rollouts(dev.h, both, &sd) == FI_OK);
    CHECK(!a0.rollout_ready() && !a1.rollout_ready());  // released
    CHECK(fi_learner_staging_bytes(dev.h) == 0);        // no staging buffer was ever allocated
    const int n0 = a0.config().num_envs, n1 = a1.config().num_envs;
    CHECK(fi_learner_batch_versions(dev.h, &bv) == FI_OK);
    CHECK(bv.min_version == 0 && bv.max_version == 3 && bv.count == (uint64_t)T * (n0 + n1) &&
          bv.sum_versions == 3ull * T * n1);
    const size_t eb = a0.rollout_entry_bytes();
    CHECK(eb == a1.rollout_entry_bytes() && eb == fi_learner_entry_bytes(host.h));
    std::vector<const void*> ptrs;
    for (int i = 0; i < n0; ++i) ptrs.push_back(e0.data() + (size_t)i * eb);
    for (int i = 0; i < n1; ++i) ptrs.push_back(e1.data() + (size_t)i * eb);
    CHECK(fi_learner_step(host.h, ptrs.data(), ptrs.size(), eb, &sh) == FI_OK);
    CHECK(sd.total_loss == sh.total_loss && sd.grad_norm == sh.grad_norm && sd.version == sh.version);
    CHECK(a0.end_rollout() && a1.end_rollout());
    std::printf("rollouts %s: loss %.9g grad_norm %.9g version %llu\n", name, sd.total_loss, sd.grad_norm,
                (unsigned long long)sd.version);
    return 0;
}

static int policy(const char* name, int arch, int T, int N0, int N1, int A, int D) {
    Learner dev, host;
    if (make_learner(arch, T, N0 + N1, A, D, dev) || make_learner(arch, T, N0 + N1, A, D, host)) return 1;
    ActorConfig c;
    c.arch = name;
    c.num_actions = A;
    c.obs_dim = D;
    c.num_envs = N0;
    c.seed = 11;
    DeviceActor a0(c);
    c.num_envs = N1;
    c.seed = 12;
    DeviceActor a1(c);
    return run(name, a0, a1, T, dev, host);
}

int main() {
    try {
        if (policy("mlp", FI_ARCH_MLP, 4, 2, 3, 18, 128)) return 1;
        if (policy("atari", FI_ARCH_ATARI, 3, 1, 2, 6, 128)) return 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
