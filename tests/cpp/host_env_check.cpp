// host_env_check.cpp -- a recording Atari DeviceActor driven by a DeviceCatchEnv
// (include/freeimpala_amd/device_actor.hpp over include/fi_env.h): two unrolls are enqueued with
// fi_env_rollout, no observation, action, reward or entry ever exists in host memory, and a learner
// handle steps from each through fi_learner_step_rollout. After each step the entries are read back
// once, and a second learner with the same parameters that steps from that host copy must report
// the same losses. Prints one line; everything is seeded, so a second run prints the same line.
#include <cstdio>
#include <string>
#include <vector>

#include "freeimpala_amd/device_actor.hpp"

using freeimpala_amd::ActorConfig;
using freeimpala_amd::DeviceActor;
using freeimpala_amd::DeviceCatchEnv;

#define CHECK(c)                                                                                       \
    do {                                                                                               \
        if (!(c)) {                                                                                    \
            std::fprintf(stderr, "CHECK failed at line %d: %s (%s)\n", __LINE__, #c, fi_last_error()); \
            return 1;                                                                                  \
        }                                                                                              \
    } while (0)

struct Learner {
    fi_learner* h = nullptr;
    ~Learner() { fi_learner_destroy(h); }
};

static int make_learner(int T, int B, int A, Learner& out) {
    fi_learner_config c;
    fi_learner_config_init(&c);
    c.arch = FI_ARCH_ATARI;
    c.seq_len = T;
    c.batch = B;
    c.num_actions = A;
    c.seed = 7;
    CHECK(fi_learner_create(&c, &out.h) == FI_OK);
    CHECK(fi_learner_set_record_format(out.h, FI_RECORDS_PLANES) == FI_OK);
    return 0;
}

static int run() {
    const int T = 10, N = 3, A = 4;  // two unrolls of 10 steps: every environment finishes one episode
    Learner dev, host;
    if (make_learner(T, N, A, dev) || make_learner(T, N, A, host)) return 1;
    ActorConfig c;
    c.arch = "atari";
    c.num_envs = N;
    c.num_actions = A;
    c.seed = 12;
    DeviceActor actor(c);
    DeviceCatchEnv env(N, 0.99f, 5);
    int32_t done = -1;
    CHECK(!env.rollout(actor, 1, &done) && done == 0);  // refused: no parameters yet
    std::vector<char> blob(fi_learner_param_bytes(dev.h));
    uint64_t version = 0;
    CHECK(fi_learner_get_params(dev.h, blob.data(), blob.size(), &version) == FI_OK);
    CHECK(actor.load(blob, 0));
    CHECK(actor.begin_rollout(T));
    fi_step_stats sd{}, sh{};
    for (int k = 0; k < 2; ++k) {
        CHECK(env.rollout(actor, k == 0 ? T + 1 : T, &done) && done == (k == 0 ? T + 1 : T));
        CHECK(actor.rollout_ready());  // known on the host at once: nothing was waited for
        if (k == 0) {
            CHECK(!env.rollout(actor, T, &done) && done == T - 1);  // unroll 0 is unreleased: the completing step is refused
            CHECK(actor.sync());
        }
        std::vector<uint8_t> entries;
        CHECK(actor.read_rollout(entries));
        CHECK(fi_learner_step_rollout(dev.h, actor.handle(), &sd) == FI_OK);
        CHECK(!actor.rollout_ready() && fi_learner_staging_bytes(dev.h) == 0);
        const size_t eb = actor.rollout_entry_bytes();
        std::vector<const void*> ptrs(N);
        for (int i = 0; i < N; ++i) ptrs[i] = entries.data() + (size_t)i * eb;
        CHECK(fi_learner_step(host.h, ptrs.data(), ptrs.size(), eb, &sh) == FI_OK);
        CHECK(sd.total_loss == sh.total_loss && sd.grad_norm == sh.grad_norm && sd.version == sh.version);
        if (k == 0) {
            // the T - 1 steps enqueued before the refusal filled unroll 1 up to its last record: one more completes it
            CHECK(env.rollout(actor, 1, &done) && done == 1 && actor.rollout_ready());
            CHECK(actor.read_rollout(entries));
            CHECK(fi_learner_step_rollout(dev.h, actor.handle(), &sd) == FI_OK);
            for (int i = 0; i < N; ++i) ptrs[i] = entries.data() + (size_t)i * eb;
            CHECK(fi_learner_step(host.h, ptrs.data(), ptrs.size(), eb, &sh) == FI_OK);
            CHECK(sd.total_loss == sh.total_loss && sd.grad_norm == sh.grad_norm && sd.version == sh.version);
        }
    }
    int64_t bad = -1;
    CHECK(actor.sync(&bad) && bad == 0);
    uint64_t episodes = 0;
    int64_t ret = 0;
    CHECK(env.stats(episodes, ret));
    // 1 + 3 T = 31 steps: every environment finished exactly one episode of 20
    CHECK(episodes == (uint64_t)N && ret >= -N && ret <= N);
    CHECK(actor.end_rollout());
    std::printf("env atari: loss %.9g grad_norm %.9g version %llu episodes %llu return %lld\n", sd.total_loss,
                sd.grad_norm, (unsigned long long)sd.version, (unsigned long long)episodes, (long long)ret);
    return 0;
}

int main() {
    try {
        return run();
    } catch (const std::exception& e) {
        std::fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 1;
    }
}
