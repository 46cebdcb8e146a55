// host_publish_check.cpp -- parameter publication on the device (include/fi_publish.h) through the
// C++ host side: a DeviceLearner (Atari, plane records) publishes with publish_dev, a recording
// DeviceActor takes the publication with set_params_dev and a DeviceCatchEnv drives one unroll; the
// learner steps from it asynchronously, publishes again and the actor pulls again, with no host wait
// in between. The actor's parameters must then equal fi_learner_get_params_fp32, bit for bit, and its
// version the learner's. Prints one line; everything is seeded, so a second run prints the same line.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "freeimpala_amd/device_actor.hpp"
#include "freeimpala_amd/device_learner.hpp"

using freeimpala_amd::ActorConfig;
using freeimpala_amd::DeviceActor;
using freeimpala_amd::DeviceCatchEnv;
using freeimpala_amd::DeviceLearner;
using freeimpala_amd::LearnerConfig;

#define CHECK(c)                                                                                       \
    do {                                                                                               \
        if (!(c)) {                                                                                    \
            std::fprintf(stderr, "CHECK failed at line %d: %s (%s)\n", __LINE__, #c, fi_last_error()); \
            return 1;                                                                                  \
        }                                                                                              \
    } while (0)

static int run() {
    const int T = 4, N = 4, A = 3;
    LearnerConfig lc;
    lc.arch = "atari";
    lc.atari_records = "planes";
    lc.batch_size = N;
    lc.seq_length = T;
    lc.num_actions = A;
    lc.seed = 7;
    DeviceLearner learner(lc);
    fi_learner* lh = learner.handle(0);
    ActorConfig ac;
    ac.arch = "atari";
    ac.num_envs = N;
    ac.num_actions = A;
    ac.seed = 12;
    DeviceActor actor(ac);
    DeviceCatchEnv env(N, 0.99f, 5);

    CHECK(!actor.set_params_dev(lh) && actor.last_error().find("published nothing") != std::string::npos);
    CHECK(fi_publish_event(lh) == nullptr);
    uint64_t tag = 99;
    CHECK(learner.publish_dev(0, tag) && tag == 0);
    CHECK(actor.set_params_dev(lh) && actor.version() == 0);
    const size_t n = learner.param_count();
    std::vector<float> want(n), got;
    CHECK(fi_learner_get_params_fp32(lh, want.data(), n) == FI_OK);
    CHECK(actor.read_params(got) && got.size() == n && std::memcmp(got.data(), want.data(), n * sizeof(float)) == 0);

    const std::vector<float> before = want;

    // one unroll, an asynchronous step from it, a publication and a hand-over: nothing waits
    CHECK(actor.begin_rollout(T));
    int32_t done = -1;
    CHECK(env.rollout(actor, T + 1, &done) && done == T + 1 && actor.rollout_ready());
    fi_actor* ah = actor.handle();
    CHECK(fi_learner_step_rollouts_async(lh, &ah, 1) == FI_OK);
    CHECK(learner.publish_dev(0, tag) && tag == 1);
    CHECK(actor.set_params_dev(lh) && actor.version() == 1);
    CHECK(learner.wait(0));
    const fi_step_stats st = learner.last_stats(0);
    CHECK(st.version == 1);

    fi_publish_state ps{};
    CHECK(fi_publish_get_state(lh, &ps) == FI_OK);
    CHECK(ps.publications == 2 && ps.slot == 1 && ps.tag == 1 && ps.version == 1 && ps.dtype == FI_PUBLISH_FP32);
    CHECK(ps.readers[0] == 1 && ps.readers[1] == 1 && fi_publish_event(lh) != nullptr);
    std::vector<float> snap(n);
    uint64_t exact = 0;
    CHECK(fi_publish_read(lh, snap.data(), n, &exact) == FI_OK && exact == 1);
    CHECK(fi_learner_get_params_fp32(lh, want.data(), n) == FI_OK);
    CHECK(actor.read_params(got) && std::memcmp(got.data(), want.data(), n * sizeof(float)) == 0);
    CHECK(std::memcmp(snap.data(), want.data(), n * sizeof(float)) == 0);
    CHECK(std::memcmp(got.data(), before.data(), n * sizeof(float)) != 0);  // the update was applied

    int64_t bad = -1;
    CHECK(actor.sync(&bad) && bad == 0);
    CHECK(actor.end_rollout());
    std::printf("publish atari: loss %.9g grad_norm %.9g version %llu tag %llu publications %llu params %zu\n", st.total_loss,
                st.grad_norm, (unsigned long long)actor.version(), (unsigned long long)tag,
                (unsigned long long)ps.publications, n);
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
