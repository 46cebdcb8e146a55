// host_explore_check.cpp -- actor exploration (include/fi_explore.h) through the C++ host side: a
// recording DeviceActor (Atari, plane records) gets a temperature and an epsilon ladder with
// set_exploration, a DeviceCatchEnv drives one unroll and a DeviceLearner steps from it. The learner's
// mu tensor (the behaviour logits the actor recorded) must then differ from its logits tensor (the
// policy's own, recomputed) while every mu row still is a log-distribution; after clear_exploration
// the next unroll steps as before and the handle has no behaviour logits to read. Prints one line;
// everything is seeded, so a second run prints the same line.
#include <cmath>
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
    const int T = 3, N = 4, A = 3;
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
    uint64_t tag = 0;
    CHECK(learner.publish_dev(0, tag));
    CHECK(actor.set_params_dev(lh));

    // refusals store nothing
    std::vector<float> ladder(N);
    for (int i = 0; i < N; ++i) ladder[i] = std::pow(0.4f, 1.f + 7.f * (float)i / (float)(N - 1));
    std::vector<float> bad = ladder;
    bad[2] = 1.5f;
    CHECK(!actor.set_exploration(2.f, bad) && actor.last_error().find("epsilon[2]") != std::string::npos);
    CHECK(!actor.set_exploration(128.f, ladder) && actor.last_error().find("temperature") != std::string::npos);
    float tau = 0.f;
    int active = -1;
    std::vector<float> eps(N, -1.f);
    CHECK(fi_explore_get(actor.handle(), &tau, eps.data(), &active) == FI_OK && tau == 1.f && active == 0 && eps[2] == 0.f);

    CHECK(actor.set_exploration(2.f, ladder));
    CHECK(fi_explore_get(actor.handle(), &tau, eps.data(), &active) == FI_OK && tau == 2.f && active == 1);
    CHECK(std::memcmp(eps.data(), ladder.data(), N * sizeof(float)) == 0);

    CHECK(actor.begin_rollout(T));
    int32_t done = -1;
    CHECK(env.rollout(actor, T + 1, &done) && done == T + 1 && actor.rollout_ready());
    fi_step_stats st{};
    CHECK(fi_learner_step_rollout(lh, actor.handle(), &st) == FI_OK);
    const size_t n = (size_t)T * N * A;
    std::vector<float> mu(n), logits(n);
    CHECK(fi_learner_read_tensor(lh, "mu", mu.data(), n * sizeof(float)) == FI_OK);
    CHECK(fi_learner_read_tensor(lh, "logits", logits.data(), n * sizeof(float)) == FI_OK);
    int differing = 0;
    for (size_t i = 0; i < n; ++i) differing += mu[i] != logits[i];
    CHECK(differing > 0);
    // every mu row is a log-distribution
    for (size_t r = 0; r < n / A; ++r) {
        double s = 0.0;
        for (int a = 0; a < A; ++a) s += std::exp((double)mu[r * A + a]);
        CHECK(std::fabs(s - 1.0) <= 1e-5);
    }
    std::vector<float> beh;
    CHECK(actor.read_behaviour(beh) && beh.size() == (size_t)N * A);

    // cleared: the next unroll is drawn by the plain rule and steps as before
    CHECK(actor.clear_exploration());
    CHECK(fi_explore_get(actor.handle(), &tau, eps.data(), &active) == FI_OK && tau == 1.f && active == 0);
    CHECK(env.rollout(actor, T, &done) && done == T && actor.rollout_ready());
    fi_step_stats st2{};
    CHECK(fi_learner_step_rollout(lh, actor.handle(), &st2) == FI_OK);
    CHECK(!actor.read_behaviour(beh) && actor.last_error().find("did not draw") != std::string::npos);

    int64_t nonfinite = -1;
    CHECK(actor.sync(&nonfinite) && nonfinite == 0);
    CHECK(actor.end_rollout());
    std::printf("explore atari: loss %.9g grad_norm %.9g mu != logits in %d of %zu\n", st.total_loss, st.grad_norm,
                differing, n);
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
