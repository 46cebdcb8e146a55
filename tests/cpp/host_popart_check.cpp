// host_popart_check.cpp -- PopArt value normalisation (include/fi_popart.h) through the C++ host side.
// A DeviceLearner (MLP) with PopArt on takes four steps on synthetic batches. A second one takes two,
// saves its state and its statistics, and a third, fresh one resumes from them -- enable_popart,
// set_popart_state, load_state -- and takes the other two. The resumed handle's state blob and
// statistics equal the straight run's byte for byte. Also the refusals, which come before any device
// call, and the neutral state of a handle that never enabled PopArt. Prints one line; everything is
// seeded, so a second run prints the same line.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "freeimpala_amd/device_learner.hpp"

using freeimpala_amd::DeviceLearner;
using freeimpala_amd::LearnerConfig;

#define CHECK(c)                                                                                       \
    do {                                                                                               \
        if (!(c)) {                                                                                    \
            std::fprintf(stderr, "CHECK failed at line %d: %s (%s)\n", __LINE__, #c, fi_last_error()); \
            return 1;                                                                                  \
        }                                                                                              \
    } while (0)

static const double kBeta = 0.125;

static bool steps(DeviceLearner& L, int first, int count) {
    fi_learner* h = L.handle(0);
    for (int k = first; k < first + count; ++k) {
        if (fi_learner_synth_batch(h, 40 + (uint64_t)k, 0, 0) != FI_OK) return false;
        fi_step_stats st{};
        if (fi_learner_step_resident(h, &st) != FI_OK) return false;
    }
    return true;
}

static int run() {
    LearnerConfig lc;
    lc.batch_size = 24;
    lc.seq_length = 5;
    lc.num_actions = 6;
    lc.obs_dim = 32;
    lc.seed = 12;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");

    DeviceLearner straight(lc);
    fi_learner* h = straight.handle(0);
    // a handle that never enabled it: off, the neutral statistics, the defaults
    fi_popart_state s{};
    CHECK(straight.popart_state(0, s) && s.enabled == 0 && s.mu == 0.0 && s.nu == 1.0 && s.sigma == 1.0 && s.updates == 0);
    CHECK(s.beta == FI_POPART_BETA && s.sigma_min == FI_POPART_SIGMA_MIN && s.sigma_max == FI_POPART_SIGMA_MAX);
    // the refusals
    const void* dev = nullptr;
    CHECK(fi_popart_set_state(h, 0.0, 1.0) == FI_ERR_STATE && fi_popart_state_dev(h, &dev) == FI_ERR_STATE);
    CHECK(fi_popart_enable(nullptr, 0.1, 1e-4, 1e6) == FI_ERR_INVALID);
    CHECK(fi_popart_enable(h, -0.1, 1e-4, 1e6) == FI_ERR_INVALID && fi_popart_enable(h, 1.5, 1e-4, 1e6) == FI_ERR_INVALID);
    CHECK(fi_popart_enable(h, nan, 1e-4, 1e6) == FI_ERR_INVALID);
    CHECK(fi_popart_enable(h, 0.1, 0.0, 1e6) == FI_ERR_INVALID && fi_popart_enable(h, 0.1, 2.0, 1e6) == FI_ERR_INVALID);
    CHECK(fi_popart_enable(h, 0.1, 1e-4, 0.5) == FI_ERR_INVALID && fi_popart_enable(h, 0.1, 1e-4, inf) == FI_ERR_INVALID);
    CHECK(!straight.enable_popart(0, 0.1, nan, 1e6) && straight.last_error().find("sigma_min") != std::string::npos);
    CHECK(straight.popart_state(0, s) && s.enabled == 0);
    CHECK(fi_popart_plan(0) == 0 && fi_popart_plan(1) == 1 && fi_popart_plan(409600) == 200);
    CHECK(fi_popart_workspace_bytes(409600) == 3200);

    CHECK(straight.enable_popart(0, kBeta));
    CHECK(fi_popart_state_dev(h, &dev) == FI_OK && dev != nullptr);
    CHECK(fi_popart_set_state(h, nan, 1.0) == FI_ERR_INVALID && fi_popart_set_state(h, 2.0, 3.0) == FI_ERR_INVALID);
    CHECK(fi_popart_set_state(h, 0.0, inf) == FI_ERR_INVALID);
    CHECK(straight.popart_state(0, s) && s.enabled == 1 && s.beta == kBeta && s.mu == 0.0 && s.sigma == 1.0 && s.updates == 0);
    CHECK(steps(straight, 0, 4));
    fi_popart_state want{};
    std::vector<char> want_blob;
    CHECK(straight.popart_state(0, want) && straight.save_state(0, want_blob));
    CHECK(want.updates == 4 && want.mu != 0.0 && want.sigma != 1.0 && want.nu >= want.mu * want.mu);
    // a second enable changes the three numbers and keeps the statistics
    CHECK(straight.enable_popart(0, 0.5, 1e-3, 1e3) && straight.popart_state(0, s));
    CHECK(s.beta == 0.5 && s.sigma_min == 1e-3 && s.sigma_max == 1e3 && s.mu == want.mu && s.nu == want.nu && s.updates == 4);

    // two steps, save; a fresh handle resumes and takes the other two
    std::vector<char> half_blob;
    fi_popart_state half{};
    {
        DeviceLearner first(lc);
        CHECK(first.enable_popart(0, kBeta) && steps(first, 0, 2));
        CHECK(first.popart_state(0, half) && first.save_state(0, half_blob) && half.updates == 2);
    }
    DeviceLearner resumed(lc);
    CHECK(resumed.enable_popart(0, kBeta) && resumed.set_popart_state(0, half.mu, half.nu) && resumed.load_state(0, half_blob));
    fi_popart_state r{};
    CHECK(resumed.popart_state(0, r) && r.mu == half.mu && r.nu == half.nu && r.sigma == half.sigma && r.updates == 0);
    CHECK(steps(resumed, 2, 2));
    std::vector<char> got_blob;
    CHECK(resumed.popart_state(0, r) && resumed.save_state(0, got_blob));
    CHECK(got_blob.size() == want_blob.size() && std::memcmp(got_blob.data(), want_blob.data(), got_blob.size()) == 0);
    CHECK(std::memcmp(&r.mu, &want.mu, 3 * sizeof(double)) == 0 && r.updates == 2);
    std::printf("popart mlp: mu %.17g nu %.17g sigma %.17g updates %llu blob %zu bytes equal\n", want.mu, want.nu,
                want.sigma, (unsigned long long)want.updates, want_blob.size());
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
