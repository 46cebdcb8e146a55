// host_target_check.cpp -- the target network (include/fi_target.h) through the C++ host side. The
// refusals, which come before any device call, and the getters before fi_target_enable; two
// DeviceLearners (MLP) take five surrogate steps around a target of period 2 on the same synthetic
// batches and end with the same state blob, the same target parameters and, after the fourth, the same
// stats block, byte for byte; the target parameters are the learner's as they stood after the fourth
// step; a third enables the target, disables it and takes the surrogate steps of a fourth that never
// heard of it: the same blob. Prints one line; everything is seeded, so a second run prints the same line.
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

static bool steps(DeviceLearner& L, int first, int count, fi_step_stats* last = nullptr) {
    fi_learner* h = L.handle(0);
    for (int k = first; k < first + count; ++k) {
        if (fi_learner_synth_batch(h, 90 + (uint64_t)k, 0, 0) != FI_OK) return false;
        fi_step_stats st{};
        if (fi_learner_step_resident(h, &st) != FI_OK) return false;
        if (last) *last = st;
    }
    return true;
}

template <typename V>
static bool same(const V& a, const V& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0;
}

static int run() {
    LearnerConfig lc;
    lc.batch_size = 24;
    lc.seq_length = 5;
    lc.num_actions = 6;
    lc.obs_dim = 32;
    lc.seed = 12;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
    const uint64_t rows = (uint64_t)lc.batch_size * lc.seq_length;

    DeviceLearner a(lc);
    fi_learner* h = a.handle(0);
    const size_t n = a.param_count();
    std::vector<float> theta_a(n), theta_b(n), params4(n), now(n);
    fi_target_params tp{};
    fi_target_stats ts{};
    const void* dev = nullptr;
    CHECK(!a.target_state(0, tp, ts) && a.last_error().find("never on") != std::string::npos);
    CHECK(fi_target_params_dev(h, &dev) == FI_ERR_STATE && fi_target_logits_dev(h, &dev) == FI_ERR_STATE);
    CHECK(fi_target_stats_dev(h, &dev) == FI_ERR_STATE && fi_target_sync(h) == FI_ERR_STATE);
    CHECK(fi_target_get_params(h, theta_a.data(), n) == FI_ERR_STATE && fi_target_set_params(h, theta_a.data(), n) == FI_ERR_STATE);
    fi_target_params p{FI_TARGET_PERIOD, FI_TARGET_TAU, {0u, 0u}};
    CHECK(fi_target_enable(nullptr, &p) == FI_ERR_INVALID && fi_target_enable(h, nullptr) == FI_ERR_INVALID);
    for (float bad : {0.f, -0.5f, 1.5f, inf, nan}) {
        fi_target_params q = p;
        q.tau = bad;
        CHECK(fi_target_enable(h, &q) == FI_ERR_INVALID);
    }
    CHECK(!a.enable_target(0, 0u) && a.last_error().find("period") != std::string::npos);
    CHECK(fi_target_disable(h) == FI_OK);                      // nothing to turn off
    CHECK(fi_target_sync(h) == FI_ERR_STATE);                  // none of the refused calls made a block
    CHECK(fi_target_workspace_bytes(100, 4096, 18) > fi_surrogate_workspace_bytes(100, 4096, 18));
    CHECK(fi_target_workspace_bytes(5, 24, 1) == 0 && fi_target_workspace_bytes(5, 24, 65) == 0);

    // two handles, five surrogate steps around a target of period 2: the same bytes
    DeviceLearner b(lc);
    fi_step_stats sa{}, sb{};
    bool on = false;
    CHECK(a.set_surrogate(0, 0.1f, true) && b.set_surrogate(0, 0.1f, true));
    CHECK(a.enable_target(0, 2u) && b.enable_target(0, 2u));
    CHECK(a.target_state(0, tp, ts, &on) && on && tp.period == 2u && tp.tau == 1.0f && ts.updates == 0 && ts.rows == 0);
    CHECK(fi_target_params_dev(h, &dev) == FI_OK && dev != nullptr && fi_target_stats_dev(h, &dev) == FI_OK && dev != nullptr);
    // the fourth step's target is the parameters of two updates ago; the update behind it makes it theirs again
    fi_target_stats ta{}, tb{};
    CHECK(steps(a, 0, 4) && fi_learner_get_params_fp32(h, params4.data(), n) == FI_OK && a.target_state(0, tp, ta));
    CHECK(steps(b, 0, 4) && b.target_state(0, tp, tb) && steps(a, 4, 1, &sa) && steps(b, 4, 1, &sb));
    std::vector<char> blob_a, blob_b;
    CHECK(a.save_state(0, blob_a) && b.save_state(0, blob_b));
    CHECK(fi_target_get_params(h, theta_a.data(), n) == FI_OK && fi_target_get_params(b.handle(0), theta_b.data(), n) == FI_OK);
    CHECK(same(blob_a, blob_b) && same(theta_a, theta_b) && std::memcmp(&ta, &tb, sizeof(ta)) == 0);
    CHECK(same(theta_a, params4) && fi_learner_get_params_fp32(h, now.data(), n) == FI_OK && !same(theta_a, now));
    CHECK(ta.updates == 2 && ta.rows == rows && std::isfinite(ta.mean_log_r) && ta.mean_sq_log_r > 0.0);
    CHECK(sa.pg_loss == sb.pg_loss && std::isfinite(sa.total_loss) && sa.grad_norm > 0.0);
    // sync: the copy now; a set / get round trip; a second enable replaces the numbers and keeps the copy
    CHECK(a.sync_target(0) && fi_target_get_params(h, theta_a.data(), n) == FI_OK && same(theta_a, now));
    CHECK(fi_target_set_params(h, params4.data(), n) == FI_OK && fi_target_get_params(h, theta_a.data(), n) == FI_OK);
    CHECK(same(theta_a, params4) && fi_target_set_params(h, params4.data(), n - 1) == FI_ERR_INVALID);
    CHECK(a.enable_target(0, 7u, 0.5f) && a.target_state(0, tp, ts) && tp.period == 7u && tp.tau == 0.5f && ts.updates == 2);

    // enabled and disabled: the surrogate steps of a handle that never enabled it
    DeviceLearner c(lc), d(lc);
    CHECK(c.set_surrogate(0, 0.1f, true) && d.set_surrogate(0, 0.1f, true));
    CHECK(c.enable_target(0, 1u) && c.disable_target(0) && c.target_state(0, tp, ts, &on) && !on && tp.period == 1u);
    CHECK(steps(c, 0, 3) && steps(d, 0, 3));
    std::vector<char> blob_c, blob_d;
    CHECK(c.save_state(0, blob_c) && d.save_state(0, blob_d) && same(blob_c, blob_d) && !same(blob_c, blob_a));
    CHECK(c.target_state(0, tp, ts) && ts.updates == 0 && ts.rows == 0);
    std::printf("target mlp: updates %llu rows %llu mean log r %.17g sq %.17g pg_loss %.17g blob %zu bytes equal\n",
                (unsigned long long)ta.updates, (unsigned long long)ta.rows, ta.mean_log_r, ta.mean_sq_log_r, sa.pg_loss,
                blob_a.size());
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
