// host_surrogate_check.cpp -- the clipped surrogate objective (include/fi_surrogate.h) through the C++
// host side. The refusals, which come before any device call, and the neutral state of a handle that
// never enabled it; two DeviceLearners (MLP) take three surrogate steps with normalised advantages on
// the same synthetic batches and end with the same state blob and the same stats block, byte for byte;
// a third enables the objective, clears it and takes the V-trace steps of a fourth that never heard of
// it: the same blob. Prints one line; everything is seeded, so a second run prints the same line.
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

static bool steps(DeviceLearner& L, int count, fi_step_stats* last = nullptr) {
    fi_learner* h = L.handle(0);
    for (int k = 0; k < count; ++k) {
        if (fi_learner_synth_batch(h, 70 + (uint64_t)k, 0, 0) != FI_OK) return false;
        fi_step_stats st{};
        if (fi_learner_step_resident(h, &st) != FI_OK) return false;
        if (last) *last = st;
    }
    return true;
}

static bool same(const std::vector<char>& a, const std::vector<char>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size()) == 0;
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
    fi_surrogate_state s{};
    CHECK(a.surrogate_state(0, s) && s.enabled == 0 && s.normalize == 0 && s.rows == 0 && s.rows_clipped == 0);
    CHECK(s.clip == FI_SURROGATE_CLIP && s.adv_eps == FI_SURROGATE_ADV_EPS);
    const void* dev = nullptr;
    CHECK(fi_surrogate_stats_dev(h, &dev) == FI_ERR_STATE);
    fi_surrogate_params p{FI_SURROGATE_CLIP, 0u, FI_SURROGATE_ADV_EPS, 0u};
    CHECK(fi_surrogate_enable(nullptr, &p) == FI_ERR_INVALID && fi_surrogate_enable(h, nullptr) == FI_ERR_INVALID);
    for (float bad : {0.f, -0.2f, inf, nan}) {
        fi_surrogate_params q = p;
        q.clip = bad;
        CHECK(fi_surrogate_enable(h, &q) == FI_ERR_INVALID);
    }
    for (float bad : {-1e-8f, inf, nan}) {
        fi_surrogate_params q = p;
        q.adv_eps = bad;
        CHECK(fi_surrogate_enable(h, &q) == FI_ERR_INVALID);
    }
    {
        fi_surrogate_params q = p;
        q.normalize = 2u;
        CHECK(fi_surrogate_enable(h, &q) == FI_ERR_INVALID);
    }
    CHECK(!a.set_surrogate(0, -1.f) && a.last_error().find("clip") != std::string::npos);
    CHECK(a.surrogate_state(0, s) && s.enabled == 0);
    CHECK(fi_surrogate_disable(h) == FI_OK);  // nothing to turn off
    CHECK(fi_surrogate_loss_blocks(100, 4096, 18) > 0 && fi_surrogate_workspace_bytes(100, 4096, 18) > 3u * 409600u * 4u);
    CHECK(fi_surrogate_loss_blocks(5, 24, 1) == 0 && fi_surrogate_workspace_bytes(5, 24, 65) == 0);

    // two handles, three normalising surrogate steps each: the same bytes
    DeviceLearner b(lc);
    fi_step_stats sa{}, sb{};
    CHECK(a.set_surrogate(0, 0.1f, true) && b.set_surrogate(0, 0.1f, true));
    CHECK(fi_surrogate_stats_dev(h, &dev) == FI_OK && dev != nullptr);
    CHECK(a.surrogate_state(0, s) && s.enabled == 1 && s.normalize == 1 && s.clip == 0.1f && s.rows == 0);
    CHECK(steps(a, 3, &sa) && steps(b, 3, &sb));
    fi_surrogate_state ta{}, tb{};
    std::vector<char> blob_a, blob_b;
    CHECK(a.surrogate_state(0, ta) && b.surrogate_state(0, tb) && a.save_state(0, blob_a) && b.save_state(0, blob_b));
    CHECK(same(blob_a, blob_b) && std::memcmp(&ta, &tb, sizeof(ta)) == 0);
    CHECK(ta.rows == rows && ta.rows_clipped <= rows && std::isfinite(ta.adv_mean) && ta.adv_std > 0.0);
    CHECK(sa.pg_loss == sb.pg_loss && std::isfinite(sa.total_loss) && sa.grad_norm > 0.0);
    // a second enable replaces the parameters; the stats block stays
    CHECK(a.set_surrogate(0, 0.3f, false) && a.surrogate_state(0, s));
    CHECK(s.clip == 0.3f && s.normalize == 0 && s.rows == rows && s.rows_clipped == ta.rows_clipped);

    // enabled and cleared: the V-trace steps of a handle that never enabled it
    DeviceLearner c(lc), d(lc);
    CHECK(c.set_surrogate(0) && c.clear_surrogate(0) && c.surrogate_state(0, s) && s.enabled == 0 && s.clip == FI_SURROGATE_CLIP);
    CHECK(steps(c, 3) && steps(d, 3));
    std::vector<char> blob_c, blob_d;
    CHECK(c.save_state(0, blob_c) && d.save_state(0, blob_d) && same(blob_c, blob_d) && !same(blob_c, blob_a));
    std::printf("surrogate mlp: rows %llu clipped %llu adv mean %.17g std %.17g pg_loss %.17g blob %zu bytes equal\n",
                (unsigned long long)ta.rows, (unsigned long long)ta.rows_clipped, ta.adv_mean, ta.adv_std, sa.pg_loss,
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
