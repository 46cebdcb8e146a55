// host_kl_check.cpp -- the adaptive KL penalty (include/fi_kl.h) through the C++ host side. The refusals,
// which come before any device call, and the getters before fi_kl_enable; two DeviceLearners (MLP) take
// four V-trace steps with the penalty on the behaviour policy and an adapting coefficient on the same
// synthetic batches and end with the same state blob and the same block, byte for byte; the coefficient
// moved; set_kl_coeff and a second enable; then the first disables the penalty and takes two further steps
// beside a twin that is given its state and never heard of the penalty: the same blob, and the block
// keeps its bytes. Prints one line; everything is seeded, so a second run prints the same line.
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
        if (fi_learner_synth_batch(h, 70 + (uint64_t)k, 0, 0) != FI_OK) return false;
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
    fi_kl_params kp{};
    fi_kl_stats ks{};
    const void* dev = nullptr;
    CHECK(!a.kl_state(0, kp, ks) && a.last_error().find("never on") != std::string::npos);
    CHECK(fi_kl_state_dev(h, &dev) == FI_ERR_STATE && fi_kl_set_coeff(h, 1.0) == FI_ERR_STATE);
    const fi_kl_params p{FI_KL_REF_BEHAVIOUR, 1u,           FI_KL_COEFF,     FI_KL_TARGET,
                         FI_KL_BAND,          FI_KL_FACTOR, FI_KL_COEFF_MIN, FI_KL_COEFF_MAX};
    CHECK(fi_kl_enable(nullptr, &p) == FI_ERR_INVALID && fi_kl_enable(h, nullptr) == FI_ERR_INVALID);
    for (float bad : {-1.f, inf, nan}) {
        fi_kl_params q = p;
        q.coeff = bad;
        CHECK(fi_kl_enable(h, &q) == FI_ERR_INVALID);
    }
    for (float bad : {0.f, -0.01f, nan}) {
        fi_kl_params q = p;
        q.kl_target = bad;
        CHECK(fi_kl_enable(h, &q) == FI_ERR_INVALID);
    }
    for (float bad : {1.f, 0.5f, nan}) {
        fi_kl_params q = p, r = p;
        q.band = bad;
        r.factor = bad;
        CHECK(fi_kl_enable(h, &q) == FI_ERR_INVALID && fi_kl_enable(h, &r) == FI_ERR_INVALID);
    }
    {
        fi_kl_params q = p, r = p, s = p;
        q.coeff_min = 0.f;
        r.coeff_min = 2.f, r.coeff_max = 1.f;
        s.reference = 2u;
        CHECK(fi_kl_enable(h, &q) == FI_ERR_INVALID && fi_kl_enable(h, &r) == FI_ERR_INVALID && fi_kl_enable(h, &s) == FI_ERR_INVALID);
    }
    CHECK(!a.enable_kl_penalty(0, FI_KL_REF_TARGET) && a.last_error().find("fi_target_enable") != std::string::npos);
    CHECK(fi_kl_disable(h) == FI_OK);                     // nothing to turn off
    CHECK(fi_kl_state_dev(h, &dev) == FI_ERR_STATE);      // none of the refused calls made a block
    CHECK(fi_kl_workspace_bytes(100, 4096, 18) >= 64 * sizeof(double) && fi_kl_workspace_bytes(100, 4096, 18) % 256 == 0);
    CHECK(fi_kl_workspace_bytes(5, 24, 1) == 0 && fi_kl_workspace_bytes(5, 24, 65) == 0 && fi_kl_workspace_bytes(0, 24, 6) == 0);

    // two handles, four V-trace steps with the penalty on mu and an adapting coefficient: the same bytes
    DeviceLearner b(lc);
    bool on = false;
    CHECK(a.enable_kl_penalty(0) && b.enable_kl_penalty(0));
    CHECK(a.kl_state(0, kp, ks, &on) && on && kp.reference == FI_KL_REF_BEHAVIOUR && kp.adapt == 1u && kp.kl_target == FI_KL_TARGET);
    CHECK(ks.coeff == 1.0 && ks.updates == 0 && ks.rows == 0 && ks.raised == 0 && ks.lowered == 0);
    CHECK(fi_kl_state_dev(h, &dev) == FI_OK && dev != nullptr);
    fi_step_stats sa{}, sb{};
    fi_kl_stats ka{}, kb{};
    CHECK(steps(a, 0, 4, &sa) && steps(b, 0, 4, &sb) && a.kl_state(0, kp, ka) && b.kl_state(0, kp, kb));
    std::vector<char> blob_a, blob_b;
    CHECK(a.save_state(0, blob_a) && b.save_state(0, blob_b));
    CHECK(same(blob_a, blob_b) && std::memcmp(&ka, &kb, sizeof(ka)) == 0 && sa.pg_loss == sb.pg_loss);
    CHECK(ka.updates == 4 && ka.rows == rows && std::isfinite(ka.mean_kl) && ka.mean_kl > 0.0 && ka.mean_kl == ka.kl_sum / (double)rows);
    CHECK(ka.raised + ka.lowered >= 1 && ka.coeff == std::ldexp(1.0, (int)ka.raised - (int)ka.lowered));
    // the coefficient from the host, behind the steps; a second enable replaces the parameters and keeps it
    CHECK(b.set_kl_coeff(0, 0.375) && b.kl_state(0, kp, kb) && kb.coeff == 0.375 && kb.updates == 4);
    CHECK(!b.set_kl_coeff(0, -1.0) && !b.set_kl_coeff(0, (double)nan));
    CHECK(b.enable_kl_penalty(0, FI_KL_REF_BEHAVIOUR, 8.f, 0.5f, false) && b.kl_state(0, kp, kb));
    CHECK(kb.coeff == 0.375 && kp.kl_target == 0.5f && kp.adapt == 0u);

    // disabled: two further steps are the steps of a twin that is given the state and never enabled it
    DeviceLearner c(lc);
    CHECK(a.disable_kl_penalty(0) && a.kl_state(0, kp, ks, &on) && !on && c.load_state(0, blob_a));
    CHECK(steps(a, 4, 2) && steps(c, 4, 2));
    std::vector<char> blob_c;
    CHECK(a.save_state(0, blob_a) && c.save_state(0, blob_c) && same(blob_a, blob_c) && !same(blob_a, blob_b));
    CHECK(a.kl_state(0, kp, ks) && std::memcmp(&ks, &ka, sizeof(ks)) == 0);  // the block keeps its bytes
    std::printf("kl mlp: coeff %.17g updates %llu raised %u lowered %u mean kl %.17g pg_loss %.17g blob %zu bytes equal\n",
                ka.coeff, (unsigned long long)ka.updates, ka.raised, ka.lowered, ka.mean_kl, sa.pg_loss, blob_a.size());
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
