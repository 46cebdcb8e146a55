// host_train_check.cpp -- the training recipe (include/fi_train.h) through the C++ host side
// (include/freeimpala_amd/device_learner.hpp): an MLP learner built from command-line flags with
// RMSProp, a learning-rate schedule and a reward clip steps three synthetic batches and saves its
// state; a second learner built from the same flags loads it; both step twice more and must hold
// the same parameters and the same two moment slabs, byte for byte. Prints OK, exits non-zero on
// any mismatch.
//
//   host_train_check        the whole check (needs the GPU)
//   host_train_check flags  the flag parsing alone (no GPU)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "freeimpala_amd/device_learner.hpp"

using freeimpala_amd::DeviceLearner;
using freeimpala_amd::LearnerConfig;

#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) {                                                              \
            std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #c); \
            return 1;                                                            \
        }                                                                        \
    } while (0)

// a batch in the MLP record schema (obs@0, mu@512, act@768, rew@772, disc@776), rewards up to +-3
static std::vector<std::vector<char>> make_batch(size_t M, int T, int A, int D, uint64_t seed) {
    uint64_t x = 0x9E3779B97F4A7C15ull ^ (seed * 0xD1342543DE82EF95ull);
    auto next = [&x]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    auto unif = [&]() { return (float)((next() >> 40) * (1.0 / 16777216.0)) * 2.f - 1.f; };
    std::vector<std::vector<char>> batch(M, std::vector<char>((size_t)(T + 1) * FI_RECORD_BYTES, 0));
    for (size_t b = 0; b < M; ++b)
        for (int t = 0; t <= T; ++t) {
            char* rec = batch[b].data() + (size_t)t * FI_RECORD_BYTES;
            for (int i = 0; i < D; ++i) {
                const float v = 1.5f * unif();
                std::memcpy(rec + 4 * i, &v, 4);
            }
            for (int i = 0; i < A; ++i) {
                const float v = 2.f * unif();
                std::memcpy(rec + 512 + 4 * i, &v, 4);
            }
            const int32_t act = (int32_t)(next() % (uint64_t)A);
            const float rew = 3.f * unif();
            const float disc = (next() % 10) == 0 ? 0.f : 0.99f;
            std::memcpy(rec + 768, &act, 4);
            std::memcpy(rec + 772, &rew, 4);
            std::memcpy(rec + 776, &disc, 4);
        }
    return batch;
}

static const char* kArgs[] = {"host_train_check", "--batch-size", "8", "--seq-length", "4", "--learner-arch", "mlp",
                              "--num-actions", "3", "--obs-dim", "7", "--hidden", "32", "--lr", "0.002",
                              "--optimizer", "rmsprop", "--rms-decay", "0.9", "--rms-momentum", "0.5", "--rms-eps", "0.001",
                              "--rms-eps-in-sqrt", "1", "--lr-end", "0.0005", "--lr-steps", "4", "--reward-clip", "1"};
static constexpr int kArgc = (int)(sizeof(kArgs) / sizeof(kArgs[0]));

template <class F>
static bool throws_invalid(F&& f) {
    try {
        f();
    } catch (const std::invalid_argument&) {
        return true;
    }
    return false;
}

static int flags_check() {
    const LearnerConfig c = LearnerConfig::from_args(kArgc, kArgs);
    CHECK(c.optimizer == "rmsprop" && c.rms_decay == 0.9f && c.rms_momentum == 0.5f && c.rms_eps == 0.001f);
    CHECK(c.rms_eps_in_sqrt && c.lr_schedule && c.lr_end == 0.0005f && c.lr_steps == 4 && c.reward_clip == 1.f);
    CHECK(c.abi_config(0).optimizer == FI_OPT_SGD);  // created as sgd is, then switched
    const char* plain[] = {"x", "--optimizer", "sgd"};
    const LearnerConfig d = LearnerConfig::from_args(3, plain);
    CHECK(!d.lr_schedule && d.reward_clip == 0.f && d.optimizer == "sgd");
    CHECK(throws_invalid([] {
        const char* a[] = {"x", "--lr-end", "0"};
        LearnerConfig::from_args(3, a);
    }));
    CHECK(throws_invalid([] {
        const char* a[] = {"x", "--lr-steps", "10"};
        LearnerConfig::from_args(3, a);
    }));
    CHECK(throws_invalid([] {
        const char* a[] = {"x", "--lr-end", "0", "--lr-steps", "0"};
        LearnerConfig::from_args(5, a);
    }));
    CHECK(throws_invalid([] {
        const char* a[] = {"x", "--optimizer", "rmsprop", "--rms-decay", "1"};
        LearnerConfig::from_args(5, a);
    }));
    CHECK(throws_invalid([] {
        const char* a[] = {"x", "--reward-clip", "-1"};
        LearnerConfig::from_args(3, a);
    }));
    CHECK(throws_invalid([] {
        const char* a[] = {"x", "--optimizer", "lion"};
        LearnerConfig::from_args(3, a);
    }));
    return 0;
}

static bool read(DeviceLearner& L, const char* name, std::vector<char>& out) {
    out.resize(L.param_count() * 4);
    return fi_learner_read_tensor(L.handle(0), name, out.data(), out.size()) == FI_OK;
}

static int gpu_check() {
    const LearnerConfig c = LearnerConfig::from_args(kArgc, kArgs);
    const int T = (int)c.seq_length, A = c.num_actions, D = c.obs_dim;
    std::vector<std::vector<std::vector<char>>> batches;
    for (uint64_t k = 0; k < 5; ++k) batches.push_back(make_batch(c.batch_size, T, A, D, k + 1));

    DeviceLearner X(c);
    fi_train_state st{};
    CHECK(fi_train_get_state(X.handle(0), &st) == FI_OK);
    CHECK(st.optimizer == FI_TRAIN_OPT_RMSPROP && st.eps_in_sqrt == 1 && st.decay == 0.9f && st.momentum == 0.5f);
    CHECK(st.schedule_on == 1 && st.lr_steps == 4 && st.lr_end == 0.0005f && st.reward_clip == 1.f);
    CHECK(st.next_update == 1 && st.lr_next == 0.002f);
    for (int k = 0; k < 3; ++k) {
        if (!X.step(0, batches[k])) std::fprintf(stderr, "step failed: %s\n", X.last_error(0).c_str());
        CHECK(X.last_error(0).empty());
    }
    CHECK(fi_train_get_state(X.handle(0), &st) == FI_OK);
    CHECK(st.next_update == 4 && st.lr_next == (float)(0.002f + ((double)0.0005f - (double)0.002f) * 3.0 / 4.0));
    std::vector<char> rew((size_t)T * c.batch_size * 4);
    CHECK(fi_learner_read_tensor(X.handle(0), "rewards", rew.data(), rew.size()) == FI_OK);
    bool at_bound = false;
    for (size_t i = 0; i < rew.size(); i += 4) {
        float r;
        std::memcpy(&r, rew.data() + i, 4);
        CHECK(r >= -1.f && r <= 1.f);
        at_bound = at_bound || r == 1.f || r == -1.f;
    }
    CHECK(at_bound);
    CHECK(fi_train_set_rmsprop(X.handle(0), 0.9f, 0.f, 0.01f, 0) == FI_ERR_STATE);

    std::vector<char> blob;
    CHECK(X.save_state(0, blob));
    DeviceLearner Y(c);  // the same flags make the same fi_train_* calls; then the state
    CHECK(Y.load_state(0, blob));
    CHECK(fi_train_get_state(Y.handle(0), &st) == FI_OK && st.next_update == 4);
    for (int k = 3; k < 5; ++k) CHECK(X.step(0, batches[k]) && Y.step(0, batches[k]));
    CHECK(X.last_stats(0).version == 5 && Y.last_stats(0).version == 5);
    CHECK(fi_train_get_state(Y.handle(0), &st) == FI_OK && st.next_update == 6 && st.lr_next == 0.0005f);

    std::vector<char> px, py, mx, my, vx, vy;
    uint64_t va = 0, vb = 0;
    CHECK(X.publish(0, px, va) && Y.publish(0, py, vb) && va == vb);
    CHECK(read(X, "adam_m", mx) && read(Y, "adam_m", my) && read(X, "adam_v", vx) && read(Y, "adam_v", vy));
    CHECK(px == py);
    CHECK(mx == my);
    CHECK(vx == vy);
    bool m_set = false, v_set = false;
    for (char b : mx) m_set = m_set || b != 0;
    for (char b : vx) v_set = v_set || b != 0;
    CHECK(m_set && v_set);  // the momentum buffer and the mean square are in use
    return 0;
}

int main(int argc, char** argv) {
    try {
        if (int rc = flags_check()) return rc;
        if (argc > 1 && std::string(argv[1]) == "flags") {
            std::printf("OK flags\n");
            return 0;
        }
        if (int rc = gpu_check()) return rc;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
