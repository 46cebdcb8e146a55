// host_diag_check.cpp -- the off-policy diagnostics (include/fi_diag.h) through the C++ host side: a
// DeviceLearner (MLP, SGD with a learning rate of 0, so its parameters never move) steps the synthetic
// resident batch, then steps host entries built from that batch with the behaviour logits replaced
// by the policy's own logits of the first step. The second step is on-policy bit for bit, and the
// diagnostics must say so exactly: mean_log_rho = kl = 0, rho = ess = 1, nothing clipped, equal
// entropies. Also the error codes: a call before any step, a read without an enqueue, a wrong column
// count. Prints one line; everything is seeded, so a second run prints the same line.
#include <cmath>
#include <cstdio>
#include <cstring>
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

template <class T>
static bool read(fi_learner* h, const char* name, std::vector<T>& v, size_t n) {
    v.resize(n);
    return fi_learner_read_tensor(h, name, v.data(), n * sizeof(T)) == FI_OK;
}

static int run() {
    const int T = 6, B = 72, A = 18, D = 128;  // two column tiles, the second partial
    LearnerConfig lc;
    lc.batch_size = B;
    lc.seq_length = T;
    lc.num_actions = A;
    lc.obs_dim = D;
    lc.optimizer = "sgd";
    lc.lr = 0.f;
    lc.seed = 9;
    DeviceLearner learner(lc);
    fi_learner* h = learner.handle(0);

    // the error codes: nothing has stepped, nothing was enqueued
    fi_offpolicy_diag d{};
    std::vector<float> ckl, clr;
    CHECK(fi_diag_enqueue(h) == FI_ERR_STATE);
    CHECK(fi_diag_read(h, &d, nullptr, nullptr, 0) == FI_ERR_STATE);
    CHECK(!learner.diagnostics(0, d) && learner.last_error().find("no step") != std::string::npos);
    CHECK(fi_diag_enqueue(nullptr) == FI_ERR_INVALID && fi_diag_read(h, nullptr, nullptr, nullptr, 0) == FI_ERR_INVALID);
    int ct = 0, ts = 0;
    CHECK(fi_diag_plan(T, B, A, &ct, &ts) == FI_OK && ct == 2 && ts == 2);
    CHECK(fi_diag_plan(T, B, 65, &ct, &ts) == FI_ERR_INVALID && fi_diag_workspace_bytes(T, B, 1) == 0);
    CHECK(fi_diag_workspace_bytes(T, B, A) > 0);

    // step 1: the synthetic batch, mu random
    CHECK(fi_learner_synth_batch(h, 4, 0, 0) == FI_OK);
    fi_step_stats st{};
    CHECK(fi_learner_step_resident(h, &st) == FI_OK);
    CHECK(fi_diag_read(h, &d, nullptr, nullptr, 0) == FI_ERR_STATE);  // a step, but still no enqueue
    CHECK(learner.diagnostics(0, d, &ckl, &clr));
    CHECK(d.struct_size == sizeof(fi_offpolicy_diag) && d.rows == (uint64_t)T * B && d.rows_used == d.rows);
    CHECK(d.kl_mu_pi > 0.0 && d.ess > 0.0 && d.ess < 1.0 && d.max_rho > 1.0 && d.min_rho < 1.0);
    CHECK(ckl.size() == (size_t)B && clr.size() == (size_t)B && ckl[B - 1] > 0.f);
    const double kl_off = d.kl_mu_pi;
    CHECK(fi_diag_read(h, &d, ckl.data(), nullptr, B + 1) == FI_ERR_INVALID);

    // host entries of the same batch (the MLP record: obs at 0, mu at 512, action / reward / discount
    // at 768 / 772 / 776) with mu := the logits step 1 computed
    std::vector<float> obs, logits, rew, disc;
    std::vector<int32_t> act;
    CHECK(read(h, "obs", obs, (size_t)(T + 1) * B * D) && read(h, "logits", logits, (size_t)(T + 1) * B * A));
    CHECK(read(h, "actions", act, (size_t)T * B) && read(h, "rewards", rew, (size_t)T * B) &&
          read(h, "discounts", disc, (size_t)T * B));
    std::vector<std::vector<char>> batch(B, std::vector<char>((size_t)(T + 1) * 1024, 0));
    for (int b = 0; b < B; ++b)
        for (int t = 0; t <= T; ++t) {
            char* rec = batch[b].data() + (size_t)t * 1024;
            const size_t e = (size_t)t * B + b;
            std::memcpy(rec, &obs[e * D], sizeof(float) * D);
            if (t == T) continue;
            std::memcpy(rec + 512, &logits[e * A], sizeof(float) * A);
            std::memcpy(rec + 768, &act[e], 4);
            std::memcpy(rec + 772, &rew[e], 4);
            std::memcpy(rec + 776, &disc[e], 4);
        }
    // step 2, enqueue, and a third step behind it before the read: the result is step 2's
    CHECK(learner.step(0, batch));
    CHECK(learner.enqueue_diagnostics(0));
    CHECK(fi_learner_synth_batch(h, 5, 0, 0) == FI_OK);
    CHECK(fi_learner_step_resident(h, nullptr) == FI_OK);
    CHECK(learner.read_diagnostics(0, d, &ckl, &clr));
    CHECK(d.rows_used == (uint64_t)T * B && d.rows_bad_action == 0 && d.rows_nonfinite == 0);
    CHECK(d.mean_log_rho == 0.0 && d.kl_mu_pi == 0.0 && d.mean_rho == 1.0 && d.max_rho == 1.0 && d.min_rho == 1.0);
    CHECK(d.ess == 1.0 && d.n_rho_clipped == 0 && d.n_c_clipped == 0 && d.n_pg_clipped == 0);
    CHECK(d.entropy_pi == d.entropy_mu && d.entropy_pi > 0.0 && std::isfinite(d.explained_variance));
    for (int b = 0; b < B; ++b) CHECK(ckl[b] == 0.f && clr[b] == 0.f);
    std::printf("diag mlp: off-policy kl %.9g on-policy kl %.9g ess %.9g entropy %.9g ev %.9g ends %llu\n", kl_off, d.kl_mu_pi,
                d.ess, d.entropy_pi, d.explained_variance, (unsigned long long)d.n_episode_ends);
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
