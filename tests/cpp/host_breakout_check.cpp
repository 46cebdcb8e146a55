// host_breakout_check.cpp -- a recording Atari DeviceActor driven by a DeviceBreakoutEnv
// (include/freeimpala_amd/device_breakout.hpp over include/fi_breakout.h): the first states are
// written with set_state, two unrolls are enqueued with fi_env_rollout, and a learner handle steps
// from each through fi_learner_step_rollout; a second learner with the same parameters that steps
// from the host copy of the entries must report the same losses. Prints two lines: the 2 T recorded
// actions (step-major), and the stats -- the learner's, the ended episodes and the reward sum of the
// 2 T recorded steps, the byte sum of every environment's plane after them (record T of unroll 1),
// and the environment's own totals after its 2 T + 1 steps. Everything is seeded, so a second run
// prints the same lines, and the numpy rule stepped with the printed actions gives the same stats.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "freeimpala_amd/device_breakout.hpp"

using freeimpala_amd::ActorConfig;
using freeimpala_amd::DeviceActor;
using freeimpala_amd::DeviceBreakoutEnv;

#define CHECK(c)                                                                                       \
    do {                                                                                               \
        if (!(c)) {                                                                                    \
            std::fprintf(stderr, "CHECK failed at line %d: %s (%s)\n", __LINE__, #c, fi_last_error()); \
            return 1;                                                                                  \
        }                                                                                              \
    } while (0)

// the plane record's header: the plane, mu[18], then action, reward, discount
constexpr size_t kPlane = 84 * 84, kRecAct = kPlane + 4 * 18, kRecReward = kRecAct + 4, kRecDiscount = kRecAct + 8;

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
    const int T = 10, N = 3, A = 4, MAX_STEPS = 16;
    Learner dev, host;
    if (make_learner(T, N, A, dev) || make_learner(T, N, A, host)) return 1;
    ActorConfig c;
    c.arch = "atari";
    c.num_envs = N;
    c.num_actions = A;
    c.seed = 12;
    DeviceActor actor(c);
    DeviceBreakoutEnv env(N, 0.99f, 5, MAX_STEPS);
    CHECK(env.max_steps() == MAX_STEPS && env.num_envs() == N);
    // environment 0 goes up into the bricks (a reward on step 2), 1 is near the paddle's row, 2 stays as reset
    DeviceBreakoutEnv::State s;
    CHECK(env.read_state(s));
    CHECK(s.r[2] == 6 && s.dr[2] == 1 && s.t[2] == 0 && s.bricks[2] == 0x7fffffffffffffffull);
    s.r[0] = 7;
    s.dr[0] = -1;
    s.r[1] = 12;
    CHECK(env.set_state(s));
    s.r[1] = 20;
    CHECK(!env.set_state(s) && env.last_error().find("r[1] = 20") != std::string::npos);  // refused, nothing written
    DeviceBreakoutEnv::State back;
    CHECK(env.read_state(back) && back.r[0] == 7 && back.r[1] == 12 && back.dr[0] == -1);
    std::vector<char> blob(fi_learner_param_bytes(dev.h));
    uint64_t version = 0;
    CHECK(fi_learner_get_params(dev.h, blob.data(), blob.size(), &version) == FI_OK);
    CHECK(actor.load(blob, 0));
    CHECK(actor.begin_rollout(T));
    fi_step_stats sd{}, sh{};
    std::vector<int32_t> actions;
    std::vector<unsigned long long> plane_sums(N, 0);
    int ended = 0;
    double reward_sum = 0;
    int32_t done = -1;
    for (int k = 0; k < 2; ++k) {
        CHECK(env.rollout(actor, k == 0 ? T + 1 : T, &done) && done == (k == 0 ? T + 1 : T));
        CHECK(actor.rollout_ready());
        std::vector<uint8_t> entries;
        CHECK(actor.read_rollout(entries));
        CHECK(fi_learner_step_rollout(dev.h, actor.handle(), &sd) == FI_OK);
        CHECK(!actor.rollout_ready() && fi_learner_staging_bytes(dev.h) == 0);
        const size_t eb = actor.rollout_entry_bytes();
        std::vector<const void*> ptrs(N);
        for (int i = 0; i < N; ++i) ptrs[i] = entries.data() + (size_t)i * eb;
        CHECK(fi_learner_step(host.h, ptrs.data(), ptrs.size(), eb, &sh) == FI_OK);
        CHECK(sd.total_loss == sh.total_loss && sd.grad_norm == sh.grad_norm && sd.version == sh.version);
        for (int t = 0; t < T; ++t)
            for (int i = 0; i < N; ++i) {
                const uint8_t* rec = entries.data() + (size_t)i * eb + (size_t)t * FI_ATARI_PLANE_RECORD_BYTES;
                int32_t a;
                float rew, disc;
                std::memcpy(&a, rec + kRecAct, 4);
                std::memcpy(&rew, rec + kRecReward, 4);
                std::memcpy(&disc, rec + kRecDiscount, 4);
                CHECK(a >= 0 && a < A && (rew == 0.f || rew == 1.f) && (disc == 0.f || disc == 0.99f));
                actions.push_back(a);
                ended += disc == 0.f;
                reward_sum += rew;
            }
        if (k == 1)
            for (int i = 0; i < N; ++i) {
                const uint8_t* plane = entries.data() + (size_t)i * eb + (size_t)T * FI_ATARI_PLANE_RECORD_BYTES;
                for (size_t b = 0; b < kPlane; ++b) plane_sums[i] += plane[b];
            }
    }
    int64_t bad = -1;
    CHECK(actor.sync(&bad) && bad == 0);
    uint64_t episodes = 0;
    int64_t scores = 0;
    CHECK(env.stats(episodes, scores));
    // the environment took one step more than the records hold outcomes of
    CHECK(episodes >= (uint64_t)ended && episodes <= (uint64_t)(ended + N) && scores >= 0);
    CHECK(actor.end_rollout());
    std::printf("breakout actions:");
    for (int32_t a : actions) std::printf(" %d", a);
    std::printf("\nbreakout atari: loss %.9g grad_norm %.9g version %llu recorded_episodes %d recorded_rewards %d plane_sums",
                sd.total_loss, sd.grad_norm, (unsigned long long)sd.version, ended, (int)reward_sum);
    for (int i = 0; i < N; ++i) std::printf(" %llu", plane_sums[i]);
    std::printf(" final_episodes %llu final_scores %lld\n", (unsigned long long)episodes, (long long)scores);
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
