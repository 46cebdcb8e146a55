// host_rollout_check.cpp -- one MLP unroll and one Atari unroll recorded on the device by a
// DeviceActor (include/freeimpala_amd/device_actor.hpp) and stepped by a learner handle through
// fi_learner_step_rollout (include/fi_rollout.h): no entry ever exists in host memory. After each
// step the entries are read back once, and a second learner with the same parameters that steps
// from that host copy must report the same losses. Prints one line per policy; everything is
// seeded, so a second run prints the same lines.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "freeimpala_amd/device_actor.hpp"

using freeimpala_amd::ActorConfig;
using freeimpala_amd::ActResult;
using freeimpala_amd::DeviceActor;

#define CHECK(c)                                                                                       \
    do {                                                                                               \
        if (!(c)) {                                                                                    \
            std::fprintf(stderr, "CHECK failed at line %d: %s (%s)\n", __LINE__, #c, fi_last_error()); \
            return 1;                                                                                  \
        }                                                                                              \
    } while (0)

static uint64_t g_x = 0x9E3779B97F4A7C15ull;
static uint64_t next() {
    g_x ^= g_x << 13;
    g_x ^= g_x >> 7;
    g_x ^= g_x << 17;
    return g_x;
}

struct Learner {
    fi_learner* h = nullptr;
    ~Learner() { fi_learner_destroy(h); }
};

static int make_learner(int arch, int T, int B, int A, int D, Learner& out) {
    fi_learner_config c;
    fi_learner_config_init(&c);
    c.arch = arch;
    c.seq_len = T;
    c.batch = B;
    c.num_actions = A;
    c.obs_dim = D;
    c.seed = 7;
    CHECK(fi_learner_create(&c, &out.h) == FI_OK);
    if (arch == FI_ARCH_ATARI) CHECK(fi_learner_set_record_format(out.h, FI_RECORDS_PLANES) == FI_OK);
    return 0;
}

// T+1 act calls with their outcomes on `actor`, then both learners step: `dev` from the device
// entries, `host` from their host copy
static int run(const char* name, DeviceActor& actor, int T, Learner& dev, Learner& host) {
    const ActorConfig& c = actor.config();
    const int N = c.num_envs;
    const bool atari = c.arch == "atari";
    std::vector<char> blob(fi_learner_param_bytes(dev.h));
    uint64_t version = 0;
    CHECK(fi_learner_get_params(dev.h, blob.data(), blob.size(), &version) == FI_OK);
    CHECK(actor.load(blob, 0));
    CHECK(actor.begin_rollout(T));
    CHECK(actor.rollout_entry_bytes() == fi_learner_entry_bytes(dev.h));
    fi_step_stats sd{}, sh{};
    CHECK(fi_learner_step_rollout(dev.h, actor.handle(), &sd) == FI_ERR_STATE);  // nothing recorded yet
    ActResult r;
    std::vector<float> obs((size_t)N * c.obs_dim), rew(N), disc(N);
    std::vector<uint8_t> planes((size_t)N * DeviceActor::kPlaneBytes), start(N);
    for (int t = 0; t <= T; ++t) {
        CHECK(!actor.rollout_ready());
        if (atari) {
            for (uint8_t& v : planes) v = (uint8_t)(next() >> 56);
            for (int i = 0; i < N; ++i) start[i] = t == 0 || (t == 2 && i == 1);
            CHECK(actor.act_planes(planes, start, r));
            if (t == 0) CHECK(!actor.act_planes(planes, start, r));  // refused: no outcome yet
        } else {
            for (float& v : obs) v = (float)((next() >> 40) * (1.0 / 16777216.0)) * 2.f - 1.f;
            CHECK(actor.act_obs(obs, r));
        }
        for (int i = 0; i < N; ++i) {
            rew[i] = (float)(int)(next() % 3) - 1.f;
            disc[i] = next() % 5 ? 0.99f : 0.f;
        }
        CHECK(actor.outcome(rew, disc));
        CHECK(!actor.outcome(rew, disc));  // refused: one outcome per step
    }
    CHECK(actor.rollout_ready());
    std::vector<uint8_t> entries;
    CHECK(actor.read_rollout(entries));
    CHECK(fi_learner_step_rollout(dev.h, actor.handle(), &sd) == FI_OK);
    CHECK(!actor.rollout_ready());                  // released
    CHECK(fi_learner_staging_bytes(dev.h) == 0);   // and no staging buffer was ever allocated
    const size_t eb = actor.rollout_entry_bytes();
    std::vector<const void*> ptrs(N);
    for (int i = 0; i < N; ++i) ptrs[i] = entries.data() + (size_t)i * eb;
    CHECK(fi_learner_step(host.h, ptrs.data(), ptrs.size(), eb, &sh) == FI_OK);
    CHECK(sd.total_loss == sh.total_loss && sd.grad_norm == sh.grad_norm && sd.version == sh.version);
    CHECK(actor.end_rollout());
    std::printf("rollout %s: loss %.9g grad_norm %.9g version %llu\n", name, sd.total_loss, sd.grad_norm,
                (unsigned long long)sd.version);
    return 0;
}

int main() {
    try {
        {
            const int T = 4, N = 5, A = 18, D = 128;
            Learner dev, host;
            if (make_learner(FI_ARCH_MLP, T, N, A, D, dev) || make_learner(FI_ARCH_MLP, T, N, A, D, host)) return 1;
            ActorConfig c;
            c.num_envs = N;
            c.num_actions = A;
            c.obs_dim = D;
            c.seed = 11;
            DeviceActor actor(c);
            if (run("mlp", actor, T, dev, host)) return 1;
        }
        {
            const int T = 3, N = 3, A = 6;
            Learner dev, host;
            if (make_learner(FI_ARCH_ATARI, T, N, A, 128, dev) || make_learner(FI_ARCH_ATARI, T, N, A, 128, host)) return 1;
            ActorConfig c;
            c.arch = "atari";
            c.num_envs = N;
            c.num_actions = A;
            c.seed = 12;
            DeviceActor actor(c);
            if (run("atari", actor, T, dev, host)) return 1;
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
