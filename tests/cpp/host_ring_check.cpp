// host_ring_check.cpp -- an MLP actor, then an Atari actor, records two unrolls and pushes each into
// a device entry ring (include/freeimpala_amd/device_ring.hpp over include/fi_ring.h) before any
// learner step: without the ring the second unroll could not complete. A learner then steps twice
// from the ring, once FIFO (n_fresh = batch) and once mixed (half fresh, half replayed). Exit 0
// only if both steps return FI_OK and the entries each step chose equal the batch rule computed
// here on the host. Prints one line per policy; everything is seeded, so a second run prints the
// same lines.
#include <cstdio>
#include <string>
#include <vector>

#include "freeimpala_amd/device_ring.hpp"

using freeimpala_amd::ActorConfig;
using freeimpala_amd::ActResult;
using freeimpala_amd::DeviceActor;
using freeimpala_amd::DeviceRing;

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

// `steps` act calls with their outcomes
static int act(DeviceActor& actor, int steps) {
    const ActorConfig& c = actor.config();
    const int N = c.num_envs;
    ActResult r;
    std::vector<float> obs((size_t)N * c.obs_dim), rew(N), disc(N);
    std::vector<uint8_t> planes((size_t)N * DeviceActor::kPlaneBytes), start(N);
    for (int t = 0; t < steps; ++t) {
        if (c.arch == "atari") {
            for (uint8_t& v : planes) v = (uint8_t)(next() >> 56);
            for (int i = 0; i < N; ++i) start[i] = t == 0 || (t == 2 && i == 1);
            CHECK(actor.act_planes(planes, start, r));
        } else {
            for (float& v : obs) v = (float)((next() >> 40) * (1.0 / 16777216.0)) * 2.f - 1.f;
            CHECK(actor.act_obs(obs, r));
        }
        for (int i = 0; i < N; ++i) {
            rew[i] = (float)(int)(next() % 3) - 1.f;
            disc[i] = next() % 5 ? 0.99f : 0.f;
        }
        CHECK(actor.outcome(rew, disc));
    }
    return 0;
}

static std::string join(const std::vector<uint64_t>& v) {
    std::string s;
    for (uint64_t e : v) s += (s.empty() ? "" : ",") + std::to_string(e);
    return s;
}

static int policy(const char* name, int arch, int T, int N, int A, int D) {
    Learner learner;
    if (make_learner(arch, T, N, A, D, learner)) return 1;
    ActorConfig c;
    c.arch = name;
    c.num_actions = A;
    c.obs_dim = D;
    c.num_envs = N;
    c.seed = 11;
    DeviceActor actor(c);
    std::vector<char> blob(fi_learner_param_bytes(learner.h));
    uint64_t version = 0;
    CHECK(fi_learner_get_params(learner.h, blob.data(), blob.size(), &version) == FI_OK);
    CHECK(actor.load(blob, 4));
    CHECK(actor.begin_rollout(T));
    DeviceRing ring(actor.rollout_entry_bytes(), 3 * N, /*seed=*/5);
    fi_step_stats st{};
    CHECK(freeimpala_amd::step_ring(learner.h, ring, N, &st) == FI_ERR_STATE);  // nothing pushed yet
    CHECK(!ring.push_rollout(actor));                                            // no unroll waits
    // two unrolls pushed before any learner step
    if (act(actor, T + 1)) return 1;
    CHECK(actor.rollout_ready() && ring.push_rollout(actor) && !actor.rollout_ready());
    if (act(actor, T)) return 1;
    CHECK(actor.rollout_ready() && ring.push_rollout(actor));
    CHECK(ring.info().head == (uint64_t)(2 * N) && ring.info().tail == 0);
    CHECK(freeimpala_amd::step_ring(learner.h, ring, N - 1, &st) == FI_ERR_STATE);  // nothing to replay yet
    CHECK(ring.info().tail == 0 && ring.info().draw == 0);

    std::vector<uint64_t> got;
    std::string line;
    const int fresh[2] = {N, N / 2};  // FIFO, then mixed
    for (int k = 0; k < 2; ++k) {
        const std::vector<uint64_t> want = freeimpala_amd::ring_batch_entries(ring.info(), N, fresh[k]);
        CHECK((int)want.size() == N);
        CHECK(freeimpala_amd::step_ring(learner.h, ring, fresh[k], &st) == FI_OK);
        CHECK(ring.last_entries(N, got));
        CHECK(got == want);
        for (int col = 0; col < N; ++col)
            CHECK(col < fresh[k] ? got[col] == (uint64_t)(k * N + col) : got[col] < (uint64_t)N);  // replayed: read in step 0
        line += std::string(k ? " mixed " : " fifo ") + join(got);
    }
    CHECK(ring.info().tail == (uint64_t)(N + N / 2) && ring.info().draw == 2);
    fi_batch_versions bv{};
    CHECK(fi_learner_batch_versions(learner.h, &bv) == FI_OK);
    CHECK(bv.min_version == 4 && bv.max_version == 4 && bv.count == (uint64_t)T * N);
    CHECK(fi_learner_staging_bytes(learner.h) == 0);
    CHECK(actor.end_rollout());
    std::printf("ring %s:%s loss %.9g version %llu\n", name, line.c_str(), st.total_loss, (unsigned long long)st.version);
    return 0;
}

int main() {
    try {
        if (policy("mlp", FI_ARCH_MLP, 4, 4, 18, 128)) return 1;
        if (policy("atari", FI_ARCH_ATARI, 3, 4, 6, 128)) return 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
