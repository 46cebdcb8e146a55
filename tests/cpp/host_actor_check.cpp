// host_actor_check.cpp -- exercises include/freeimpala_amd/device_actor.hpp the way an actor
// process would: an MLP actor and an Atari actor take the blob a learner handle publishes, act
// twice each (the Atari one on planes, its stacks on the device) and print their actions, one
// line per actor. Inputs, parameters and draws are all seeded: a second run prints the same lines.
#include <cstdio>
#include <string>
#include <vector>

#include "freeimpala_amd/device_actor.hpp"

using freeimpala_amd::ActorConfig;
using freeimpala_amd::ActResult;
using freeimpala_amd::DeviceActor;

#define CHECK(c)                                                                                           \
    do {                                                                                                   \
        if (!(c)) {                                                                                        \
            std::fprintf(stderr, "CHECK failed at line %d: %s (%s)\n", __LINE__, #c, fi_last_error());     \
            return 1;                                                                                      \
        }                                                                                                  \
    } while (0)

static uint64_t g_x = 0x9E3779B97F4A7C15ull;
static uint64_t next() {
    g_x ^= g_x << 13;
    g_x ^= g_x >> 7;
    g_x ^= g_x << 17;
    return g_x;
}

// the blob of a fresh learner handle of the same policy (what ModelManager would hand an actor)
static int learner_blob(int arch, int A, int publish, std::vector<char>& blob, uint64_t& version) {
    fi_learner_config c;
    fi_learner_config_init(&c);
    c.arch = arch;
    c.seq_len = 1;
    c.batch = 2;
    c.num_actions = A;
    c.publish_dtype = publish;
    c.seed = 7;
    fi_learner* l = nullptr;
    CHECK(fi_learner_create(&c, &l) == FI_OK);
    blob.resize(fi_learner_param_bytes(l));
    const int rc = fi_learner_get_params(l, blob.data(), blob.size(), &version);
    fi_learner_destroy(l);
    CHECK(rc == FI_OK);
    return 0;
}

static void print_line(const char* name, const ActResult& a, const ActResult& b) {
    std::printf("actions %s:", name);
    for (int32_t x : a.actions) std::printf(" %d", x);
    std::printf(" |");
    for (int32_t x : b.actions) std::printf(" %d", x);
    std::printf("\n");
}

int main() {
    try {
        std::vector<char> blob;
        uint64_t version = 0;
        {
            ActorConfig c;
            c.num_envs = 5;
            c.num_actions = 18;
            c.seed = 11;
            DeviceActor actor(c);
            ActResult r0, r1;
            std::vector<float> obs((size_t)c.num_envs * c.obs_dim);
            for (float& v : obs) v = (float)((next() >> 40) * (1.0 / 16777216.0)) * 2.f - 1.f;
            CHECK(!actor.act_obs(obs, r0) && actor.last_error().find("no parameters") != std::string::npos);
            if (learner_blob(FI_ARCH_MLP, c.num_actions, FI_PUBLISH_FP32, blob, version)) return 1;
            CHECK(blob.size() == 4 * actor.param_count());
            CHECK(actor.load(blob, 3) && actor.version() == 3);
            CHECK(actor.act_obs(obs, r0) && actor.act_obs(obs, r1));
            CHECK(r0.logits == r1.logits && r0.values == r1.values);  // the same rows, another draw
            print_line("mlp", r0, r1);
        }
        {
            ActorConfig c;
            c.arch = "atari";
            c.num_envs = 3;
            c.num_actions = 6;
            c.seed = 12;
            DeviceActor actor(c);
            if (learner_blob(FI_ARCH_ATARI, c.num_actions, FI_PUBLISH_BF16, blob, version)) return 1;
            CHECK(blob.size() == 2 * actor.param_count());
            CHECK(actor.load(blob, version));
            ActResult r0, r1;
            std::vector<uint8_t> planes((size_t)c.num_envs * DeviceActor::kPlaneBytes), stacks;
            for (uint8_t& v : planes) v = (uint8_t)(next() >> 56);
            CHECK(actor.act_planes(planes, std::vector<uint8_t>(c.num_envs, 1), r0));
            const uint8_t first = planes[0];
            for (uint8_t& v : planes) v = (uint8_t)(next() >> 56);
            CHECK(actor.act_planes(planes, std::vector<uint8_t>(c.num_envs, 0), r1));
            CHECK(actor.read_stacks(stacks));
            // pixel 0 of environment 0: three channels of the first plane, then the second
            CHECK(stacks[0] == first && stacks[1] == first && stacks[2] == first && stacks[3] == planes[0]);
            CHECK(!actor.act_obs(std::vector<float>((size_t)c.num_envs * c.obs_dim), r0));
            print_line("atari", r0, r1);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
