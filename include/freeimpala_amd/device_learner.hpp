// device_learner.hpp -- C++ host side of the MI355X learner step, above the C ABI.
//
// What the reference's Learner needs to move its step on-device, with the reference's
// own vocabulary and signatures:
//   * LearnerConfig::from_args   -- the learner flags of cmd/freeimpala (reference
//     cmd/freeimpala/main.cpp: --players, --batch-size, --seq-length, --entry-size) plus
//     the device-learner hyper-parameters (--learner-arch, --num-actions, --lr, ...).
//   * DeviceLearner::step(player_index, batch) -- same parameters as
//     Learner::trainModel (reference include/freeimpala/learner.h:32) and the same
//     `batch` that SharedBuffer::readBatch returns (data_structures.h:267-300):
//     M entries of S * ELEMENT_SIZE bytes, record schemas in DESIGN.md section 3 (one element
//     per step for the MLP, 28 per step -- frame + header -- for the Atari policy, or with
//     --atari-records planes 7 per step -- newest plane + header -- and a 21-element history
//     block after the T+1 records).
//   * DeviceLearner::publish(player_index, blob, version) -- the bytes and version that go
//     into Model::update / ModelManager::updateModel (data_structures.h:141-148, 441-451);
//     blob size == param_bytes() is the ModelManager model_size.
// One fi_learner handle per player (the reference runs one worker thread per player,
// learner.h:158-163): handles own their HIP stream and device memory, so different
// players may call step() concurrently from their own threads. Failures never throw
// across step(): it returns false and last_error() holds the message, matching the
// reference's log-and-continue style (data_structures.h:420-421). Construction throws
// std::runtime_error when the HIP library or device is unusable -- there is no CPU
// fallback.
#pragma once

#include <cstdint>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "fi_diag.h"
#include "fi_kl.h"
#include "fi_learner.h"
#include "fi_popart.h"
#include "fi_publish.h"
#include "fi_surrogate.h"
#include "fi_target.h"
#include "fi_train.h"

namespace freeimpala_amd {

struct LearnerConfig {
    size_t players = 1;        // --players
    size_t batch_size = 32;    // --batch-size (M entries per step)
    size_t seq_length = 100;   // --seq-length (T); entries carry T+1 records
    size_t entry_size = 0;     // --entry-size in ELEMENT_SIZE units (0: T+1 records)
    std::string arch = "mlp";  // --learner-arch mlp|atari
    std::string atari_records = "stacked";  // --atari-records stacked|planes (atari only)
    int num_actions = 18;      // --num-actions
    int obs_dim = 128;         // --obs-dim
    int hidden = 256;          // --hidden
    std::string optimizer = "adam";  // --optimizer adam|sgd|rmsprop
    // the training recipe (fi_train.h), applied to every handle right after fi_learner_create (so a
    // --starting-model resume loads its state behind it); the defaults change nothing
    float rms_decay = 0.99f;       // --rms-decay      (--optimizer rmsprop; monobeast's numbers)
    float rms_momentum = 0.f;      // --rms-momentum
    float rms_eps = 0.01f;         // --rms-eps
    bool rms_eps_in_sqrt = false;  // --rms-eps-in-sqrt 0|1 (1: sqrt(v + eps), TensorFlow / the paper)
    bool lr_schedule = false;      // --lr-end and --lr-steps, both or neither: anneal --lr linearly
    float lr_end = 0.f;            //   to --lr-end over --lr-steps updates
    uint64_t lr_steps = 0;
    float reward_clip = 0.f;       // --reward-clip c: rewards clamped to [-c, c] before V-trace (0: off)
    std::string publish = "fp32";    // --publish fp32|bf16
    float lr = 5e-4f;          // --lr  (reference README.md:112 default)
    float max_grad_norm = 40.f;      // --max-grad-norm
    float gamma = 0.99f;       // --gamma (synthetic generator only)
    fi_vtrace_hparams hp{1.f, 1.f, 1.f, 1.f, 0.5f, 0.01f};
    std::vector<int> devices{0};     // --devices 0,1,... (player p -> devices[p % n])
    size_t data_parallel = 1;  // --data-parallel G: each player's batch split over G devices
                               // (shard g of player p on devices[(p G + g) % n]; RCCL all-reduce)
    uint64_t seed = 42;        // --seed (parameter init)

    bool planes() const { return arch == "atari" && atari_records == "planes"; }
    // ELEMENT_SIZE units one step's record takes: 1 (MLP), 28 (Atari: 84x84x4 frame + header),
    // 7 (Atari plane records: the newest 84x84 plane + header)
    size_t record_elements() const {
        if (arch != "atari") return 1;
        return planes() ? (size_t)FI_ATARI_PLANE_RECORD_ELEMENTS : (size_t)FI_ATARI_RECORD_ELEMENTS;
    }
    // ELEMENT_SIZE units after an entry's records: the history block of the plane records
    size_t entry_tail_elements() const { return planes() ? (size_t)FI_ATARI_HISTORY_ELEMENTS : 0; }
    // whole records an entry holds (beside its tail)
    size_t entry_records() const { return records_in(entry_size ? entry_size : min_entry_size()); }
    size_t records_in(size_t elements) const {
        return elements > entry_tail_elements() ? (elements - entry_tail_elements()) / record_elements() : 0;
    }
    // the smallest --entry-size for seq_length + 1 records
    size_t min_entry_size() const { return record_elements() * (seq_length + 1) + entry_tail_elements(); }
    // "28 * (seq_length + 1)", "7 * (seq_length + 1) + 21"
    std::string min_entry_size_formula() const {
        return std::to_string(record_elements()) + " * (seq_length + 1)" +
               (entry_tail_elements() ? " + " + std::to_string(entry_tail_elements()) : "");
    }

    // Parses the flags above from argv (unknown flags are ignored so the reference's own
    // parser can own the rest of the command line). Throws std::invalid_argument on a
    // malformed value.
    static LearnerConfig from_args(int argc, const char* const* argv) {
        return from_args(argc, argv, LearnerConfig());
    }
    static LearnerConfig from_args(int argc, const char* const* argv, LearnerConfig c) {
        auto num = [](const std::string& f, const char* v) -> double {
            char* end = nullptr;
            const double x = std::strtod(v, &end);
            if (!v[0] || (end && *end)) throw std::invalid_argument("bad value for " + f + ": " + v);
            return x;
        };
        bool have_end = false, have_steps = false;
        for (int i = 1; i + 1 < argc; ++i) {
            const std::string f = argv[i];
            const char* v = argv[i + 1];
            bool used = true;
            if (f == "--players" || f == "-p") c.players = (size_t)num(f, v);
            else if (f == "--batch-size" || f == "-M") c.batch_size = (size_t)num(f, v);
            else if (f == "--seq-length") c.seq_length = (size_t)num(f, v);
            else if (f == "--entry-size" || f == "-S") c.entry_size = (size_t)num(f, v);
            else if (f == "--learner-arch") c.arch = v;
            else if (f == "--atari-records") c.atari_records = v;
            else if (f == "--num-actions") c.num_actions = (int)num(f, v);
            else if (f == "--obs-dim") c.obs_dim = (int)num(f, v);
            else if (f == "--hidden") c.hidden = (int)num(f, v);
            else if (f == "--optimizer") c.optimizer = v;
            else if (f == "--publish") c.publish = v;
            else if (f == "--lr") c.lr = (float)num(f, v);
            else if (f == "--max-grad-norm") c.max_grad_norm = (float)num(f, v);
            else if (f == "--gamma") c.gamma = (float)num(f, v);
            else if (f == "--seed") c.seed = (uint64_t)num(f, v);
            else if (f == "--data-parallel") c.data_parallel = (size_t)num(f, v);
            else if (f == "--rms-decay") c.rms_decay = (float)num(f, v);
            else if (f == "--rms-momentum") c.rms_momentum = (float)num(f, v);
            else if (f == "--rms-eps") c.rms_eps = (float)num(f, v);
            else if (f == "--rms-eps-in-sqrt") c.rms_eps_in_sqrt = num(f, v) != 0;
            else if (f == "--lr-end") { c.lr_end = (float)num(f, v); have_end = true; }
            else if (f == "--lr-steps") { c.lr_steps = steps_of(num(f, v)); have_steps = true; }
            else if (f == "--reward-clip") c.reward_clip = (float)num(f, v);
            else if (f == "--devices") {
                c.devices.clear();
                std::string s = v;
                size_t p = 0;
                while (p <= s.size()) {
                    const size_t q = s.find(',', p);
                    const std::string tok = s.substr(p, q == std::string::npos ? std::string::npos : q - p);
                    if (!tok.empty()) c.devices.push_back((int)num(f, tok.c_str()));
                    if (q == std::string::npos) break;
                    p = q + 1;
                }
                if (c.devices.empty()) throw std::invalid_argument("--devices: empty list");
            } else used = false;
            if (used) ++i;
        }
        if (c.players == 0 || c.batch_size == 0 || c.seq_length == 0)
            throw std::invalid_argument("--players, --batch-size and --seq-length must be > 0");
        if (c.arch != "mlp" && c.arch != "atari") throw std::invalid_argument("--learner-arch: mlp|atari");
        if (c.atari_records != "stacked" && c.atari_records != "planes")
            throw std::invalid_argument("--atari-records: stacked|planes");
        if (c.atari_records != "stacked" && c.arch != "atari")
            throw std::invalid_argument("--atari-records planes needs --learner-arch atari");
        if (c.planes() && c.num_actions > 18)
            throw std::invalid_argument("--atari-records planes: the plane record's header holds mu[18], --num-actions " +
                                        std::to_string(c.num_actions) + " > 18 needs stacked records");
        if (c.entry_records() < c.seq_length + 1)
            throw std::invalid_argument(
                c.record_elements() == 1
                    ? std::string("--entry-size must hold seq_length + 1 records")
                    : "--entry-size must be >= " + std::to_string(c.min_entry_size()) + " = " +
                          c.min_entry_size_formula() + " for --learner-arch " + c.arch +
                          (c.planes() ? " --atari-records planes" : ""));
        if (c.optimizer != "adam" && c.optimizer != "sgd" && c.optimizer != "rmsprop")
            throw std::invalid_argument("--optimizer: adam|sgd|rmsprop");
        if (have_end != have_steps) throw std::invalid_argument("--lr-end and --lr-steps go together: both or neither");
        if (have_end) c.lr_schedule = true;
        c.check_recipe();
        if (c.publish != "fp32" && c.publish != "bf16") throw std::invalid_argument("--publish: fp32|bf16");
        if (c.data_parallel == 0 || c.batch_size % c.data_parallel != 0)
            throw std::invalid_argument("--data-parallel must divide --batch-size");
        return c;
    }

    // --lr-steps as an integer >= 1 (checked before the cast: a negative double has no uint64_t)
    static uint64_t steps_of(double x) {
        if (!(x >= 1.0 && x < 1.8e19)) throw std::invalid_argument("--lr-steps must be >= 1");
        return (uint64_t)x;
    }

    // the ranges fi_train.h's setters accept, so a bad flag fails at the command line
    void check_recipe() const {
        if (!(rms_decay >= 0.f && rms_decay < 1.f)) throw std::invalid_argument("--rms-decay must be in [0, 1)");
        if (!(rms_momentum >= 0.f && rms_momentum < 1.f)) throw std::invalid_argument("--rms-momentum must be in [0, 1)");
        if (!(rms_eps > 0.f && rms_eps <= 3.4e38f)) throw std::invalid_argument("--rms-eps must be positive and finite");
        if (lr_schedule && !(lr_end >= 0.f && lr_end <= 3.4e38f && lr_steps >= 1))
            throw std::invalid_argument("--lr-end must be >= 0 and finite, --lr-steps >= 1");
        if (!(reward_clip >= 0.f && reward_clip <= 3.4e38f)) throw std::invalid_argument("--reward-clip must be >= 0 and finite");
    }

    // Learner flags through a strict parser (freeimpala_amd::ArgumentParser or the argparse
    // library of the reference binaries): the reference's own -p/--players, -M/--batch-size and
    // -S/--entry-size (registered by its setupArgumentParser, cmd/freeimpala/main.cpp:45-72)
    // plus the flags add_learner_arguments() registers. Throws std::invalid_argument.
    // (two overloads, not a defaulted `LearnerConfig()` argument: clang rejects a default
    // argument that needs the class's member initializers inside the class definition)
    template <class Parser>
    static LearnerConfig from_parser(const Parser& program) {
        return from_parser(program, LearnerConfig());
    }
    template <class Parser>
    static LearnerConfig from_parser(const Parser& program, LearnerConfig c) {
        auto num = [](const std::string& f, const std::string& v) -> double {
            char* end = nullptr;
            const double x = std::strtod(v.c_str(), &end);
            if (v.empty() || (end && *end)) throw std::invalid_argument("bad value for " + f + ": " + v);
            return x;
        };
        auto str = [&](const char* f) { return program.template get<std::string>(f); };
        c.players = (size_t)program.template get<int>("--players");
        c.batch_size = (size_t)program.template get<int>("--batch-size");
        c.entry_size = (size_t)program.template get<int>("--entry-size");
        c.seq_length = (size_t)num("--seq-length", str("--seq-length"));
        c.arch = str("--learner-arch");
        c.atari_records = str("--atari-records");
        c.num_actions = (int)num("--num-actions", str("--num-actions"));
        c.obs_dim = (int)num("--obs-dim", str("--obs-dim"));
        c.hidden = (int)num("--hidden", str("--hidden"));
        c.optimizer = str("--optimizer");
        c.publish = str("--publish");
        c.lr = (float)num("--lr", str("--lr"));
        c.max_grad_norm = (float)num("--max-grad-norm", str("--max-grad-norm"));
        c.gamma = (float)num("--gamma", str("--gamma"));
        c.seed = (uint64_t)num("--learner-seed", str("--learner-seed"));
        c.data_parallel = (size_t)num("--data-parallel", str("--data-parallel"));
        c.rms_decay = (float)num("--rms-decay", str("--rms-decay"));
        c.rms_momentum = (float)num("--rms-momentum", str("--rms-momentum"));
        c.rms_eps = (float)num("--rms-eps", str("--rms-eps"));
        c.rms_eps_in_sqrt = num("--rms-eps-in-sqrt", str("--rms-eps-in-sqrt")) != 0;
        c.reward_clip = (float)num("--reward-clip", str("--reward-clip"));
        // "" (the default): not given
        const std::string end = str("--lr-end"), steps = str("--lr-steps");
        if (end.empty() != steps.empty()) throw std::invalid_argument("--lr-end and --lr-steps go together: both or neither");
        if (!end.empty()) {
            c.lr_end = (float)num("--lr-end", end);
            c.lr_steps = steps_of(num("--lr-steps", steps));
            c.lr_schedule = true;
        }
        const char* argv[] = {"", "--devices", nullptr};
        const std::string dev = str("--devices");
        argv[2] = dev.c_str();
        // (validation as from_args; an entry size too small for seq_length + 1 records is left
        // to the Learner, which lowers seq_length with a warning)
        LearnerConfig v = c;
        v.entry_size = 0;
        c.devices = from_args(3, argv, v).devices;
        return c;
    }

    // The C-ABI configuration of player p's handle (shard g of it under --data-parallel: the
    // same seed, so every replica starts from the same parameters).
    fi_learner_config abi_config(size_t p, size_t g = 0) const {
        fi_learner_config k;
        fi_learner_config_init(&k);
        k.arch = arch == "atari" ? FI_ARCH_ATARI : FI_ARCH_MLP;
        k.seq_len = (int32_t)seq_length;
        k.batch = (int32_t)(batch_size / data_parallel);
        k.num_actions = num_actions;
        k.obs_dim = obs_dim;
        k.hidden = hidden;
        // rmsprop: created as sgd is, then switched by fi_train_set_rmsprop
        k.optimizer = optimizer == "sgd" || optimizer == "rmsprop" ? FI_OPT_SGD : FI_OPT_ADAM;
        k.publish_dtype = publish == "bf16" ? FI_PUBLISH_BF16 : FI_PUBLISH_FP32;
        k.device = devices[(p * data_parallel + g) % devices.size()];
        k.gamma = gamma;
        k.hp = hp;
        k.lr = lr;
        k.max_grad_norm = max_grad_norm;
        k.seed = seed + p;
        return k;
    }
};

// Registers the device-learner flags with a strict parser (string-valued, so the same calls
// work on argparse::ArgumentParser); values are checked by LearnerConfig::from_parser. --seed
// stays the reference's own (rand() seeding, main.cpp:111-114): parameter init is
// --learner-seed.
template <class Parser>
void add_learner_arguments(Parser& program) {
    const LearnerConfig d;
    program.add_argument("--seq-length").help("Trajectory length T (entries carry T+1 records)")
        .default_value(std::to_string(d.seq_length));
    program.add_argument("--learner-arch").help("Policy network: mlp | atari").default_value(d.arch);
    program.add_argument("--atari-records")
        .help("Atari host records: stacked (84x84x4 per step) | planes (84x84 per step, stack rebuilt on the device)")
        .default_value(d.atari_records);
    program.add_argument("--num-actions").help("Number of actions A").default_value(std::to_string(d.num_actions));
    program.add_argument("--obs-dim").help("MLP observation width (<= 128)").default_value(std::to_string(d.obs_dim));
    program.add_argument("--hidden").help("MLP hidden width").default_value(std::to_string(d.hidden));
    program.add_argument("--optimizer").help("adam | sgd | rmsprop").default_value(d.optimizer);
    program.add_argument("--rms-decay").help("RMSProp: decay of the mean square").default_value(std::string("0.99"));
    program.add_argument("--rms-momentum").help("RMSProp: momentum (0: none)").default_value(std::string("0"));
    program.add_argument("--rms-eps").help("RMSProp: epsilon").default_value(std::string("0.01"));
    program.add_argument("--rms-eps-in-sqrt").help("RMSProp: 0 = sqrt(v) + eps (torch), 1 = sqrt(v + eps) (TensorFlow)")
        .default_value(std::string("0"));
    program.add_argument("--lr-end").help("Anneal --lr linearly to this rate over --lr-steps updates (with --lr-steps)")
        .default_value(std::string(""));
    program.add_argument("--lr-steps").help("Updates the linear anneal takes (with --lr-end)").default_value(std::string(""));
    program.add_argument("--reward-clip").help("Clamp rewards to [-c, c] before V-trace (0: off)")
        .default_value(std::string("0"));
    program.add_argument("--publish").help("Published weights dtype: fp32 | bf16").default_value(d.publish);
    program.add_argument("--lr").help("Learning rate").default_value(std::string("0.0005"));
    program.add_argument("--max-grad-norm").help("Global-norm gradient clip (<= 0: off)")
        .default_value(std::string("40"));
    program.add_argument("--gamma").help("Discount of the synthetic trajectories").default_value(std::string("0.99"));
    program.add_argument("--learner-seed").help("Parameter-initialisation seed").default_value(std::to_string(d.seed));
    program.add_argument("--devices").help("HIP devices, comma separated (player p -> devices[p % n])")
        .default_value(std::string("0"));
    program.add_argument("--data-parallel").help("Devices per player: the batch is split over them, RCCL all-reduce")
        .default_value(std::string("1"));
}

class DeviceLearner {
public:
    explicit DeviceLearner(const LearnerConfig& cfg) : cfg_(cfg), stats_(cfg.players), err_(cfg.players) {
        if (fi_abi_version() != FI_ABI_VERSION)
            throw std::runtime_error("libfi_learner ABI version mismatch");
        const size_t G = cfg.data_parallel ? cfg.data_parallel : 1;
        handles_.resize(cfg.players, nullptr);
        shards_.assign(cfg.players, std::vector<fi_learner*>(G, nullptr));
        for (size_t p = 0; p < cfg.players; ++p) {
            for (size_t g = 0; g < G; ++g) {
                const fi_learner_config k = cfg.abi_config(p, g);
                if (fi_learner_create(&k, &shards_[p][g]) != FI_OK) {
                    const std::string msg = std::string("fi_learner_create(player ") + std::to_string(p) +
                                            ", shard " + std::to_string(g) + "): " + fi_last_error();
                    release();
                    throw std::runtime_error(msg);
                }
                if (cfg.planes() && fi_learner_set_record_format(shards_[p][g], FI_RECORDS_PLANES) != FI_OK) {
                    const std::string msg = std::string("fi_learner_set_record_format(player ") + std::to_string(p) +
                                            ", shard " + std::to_string(g) + "): " + fi_last_error();
                    release();
                    throw std::runtime_error(msg);
                }
                if (!apply_recipe(shards_[p][g])) {
                    const std::string msg = std::string("training recipe (player ") + std::to_string(p) + ", shard " +
                                            std::to_string(g) + "): " + fi_last_error();
                    release();
                    throw std::runtime_error(msg);
                }
            }
            handles_[p] = shards_[p][0];
            // one RCCL communicator per player over its G devices: the in-step all-reduce sums
            // the shards' gradients, every replica applies the same update
            if (G > 1 && fi_comm_init_all(shards_[p].data(), (int)G) != FI_OK) {
                const std::string msg = std::string("fi_comm_init_all(player ") + std::to_string(p) + "): " + fi_last_error();
                release();
                throw std::runtime_error(msg);
            }
        }
    }
    ~DeviceLearner() { release(); }
    DeviceLearner(const DeviceLearner&) = delete;
    DeviceLearner& operator=(const DeviceLearner&) = delete;

    // Learner::step(player_index, batch): the body of Learner::trainModel on the device.
    bool step(size_t player_index, const std::vector<std::vector<char>>& batch) {
        if (player_index >= handles_.size()) return fail(0, "player_index out of range");
        if (batch.empty()) return fail(player_index, "empty batch");
        const size_t eb = batch[0].size();
        std::vector<const void*> ptrs(batch.size());
        for (size_t i = 0; i < batch.size(); ++i) {
            if (batch[i].size() != eb) return fail(player_index, "entries of different sizes");
            ptrs[i] = batch[i].data();
        }
        if (shards_[player_index].size() > 1) return step_sharded(player_index, ptrs, eb);
        fi_step_stats st{};
        if (fi_learner_step(handles_[player_index], ptrs.data(), ptrs.size(), eb, &st) != FI_OK)
            return fail(player_index, fi_last_error());
        stats_[player_index] = st;
        return true;
    }

    // Asynchronous step: returns once the batch is copied into pinned memory (the caller may
    // drop it and block in readBatch for the next one); wait() completes it.
    bool step_async(size_t player_index, const std::vector<std::vector<char>>& batch) {
        if (player_index >= handles_.size()) return fail(0, "player_index out of range");
        if (shards_[player_index].size() > 1) return fail(player_index, "step_async: not with --data-parallel > 1");
        if (batch.empty()) return fail(player_index, "empty batch");
        const size_t eb = batch[0].size();
        std::vector<const void*> ptrs(batch.size());
        for (size_t i = 0; i < batch.size(); ++i) {
            if (batch[i].size() != eb) return fail(player_index, "entries of different sizes");
            ptrs[i] = batch[i].data();
        }
        if (fi_learner_step_async(handles_[player_index], ptrs.data(), ptrs.size(), eb) != FI_OK)
            return fail(player_index, fi_last_error());
        return true;
    }
    // Zero-copy step: fill(dst, entry_stride, n) writes n entries straight into the pinned
    // staging buffer (SharedBuffer::readBatchInto, under the buffer's own mutex) and returns
    // false when there is no batch (draining, data_structures.h:278-280): then nothing is
    // submitted and the same buffer is handed out next time. async as in step_async.
    template <class Fill>
    bool step_staged(size_t player_index, Fill&& fill, bool async = false) {
        if (player_index >= handles_.size()) return fail(0, "player_index out of range");
        if (shards_[player_index].size() > 1) return fail(player_index, "step_staged: not with --data-parallel > 1");
        fi_learner* h = handles_[player_index];
        void* dst = nullptr;
        size_t stride = 0;
        if (fi_learner_acquire_staging(h, &dst, &stride) != FI_OK) return fail(player_index, fi_last_error());
        if (!fill(static_cast<char*>(dst), stride, cfg_.batch_size)) return false;
        if (async) {
            if (fi_learner_step_staged_async(h) != FI_OK) return fail(player_index, fi_last_error());
            return true;
        }
        fi_step_stats st{};
        if (fi_learner_step_staged(h, &st) != FI_OK) return fail(player_index, fi_last_error());
        stats_[player_index] = st;
        return true;
    }

    bool wait(size_t p) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        fi_step_stats st{};
        if (fi_learner_wait(handles_[p], &st) != FI_OK) return fail(p, fi_last_error());
        stats_[p] = st;
        return true;
    }

    // Full learner state (params + Adam moments + counters) for checkpoint / resume.
    bool save_state(size_t p, std::vector<char>& blob) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        blob.resize(fi_learner_state_bytes(handles_[p]));
        if (fi_learner_save_state(handles_[p], blob.data(), blob.size()) != FI_OK) return fail(p, fi_last_error());
        return true;
    }
    bool load_state(size_t p, const std::vector<char>& blob) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        for (fi_learner* h : shards_[p])
            if (fi_learner_load_state(h, blob.data(), blob.size()) != FI_OK) return fail(p, fi_last_error());
        return true;
    }

    // Parameters of player p as the published Model blob (fp32 or bf16, little endian,
    // DESIGN.md section 3 order); resizes `blob` to param_bytes().
    bool publish(size_t p, std::vector<char>& blob, uint64_t& version) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        blob.resize(param_bytes());
        if (fi_learner_get_params(handles_[p], blob.data(), blob.size(), &version) != FI_OK)
            return fail(p, fi_last_error());
        return true;
    }
    // The same parameters published on the device (include/fi_publish.h): enqueued on the learner's
    // stream into a snapshot slot, nothing waits. An actor on the same device takes the newest one
    // with DeviceActor::set_params_dev(handle(p)). tag: the count of updates enqueued so far.
    bool publish_dev(size_t p, uint64_t& tag) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        if (fi_publish_params(handles_[p], &tag) != FI_OK) return fail(p, fi_last_error());
        return true;
    }
    // Off-policy diagnostics of player p's most recent step (include/fi_diag.h): rho statistics,
    // KL(mu | pi), ESS, clip rates and the explained variance, reduced on the device beside the step.
    // enqueue_diagnostics() only enqueues, behind the step on the learner's stream; read_diagnostics()
    // waits for that result alone; diagnostics() is both. col_kl / col_log_rho (nullable): the per-column
    // means, resized to the batch. With --data-parallel > 1 they describe shard 0.
    bool enqueue_diagnostics(size_t p) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        if (fi_diag_enqueue(handles_[p]) != FI_OK) return fail(p, fi_last_error());
        return true;
    }
    bool read_diagnostics(size_t p, fi_offpolicy_diag& out, std::vector<float>* col_kl = nullptr,
                          std::vector<float>* col_log_rho = nullptr) {
        return diag_call(p, fi_diag_read, out, col_kl, col_log_rho);
    }
    bool diagnostics(size_t p, fi_offpolicy_diag& out, std::vector<float>* col_kl = nullptr,
                     std::vector<float>* col_log_rho = nullptr) {
        return diag_call(p, fi_diag_learner, out, col_kl, col_log_rho);
    }
    // PopArt value normalisation on player p (include/fi_popart.h): every later step denormalises the
    // value head's output with the statistics on the device, divides the value gradient by sigma and,
    // behind the optimiser, moves mu, sigma and rewrites the value column so that sigma n + mu is
    // preserved. The statistics are not in save_state()'s blob: a resuming process calls
    // enable_popart, set_popart_state, then load_state. With --data-parallel > 1 the handles share a
    // communicator and the call is refused.
    bool enable_popart(size_t p, double beta = FI_POPART_BETA, double sigma_min = FI_POPART_SIGMA_MIN,
                       double sigma_max = FI_POPART_SIGMA_MAX) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        for (fi_learner* h : shards_[p])
            if (fi_popart_enable(h, beta, sigma_min, sigma_max) != FI_OK) return fail(p, fi_last_error());
        return true;
    }
    bool popart_state(size_t p, fi_popart_state& out) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        if (fi_popart_get_state(handles_[p], &out) != FI_OK) return fail(p, fi_last_error());
        return true;
    }
    bool set_popart_state(size_t p, double mu, double nu) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        for (fi_learner* h : shards_[p])
            if (fi_popart_set_state(h, mu, nu) != FI_OK) return fail(p, fi_last_error());
        return true;
    }
    // The clipped surrogate objective on player p (include/fi_surrogate.h): every later step runs
    // -min(rho A, clip(rho, 1 - clip, 1 + clip) A) on V-trace's targets in place of the V-trace policy
    // gradient, until clear_surrogate(). With --data-parallel > 1 the handles share a communicator and
    // normalize_advantages is refused (the moments would need an all-reduce); plain clipping is fine.
    bool set_surrogate(size_t p, float clip = FI_SURROGATE_CLIP, bool normalize_advantages = false,
                       float adv_eps = FI_SURROGATE_ADV_EPS) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        const fi_surrogate_params prm{clip, normalize_advantages ? 1u : 0u, adv_eps, 0u};
        for (fi_learner* h : shards_[p])
            if (fi_surrogate_enable(h, &prm) != FI_OK) return fail(p, fi_last_error());
        return true;
    }
    bool clear_surrogate(size_t p) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        for (fi_learner* h : shards_[p])
            if (fi_surrogate_disable(h) != FI_OK) return fail(p, fi_last_error());
        return true;
    }
    bool surrogate_state(size_t p, fi_surrogate_state& out) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        if (fi_surrogate_get_state(handles_[p], &out) != FI_OK) return fail(p, fi_last_error());
        return true;
    }
    // The target network on player p (include/fi_target.h): a slowly moving copy of the parameters. A
    // surrogate step takes V-trace's importance weights against it and its trust region around it; every
    // period-th update moves it by tau towards the parameters. The copy is not in save_state()'s blob: a
    // resuming process calls enable_target, fi_target_set_params on the handles, then load_state; a
    // process that only wants the copy to follow a loaded state calls sync_target after the load.
    bool enable_target(size_t p, uint32_t period = FI_TARGET_PERIOD, float tau = FI_TARGET_TAU) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        const fi_target_params prm{period, tau, {0u, 0u}};
        for (fi_learner* h : shards_[p])
            if (fi_target_enable(h, &prm) != FI_OK) return fail(p, fi_last_error());
        return true;
    }
    bool disable_target(size_t p) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        for (fi_learner* h : shards_[p])
            if (fi_target_disable(h) != FI_OK) return fail(p, fi_last_error());
        return true;
    }
    bool sync_target(size_t p) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        for (fi_learner* h : shards_[p])
            if (fi_target_sync(h) != FI_OK) return fail(p, fi_last_error());
        return true;
    }
    bool target_state(size_t p, fi_target_params& params, fi_target_stats& stats, bool* enabled = nullptr) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        uint32_t on = 0;
        if (fi_target_get_state(handles_[p], &params, &stats, &on) != FI_OK) return fail(p, fi_last_error());
        if (enabled) *enabled = on != 0;
        return true;
    }
    // The adaptive KL penalty on player p (include/fi_kl.h): coeff * KL(q || pi) in the loss, q the batch's
    // behaviour policy (FI_KL_REF_BEHAVIOUR) or the target network's (FI_KL_REF_TARGET, after enable_target);
    // with adapt the coefficient moves on the device towards kl_target. With --data-parallel > 1 the handles
    // share a communicator and adapt is refused (each shard would see its own mean); a fixed coefficient is
    // fine. The block is not in save_state()'s blob: a resuming process calls enable_kl_penalty, set_kl_coeff,
    // load_state.
    bool enable_kl_penalty(size_t p, uint32_t reference = FI_KL_REF_BEHAVIOUR, float coeff = FI_KL_COEFF,
                           float kl_target = FI_KL_TARGET, bool adapt = true, float band = FI_KL_BAND,
                           float factor = FI_KL_FACTOR, float coeff_min = FI_KL_COEFF_MIN, float coeff_max = FI_KL_COEFF_MAX) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        const fi_kl_params prm{reference, adapt ? 1u : 0u, coeff, kl_target, band, factor, coeff_min, coeff_max};
        for (fi_learner* h : shards_[p])
            if (fi_kl_enable(h, &prm) != FI_OK) return fail(p, fi_last_error());
        return true;
    }
    bool disable_kl_penalty(size_t p) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        for (fi_learner* h : shards_[p])
            if (fi_kl_disable(h) != FI_OK) return fail(p, fi_last_error());
        return true;
    }
    bool set_kl_coeff(size_t p, double c) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        for (fi_learner* h : shards_[p])
            if (fi_kl_set_coeff(h, c) != FI_OK) return fail(p, fi_last_error());
        return true;
    }
    bool kl_state(size_t p, fi_kl_params& params, fi_kl_stats& stats, bool* enabled = nullptr) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        uint32_t on = 0;
        if (fi_kl_get_state(handles_[p], &params, &stats, &on) != FI_OK) return fail(p, fi_last_error());
        if (enabled) *enabled = on != 0;
        return true;
    }
    // --starting-model resume (Model::loadFromDisk bytes + version).
    bool load(size_t p, const std::vector<char>& blob, uint64_t version) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        for (fi_learner* h : shards_[p])
            if (fi_learner_set_params(h, blob.data(), blob.size(), version) != FI_OK) return fail(p, fi_last_error());
        return true;
    }

    size_t param_bytes() const { return fi_learner_param_bytes(handles_[0]); }
    size_t param_count() const { return fi_learner_param_count(handles_[0]); }
    size_t entry_bytes() const { return fi_learner_entry_bytes(handles_[0]); }
    size_t players() const { return handles_.size(); }
    const fi_step_stats& last_stats(size_t p) const { return stats_.at(p); }
    std::string last_error(size_t p = 0) const {
        std::lock_guard<std::mutex> g(mu_);
        return err_.at(p);
    }
    fi_learner* handle(size_t p) { return handles_.at(p); }
    size_t shards(size_t p = 0) const { return shards_.at(p).size(); }
    const LearnerConfig& config() const { return cfg_; }

private:
    bool diag_call(size_t p, int (*fn)(fi_learner*, fi_offpolicy_diag*, float*, float*, int32_t), fi_offpolicy_diag& out,
                   std::vector<float>* col_kl, std::vector<float>* col_log_rho) {
        if (p >= handles_.size()) return fail(0, "player_index out of range");
        const size_t B = cfg_.batch_size / (cfg_.data_parallel ? cfg_.data_parallel : 1);
        if (col_kl) col_kl->resize(B);
        if (col_log_rho) col_log_rho->resize(B);
        if (fn(handles_[p], &out, col_kl ? col_kl->data() : nullptr, col_log_rho ? col_log_rho->data() : nullptr,
               (int32_t)B) != FI_OK)
            return fail(p, fi_last_error());
        return true;
    }

    // the fi_train.h calls the configuration asks for; none with the defaults
    bool apply_recipe(fi_learner* h) const {
        if (cfg_.optimizer == "rmsprop" &&
            fi_train_set_rmsprop(h, cfg_.rms_decay, cfg_.rms_momentum, cfg_.rms_eps, cfg_.rms_eps_in_sqrt ? 1 : 0) != FI_OK)
            return false;
        if (cfg_.lr_schedule && fi_train_set_lr_schedule(h, cfg_.lr_end, cfg_.lr_steps) != FI_OK) return false;
        if (cfg_.reward_clip > 0.f && fi_train_set_reward_clip(h, cfg_.reward_clip) != FI_OK) return false;
        return true;
    }

    // --data-parallel: contiguous shards of the M entries, one per device, stepped
    // concurrently (the in-step all-reduce needs every rank); loss sums added over the shards
    bool step_sharded(size_t p, const std::vector<const void*>& ptrs, size_t eb) {
        const size_t G = shards_[p].size();
        if (ptrs.size() % G != 0) return fail(p, "batch not divisible by --data-parallel");
        const size_t per = ptrs.size() / G;
        std::vector<fi_step_stats> st(G);
        std::vector<int> rc(G, FI_OK);
        std::vector<std::string> why(G);
        auto run = [&](size_t g) {
            rc[g] = fi_learner_step(shards_[p][g], ptrs.data() + g * per, per, eb, &st[g]);
            if (rc[g] != FI_OK) why[g] = fi_last_error();  // thread-local: read on the same thread
        };
        std::vector<std::thread> th;
        for (size_t g = 1; g < G; ++g) th.emplace_back(run, g);
        run(0);
        for (auto& t : th) t.join();
        // A rejected batch (an out-of-range action in any shard) fails on EVERY shard: the
        // reject counter is all-reduced with the gradient before the optimizer, so all
        // replicas skip the update together and stay identical; one rejection is reported.
        for (size_t g = 0; g < G; ++g)
            if (rc[g] != FI_OK) return fail(p, "shard " + std::to_string(g) + ": " + why[g]);
        fi_step_stats sum = st[0];
        for (size_t g = 1; g < G; ++g) {
            sum.pg_loss += st[g].pg_loss;
            sum.baseline_loss += st[g].baseline_loss;
            sum.entropy_loss += st[g].entropy_loss;
            sum.total_loss += st[g].total_loss;
            sum.step_ms = std::max(sum.step_ms, st[g].step_ms);
        }
        stats_[p] = sum;
        return true;
    }

    bool fail(size_t p, const std::string& m) {
        std::lock_guard<std::mutex> g(mu_);
        err_.at(p < err_.size() ? p : 0) = m;
        return false;
    }
    void release() {
        for (auto& v : shards_)
            for (auto& h : v) {
                if (h) fi_learner_destroy(h);
                h = nullptr;
            }
        for (auto& h : handles_) h = nullptr;
    }

    LearnerConfig cfg_;
    std::vector<fi_learner*> handles_;               // per player: shard 0 (publishes, checkpoints)
    std::vector<std::vector<fi_learner*>> shards_;  // per player: its G data-parallel replicas
    std::vector<fi_step_stats> stats_;
    mutable std::mutex mu_;
    std::vector<std::string> err_;
};

}  // namespace freeimpala_amd
