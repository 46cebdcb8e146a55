// learner.cpp -- fi_learner: one device learner per player, behind the C ABI of
// include/fi_learner.h. Replaces the body of Learner::trainModel
// (reference include/freeimpala/learner.h:32-49): ingest -> policy forward -> V-trace +
// loss + analytic grads -> policy backward -> [RCCL all-reduce over xGMI] -> optimizer ->
// new parameter version (published through ModelManager::updateModel by the C++ caller,
// reference data_structures.h:441-451).
//
// Everything runs on one HIP stream per handle; no global mutable state, so handles of
// different players may step concurrently from different threads (reference learner.h:
// 158-163 runs one worker thread per player).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "atari.h"
#include "fi_common.h"
#include "fi_rollout.h"
#include "fi_train.h"
#include "host_util.h"
#include "kernels.h"

namespace fi {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

}  // namespace fi

using namespace fi;

struct fi_learner {
    fi_learner_config cfg{};
    int dev = 0;
    hipStream_t stream = nullptr;
    int T = 0, B = 0, A = 0, D = 0, H = 0;
    int rows = 0, TB = 0;
    size_t nparams = 0;
    // parameters / optimizer
    float* params = nullptr;
    float* grads = nullptr;
    float* opt_m = nullptr;
    float* opt_v = nullptr;
    // batch (time-major SoA)
    float* obs = nullptr;
    uint8_t* frames = nullptr;
    float* mu = nullptr;
    int32_t* act = nullptr;
    float* rew = nullptr;
    float* disc = nullptr;
    // network / loss tensors
    float* h1 = nullptr;  // MLP
    float* h2 = nullptr;
    float* dz1 = nullptr;
    float* dz2 = nullptr;
    float* logits = nullptr;
    float* values = nullptr;
    float* vs = nullptr;
    float* pg_adv = nullptr;
    float* dlogits = nullptr;
    float* dvalue = nullptr;
    double* small = nullptr;  // [0..2] losses, [3] grad sqnorm, [8..] sqnorm partials
    int* bad = nullptr;       // actions outside [0, A) in the current step's batch
    void* vt_ws = nullptr;
    size_t vt_ws_bytes = 0;
    float* slab = nullptr;
    size_t slab_floats = 0;
    int splits = 1;
    AtariNet* atari = nullptr;
    // host entry staging, double-buffered on both sides of PCIe: the host copy of batch k+1
    // into pinned2[s] and its H2D into rec_slot[s] (on copy_stream) overlap the device step
    // of batch k (fi_learner_step_async). h2d_done[s] marks the end of the H2D that reads
    // pinned2[s] / writes rec_slot[s]; ingest_done[s] the end of the ingest kernel that reads
    // rec_slot[s].
    char* pinned2[2] = {nullptr, nullptr};
    char* rec_slot[2] = {nullptr, nullptr};
    hipEvent_t h2d_done[2] = {nullptr, nullptr};
    hipEvent_t ingest_done[2] = {nullptr, nullptr};
    hipStream_t copy_stream = nullptr;
    int stage = 0;
    int cur = 0;             // slot the next host step ingests from
    int acquired = -1;       // slot handed out by acquire_slot and not yet submitted
    bool in_flight = false;  // an async step was enqueued and not yet waited for
    size_t rec_bytes = 0;
    size_t rec_entry_bytes = 0;
    int rec_format = FI_RECORDS_STACKED;  // Atari host entries: whole stacks, or single planes
    // entries already in device memory (fi_rollout.h): recorded after the ingest that read them
    hipEvent_t entries_consumed = nullptr;
    // a batch gathered from segments (fi_gather.h): the column table, B base addresses, and behind
    // it the version block {min u32, max u32, sum u64}; one allocation, on the first such step
    const void** cols = nullptr;
    uint32_t* versions = nullptr;
    bool have_versions = false;
    // per-column loss weights (fi_weights.h): B floats, allocated by the first set
    float* col_w = nullptr;
    bool col_w_on = false;
    ScaleFn col_scale = nullptr;
    // the training recipe (fi_train.h): configuration, not part of the state blob
    int opt_kind = FI_OPT_ADAM;  // cfg.optimizer until fi_train_set_rmsprop
    RmsPropHp rms{0.f, 0.f, 0.f, false};
    float lr_base = 0.f;  // cfg.lr until fi_train_set_lr
    float lr_end = 0.f;
    uint64_t lr_steps = 0;
    bool lr_sched = false;
    float reward_clip = 0.f;  // 0: off
    // the publication block (fi_publish.h): made and freed by publish.hip, which hands its free
    // function in with it; atomic because an actor's thread may look it up (fi_actor_set_params_dev)
    std::atomic<void*> publish{nullptr};
    void (*publish_free)(void*) = nullptr;
    // the diagnostics block (fi_diag.h): made and freed by diag.hip in the same way; `stepped`: a step
    // has been enqueued on the handle, so the loss tensors hold a step's values
    void* diag = nullptr;
    void (*diag_free)(void*) = nullptr;
    bool stepped = false;
    // PopArt (fi_popart.h): the block is popart.hip's, with its launchers and its free function
    PopartBlock* popart = nullptr;
    void (*popart_free)(void*) = nullptr;
    // the clipped surrogate objective (fi_surrogate.h): the block is surrogate.hip's, with its launcher
    SurrogateBlock* surrogate = nullptr;
    void (*surrogate_free)(void*) = nullptr;
    // the target network (fi_target.h): the block is target.hip's, with its launchers
    TargetBlock* target = nullptr;
    void (*target_free)(void*) = nullptr;
    // the KL penalty (fi_kl.h): the block is kl.hip's, with its launchers
    KlBlock* kl = nullptr;
    void (*kl_free)(void*) = nullptr;
    // data parallel
    ncclComm_t comm = nullptr;
    int rank = 0, nranks = 1;
    // bucketed gradient all-reduce: buckets start on comm_stream as the backward finalises
    // them (reverse layer order); the optimizer waits for the last one (comm_done)
    hipStream_t comm_stream = nullptr;
    std::vector<hipEvent_t> bucket_ev;
    hipEvent_t comm_done = nullptr;
    hipEvent_t bad_ready = nullptr;  // orders the reject-flag all-reduce when no bucket ran
    int buckets = 0;  // buckets issued in the last step (introspection)
    // bookkeeping
    uint64_t version = 0;
    int step_count = 0;
    bool profiling = false;
    hipEvent_t ev[FI_PHASE_COUNT + 1] = {};
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    double phase_sum[FI_PHASE_COUNT] = {};
    int phase_steps = 0;
    // per-launch tags (profiling mode): event pairs consumed in launch order each step
    std::vector<hipEvent_t> tag_ev;
    std::vector<const char*> tag_name;
    int tag_used = 0;
    std::vector<std::pair<std::string, std::pair<double, int>>> tag_sum;
    std::vector<void*> allocs;
};

static constexpr int kSqParts = 512;

static int dalloc(fi_learner* l, void** p, size_t bytes) {
    FI_TRY(dev_alloc(p, bytes ? bytes : 16, "learner"));
    l->allocs.push_back(*p);
    return FI_OK;
}

template <typename T>
static int dalloc_n(fi_learner* l, T** p, size_t n) {
    return dalloc(l, (void**)p, n * sizeof(T));
}

// ------------------------------------------------------------------ parameters
static uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Glorot-uniform weights (U(-l, l), l = sqrt(6/(fan_in+fan_out))), zero biases.
static void glorot(std::vector<float>& p, size_t off, size_t n, int fan_in, int fan_out,
                   uint64_t& st) {
    const double lim = std::sqrt(6.0 / (double)(fan_in + fan_out));
    for (size_t i = 0; i < n; ++i) {
        const double u = (double)(splitmix64(st) >> 11) * (1.0 / 9007199254740992.0);
        p[off + i] = (float)((2.0 * u - 1.0) * lim);
    }
}

static void init_mlp_params(const fi_learner* l, std::vector<float>& p) {
    const int D = l->D, H = l->H, O = l->A + 1;
    p.assign(l->nparams, 0.f);
    uint64_t st = l->cfg.seed;
    size_t o = 0;
    glorot(p, o, (size_t)D * H, D, H, st); o += (size_t)D * H + H;
    glorot(p, o, (size_t)H * H, H, H, st); o += (size_t)H * H + H;
    glorot(p, o, (size_t)H * O, H, O, st);
}

// ------------------------------------------------------------------ lifecycle
extern "C" int fi_abi_version(void) { return FI_ABI_VERSION; }
extern "C" const char* fi_last_error(void) { return fi::g_err.c_str(); }

extern "C" void fi_learner_config_init(fi_learner_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = sizeof(*c);
    c->arch = FI_ARCH_MLP;
    c->seq_len = 100;
    c->batch = 32;
    c->num_actions = 18;
    c->obs_dim = 128;
    c->hidden = 256;
    c->optimizer = FI_OPT_ADAM;
    c->publish_dtype = FI_PUBLISH_FP32;
    c->device = 0;
    c->gamma = 0.99f;
    c->hp = fi_vtrace_hparams{1.f, 1.f, 1.f, 1.f, 0.5f, 0.01f};
    c->lr = 5e-4f;
    c->beta1 = 0.9f;
    c->beta2 = 0.999f;
    c->eps = 1e-8f;
    c->max_grad_norm = 40.f;
    c->seed = 1;
}

static void destroy(fi_learner* l) {
    if (!l) return;
    if (l->stream) hipStreamSynchronize(l->stream);
    if (l->copy_stream) hipStreamSynchronize(l->copy_stream);
    if (void* pb = l->publish.load()) l->publish_free(pb);
    if (l->diag) l->diag_free(l->diag);
    if (l->popart) l->popart_free(l->popart);
    if (l->surrogate) l->surrogate_free(l->surrogate);
    if (l->target) l->target_free(l->target);
    if (l->kl) l->kl_free(l->kl);
    if (l->comm) ncclCommDestroy(l->comm);
    for (hipEvent_t e : l->bucket_ev) hipEventDestroy(e);
    if (l->entries_consumed) hipEventDestroy(l->entries_consumed);
    if (l->comm_done) hipEventDestroy(l->comm_done);
    if (l->bad_ready) hipEventDestroy(l->bad_ready);
    if (l->comm_stream) hipStreamDestroy(l->comm_stream);
    atari_destroy(l->atari);
    for (void* p : l->allocs) hipFree(p);
    for (int i = 0; i < 2; ++i) {
        if (l->pinned2[i]) hipHostFree(l->pinned2[i]);
        if (l->h2d_done[i]) hipEventDestroy(l->h2d_done[i]);
        if (l->ingest_done[i]) hipEventDestroy(l->ingest_done[i]);
    }
    for (auto& e : l->ev)
        if (e) hipEventDestroy(e);
    for (auto& e : l->tag_ev)
        if (e) hipEventDestroy(e);
    if (l->ev_a) hipEventDestroy(l->ev_a);
    if (l->ev_b) hipEventDestroy(l->ev_b);
    if (l->stream) hipStreamDestroy(l->stream);
    if (l->copy_stream) hipStreamDestroy(l->copy_stream);
    delete l;
}

extern "C" void fi_learner_destroy(fi_learner* l) {
    if (!l) return;
    hipSetDevice(l->dev);
    destroy(l);
}

static int create(const fi_learner_config* cfg, fi_learner** out) {
    FI_REQUIRE(cfg && out, "create: null argument");
    FI_REQUIRE(cfg->struct_size == sizeof(fi_learner_config), "create: struct_size mismatch");
    FI_REQUIRE(cfg->seq_len >= 1 && cfg->batch >= 1, "create: T and B must be >= 1");
    FI_REQUIRE(cfg->num_actions >= 2 && cfg->num_actions <= 64, "create: 2 <= A <= 64");
    FI_REQUIRE(cfg->arch == FI_ARCH_MLP || cfg->arch == FI_ARCH_ATARI, "create: unknown arch");
    FI_REQUIRE(cfg->optimizer == FI_OPT_ADAM || cfg->optimizer == FI_OPT_SGD, "create: optimizer");
    if (cfg->arch == FI_ARCH_MLP)
        FI_REQUIRE(cfg->obs_dim >= 1 && cfg->obs_dim <= 128 && cfg->hidden >= 1 && cfg->hidden <= 4096,
                   "create: MLP needs 1 <= obs_dim <= 128 (record schema), hidden <= 4096");
    FI_TRY(use_device(cfg->device, "create"));

    fi_learner* l = new (std::nothrow) fi_learner();
    FI_REQUIRE(l, "create: out of host memory");
    *out = nullptr;
    std::unique_ptr<fi_learner, void (*)(fi_learner*)> guard(l, destroy);

    l->cfg = *cfg;
    l->opt_kind = cfg->optimizer;
    l->lr_base = cfg->lr;
    l->dev = cfg->device;
    l->T = cfg->seq_len;
    l->B = cfg->batch;
    l->A = cfg->num_actions;
    l->D = cfg->obs_dim;
    l->H = cfg->hidden;
    l->rows = (l->T + 1) * l->B;
    l->TB = l->T * l->B;
    FI_HIP_CHECK(hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking));
    for (auto& e : l->ev) FI_HIP_CHECK(hipEventCreate(&e));
    FI_HIP_CHECK(hipEventCreate(&l->ev_a));
    FI_HIP_CHECK(hipEventCreate(&l->ev_b));

    const size_t rows = l->rows, TB = l->TB;
    const int A = l->A;
    std::vector<float> init;
    if (cfg->arch == FI_ARCH_MLP) {
        const int D = l->D, H = l->H, O = A + 1;
        l->nparams = (size_t)D * H + H + (size_t)H * H + H + (size_t)H * O + O;
        init_mlp_params(l, init);
        FI_TRY(dalloc_n(l, &l->obs, rows * D));
        FI_TRY(dalloc_n(l, &l->h1, rows * H));
        FI_TRY(dalloc_n(l, &l->h2, rows * H));
        FI_TRY(dalloc_n(l, &l->dz1, rows * H));
        FI_TRY(dalloc_n(l, &l->dz2, rows * H));
        // weight-gradient R-slices: 384 at R = 413,696 gives the K = 128 layer 1,536 workgroups
        // (6 per CU, the kernel's occupancy) -- with 128 its 512 workgroups left the CUs
        // latency-bound (wgrad_l1 0.44 -> 0.29 ms, wgrad_l2 0.60 -> 0.54 ms; 512 slices measured
        // slower: the slab sums grow)
        l->splits = (int)std::min<size_t>(384, std::max<size_t>(1, rows / 1024));
        // the largest weight gradient: the heads' H x (A + 1) too -- with A + 1 > max(D, H) its slabs
        // would otherwise run into the bias column sums behind them
        const size_t big = std::max<size_t>({(size_t)D * H, (size_t)H * H, (size_t)H * (A + 1)});
        l->slab_floats = (size_t)l->splits * (big + 4096);  // wgrad slabs | bias colsum slabs
        FI_TRY(dalloc_n(l, &l->slab, l->slab_floats));
    } else {
        l->atari = atari_create(l->B, l->T, A);
        FI_REQUIRE(l->atari, "create: Atari net allocation failed: " + std::string(fi_last_error()));
        l->nparams = atari_param_count(A);
        atari_init_params(A, cfg->seed, init);
        FI_TRY(dalloc_n(l, &l->frames, rows * AtariNet::kFrameBytes));
    }
    FI_TRY(dalloc_n(l, &l->params, l->nparams));
    FI_TRY(dalloc_n(l, &l->grads, l->nparams));
    FI_TRY(dalloc_n(l, &l->opt_m, l->nparams));
    FI_TRY(dalloc_n(l, &l->opt_v, l->nparams));
    FI_TRY(dalloc_n(l, &l->mu, TB * A));
    FI_TRY(dalloc_n(l, &l->act, TB));
    FI_TRY(dalloc_n(l, &l->rew, TB));
    FI_TRY(dalloc_n(l, &l->disc, TB));
    FI_TRY(dalloc_n(l, &l->logits, rows * A));
    FI_TRY(dalloc_n(l, &l->values, rows));
    FI_TRY(dalloc_n(l, &l->vs, TB));
    FI_TRY(dalloc_n(l, &l->pg_adv, TB));
    FI_TRY(dalloc_n(l, &l->dlogits, TB * A));
    FI_TRY(dalloc_n(l, &l->dvalue, rows));
    FI_TRY(dalloc_n(l, &l->small, 8 + kSqParts));
    FI_TRY(dalloc_n(l, &l->bad, 64));
    FI_HIP_CHECK(hipMemsetAsync(l->bad, 0, 64 * sizeof(int), l->stream));
    l->vt_ws_bytes = vtrace_workspace_bytes(l->T, l->B, A);
    FI_TRY(dalloc(l, &l->vt_ws, l->vt_ws_bytes));

    FI_HIP_CHECK(hipMemcpyAsync(l->params, init.data(), l->nparams * sizeof(float),
                                hipMemcpyHostToDevice, l->stream));
    FI_HIP_CHECK(hipMemsetAsync(l->opt_m, 0, l->nparams * sizeof(float), l->stream));
    FI_HIP_CHECK(hipMemsetAsync(l->opt_v, 0, l->nparams * sizeof(float), l->stream));
    FI_HIP_CHECK(hipMemsetAsync(l->grads, 0, l->nparams * sizeof(float), l->stream));
    // a defined (all-zero) batch until the first synth/step
    if (l->obs) FI_HIP_CHECK(hipMemsetAsync(l->obs, 0, rows * l->D * sizeof(float), l->stream));
    if (l->frames) FI_HIP_CHECK(hipMemsetAsync(l->frames, 0, rows * AtariNet::kFrameBytes, l->stream));
    FI_HIP_CHECK(hipMemsetAsync(l->mu, 0, TB * A * sizeof(float), l->stream));
    FI_HIP_CHECK(hipMemsetAsync(l->act, 0, TB * sizeof(int32_t), l->stream));
    FI_HIP_CHECK(hipMemsetAsync(l->rew, 0, TB * sizeof(float), l->stream));
    FI_HIP_CHECK(hipMemsetAsync(l->disc, 0, TB * sizeof(float), l->stream));
    if (l->atari) FI_TRY(atari_sync_weights(l->atari, l->params, l->stream));
    FI_HIP_CHECK(hipStreamSynchronize(l->stream));
    *out = guard.release();
    return FI_OK;
}

extern "C" int fi_learner_create(const fi_learner_config* cfg, fi_learner** out) {
    return guarded("create", FI_ERR_OOM, [&] { return create(cfg, out); });
}

extern "C" size_t fi_learner_param_count(const fi_learner* l) { return l ? l->nparams : 0; }
extern "C" size_t fi_learner_param_bytes(const fi_learner* l) {
    if (!l) return 0;
    return l->nparams * (l->cfg.publish_dtype == FI_PUBLISH_BF16 ? 2 : 4);
}
// one step's record in a host entry: a 1 KiB ELEMENT (MLP), 28 of them (Atari: frame + header),
// 7 (Atari planes: the newest plane + header)
static size_t record_bytes(const fi_learner* l) {
    if (l->cfg.arch != FI_ARCH_ATARI) return (size_t)FI_RECORD_BYTES;
    return l->rec_format == FI_RECORDS_PLANES ? (size_t)FI_ATARI_PLANE_RECORD_BYTES : (size_t)FI_ATARI_RECORD_BYTES;
}
// what follows an entry's T+1 records: the history block of the planes format
static size_t entry_tail_bytes(const fi_learner* l) {
    return l->cfg.arch == FI_ARCH_ATARI && l->rec_format == FI_RECORDS_PLANES ? (size_t)FI_ATARI_HISTORY_BYTES : 0;
}
static size_t entry_bytes_min(const fi_learner* l) { return (size_t)(l->T + 1) * record_bytes(l) + entry_tail_bytes(l); }
extern "C" size_t fi_learner_record_bytes(const fi_learner* l) { return l ? record_bytes(l) : 0; }
extern "C" size_t fi_learner_entry_bytes(const fi_learner* l) { return l ? entry_bytes_min(l) : 0; }
extern "C" int fi_learner_set_record_format(fi_learner* l, int fmt) {
    FI_REQUIRE(l, "set_record_format: null learner");
    FI_REQUIRE(l->cfg.arch == FI_ARCH_ATARI, "set_record_format: only the Atari policy has record formats");
    FI_REQUIRE(fmt == FI_RECORDS_STACKED || fmt == FI_RECORDS_PLANES, "set_record_format: unknown format");
    FI_REQUIRE(fmt != FI_RECORDS_PLANES || l->A <= 18,
               "set_record_format: the plane record's header holds mu[18]: num_actions = " + std::to_string(l->A) +
                   " > 18 needs the stacked format");
    if (l->rec_bytes != 0)
        return fail(FI_ERR_STATE, "set_record_format: the staging buffers exist (choose the format before the "
                                  "first host batch)");
    l->rec_format = fmt;
    return FI_OK;
}
extern "C" void* fi_learner_stream(fi_learner* l) { return l ? (void*)l->stream : nullptr; }
extern "C" int fi_learner_sync(fi_learner* l) {
    FI_REQUIRE(l, "sync: null");
    FI_HIP_CHECK(hipSetDevice(l->dev));
    FI_HIP_CHECK(hipStreamSynchronize(l->stream));
    return FI_OK;
}

// ------------------------------------------------------------------ the step
static void mark(fi_learner* l, int phase) {
    if (l->profiling) hipEventRecord(l->ev[phase], l->stream);
}

// RAII launch tag: records an event pair around the launches in its scope when profiling.
struct Tag {
    fi_learner* l;
    int idx = -1;
    Tag(fi_learner* l_, const char* name) : l(l_) {  // name == nullptr: no tag
        if (!l->profiling || !name) return;
        if ((size_t)(2 * l->tag_used + 2) > l->tag_ev.size()) {
            hipEvent_t a = nullptr, b = nullptr;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
            l->tag_ev.push_back(a);
            l->tag_ev.push_back(b);
            l->tag_name.push_back(nullptr);
        }
        idx = l->tag_used++;
        l->tag_name[idx] = name;
        (void)hipEventRecord(l->tag_ev[2 * idx], l->stream);
    }
    ~Tag() {
        if (idx >= 0) (void)hipEventRecord(l->tag_ev[2 * idx + 1], l->stream);
    }
};

// the same events, driven from inside the Atari net's launch sequence
struct LearnerTagger : KernelTagger {
    fi_learner* l;
    std::vector<Tag*> open;
    explicit LearnerTagger(fi_learner* l_) : l(l_) {}
    void begin(const char* name) override { open.push_back(new Tag(l, name)); }
    void end() override {
        delete open.back();
        open.pop_back();
    }
    ~LearnerTagger() override {
        for (Tag* t : open) delete t;
    }
};

static void collect_tags(fi_learner* l) {
    for (int i = 0; i < l->tag_used; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, l->tag_ev[2 * i], l->tag_ev[2 * i + 1]) != hipSuccess) continue;
        bool found = false;
        for (auto& e : l->tag_sum)
            if (e.first == l->tag_name[i]) {
                e.second.first += ms;
                e.second.second += 1;
                found = true;
                break;
            }
        if (!found) l->tag_sum.push_back({l->tag_name[i], {ms, 1}});
    }
    l->tag_used = 0;
}

// Gradient buckets in reverse layer order: once the backward has enqueued
// the final write of grads[off, off+n), an event on the compute stream gates that bucket's
// in-place ncclAllReduce(sum) on comm_stream, so the reduction of the fc/heads gradients
// (95 % of the Atari net's bytes) overlaps the conv backward. Every rank issues the same
// buckets in the same order. Without a communicator the hook does nothing.
struct BucketAllReduce : GradReadyHook {
    fi_learner* l;
    int n = 0;
    explicit BucketAllReduce(fi_learner* l_) : l(l_) {}
    int ready(size_t off, size_t count) override {
        if (!l->comm || count == 0) return FI_OK;
        if ((size_t)n >= l->bucket_ev.size()) {
            hipEvent_t e;
            FI_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            l->bucket_ev.push_back(e);
        }
        FI_HIP_CHECK(hipEventRecord(l->bucket_ev[n], l->stream));
        FI_HIP_CHECK(hipStreamWaitEvent(l->comm_stream, l->bucket_ev[n], 0));
        ++n;
        ncclResult_t r = ncclAllReduce(l->grads + off, l->grads + off, count, ncclFloat, ncclSum,
                                       l->comm, l->comm_stream);
        if (r != ncclSuccess) return fail(FI_ERR_COMM, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
        return FI_OK;
    }
    // The reject decision is agreed before anything is applied: after the last bucket the
    // int counter of out-of-range actions (written by ingest and the V-trace kernel, both
    // ordered before the first bucket's event) is summed over the ranks on the same stream,
    // so the optimizer of EVERY replica sees the group's count and all of them skip the
    // update together -- a shard's gradient from clamped actions is in the summed gradient,
    // and no replica may apply it (reference log-and-skip: data_structures.h:420-421,
    // agent.h:88-91). The compute stream then waits for every bucket before the optimizer
    // reads the gradients.
    int join() {
        l->buckets = n;
        if (!l->comm) return FI_OK;
        if (n == 0) {  // a backward without buckets still has to agree on the reject flag
            FI_HIP_CHECK(hipEventRecord(l->bad_ready, l->stream));
            FI_HIP_CHECK(hipStreamWaitEvent(l->comm_stream, l->bad_ready, 0));
        }
        ncclResult_t r = ncclAllReduce(l->bad, l->bad, 1, ncclInt32, ncclSum, l->comm, l->comm_stream);
        if (r != ncclSuccess) return fail(FI_ERR_COMM, std::string("ncclAllReduce(reject flag): ") + ncclGetErrorString(r));
        FI_HIP_CHECK(hipEventRecord(l->comm_done, l->comm_stream));
        FI_HIP_CHECK(hipStreamWaitEvent(l->stream, l->comm_done, 0));
        return FI_OK;
    }
};

// params: the learner's slab, or another of its layout (the target network's, fi_target.h: its launches
// carry no tags of their own, one tag stands around the call)
static int mlp_forward(fi_learner* l, const float* params, float* logits, float* values) {
    const int D = l->D, H = l->H, A = l->A;
    const bool own = params == l->params;
    const float* W1 = params;
    const float* b1 = W1 + (size_t)D * H;
    const float* W2 = b1 + H;
    const float* b2 = W2 + (size_t)H * H;
    const float* Wh = b2 + H;
    const float* bh = Wh + (size_t)H * (A + 1);
    { Tag t(l, own ? "mlp_fwd_l1" : nullptr); FI_TRY(f32_linear_fwd(l->obs, l->rows, D, W1, b1, H, true, l->h1, l->stream)); }
    { Tag t(l, own ? "mlp_fwd_l2" : nullptr); FI_TRY(f32_linear_fwd(l->h1, l->rows, H, W2, b2, H, true, l->h2, l->stream)); }
    { Tag t(l, own ? "mlp_fwd_heads" : nullptr); FI_TRY(f32_heads_fwd(l->h2, l->rows, H, Wh, bh, A, logits, values, l->stream)); }
    return FI_OK;
}

static int wgrad(fi_learner* l, const char* tag, const float* X, int I, const float* dY, int N,
                 float* gW, float* gb) {
    float* cs = l->slab + l->slab_floats - (size_t)l->splits * 4096;
    { Tag t(l, tag); FI_TRY(f32_linear_wgrad_partial(X, l->rows, I, dY, N, l->splits, l->slab, cs, l->stream)); }
    { Tag t(l, "reduce_slabs"); FI_TRY(reduce_slabs(l->slab, l->splits, (size_t)I * N, gW, l->stream)); }
    { Tag t(l, "reduce_slabs"); FI_TRY(reduce_slabs(cs, l->splits, (size_t)N, gb, l->stream)); }
    return FI_OK;
}

static int mlp_backward(fi_learner* l, GradReadyHook* gr) {
    const int D = l->D, H = l->H, A = l->A, O = A + 1;
    const float* W2 = l->params + (size_t)D * H + H;
    const float* Wh = W2 + (size_t)H * H + H;
    float* gW1 = l->grads;
    float* gb1 = gW1 + (size_t)D * H;
    float* gW2 = gb1 + H;
    float* gb2 = gW2 + (size_t)H * H;
    float* gWh = gb2 + H;
    float* gbh = gWh + (size_t)H * O;
    HeadsGrad g{l->dlogits, l->dvalue, l->rows, l->TB, A};
    float* cs = l->slab + l->slab_floats - (size_t)l->splits * 4096;
    if (f32_heads_bwd_fused_supported(H, A) && (size_t)kHeadsFusedGrid * (H * O + O) <= l->slab_floats) {
        // both heads gradients in one pass over h2 (weight-gradient slabs, then dz2)
        float* hcs = l->slab + (size_t)kHeadsFusedGrid * H * O;
        { Tag t(l, "mlp_heads_bwd"); FI_TRY(f32_heads_bwd_fused(g, l->h2, Wh, H, l->dz2, l->slab, hcs, kHeadsFusedGrid, l->stream)); }
        { Tag t(l, "reduce_slabs"); FI_TRY(reduce_slabs(l->slab, kHeadsFusedGrid, (size_t)H * O, gWh, l->stream)); }
        { Tag t(l, "reduce_slabs"); FI_TRY(reduce_slabs(hcs, kHeadsFusedGrid, (size_t)O, gbh, l->stream)); }
        FI_TRY(gr->ready((size_t)(gWh - l->grads), (size_t)H * O + O));
    } else {
        { Tag t(l, "mlp_wgrad_heads"); FI_TRY(f32_heads_wgrad_partial(l->h2, H, g, l->splits, l->slab, cs, l->stream)); }
        { Tag t(l, "reduce_slabs"); FI_TRY(reduce_slabs(l->slab, l->splits, (size_t)H * O, gWh, l->stream)); }
        { Tag t(l, "reduce_slabs"); FI_TRY(reduce_slabs(cs, l->splits, (size_t)O, gbh, l->stream)); }
        FI_TRY(gr->ready((size_t)(gWh - l->grads), (size_t)H * O + O));
        { Tag t(l, "mlp_dgrad_heads"); FI_TRY(f32_heads_dgrad(g, Wh, H, l->h2, l->dz2, l->stream)); }
    }
    FI_TRY(wgrad(l, "mlp_wgrad_l2", l->h1, H, l->dz2, H, gW2, gb2));
    FI_TRY(gr->ready((size_t)(gW2 - l->grads), (size_t)H * H + H));
    { Tag t(l, "mlp_dgrad_l2"); FI_TRY(f32_linear_dgrad(l->dz2, l->rows, H, W2, H, l->h1, l->dz1, l->stream)); }
    FI_TRY(wgrad(l, "mlp_wgrad_l1", l->obs, D, l->dz1, H, gW1, gb1));
    FI_TRY(gr->ready(0, (size_t)D * H + H));
    return FI_OK;
}

// A batch with actions outside [0, A) (a corrupt record, or actors configured with another
// --num-actions) is rejected: the optimizer kernels see the device counter and leave the
// parameters and moments untouched, and the step reports FI_ERR_INVALID once it has
// completed (the oracle rejects the same batch, oracle/impala_oracle.c). Called after the
// stream has been synchronised.
// The flag words l->bad (csrc/misc.hip, skip_update): [0] out-of-range actions of the current
// step (all-reduced), [1] its gradient norm was NaN / Inf (taken from the all-reduced gradient,
// so every replica sees the same value), [2] updates skipped since the last check, [3] their
// reasons (1 = actions, 2 = non-finite). Every replica skips the same updates. A synchronous
// step checks its own; fi_learner_wait checks every step enqueued since the last check, so a
// skipped step behind others still in flight is reported, and the version counts applied
// updates only (an enqueued step behind a skipped one keeps the Adam step number it was given).
static int check_rejected(fi_learner* l) {
    int bad[4] = {0, 0, 0, 0};
    FI_HIP_CHECK(hipMemcpy(bad, l->bad, sizeof(bad), hipMemcpyDeviceToHost));
    const int skipped = bad[2], why = bad[3];
    if (skipped == 0) return FI_OK;
    FI_HIP_CHECK(hipMemsetAsync(l->bad + 2, 0, 2 * sizeof(int), l->stream));  // ordered before the next step
    l->step_count -= skipped;
    l->version -= (uint64_t)skipped;
    const std::string n = skipped > 1 ? std::to_string(skipped) + " of the enqueued updates skipped" : "update skipped";
    if (!(why & 1))
        return fail(FI_ERR_NONFINITE, "step: the gradient norm is not finite (NaN / Inf in the batch's losses or "
                                      "gradients); " + n + ", parameters unchanged");
    const std::string acts = bad[0] > 0 ? std::to_string(bad[0]) + " action(s)" : "action(s)";
    if (l->comm && l->nranks > 1)
        return fail(FI_ERR_INVALID, "step: " + acts + " outside [0, " + std::to_string(l->A) +
                                        ") in the data-parallel group's batch (all-reduced reject flag); batch "
                                        "rejected on every replica, " + n + ", parameters unchanged");
    return fail(FI_ERR_INVALID, "step: " + acts + " outside [0, " + std::to_string(l->A) + ") in the batch; batch "
                                "rejected, " + n + ", parameters unchanged");
}

static void fill_stats(fi_learner* l, fi_step_stats* out) {
    double h[4];
    if (hipMemcpy(h, l->small, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess)
        for (double& x : h) x = std::nan("");
    const fi_vtrace_hparams& hp = l->cfg.hp;
    out->pg_loss = h[0];
    out->baseline_loss = h[1];
    out->entropy_loss = h[2];
    out->total_loss = h[0] + hp.baseline_cost * h[1] + hp.entropy_cost * h[2];
    out->grad_norm = std::sqrt(h[3]);
    out->version = l->version;
    out->step_ms = 0.f;
}

// Where a step's batch comes from; nullptr = the resident batch (fi_learner_step_resident, the
// synthetic one). `ingest` is a plain function and `ctx` what it reads: nothing is allocated per
// step, and gather.hip's and ring.hip's ingests arrive as pointers (kernels.h), so a library of the
// learner alone, without them, links.
struct BatchSource {
    const hipEvent_t* wait;  // the learner's stream waits for these first (null entries are skipped)
    int n_wait;
    IngestFn ingest;
    const void* ctx;
    hipEvent_t done;  // recorded behind the ingest: ingest_done[slot], or entries_consumed
    bool versions;    // the ingest fills the version block
    const float* weights;  // nullable: column weights the ingest writes, in place of the handle's (fi_weights.h)
    ScaleFn scale;         // what applies them
};

// the learning rate of the update numbered s >= 1 (fi_train.h): lr_base, or the linear anneal from
// lr_base at s = 1 to lr_end at s = lr_steps + 1 and beyond, in double
static float lr_of(const fi_learner* l, uint64_t s) {
    if (!l->lr_sched) return l->lr_base;
    const uint64_t k = std::min(s - 1, l->lr_steps);
    if (k == l->lr_steps) return l->lr_end;  // exactly, whatever (x * n) / n rounds to
    return (float)((double)l->lr_base + ((double)l->lr_end - (double)l->lr_base) * (double)k / (double)l->lr_steps);
}

// the width of the layer under the heads: both policies end in (inputs x (A + 1)) weights, then A + 1
// biases, with the value head in column A (mlp_forward; atari.hip's Offsets: hw, hb, fc width 512)
static int head_inputs(const fi_learner* l) { return l->cfg.arch == FI_ARCH_ATARI ? 512 : l->H; }

static BatchTensors batch_tensors(const fi_learner* l) {
    return BatchTensors{l->cfg.arch, l->T,   l->B,    l->A,   l->D,    l->obs,      l->frames, l->mu,
                        l->act,      l->rew, l->disc, l->bad, l->cols, l->versions, l->stream};
}

// The target network's logits of this batch (fi_target.h, 1.): the learner's own net and activations on
// the target parameters, in front of the learner's forward, which overwrites the activations again
static int target_forward(fi_learner* l) {
    const TargetBlock* tb = l->target;
    if (l->cfg.arch == FI_ARCH_MLP) {
        Tag t(l, "target_forward");
        return mlp_forward(l, tb->theta, tb->tlogits, tb->tvalues);
    }
    // the net points at theta- between the two syncs only: the way back is taken whatever the forward returned
    int rc;
    { Tag t(l, "target_weights_bf16"); rc = atari_sync_weights(l->atari, tb->theta, l->stream); }
    if (rc == FI_OK) {
        Tag t(l, "target_forward");
        rc = atari_forward(l->atari, l->frames, tb->tlogits, tb->tvalues, l->stream, nullptr);
    }
    int back;
    { Tag t(l, "target_weights_back"); back = atari_sync_weights(l->atari, l->params, l->stream); }
    return rc != FI_OK ? rc : back;
}

static int run_step(fi_learner* l, const BatchSource* src, fi_step_stats* out) {
    const bool sync = out != nullptr || l->profiling;
    l->tag_used = 0;
    if (out) FI_HIP_CHECK(hipEventRecord(l->ev_a, l->stream));
    mark(l, FI_PHASE_INGEST);
    FI_HIP_CHECK(hipMemsetAsync(l->bad, 0, sizeof(int), l->stream));
    if (src) {
        for (int k = 0; k < src->n_wait; ++k)
            if (src->wait[k]) FI_HIP_CHECK(hipStreamWaitEvent(l->stream, src->wait[k], 0));
        {
            Tag t(l, "ingest");
            FI_TRY(src->ingest(src->ctx, batch_tensors(l)));
        }
        FI_HIP_CHECK(hipEventRecord(src->done, l->stream));
        if (src->versions) l->have_versions = true;
    }
    if (l->reward_clip > 0.f) {  // in place and idempotent: a resident batch stepped again is clipped once in effect
        Tag t(l, "clip_rewards");
        FI_TRY(clip_rewards_launch(l->rew, (size_t)l->TB, l->reward_clip, l->stream));
    }
    mark(l, FI_PHASE_FORWARD);
    const bool sur_on = l->surrogate && l->surrogate->on, tgt_on = l->target && l->target->on;
    if (sur_on && tgt_on) FI_TRY(target_forward(l));
    if (l->cfg.arch == FI_ARCH_MLP) FI_TRY(mlp_forward(l, l->params, l->logits, l->values));
    else {
        LearnerTagger tg(l);
        FI_TRY(atari_forward(l->atari, l->frames, l->logits, l->values, l->stream, l->profiling ? &tg : nullptr));
    }
    if (l->popart) {  // the head predicts normalised values: everything behind this sees sigma n + mu
        Tag t(l, "popart_denorm");
        FI_TRY(l->popart->denorm(l->values, (size_t)l->rows, l->popart->state, l->stream));
    }
    mark(l, FI_PHASE_VTRACE);
    int vt_nblk = 0;
    const double* loss_part = nullptr;  // [vt_nblk][3], summed by the gradient-norm kernel
    if (sur_on && tgt_on) {
        // the surrogate around the target network (fi_target.h): the same outputs again
        LearnerTagger tg(l);
        FI_TRY(l->target->launch(l->target, l->surrogate, l->T, l->B, l->A, l->logits, l->mu, l->act, l->rew, l->disc,
                                 l->values, l->cfg.hp, l->vs, l->pg_adv, l->dlogits, l->dvalue, l->bad, l->stream,
                                 l->profiling ? &tg : nullptr, &loss_part, &vt_nblk));
    } else if (sur_on) {
        // the second objective (fi_surrogate.h) in V-trace's place: the same outputs, its own tags
        LearnerTagger tg(l);
        FI_TRY(l->surrogate->launch(l->surrogate, l->T, l->B, l->A, l->logits, l->mu, l->act, l->rew, l->disc, l->values,
                                    l->cfg.hp, l->vs, l->pg_adv, l->dlogits, l->dvalue, l->bad, l->stream,
                                    l->profiling ? &tg : nullptr, &loss_part, &vt_nblk));
    } else {
        // scan + loss + gradients; the loss partials are summed by the gradient-norm kernel
        Tag t(l, "vtrace");
        FI_TRY(vtrace_launch(0, l->T, l->B, l->A, l->logits, l->mu, l->act, l->rew, l->disc,
                             l->values, l->cfg.hp, l->vs, l->pg_adv, l->dlogits, l->dvalue,
                             l->small, l->vt_ws, l->vt_ws_bytes, l->stream, false, &vt_nblk,
                             l->bad));
        loss_part = vtrace_partials(l->vt_ws);
    }
    // the KL penalty (fi_kl.h): c (pi - q) onto dlogits, q the batch's mu or this step's target logits; a
    // step without the reference's logits enqueues neither this nor kl_adapt
    const KlBlock* kb = l->kl && l->kl->on ? l->kl : nullptr;
    const float* kl_q = !kb ? nullptr
                            : (kb->prm.reference == FI_KL_REF_BEHAVIOUR ? l->mu
                                                                        : (sur_on && tgt_on ? l->target->tlogits : nullptr));
    if (kl_q) {
        Tag t(l, "kl_penalty");
        FI_TRY(kb->penalty(kb, l->T, l->B, l->A, l->logits, kl_q, l->dlogits, l->stream));
    }
    if (l->popart) {  // d/dv -> d/dn: one division by sigma; row T (no gradient) is not touched
        Tag t(l, "popart_scale");
        FI_TRY(l->popart->scale(l->dvalue, (size_t)l->TB, l->popart->state, l->stream));
    }
    // the loss is a plain sum over the columns: w_b times column b's gradient is the gradient of
    // sum_b w_b L_b (fi_weights.h). vs, pg_adv and the loss partials stay unweighted
    const bool own = src && src->weights && src->scale;
    if (const float* w = own ? src->weights : (l->col_w_on ? l->col_w : nullptr)) {
        Tag t(l, "scale_columns");
        FI_TRY((own ? src->scale : l->col_scale)(l->dlogits, l->dvalue, w, l->T, l->B, l->A, l->stream));
    }
    mark(l, FI_PHASE_BACKWARD);
    BucketAllReduce bar(l);
    if (l->cfg.arch == FI_ARCH_MLP) FI_TRY(mlp_backward(l, &bar));
    else {
        LearnerTagger tg(l);
        FI_TRY(atari_backward(l->atari, l->frames, l->dlogits, l->dvalue, l->grads, l->stream,
                              l->profiling ? &tg : nullptr, &bar));
    }
    // the "allreduce" phase is the exposed tail: the wait for the buckets still in flight
    // when the backward has finished
    mark(l, FI_PHASE_ALLREDUCE);
    {
        Tag t(l, "allreduce_wait");
        FI_TRY(bar.join());
    }
    mark(l, FI_PHASE_OPTIMIZER);
    {
        Tag t(l, "grad_norm");  // + the V-trace loss sums (losses land in small[0..2])
        FI_TRY(grad_sqnorm(l->grads, l->nparams, l->small + 8, kSqParts, l->small + 3, l->stream,
                           loss_part, vt_nblk, l->small, l->bad + 1));
    }
    const int step = l->step_count + 1;
    const double bc1 = 1.0 - std::pow((double)l->cfg.beta1, step);
    const double bc2 = 1.0 - std::pow((double)l->cfg.beta2, step);
    {
        Tag t(l, "optimizer");
        // the rate of update `step` (fi_train.h) travels by value: an enqueued step keeps it
        FI_TRY(optimizer_step(l->opt_kind, l->params, l->grads, l->opt_m, l->opt_v, l->nparams,
                              lr_of(l, (uint64_t)step), l->cfg.beta1, l->cfg.beta2, l->cfg.eps, bc1, bc2,
                              l->small + 3, l->cfg.max_grad_norm, l->stream, l->bad, &l->rms));
    }
    if (l->popart) {
        // the statistics move with this step's targets and the value column is rewritten so that
        // sigma n + mu is preserved; skipped with the update (the words the optimiser read)
        Tag t(l, "popart_update");
        const PopartBlock* pa = l->popart;
        const int O = l->A + 1, Hh = head_inputs(l);
        float* b = l->params + l->nparams - 1;                   // the last bias of the heads
        float* w = l->params + l->nparams - O - (size_t)Hh * O + l->A;  // column A of the Hh x O weights
        FI_TRY(pa->update(l->vs, (size_t)l->TB, pa->state, w, (size_t)O, Hh, b, pa->beta, pa->sigma_min, pa->sigma_max,
                          l->bad, pa->ws, pa->ws_bytes, l->stream));
    }
    if (tgt_on && (uint64_t)step % l->target->period == 0) {
        // the target moves towards the parameters this update left; skipped with the update
        Tag t(l, "target_update");
        FI_TRY(l->target->update(l->target, l->params, l->bad, l->stream));
    }
    if (kl_q) {
        // the coefficient moves on this step's mean KL; not when the update was skipped
        Tag t(l, "kl_adapt");
        FI_TRY(kb->adapt(kb, l->T, l->B, l->A, l->bad, l->stream));
    }
    if (l->atari) {
        Tag t(l, "weights_bf16");
        FI_TRY(atari_sync_weights(l->atari, l->params, l->stream));
    }
    mark(l, FI_PHASE_COUNT);
    if (out) FI_HIP_CHECK(hipEventRecord(l->ev_b, l->stream));
    l->step_count = step;
    l->version++;
    if (sync) {
        FI_HIP_CHECK(hipStreamSynchronize(l->stream));
        if (l->profiling) {
            for (int p = 0; p < FI_PHASE_COUNT; ++p) {
                float ms = 0.f;
                FI_HIP_CHECK(hipEventElapsedTime(&ms, l->ev[p], l->ev[p + 1]));
                l->phase_sum[p] += ms;
            }
            l->phase_steps++;
            collect_tags(l);
        }
    }
    if (out) {
        FI_TRY(check_rejected(l));
        fill_stats(l, out);
        float ms = 0.f;
        FI_HIP_CHECK(hipEventElapsedTime(&ms, l->ev_a, l->ev_b));
        out->step_ms = ms;
    }
    return FI_OK;
}

extern "C" int fi_learner_step_resident(fi_learner* l, fi_step_stats* out) {
    FI_REQUIRE(l, "step: null learner");
    FI_HIP_CHECK(hipSetDevice(l->dev));
    l->stepped = true;
    return guarded("step", FI_ERR_STATE, [&] { return run_step(l, nullptr, out); });
}

static void parallel_copy(char* dst, const void* const* entries, size_t n, size_t entry_bytes,
                          size_t stride) {
    const size_t total = n * entry_bytes;
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const size_t nt = std::min<size_t>({n, (size_t)std::min(hw, 16u), 1 + total / (64u << 20)});
    auto work = [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) std::memcpy(dst + i * stride, entries[i], entry_bytes);
    };
    if (nt <= 1) {
        work(0, n);
        return;
    }
    std::vector<std::thread> th;
    const size_t per = (n + nt - 1) / nt;
    for (size_t t = 0; t < nt; ++t) {
        const size_t lo = t * per, hi = std::min(n, lo + per);
        if (lo < hi) th.emplace_back(work, lo, hi);
    }
    for (auto& t : th) t.join();
}

// Host staging, double-buffered: acquire_slot() hands out the next pinned buffer once the
// H2D that last read it is done; submit_slot() enqueues its H2D on the copy stream (after the
// ingest that last read the device slot) and makes it the batch the next run_step ingests.
static int ensure_staging(fi_learner* l) {
    const size_t need = entry_bytes_min(l);
    const size_t bytes = (size_t)l->B * need;
    if (bytes <= l->rec_bytes) return FI_OK;
    FI_HIP_CHECK(hipStreamSynchronize(l->stream));
    if (l->copy_stream) FI_HIP_CHECK(hipStreamSynchronize(l->copy_stream));
    else FI_HIP_CHECK(hipStreamCreateWithFlags(&l->copy_stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        if (l->pinned2[i]) hipHostFree(l->pinned2[i]);
        l->pinned2[i] = nullptr;
        if (l->rec_slot[i]) {
            hipFree(l->rec_slot[i]);
            l->allocs.erase(std::find(l->allocs.begin(), l->allocs.end(), (void*)l->rec_slot[i]));
        }
        l->rec_slot[i] = nullptr;
    }
    l->rec_bytes = 0;
    for (int i = 0; i < 2; ++i) {
        const hipError_t e = hipHostMalloc((void**)&l->pinned2[i], bytes, hipHostMallocDefault);
        if (e != hipSuccess) {
            l->pinned2[i] = nullptr;
            (void)hipGetLastError();
            return fail(FI_ERR_OOM, "step: hipHostMalloc(" + std::to_string(bytes) + ") for staging buffer " +
                                        std::to_string(i) + " of 2: " + hipGetErrorString(e));
        }
        FI_TRY(dalloc(l, (void**)&l->rec_slot[i], bytes));
        if (!l->h2d_done[i]) FI_HIP_CHECK(hipEventCreateWithFlags(&l->h2d_done[i], hipEventDisableTiming));
        if (!l->ingest_done[i]) FI_HIP_CHECK(hipEventCreateWithFlags(&l->ingest_done[i], hipEventDisableTiming));
        FI_HIP_CHECK(hipEventRecord(l->h2d_done[i], l->copy_stream));
        FI_HIP_CHECK(hipEventRecord(l->ingest_done[i], l->stream));
    }
    l->rec_bytes = bytes;
    l->rec_entry_bytes = need;
    return FI_OK;
}

static bool stage_timing() {
    static const bool on = std::getenv("FI_STAGE_TIMING") != nullptr;
    return on;
}

static int acquire_slot(fi_learner* l, int* slot) {
    FI_TRY(ensure_staging(l));
    if (l->acquired < 0) {
        const auto t0 = std::chrono::steady_clock::now();
        // pinned2[s] is free once the H2D that read it (two steps ago) is done
        FI_HIP_CHECK(hipEventSynchronize(l->h2d_done[l->stage]));
        l->acquired = l->stage;
        l->stage ^= 1;
        if (stage_timing())
            std::fprintf(stderr, "[fi stage] slot %d wait %.3f ms\n", l->acquired,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    *slot = l->acquired;
    return FI_OK;
}

static int submit_slot(fi_learner* l) {
    FI_REQUIRE(l->acquired >= 0, "step_staged: no staging slot acquired (fi_learner_acquire_staging)");
    const int s = l->acquired;
    // the device slot is rewritten after the ingest kernel of two steps ago has read it; the
    // copy runs on its own stream, beside the device step of the previous batch
    FI_HIP_CHECK(hipStreamWaitEvent(l->copy_stream, l->ingest_done[s], 0));
    FI_HIP_CHECK(hipMemcpyAsync(l->rec_slot[s], l->pinned2[s], l->rec_bytes, hipMemcpyHostToDevice,
                                l->copy_stream));
    FI_HIP_CHECK(hipEventRecord(l->h2d_done[s], l->copy_stream));
    l->cur = s;
    l->acquired = -1;
    return FI_OK;
}

// stage M host entries (only their first T+1 records) through the next pinned buffer; returns
// once the host copy is done (the entries may then be freed)
static int stage_entries(fi_learner* l, const void* const* entries, size_t n_entries, size_t entry_bytes) {
    FI_REQUIRE(l && entries, "step: null argument");
    FI_REQUIRE(n_entries == (size_t)l->B, "step: n_entries must equal the configured batch");
    const size_t need = entry_bytes_min(l);
    FI_REQUIRE(entry_bytes >= need, "step: entry_bytes " + std::to_string(entry_bytes) + " < " +
                                        std::to_string(need) + " = (T+1)*" + std::to_string(record_bytes(l)) +
                                        (entry_tail_bytes(l) ? " + " + std::to_string(entry_tail_bytes(l)) : ""));
    for (size_t i = 0; i < n_entries; ++i) FI_REQUIRE(entries[i], "step: null entry");
    FI_HIP_CHECK(hipSetDevice(l->dev));
    int s = 0;
    FI_TRY(acquire_slot(l, &s));
    const auto t0 = std::chrono::steady_clock::now();
    parallel_copy(l->pinned2[s], entries, n_entries, need, need);
    if (stage_timing()) {
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::fprintf(stderr, "[fi stage] slot %d copy %.3f ms (%.1f GB/s)\n", s, ms, l->rec_bytes / 1e6 / ms);
    }
    return submit_slot(l);
}

// Runs the step from `src` and ends it. wait: returns when the device step has completed,
// statistics or not, and reports a batch it rejected; otherwise the step is enqueued only (no
// sync) and fi_learner_wait reports it.
static int finish_step(fi_learner* l, const BatchSource& src, fi_step_stats* out, bool wait) {
    l->stepped = true;
    if (!wait) {
        FI_TRY(run_step(l, &src, nullptr));
        l->in_flight = true;
        return FI_OK;
    }
    l->in_flight = false;
    FI_TRY(run_step(l, &src, out));
    if (!out) {
        FI_HIP_CHECK(hipStreamSynchronize(l->stream));
        FI_TRY(check_rejected(l));
    }
    return FI_OK;
}

// the contiguous ingests (misc.hip): ctx names the entries
struct Entries {
    const void* ptr;
    size_t stride;
    int format;  // Atari: FI_RECORDS_*
};
static int ingest_entries(const void* ctx, const BatchTensors& to) {
    const Entries& e = *(const Entries*)ctx;
    if (to.arch == FI_ARCH_MLP) return ingest_launch(e.ptr, e.stride, to);
    if (e.format == FI_RECORDS_PLANES) return ingest_atari_planes_launch(e.ptr, e.stride, to);
    // frames (like mu / act / rew / disc) is rewritten in place: every kernel that read it in the
    // previous step -- the forward and the backward's conv1 weight gradient -- was enqueued on
    // this same stream, so stream order puts them before the ingest. The only other stream with
    // work of the previous step, comm_stream, touches grads and the reject flag alone, and was
    // joined before that step's optimizer (BucketAllReduce::join).
    return ingest_atari_launch(e.ptr, e.stride, to);
}

// the step from the staged host batch in device slot l->cur
static int step_staged_slot(fi_learner* l, fi_step_stats* out, bool wait) {
    const int s = l->cur;
    const Entries e{l->rec_slot[s], l->rec_entry_bytes, l->rec_format};
    return finish_step(l, BatchSource{&l->h2d_done[s], 1, ingest_entries, &e, l->ingest_done[s], false, nullptr, nullptr},
                       out, wait);
}

extern "C" int fi_learner_step(fi_learner* l, const void* const* entries, size_t n_entries,
                               size_t entry_bytes, fi_step_stats* out) {
    return guarded("step", FI_ERR_STATE, [&]() -> int {
        FI_TRY(stage_entries(l, entries, n_entries, entry_bytes));
        return step_staged_slot(l, out, true);
    });
}

extern "C" int fi_learner_step_async(fi_learner* l, const void* const* entries, size_t n_entries,
                                     size_t entry_bytes) {
    return guarded("step_async", FI_ERR_STATE, [&]() -> int {
        FI_TRY(stage_entries(l, entries, n_entries, entry_bytes));
        return step_staged_slot(l, nullptr, false);
    });
}

extern "C" int fi_learner_acquire_staging(fi_learner* l, void** dst, size_t* entry_stride) {
    FI_REQUIRE(l && dst, "acquire_staging: null argument");
    return guarded("acquire_staging", FI_ERR_STATE, [&]() -> int {
        FI_HIP_CHECK(hipSetDevice(l->dev));
        int s = 0;
        FI_TRY(acquire_slot(l, &s));
        *dst = l->pinned2[s];
        if (entry_stride) *entry_stride = l->rec_entry_bytes;
        return FI_OK;
    });
}

extern "C" int fi_learner_step_staged(fi_learner* l, fi_step_stats* out) {
    FI_REQUIRE(l, "step_staged: null learner");
    return guarded("step_staged", FI_ERR_STATE, [&]() -> int {
        FI_HIP_CHECK(hipSetDevice(l->dev));
        FI_TRY(submit_slot(l));
        return step_staged_slot(l, out, true);
    });
}

extern "C" int fi_learner_step_staged_async(fi_learner* l) {
    FI_REQUIRE(l, "step_staged_async: null learner");
    return guarded("step_staged_async", FI_ERR_STATE, [&]() -> int {
        FI_HIP_CHECK(hipSetDevice(l->dev));
        FI_TRY(submit_slot(l));
        return step_staged_slot(l, nullptr, false);
    });
}

extern "C" int fi_learner_wait(fi_learner* l, fi_step_stats* out) {
    FI_REQUIRE(l, "wait: null learner");
    FI_HIP_CHECK(hipSetDevice(l->dev));
    FI_HIP_CHECK(hipStreamSynchronize(l->stream));
    const bool was_in_flight = l->in_flight;
    l->in_flight = false;
    if (was_in_flight) FI_TRY(check_rejected(l));
    if (out) fill_stats(l, out);  // step_ms = 0: not timed on the asynchronous path
    return FI_OK;
}

// ------------------------------------------------------------------ entries in device memory (fi_rollout.h)
// the span check of host_util.h with the handle's own entry size, on the handle's device
static int check_entry_span(fi_learner* l, const void* entries, size_t stride, int n, const std::string& nm) {
    const size_t need = entry_bytes_min(l);
    FI_HIP_CHECK(hipSetDevice(l->dev));
    return fi::check_entry_span(l->dev, entries, stride, n, need, nm, std::to_string(need) + " = fi_learner_entry_bytes()");
}

// an Atari handle reads device entries in the planes format only (the stacked one is a host format)
static bool dev_entries_ok(const fi_learner* l) {
    return l->cfg.arch != FI_ARCH_ATARI || l->rec_format == FI_RECORDS_PLANES;
}

// entries_consumed, created by the first step from device entries
static int ensure_entries_consumed(fi_learner* l) {
    if (!l->entries_consumed) FI_HIP_CHECK(hipEventCreateWithFlags(&l->entries_consumed, hipEventDisableTiming));
    return FI_OK;
}

static int step_entries_dev(fi_learner* l, const void* entries, size_t stride, void* ready, fi_step_stats* out,
                            bool wait, const char* who) {
    return guarded(who, FI_ERR_STATE, [&]() -> int {
        const std::string nm = who;
        FI_REQUIRE(l && entries, nm + ": null argument");
        FI_TRY(require_dev_entries(dev_entries_ok(l), nm));
        FI_TRY(check_entry_span(l, entries, stride, l->B, nm));
        FI_TRY(ensure_entries_consumed(l));
        const hipEvent_t ev = (hipEvent_t)ready;
        const Entries e{entries, stride, l->rec_format};
        return finish_step(l, BatchSource{&ev, 1, ingest_entries, &e, l->entries_consumed, false, nullptr, nullptr}, out, wait);
    });
}

extern "C" int fi_learner_step_entries_dev(fi_learner* l, const void* entries_dev, size_t entry_stride,
                                           void* ready_event, fi_step_stats* out) {
    return step_entries_dev(l, entries_dev, entry_stride, ready_event, out, true, "step_entries_dev");
}

extern "C" int fi_learner_step_entries_dev_async(fi_learner* l, const void* entries_dev, size_t entry_stride,
                                                 void* ready_event) {
    return step_entries_dev(l, entries_dev, entry_stride, ready_event, nullptr, false, "step_entries_dev_async");
}

extern "C" void* fi_learner_entries_consumed_event(fi_learner* l) { return l ? (void*)l->entries_consumed : nullptr; }
extern "C" size_t fi_learner_staging_bytes(const fi_learner* l) { return l ? 4 * l->rec_bytes : 0; }

// ------------------------------------------------------------------ a batch read through the column table
// (fi_gather.h, fi_ring.h). The C entry points are gather.hip's and ring.hip's: they pass their
// ingest in, so learner.cpp names none of their launchers and a library of the learner alone
// still links (as with actor.hip above).
// the column table and the version block on first use, then the step, waited for or enqueued only
static int step_gathered(fi_learner* l, const hipEvent_t* ready, int n_ready, IngestFn ingest, const void* ctx,
                         fi_step_stats* out, bool wait, const float* weights = nullptr, ScaleFn scale = nullptr) {
    FI_HIP_CHECK(hipSetDevice(l->dev));
    if (!l->cols) {
        void* p = nullptr;
        FI_TRY(dalloc(l, &p, 8 * (size_t)l->B + 16));
        l->cols = (const void**)p;
        l->versions = (uint32_t*)((char*)p + 8 * (size_t)l->B);
    }
    FI_TRY(ensure_entries_consumed(l));
    return finish_step(l, BatchSource{ready, n_ready, ingest, ctx, l->entries_consumed, true, weights, scale},
                       out, wait);
}

int fi::learner_step_segments(fi_learner* l, const fi_entry_segment* segs, int32_t n_segs, fi_step_stats* out,
                              bool wait, const char* who, IngestFn ingest) {
    return guarded(who, FI_ERR_STATE, [&]() -> int {
        const std::string nm = who;
        FI_REQUIRE(l && segs && ingest, nm + ": null argument");
        FI_TRY(require_dev_entries(dev_entries_ok(l), nm));
        FI_REQUIRE(n_segs >= 1 && n_segs <= FI_MAX_SEGMENTS,
                   nm + ": " + std::to_string(n_segs) + " segments, 1 .. " + std::to_string(FI_MAX_SEGMENTS) + " are taken");
        SegTable tab{};
        hipEvent_t ready[FI_MAX_SEGMENTS];
        int64_t cols = 0;
        for (int k = 0; k < n_segs; ++k) {
            const std::string sk = nm + ": segment " + std::to_string(k);
            FI_REQUIRE(segs[k].entries_dev, sk + ": null entries_dev");
            FI_REQUIRE(segs[k].num_entries >= 1, sk + ": num_entries " + std::to_string(segs[k].num_entries) + " < 1");
            FI_TRY(check_entry_span(l, segs[k].entries_dev, segs[k].entry_stride, segs[k].num_entries, sk));
            FI_REQUIRE(cols + segs[k].num_entries <= l->B,
                       sk + ": columns " + std::to_string(cols) + " .. " + std::to_string(cols + segs[k].num_entries) +
                           " pass the learner's batch " + std::to_string(l->B));
            tab.seg[k] = {(const char*)segs[k].entries_dev, segs[k].entry_stride, (int32_t)cols, segs[k].num_entries};
            ready[k] = (hipEvent_t)segs[k].ready_event;
            cols += segs[k].num_entries;
        }
        tab.n = n_segs;
        FI_REQUIRE(cols == l->B, nm + ": the segments hold " + std::to_string(cols) + " entries, the learner's batch is " +
                                     std::to_string(l->B));
        return step_gathered(l, ready, n_segs, ingest, &tab, out, wait);
    });
}

int fi::learner_step_columns(fi_learner* l, hipEvent_t ready, IngestFn ingest, const void* ctx, fi_step_stats* out,
                             bool wait, const char* who, const float* weights, ScaleFn scale) {
    return guarded(who, FI_ERR_STATE, [&]() -> int {
        const std::string nm = who;
        FI_REQUIRE(l && ingest, nm + ": null argument");
        FI_TRY(require_dev_entries(dev_entries_ok(l), nm));
        return step_gathered(l, &ready, 1, ingest, ctx, out, wait, weights, scale);
    });
}

extern "C" int fi_learner_batch_versions(fi_learner* l, fi_batch_versions* out) {
    FI_REQUIRE(l && out, "batch_versions: null argument");
    if (!l->have_versions)
        return fail(FI_ERR_STATE, "batch_versions: no step from segments yet (fi_learner_step_segments_dev, "
                                  "fi_learner_step_rollouts)");
    FI_HIP_CHECK(hipSetDevice(l->dev));
    FI_HIP_CHECK(hipStreamSynchronize(l->stream));
    uint32_t h[4];
    FI_HIP_CHECK(hipMemcpy(h, l->versions, sizeof(h), hipMemcpyDeviceToHost));
    out->min_version = h[0];
    out->max_version = h[1];
    out->sum_versions = (uint64_t)h[2] | ((uint64_t)h[3] << 32);
    out->count = (uint64_t)l->T * (uint64_t)l->B;
    return FI_OK;
}

// what fi_learner_step_rollout (actor.hip: it needs both handles) compares with the actor
int fi::learner_info(const fi_learner* l, LearnerInfo* out) {
    FI_REQUIRE(l && out, "learner_info: null argument");
    *out = LearnerInfo{l->dev, l->cfg.arch, l->B, l->A, l->D, l->T, dev_entries_ok(l), l->col_w_on};
    return FI_OK;
}

// ------------------------------------------------------------------ per-column loss weights (fi_weights.h)
// The C entry points are weights.hip's: it hands its launcher in, as gather.hip and ring.hip hand in
// their ingests, so a library of the learner alone still links.
int fi::learner_set_column_weights(fi_learner* l, const float* w_host, int32_t n, ScaleFn scale) {
    FI_REQUIRE(l && w_host && scale, "set_column_weights: null argument");
    FI_REQUIRE(n == l->B, "set_column_weights: n = " + std::to_string(n) + " != the learner's batch " + std::to_string(l->B));
    for (int32_t i = 0; i < n; ++i)
        FI_REQUIRE(std::isfinite(w_host[i]) && w_host[i] >= 0.f, "set_column_weights: weight " + std::to_string(w_host[i]) +
                                                                     " at index " + std::to_string(i) +
                                                                     " is negative or not finite");
    FI_HIP_CHECK(hipSetDevice(l->dev));
    if (!l->col_w) FI_TRY(dalloc_n(l, &l->col_w, (size_t)l->B));
    // behind every step enqueued so far, which may still read the old weights
    FI_HIP_CHECK(hipMemcpyAsync(l->col_w, w_host, 4 * (size_t)n, hipMemcpyHostToDevice, l->stream));
    FI_HIP_CHECK(hipStreamSynchronize(l->stream));
    l->col_scale = scale;
    l->col_w_on = true;
    return FI_OK;
}

int fi::learner_clear_column_weights(fi_learner* l) {
    FI_REQUIRE(l, "clear_column_weights: null learner");
    l->col_w_on = false;
    return FI_OK;
}

int fi::learner_column_weights(fi_learner* l, float* dst, int32_t n) {
    FI_REQUIRE(l && dst, "column_weights: null argument");
    FI_REQUIRE(n == l->B, "column_weights: n = " + std::to_string(n) + " != the learner's batch " + std::to_string(l->B));
    if (!l->col_w_on) {
        for (int32_t i = 0; i < n; ++i) dst[i] = 1.f;
        return FI_OK;
    }
    FI_HIP_CHECK(hipSetDevice(l->dev));
    FI_HIP_CHECK(hipMemcpyAsync(dst, l->col_w, 4 * (size_t)n, hipMemcpyDeviceToHost, l->stream));
    FI_HIP_CHECK(hipStreamSynchronize(l->stream));
    return FI_OK;
}

// ------------------------------------------------------------------ the training recipe (fi_train.h)
static int check_rmsprop(const char* who, float decay, float momentum, float eps) {
    const std::string w = who;
    FI_REQUIRE(decay >= 0.f && decay < 1.f, w + ": decay " + std::to_string(decay) + " outside [0, 1)");
    FI_REQUIRE(momentum >= 0.f && momentum < 1.f, w + ": momentum " + std::to_string(momentum) + " outside [0, 1)");
    FI_REQUIRE(std::isfinite(eps) && eps > 0.f, w + ": eps " + std::to_string(eps) + " is not positive and finite");
    return FI_OK;
}

extern "C" int fi_train_set_rmsprop(fi_learner* l, float decay, float momentum, float eps, int eps_in_sqrt) {
    FI_REQUIRE(l, "train_set_rmsprop: null learner");
    FI_TRY(check_rmsprop("train_set_rmsprop", decay, momentum, eps));
    if (l->step_count != 0 || l->in_flight)
        return fail(FI_ERR_STATE, "train_set_rmsprop: an update has been enqueued (step_count " +
                                      std::to_string(l->step_count) + (l->in_flight ? ", a step in flight" : "") +
                                      "): choose the optimiser before the first step");
    l->rms = RmsPropHp{decay, momentum, eps, eps_in_sqrt != 0};
    l->opt_kind = FI_TRAIN_OPT_RMSPROP;
    return FI_OK;
}

extern "C" int fi_train_set_lr(fi_learner* l, float lr) {
    FI_REQUIRE(l, "train_set_lr: null learner");
    FI_REQUIRE(std::isfinite(lr) && lr >= 0.f, "train_set_lr: lr " + std::to_string(lr) + " is negative or not finite");
    l->lr_base = lr;
    return FI_OK;
}

extern "C" int fi_train_set_lr_schedule(fi_learner* l, float lr_end, uint64_t n_steps) {
    FI_REQUIRE(l, "train_set_lr_schedule: null learner");
    FI_REQUIRE(std::isfinite(lr_end) && lr_end >= 0.f,
               "train_set_lr_schedule: lr_end " + std::to_string(lr_end) + " is negative or not finite");
    FI_REQUIRE(n_steps >= 1, "train_set_lr_schedule: n_steps 0 (at least 1)");
    l->lr_end = lr_end;
    l->lr_steps = n_steps;
    l->lr_sched = true;
    return FI_OK;
}

extern "C" int fi_train_clear_lr_schedule(fi_learner* l) {
    FI_REQUIRE(l, "train_clear_lr_schedule: null learner");
    l->lr_sched = false;
    return FI_OK;
}

extern "C" int fi_train_set_reward_clip(fi_learner* l, float c) {
    FI_REQUIRE(l, "train_set_reward_clip: null learner");
    FI_REQUIRE(std::isfinite(c) && c >= 0.f, "train_set_reward_clip: c " + std::to_string(c) +
                                                 " is negative or not finite (0 turns the clip off)");
    l->reward_clip = c;
    return FI_OK;
}

extern "C" int fi_train_get_state(fi_learner* l, fi_train_state* out) {
    FI_REQUIRE(l && out, "train_get_state: null argument");
    std::memset(out, 0, sizeof(*out));
    out->optimizer = (uint32_t)l->opt_kind;
    out->eps_in_sqrt = l->rms.eps_in_sqrt ? 1u : 0u;
    out->decay = l->rms.decay;
    out->momentum = l->rms.momentum;
    out->eps = l->rms.eps;
    out->lr_base = l->lr_base;
    out->lr_end = l->lr_end;
    out->next_update = (uint64_t)l->step_count + 1;
    out->lr_next = lr_of(l, out->next_update);
    out->reward_clip = l->reward_clip;
    out->schedule_on = l->lr_sched ? 1u : 0u;
    out->lr_steps = l->lr_steps;
    return FI_OK;
}

extern "C" int fi_train_rmsprop_update(float* p, const float* g, float* v, float* m, size_t n, float lr, float decay,
                                       float momentum, float eps, int eps_in_sqrt, const double* sqnorm_dev,
                                       float max_norm, int* skip_dev, void* stream) {
    FI_REQUIRE(p && g && v && n >= 1, "train_rmsprop_update: null argument or n = 0");
    FI_TRY(check_rmsprop("train_rmsprop_update", decay, momentum, eps));
    FI_REQUIRE(m || momentum == 0.f, "train_rmsprop_update: momentum " + std::to_string(momentum) + " needs m");
    FI_REQUIRE(std::isfinite(lr) && lr >= 0.f, "train_rmsprop_update: lr " + std::to_string(lr) + " is negative or not finite");
    FI_REQUIRE(sqnorm_dev || !(max_norm > 0.f), "train_rmsprop_update: max_norm " + std::to_string(max_norm) + " needs sqnorm_dev");
    FI_REQUIRE(((uintptr_t)p | (uintptr_t)g | (uintptr_t)v | (uintptr_t)m) % 4 == 0, "train_rmsprop_update: pointers must be 4-byte aligned");
    return rmsprop_step(p, g, v, m, n, lr, RmsPropHp{decay, momentum, eps, eps_in_sqrt != 0}, sqnorm_dev, max_norm,
                        (hipStream_t)stream, skip_dev);
}

extern "C" int fi_train_clip_rewards(float* r, size_t n, float c, void* stream) {
    FI_REQUIRE(r && n >= 1 && (uintptr_t)r % 4 == 0, "train_clip_rewards: null or misaligned r, or n = 0");
    FI_REQUIRE(std::isfinite(c) && c > 0.f, "train_clip_rewards: c " + std::to_string(c) + " is not positive and finite");
    return clip_rewards_launch(r, n, c, (hipStream_t)stream);
}

extern "C" int fi_learner_synth_batch(fi_learner* l, uint64_t seed, int32_t b_global,
                                      int32_t b_offset) {
    FI_REQUIRE(l, "synth: null learner");
    if (b_global <= 0) b_global = l->B;
    FI_REQUIRE(b_offset >= 0 && b_offset + l->B <= b_global, "synth: shard outside global batch");
    FI_HIP_CHECK(hipSetDevice(l->dev));
    FI_TRY(synth_launch(seed, l->T, l->B, b_global, b_offset, l->A, l->D, l->cfg.gamma, l->obs, l->mu,
                        l->act, l->rew, l->disc, l->frames, l->stream));
    FI_HIP_CHECK(hipStreamSynchronize(l->stream));
    return FI_OK;
}

// what publish.hip (fi_publish.h) reads of a learner; the block itself is publish.hip's
int fi::learner_publish_view(fi_learner* l, PublishView* out) {
    FI_REQUIRE(l && out, "learner_publish_view: null argument");
    *out = PublishView{l->dev,    l->cfg.arch, l->A,      l->D,       l->H, l->cfg.publish_dtype, l->nparams,
                       l->params, l->bad + 2,  l->stream, l->version, l->publish.load(std::memory_order_acquire)};
    return FI_OK;
}

void* fi::learner_publish_block(const fi_learner* l) { return l ? l->publish.load(std::memory_order_acquire) : nullptr; }

void fi::learner_set_publish_block(fi_learner* l, void* block, void (*free_fn)(void*)) {
    l->publish_free = free_fn;
    l->publish.store(block, std::memory_order_release);
}

// what diag.hip (fi_diag.h) reads of a learner: the tensors of the most recently enqueued step, the
// thresholds and the stream; the block itself is diag.hip's
int fi::learner_diag_view(fi_learner* l, DiagView* out) {
    FI_REQUIRE(l && out, "learner_diag_view: null argument");
    *out = DiagView{l->dev, l->T,  l->B,      l->A,  l->logits, l->mu,     l->act,     l->rew,
                    l->disc, l->values, l->vs, l->cfg.hp, l->stream, l->stepped, l->diag};
    return FI_OK;
}

void fi::learner_set_diag_block(fi_learner* l, void* block, void (*free_fn)(void*)) {
    l->diag_free = free_fn;
    l->diag = block;
}

// what popart.hip (fi_popart.h) reads of a learner; the block itself is popart.hip's
int fi::learner_popart_view(fi_learner* l, PopartView* out) {
    FI_REQUIRE(l && out, "learner_popart_view: null argument");
    *out = PopartView{l->dev, l->TB, l->comm ? l->nranks : 1, l->stream, l->popart};
    return FI_OK;
}

void fi::learner_set_popart_block(fi_learner* l, PopartBlock* block, void (*free_fn)(void*)) {
    l->popart_free = free_fn;
    l->popart = block;
}

// what surrogate.hip (fi_surrogate.h) reads of a learner; the block itself is surrogate.hip's
int fi::learner_surrogate_view(fi_learner* l, SurrogateView* out) {
    FI_REQUIRE(l && out, "learner_surrogate_view: null argument");
    *out = SurrogateView{l->dev, l->T, l->B, l->A, l->comm ? l->nranks : 1, l->stream, l->surrogate};
    return FI_OK;
}

void fi::learner_set_surrogate_block(fi_learner* l, SurrogateBlock* block, void (*free_fn)(void*)) {
    l->surrogate_free = free_fn;
    l->surrogate = block;
}

// what target.hip (fi_target.h) reads of a learner; the block itself is target.hip's
int fi::learner_target_view(fi_learner* l, TargetView* out) {
    FI_REQUIRE(l && out, "learner_target_view: null argument");
    *out = TargetView{l->dev, l->T, l->B, l->A, l->comm ? l->nranks : 1, l->nparams, l->params, l->stream, l->target};
    return FI_OK;
}

void fi::learner_set_target_block(fi_learner* l, TargetBlock* block, void (*free_fn)(void*)) {
    l->target_free = free_fn;
    l->target = block;
}

// what kl.hip (fi_kl.h) reads of a learner; the block itself is kl.hip's
int fi::learner_kl_view(fi_learner* l, KlView* out) {
    FI_REQUIRE(l && out, "learner_kl_view: null argument");
    *out = KlView{l->dev, l->T, l->B, l->A, l->comm ? l->nranks : 1, l->target != nullptr, l->stream, l->kl};
    return FI_OK;
}

void fi::learner_set_kl_block(fi_learner* l, KlBlock* block, void (*free_fn)(void*)) {
    l->kl_free = free_fn;
    l->kl = block;
}

// ------------------------------------------------------------------ params
extern "C" int fi_learner_get_params_fp32(fi_learner* l, float* dst, size_t count) {
    FI_REQUIRE(l && dst && count == l->nparams, "get_params_fp32: bad arguments");
    FI_HIP_CHECK(hipSetDevice(l->dev));
    FI_HIP_CHECK(hipMemcpyAsync(dst, l->params, count * sizeof(float), hipMemcpyDeviceToHost,
                                l->stream));
    FI_HIP_CHECK(hipStreamSynchronize(l->stream));
    return FI_OK;
}

static uint16_t f2bf(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)((u >> 16) | ((u & 0xffff) ? 0x40 : 0));
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

extern "C" int fi_learner_get_params(fi_learner* l, void* dst, size_t bytes, uint64_t* version) {
    FI_REQUIRE(l && dst, "get_params: null argument");
    FI_REQUIRE(bytes == fi_learner_param_bytes(l), "get_params: bytes != fi_learner_param_bytes");
    if (l->cfg.publish_dtype == FI_PUBLISH_FP32) {
        FI_TRY(fi_learner_get_params_fp32(l, (float*)dst, l->nparams));
    } else {
        std::vector<float> tmp(l->nparams);
        FI_TRY(fi_learner_get_params_fp32(l, tmp.data(), l->nparams));
        uint16_t* o = (uint16_t*)dst;
        for (size_t i = 0; i < l->nparams; ++i) o[i] = f2bf(tmp[i]);
    }
    if (version) {
        // updates skipped by steps not yet checked (asynchronous submission, reported by the
        // next fi_learner_wait) are not counted, so the published version never goes back
        int pending = 0;
        FI_HIP_CHECK(hipMemcpy(&pending, l->bad + 2, sizeof(int), hipMemcpyDeviceToHost));
        *version = l->version - (uint64_t)pending;
    }
    return FI_OK;
}

extern "C" int fi_learner_set_params(fi_learner* l, const void* src, size_t bytes,
                                     uint64_t version) {
    FI_REQUIRE(l && src, "set_params: null argument");
    FI_HIP_CHECK(hipSetDevice(l->dev));
    std::vector<float> tmp;
    const float* p;
    if (bytes == l->nparams * 4) {
        p = (const float*)src;
    } else if (bytes == l->nparams * 2) {
        tmp.resize(l->nparams);
        const uint16_t* s = (const uint16_t*)src;
        for (size_t i = 0; i < l->nparams; ++i) {
            uint32_t u = (uint32_t)s[i] << 16;
            std::memcpy(&tmp[i], &u, 4);
        }
        p = tmp.data();
    } else {
        return fail(FI_ERR_INVALID, "set_params: size is neither fp32 nor bf16 blob");
    }
    FI_HIP_CHECK(hipMemcpyAsync(l->params, p, l->nparams * 4, hipMemcpyHostToDevice, l->stream));
    if (l->atari) FI_TRY(atari_sync_weights(l->atari, l->params, l->stream));
    FI_HIP_CHECK(hipMemsetAsync(l->bad + 2, 0, 2 * sizeof(int), l->stream));  // a new version line
    FI_HIP_CHECK(hipStreamSynchronize(l->stream));
    l->version = version;
    return FI_OK;
}

// ------------------------------------------------------------------ checkpoint / resume
// State blob: header {magic, abi, arch, nparams, step_count, version} then fp32 params, Adam
// m, Adam v (little endian). Together with the published Model blob this lets a restarted
// learner continue bit-identically.
namespace {
struct StateHeader {
    uint32_t magic, abi;
    int32_t arch, step_count;
    uint64_t nparams, version;
};
constexpr uint32_t kStateMagic = 0x46495354u;  // "FIST"
}  // namespace

extern "C" size_t fi_learner_state_bytes(const fi_learner* l) {
    return l ? sizeof(StateHeader) + 3 * l->nparams * sizeof(float) : 0;
}

extern "C" int fi_learner_save_state(fi_learner* l, void* dst, size_t bytes) {
    FI_REQUIRE(l && dst, "save_state: null argument");
    FI_REQUIRE(bytes == fi_learner_state_bytes(l), "save_state: bytes != fi_learner_state_bytes");
    FI_HIP_CHECK(hipSetDevice(l->dev));
    StateHeader h{kStateMagic, FI_ABI_VERSION, l->cfg.arch, l->step_count, l->nparams, l->version};
    char* o = (char*)dst;
    std::memcpy(o, &h, sizeof(h));
    float* f = (float*)(o + sizeof(h));
    FI_HIP_CHECK(hipMemcpyAsync(f, l->params, l->nparams * 4, hipMemcpyDeviceToHost, l->stream));
    FI_HIP_CHECK(hipMemcpyAsync(f + l->nparams, l->opt_m, l->nparams * 4, hipMemcpyDeviceToHost, l->stream));
    FI_HIP_CHECK(hipMemcpyAsync(f + 2 * l->nparams, l->opt_v, l->nparams * 4, hipMemcpyDeviceToHost, l->stream));
    FI_HIP_CHECK(hipStreamSynchronize(l->stream));
    return FI_OK;
}

extern "C" int fi_learner_load_state(fi_learner* l, const void* src, size_t bytes) {
    FI_REQUIRE(l && src, "load_state: null argument");
    FI_REQUIRE(bytes == fi_learner_state_bytes(l), "load_state: bytes != fi_learner_state_bytes");
    StateHeader h;
    std::memcpy(&h, src, sizeof(h));
    FI_REQUIRE(h.magic == kStateMagic && h.abi == FI_ABI_VERSION, "load_state: not a learner state blob");
    FI_REQUIRE(h.arch == l->cfg.arch && h.nparams == l->nparams, "load_state: state of a different network");
    FI_HIP_CHECK(hipSetDevice(l->dev));
    const float* f = (const float*)((const char*)src + sizeof(h));
    FI_HIP_CHECK(hipMemcpyAsync(l->params, f, l->nparams * 4, hipMemcpyHostToDevice, l->stream));
    FI_HIP_CHECK(hipMemcpyAsync(l->opt_m, f + l->nparams, l->nparams * 4, hipMemcpyHostToDevice, l->stream));
    FI_HIP_CHECK(hipMemcpyAsync(l->opt_v, f + 2 * l->nparams, l->nparams * 4, hipMemcpyHostToDevice, l->stream));
    if (l->atari) FI_TRY(atari_sync_weights(l->atari, l->params, l->stream));
    FI_HIP_CHECK(hipMemsetAsync(l->bad + 2, 0, 2 * sizeof(int), l->stream));
    FI_HIP_CHECK(hipStreamSynchronize(l->stream));
    l->step_count = h.step_count;
    l->version = h.version;
    return FI_OK;
}

// ------------------------------------------------------------------ data parallel
static int ensure_comm_stream(fi_learner* l) {
    if (!l->comm_stream) FI_HIP_CHECK(hipStreamCreateWithFlags(&l->comm_stream, hipStreamNonBlocking));
    if (!l->comm_done) FI_HIP_CHECK(hipEventCreateWithFlags(&l->comm_done, hipEventDisableTiming));
    if (!l->bad_ready) FI_HIP_CHECK(hipEventCreateWithFlags(&l->bad_ready, hipEventDisableTiming));
    return FI_OK;
}

extern "C" int fi_comm_unique_id_bytes(void) { return (int)sizeof(ncclUniqueId); }

extern "C" int fi_comm_get_unique_id(void* dst, size_t bytes) {
    FI_REQUIRE(dst && bytes >= sizeof(ncclUniqueId), "comm_get_unique_id: buffer too small");
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(FI_ERR_COMM, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
    std::memcpy(dst, &id, sizeof(id));
    return FI_OK;
}

extern "C" int fi_learner_attach_comm(fi_learner* l, const void* uid, size_t bytes, int rank,
                                      int nranks) {
    FI_REQUIRE(l && uid && bytes >= sizeof(ncclUniqueId), "attach_comm: bad arguments");
    FI_REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, "attach_comm: bad rank");
    FI_HIP_CHECK(hipSetDevice(l->dev));
    if (l->comm) {
        ncclCommDestroy(l->comm);
        l->comm = nullptr;
    }
    // one rank: no communicator (the sum over one rank is the identity), unless FI_COMM_SINGLE
    // asks for one -- the tests use it to run the in-step all-reduce path on a single GPU
    if (nranks == 1 && !std::getenv("FI_COMM_SINGLE")) return FI_OK;
    ncclUniqueId id;
    std::memcpy(&id, uid, sizeof(id));
    FI_TRY(ensure_comm_stream(l));
    ncclResult_t r = ncclCommInitRank(&l->comm, nranks, id, rank);
    if (r != ncclSuccess) return fail(FI_ERR_COMM, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    l->rank = rank;
    l->nranks = nranks;
    return FI_OK;
}

// One process driving several devices (one handle per device, e.g. the threaded
// cmd/freeimpala with --devices 0,1,...): the per-device ncclCommInitRank calls are one group,
// so a single thread can attach them all (called one by one, the first would block waiting
// for its peers). Handle i becomes rank i of n.
extern "C" int fi_comm_init_all(fi_learner* const* handles, int n) {
    FI_REQUIRE(handles && n >= 1, "comm_init_all: bad arguments");
    for (int i = 0; i < n; ++i) {
        FI_REQUIRE(handles[i], "comm_init_all: null handle");
        for (int j = 0; j < i; ++j)
            FI_REQUIRE(handles[j]->dev != handles[i]->dev, "comm_init_all: two handles on one device");
    }
    if (n == 1 && !std::getenv("FI_COMM_SINGLE")) return FI_OK;
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(FI_ERR_COMM, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
    for (int i = 0; i < n; ++i) {
        fi_learner* l = handles[i];
        FI_HIP_CHECK(hipSetDevice(l->dev));
        if (l->comm) {
            ncclCommDestroy(l->comm);
            l->comm = nullptr;
        }
        FI_TRY(ensure_comm_stream(l));
    }
    r = ncclGroupStart();
    if (r != ncclSuccess) return fail(FI_ERR_COMM, std::string("ncclGroupStart: ") + ncclGetErrorString(r));
    for (int i = 0; i < n; ++i) {
        FI_HIP_CHECK(hipSetDevice(handles[i]->dev));
        r = ncclCommInitRank(&handles[i]->comm, n, id, i);
        if (r != ncclSuccess) {
            ncclGroupEnd();
            return fail(FI_ERR_COMM, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
        }
    }
    r = ncclGroupEnd();
    if (r != ncclSuccess) return fail(FI_ERR_COMM, std::string("ncclGroupEnd: ") + ncclGetErrorString(r));
    for (int i = 0; i < n; ++i) {
        handles[i]->rank = i;
        handles[i]->nranks = n;
    }
    return FI_OK;
}

// what RCCL reports for the handle's communicator (1 / 0 / 0 without one)
extern "C" int fi_learner_comm_info(fi_learner* l, int* nranks, int* rank, int* buckets) {
    FI_REQUIRE(l, "comm_info: null learner");
    int n = 1, r = 0;
    if (l->comm) {
        ncclResult_t e = ncclCommCount(l->comm, &n);
        if (e == ncclSuccess) e = ncclCommUserRank(l->comm, &r);
        if (e != ncclSuccess) return fail(FI_ERR_COMM, std::string("ncclCommCount: ") + ncclGetErrorString(e));
    }
    if (nranks) *nranks = n;
    if (rank) *rank = r;
    if (buckets) *buckets = l->comm ? l->buckets : 0;
    return FI_OK;
}

// ------------------------------------------------------------------ introspection
extern "C" int fi_learner_read_tensor(fi_learner* l, const char* name, void* dst, size_t bytes) {
    FI_REQUIRE(l && name && dst, "read_tensor: null argument");
    void* p = nullptr;
    size_t have = 0;
    FI_TRY(fi_learner_tensor(l, name, &p, &have));
    FI_REQUIRE(bytes <= have, std::string("read_tensor: ") + name + " holds " + std::to_string(have) + " bytes");
    FI_HIP_CHECK(hipSetDevice(l->dev));
    FI_HIP_CHECK(hipStreamSynchronize(l->stream));
    FI_HIP_CHECK(hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost));
    return FI_OK;
}

extern "C" int fi_learner_tensor(fi_learner* l, const char* name, void** ptr, size_t* bytes) {
    FI_REQUIRE(l && name && ptr && bytes, "tensor: null argument");
    const size_t rows = l->rows, TB = l->TB, A = l->A;
    struct E {
        const char* n;
        void* p;
        size_t b;
    };
    std::vector<E> t = {
        {"params", l->params, l->nparams * 4},  {"grads", l->grads, l->nparams * 4},
        {"adam_m", l->opt_m, l->nparams * 4},   {"adam_v", l->opt_v, l->nparams * 4},
        {"obs", l->obs, l->obs ? rows * l->D * 4 : 0},
        {"frames", l->frames, l->frames ? rows * AtariNet::kFrameBytes : 0},
        {"mu", l->mu, TB * A * 4},               {"actions", l->act, TB * 4},
        {"rewards", l->rew, TB * 4},             {"discounts", l->disc, TB * 4},
        {"logits", l->logits, rows * A * 4},     {"values", l->values, rows * 4},
        {"vs", l->vs, TB * 4},                   {"pg_adv", l->pg_adv, TB * 4},
        {"dlogits", l->dlogits, TB * A * 4},     {"dvalue", l->dvalue, rows * 4},
        {"losses", l->small, 3 * 8},             {"h1", l->h1, l->h1 ? rows * l->H * 4 : 0},
        {"h2", l->h2, l->h2 ? rows * l->H * 4 : 0},
    };
    for (auto& e : t)
        if (std::strcmp(e.n, name) == 0) {
            *ptr = e.p;
            *bytes = e.b;
            return e.p ? FI_OK : fail(FI_ERR_INVALID, std::string("tensor: not present: ") + name);
        }
    if (l->atari) {
        void* p = nullptr;
        size_t b = 0;
        if (atari_tensor(l->atari, name, &p, &b)) {
            *ptr = p;
            *bytes = b;
            return FI_OK;
        }
    }
    return fail(FI_ERR_INVALID, std::string("tensor: unknown name: ") + name);
}

extern "C" int fi_learner_set_profiling(fi_learner* l, int on) {
    FI_REQUIRE(l, "set_profiling: null");
    l->profiling = on != 0;
    for (double& s : l->phase_sum) s = 0.0;
    l->phase_steps = 0;
    l->tag_sum.clear();
    l->tag_used = 0;
    return FI_OK;
}

extern "C" int fi_learner_phase_times(fi_learner* l, float* ms, int n, int* n_steps) {
    FI_REQUIRE(l && ms && n >= 1, "phase_times: bad arguments");
    for (int p = 0; p < n && p < FI_PHASE_COUNT; ++p)
        ms[p] = l->phase_steps ? (float)(l->phase_sum[p] / l->phase_steps) : 0.f;
    if (n_steps) *n_steps = l->phase_steps;
    return FI_OK;
}

// Mean device ms per launch of every tagged kernel site seen while profiling.
// names: '\n'-separated, written into names_buf; returns the number of entries (<= max).
extern "C" int fi_learner_kernel_times(fi_learner* l, char* names_buf, size_t buflen, float* ms,
                                       int* counts, int max) {
    FI_REQUIRE(l && names_buf && buflen > 0 && ms && counts && max >= 1, "kernel_times: args");
    std::string all;
    int n = 0;
    for (auto& e : l->tag_sum) {
        if (n >= max) break;
        ms[n] = (float)(e.second.first / std::max(1, e.second.second));
        counts[n] = e.second.second;
        all += e.first;
        all += '\n';
        ++n;
    }
    std::strncpy(names_buf, all.c_str(), buflen - 1);
    names_buf[buflen - 1] = 0;
    return n;
}
