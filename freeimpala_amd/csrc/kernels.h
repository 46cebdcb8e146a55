// kernels.h -- internal launchers of libfi_learner.so (not part of the C ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "fi_diag.h"
#include "fi_gather.h"
#include "fi_kl.h"
#include "fi_learner.h"
#include "fi_surrogate.h"

namespace fi {

// the heads' upstream gradient: virtual [rows][A+1] = dlogits (TB rows, then 0) | dvalue
struct HeadsGrad {
    const float* dlog;  // (TB, A)
    const float* dval;  // (rows)
    int rows;           // (T+1)*B
    int TB;             // T*B
    int A;
};

// vtrace.hip
size_t vtrace_workspace_bytes(int T, int B, int A);
int vtrace_launch(int variant, int T, int B, int A, const float* pi, const float* mu,
                  const int32_t* act, const float* rew, const float* disc, const float* val,
                  const fi_vtrace_hparams& hp, float* vs, float* adv, float* dlog, float* dval,
                  double* losses, void* ws, size_t ws_bytes, hipStream_t stream,
                  bool finalize = true, int* nblk_out = nullptr, int* bad = nullptr);
// bad: device counter of out-of-range actions (nullptr: a counter inside ws, zeroed here; with
// finalize the loss scalars become NaN when it is non-zero)
int vtrace_finalize_launch(void* ws, int nblk, double* losses, hipStream_t stream,
                           const int* bad = nullptr);
// per-workgroup loss partials [nblk][3] inside a vtrace workspace
const double* vtrace_partials(const void* ws);

// gemm_f32.hip (MLP, exact fp32)
int f32_linear_fwd(const float* X, int M, int K, const float* W, const float* bias, int N,
                   bool relu, float* Y, hipStream_t s);
int f32_heads_fwd(const float* X, int M, int K, const float* W, const float* bias, int A,
                  float* logits, float* values, hipStream_t s);
int f32_linear_dgrad(const float* dY, int M, int N, const float* W, int K, const float* act,
                     float* dX, hipStream_t s);
int f32_heads_dgrad(const HeadsGrad& g, const float* W, int K, const float* act, float* dX,
                    hipStream_t s);
int f32_linear_wgrad_partial(const float* X, int M, int I, const float* dY, int N, int splits,
                             float* slab, float* cs_slab, hipStream_t s);
int f32_heads_wgrad_partial(const float* X, int I, const HeadsGrad& g, int splits, float* slab,
                            float* cs_slab, hipStream_t s);
// heads weight gradient (slab [grid][H][A+1] + bias partials [grid][A+1]) and masked data
// gradient dz2 in one pass over h2 (H = 256, A = 18)
bool f32_heads_bwd_fused_supported(int H, int A);
constexpr int kHeadsFusedGrid = 512;
int f32_heads_bwd_fused(const HeadsGrad& g, const float* h2, const float* Wh, int H, float* dz2, float* slab,
                        float* cs_slab, int grid, hipStream_t s);

// weights.hip: dlog (T, B, A) and the first T rows of dval times w[b] in place (include/fi_weights.h).
// learner.cpp takes it as a pointer, as it takes the ingests below
int scale_columns_launch(float* dlog, float* dval, const float* w, int T, int B, int A, hipStream_t s);
typedef int (*ScaleFn)(float* dlog, float* dval, const float* w, int T, int B, int A, hipStream_t s);

// misc.hip
int colsum_partial(const float* Y, int M, int N, int splits, float* slab, hipStream_t s);
int heads_colsum_partial(const HeadsGrad& g, int splits, float* slab, hipStream_t s);
// PyTorch-layout (W[N][K]) fp32 GEMMs on the same MFMA kernel (farmer.hip)
int f32_gemm_nt(const float* X, int ldx, int M, int K, const float* W, const float* bias, int N,
                bool relu, float* Y, hipStream_t s);
int f32_gemm_nn_dgrad(const float* dY, int M, int N, const float* W, int K, const float* act, float* dX,
                      hipStream_t s);
int f32_gemm_tn_wgrad(const float* dY, int M, int N, const float* X, int ldx, int K, int splits, float* slab,
                      hipStream_t s);
// fc_gemm.hip (the Atari fc layer, 3136 -> 512, rows = (T+1)*B)
int fc_fwd_launch(const __bf16* a3, const __bf16* wT, const float* bias, __bf16* h, int rows, hipStream_t s);
// da3 unmasked; ring: the LDS-ring kernel that stages both operands (the A/B baseline) instead of
// the default with W in registers -- bit-identical results
int fc_dgrad_launch(const __bf16* dh, const __bf16* w, __bf16* da3, int rows, hipStream_t s, bool ring = false);
int fc_wgrad_splits(int rows);  // R-slices (fp32 slabs of 3136 x 512) fc_wgrad_launch uses
int fc_wgrad_launch(const __bf16* a3, const __bf16* dh, float* slab, float* dw, int rows, hipStream_t s);
int reduce_slabs(float* slab, int splits, size_t count, float* out, hipStream_t s);  // slab is scratch (overwritten)
// squared L2 norm of g -> *out; optionally also sums vt_nblk V-trace loss partials [i][3]
// into vt_losses[0..2] in the same (final) launch; *nonfinite = 1 when the norm is NaN / Inf
int grad_sqnorm(const float* g, size_t n, double* part, int nblk, double* out, hipStream_t s,
                const double* vt_part = nullptr, int vt_nblk = 0, double* vt_losses = nullptr,
                int* nonfinite = nullptr);
// RMSProp's hyper-parameters (include/fi_train.h): opt == FI_TRAIN_OPT_RMSPROP takes them from rms
struct RmsPropHp {
    float decay, momentum, eps;
    bool eps_in_sqrt;
};
int optimizer_step(int opt, float* p, const float* g, float* m, float* v, size_t n, float lr,
                   float b1, float b2, float eps, double bc1, double bc2, const double* sqnorm,
                   float max_norm, hipStream_t s, int* skip = nullptr,  // skip: int[4], see misc.hip
                   const RmsPropHp* rms = nullptr);
// one RMSProp update: the mean square in v, the momentum buffer in m (not touched, and nullable,
// when hp.momentum == 0); 16 bytes per lane when every pointer is 16-byte aligned
int rmsprop_step(float* p, const float* g, float* v, float* m, size_t n, float lr, const RmsPropHp& hp,
                 const double* sqnorm, float max_norm, hipStream_t s, int* skip = nullptr);
// r[i] clamped to [-c, c] in place, NaN kept
int clip_rewards_launch(float* r, size_t n, float c, hipStream_t s);
int to_bf16(const float* src, uint16_t* dst, size_t n, hipStream_t s);
int fill_hash_bf16(void* dst, size_t n, uint32_t seed, hipStream_t s);
int synth_launch(uint64_t seed, int T, int B, int B_glob, int b_off, int A, int D, float gamma,
                 float* obs, float* mu, int32_t* act, float* rew, float* disc, uint8_t* frames,
                 hipStream_t s);

// The tensors an ingest fills: a learner's batch (learner.cpp) or the outputs a standalone entry
// point names. Unused ones are nullptr.
struct BatchTensors {
    int arch, T, B, A, D;
    float* obs;       // MLP
    uint8_t* frames;  // Atari
    float* mu;
    int32_t* act;
    float* rew;
    float* disc;
    int* bad;            // nullable: actions outside [0, A) are counted here (and stored clamped)
    const void** cols;   // the gathering ingests: B entry addresses
    uint32_t* versions;  // the gathering ingests, nullable: {min u32, max u32, sum u64} of the flags words
    hipStream_t stream;
};

// misc.hip: B entries in one buffer, entry_bytes apart (ingest_kernels.h with the Strided locator;
// record schemas: records.h). MLP records into obs / mu / act / rew / disc
int ingest_launch(const void* rec, size_t entry_bytes, const BatchTensors& to);
// stacked Atari records: frames (T+1, B, 84, 84, 4) u8 plus the same header tensors; entry_bytes
// % 16 == 0, rec and frames 16-byte aligned
int ingest_atari_launch(const void* rec, size_t entry_bytes, const BatchTensors& to);
// Atari plane records, then the 3-plane history block: the same outputs, the 4-frame stack rebuilt
// from single planes and episode_start; A <= 18
int ingest_atari_planes_launch(const void* rec, size_t entry_bytes, const BatchTensors& to);

// gather.hip: the same ingests with column b's entry at to.cols[b], a table of B base addresses in
// device memory (include/fi_gather.h; ingest_kernels.h with the Table locator). The table is built
// on the device from segments that travel as the kernel argument: segment k covers the columns
// [first, first + count), column c at base + (c - first) * stride; the segments continue one
// another from column 0 to B.
struct SegTable {
    struct Seg {
        const char* base;
        size_t stride;
        int32_t first, count;
    } seg[FI_MAX_SEGMENTS];
    int32_t n;
};
// versions (nullable, 16 bytes): set to {min = ~0, max = 0, sum = 0}, what the gathers below fold into
int fill_columns_launch(const SegTable& tab, const void** cols, int B, uint32_t* versions, hipStream_t s);
// to.versions: by integer atomics into the state fill_columns_launch leaves
int gather_records_launch(const BatchTensors& to);
int gather_atari_planes_launch(const BatchTensors& to);
// the gathering launcher for to.arch, behind a kernel that wrote to.cols: what a step from segments
// and a step from a ring (ring.hip) both end their ingest in
int gather_ingest(const BatchTensors& to);

// rollout.hip: one acting step into the learner's entry format (include/fi_rollout.h). logits ==
// nullptr: the plane and episode_start (the observation) only
int record_planes_launch(void* entries, size_t stride, int t, const uint8_t* planes, const uint8_t* start,
                         const float* logits, const int32_t* actions, uint32_t flags, int N, int A, hipStream_t s);
int extract_history_launch(void* entries, size_t stride, size_t hist_off, const uint8_t* stacks, int N, hipStream_t s);
int record_obs_launch(void* entries, size_t stride, int t, const float* obs, int D, const float* logits,
                      const int32_t* actions, uint32_t flags, int N, int A, hipStream_t s);
// out: N rewards then N discounts; field: byte offset of the reward in entry 0 (the record's
// offset plus the reward's in a record, records.h: the discount follows it)
int scatter_outcome_launch(void* entries, size_t stride, size_t field, const float* out, int N, hipStream_t s);
// the same from two arrays of N floats (fi_env.h: the rewards and discounts are in device memory already)
int scatter_outcome_launch(void* entries, size_t stride, size_t field, const float* rewards, const float* discounts,
                           int N, hipStream_t s);

// learner.cpp: what fi_learner_step_rollout (actor.hip: it holds both handles) compares with the
// actor. learner.cpp itself calls nothing of actor.hip, so a library of the learner alone links
struct LearnerInfo {
    int dev, arch, B, A, D, T;
    bool dev_entries_ok;  // MLP, or Atari in the planes format
    bool column_weights;  // fi_learner_set_column_weights holds (fi_weights.h)
};
int learner_info(const fi_learner* l, LearnerInfo* out);

// learner.cpp: a step's batch source, for the C entry points that live outside it. `ingest` fills the
// learner's tensors from what ctx names; gather.hip and ring.hip hand theirs in, so learner.cpp names
// nothing of either and a library of the learner alone links.
typedef int (*IngestFn)(const void* ctx, const BatchTensors& to);
// the step from segments (fi_gather.h): the checks of the segments, then ingest(&SegTable, tensors)
int learner_step_segments(fi_learner* l, const fi_entry_segment* segs, int32_t n_segs, fi_step_stats* out, bool wait,
                          const char* who, IngestFn ingest);
// the step from a source that writes the column table itself (fi_ring.h: ring.hip has checked the
// ring against learner_info()); the learner's stream waits for `ready` (nullable) first. weights
// (nullable): B floats in device memory that the ingest writes, the step's column weights in place
// of the handle's (fi_weights.h: a prioritised step's importance weights), applied by `scale`
int learner_step_columns(fi_learner* l, hipEvent_t ready, IngestFn ingest, const void* ctx, fi_step_stats* out,
                         bool wait, const char* who, const float* weights = nullptr, ScaleFn scale = nullptr);
// learner.cpp: the handle's column weights (fi_weights.h; the C entry points are weights.hip's, which
// hands its launcher in: learner.cpp names nothing of weights.hip)
int learner_set_column_weights(fi_learner* l, const float* w_host, int32_t n, ScaleFn scale);
int learner_clear_column_weights(fi_learner* l);
int learner_column_weights(fi_learner* l, float* dst, int32_t n);

// learner.cpp: what publish.hip (fi_publish.h) reads of a learner, and where its publication block
// hangs. learner.cpp names nothing of publish.hip: the block arrives with its free function, which
// fi_learner_destroy calls behind the wait for the learner's streams.
struct PublishView {
    int dev, arch, A, D, H, dtype;
    size_t nparams;
    const float* params;
    const int* skipped;  // the device word that counts updates skipped since the last check
    hipStream_t stream;
    uint64_t version;  // the count of enqueued updates
    void* block;
};
int learner_publish_view(fi_learner* l, PublishView* out);
// the block alone, an atomic load: the one thing of a learner another handle's thread may read
void* learner_publish_block(const fi_learner* l);
void learner_set_publish_block(fi_learner* l, void* block, void (*free_fn)(void*));

// diag.hip: the off-policy diagnostics (include/fi_diag.h, where the rule stands). Workgroup (c, s)
// of diag_plan()'s grid writes its partial sums into ws; one finalize workgroup adds them in a fixed
// order and writes *out, col_kl and col_log_rho (nullable, B floats each) to device memory
struct DiagPlan {
    int column_tiles, time_slices, slice_len;  // slice s: the time steps [s * slice_len, min(T, (s + 1) * slice_len))
};
int diag_plan(int T, int B, int A, DiagPlan* out);
size_t diag_workspace_bytes(int T, int B, int A);  // 0 for a refused shape
int offpolicy_diag_launch(int T, int B, int A, const float* pi, const float* mu, const int32_t* act, const float* rew,
                          const float* disc, const float* val, const float* vs, const fi_vtrace_hparams& hp,
                          fi_offpolicy_diag* out, float* col_kl, float* col_log_rho, void* ws, size_t ws_bytes,
                          hipStream_t stream);

// learner.cpp: what diag.hip reads of a learner, and where its diagnostics block hangs (as the
// publication block does: learner.cpp names nothing of diag.hip, the block arrives with its free
// function, which fi_learner_destroy calls behind the wait for the learner's streams)
struct DiagView {
    int dev, T, B, A;
    const float* logits;  // (T+1, B, A): the first T * B rows are pi
    const float* mu;
    const int32_t* act;
    const float* rew;
    const float* disc;
    const float* values;  // (T+1, B)
    const float* vs;
    fi_vtrace_hparams hp;
    hipStream_t stream;
    bool stepped;  // a step has been enqueued on the handle
    void* block;
};
int learner_diag_view(fi_learner* l, DiagView* out);
void learner_set_diag_block(fi_learner* l, void* block, void (*free_fn)(void*));

// popart.hip: PopArt value normalisation (include/fi_popart.h, where the rule stands). `state` is the
// 32-byte device block {double mu, nu, sigma; uint64_t updates}; every kernel reads it there
constexpr int kPopartStreamGridMax = 1024;  // workgroups of the two streaming kernels, at most
int popart_plan(size_t n);                  // workgroups of the moments kernel: a fixed function of n
size_t popart_workspace_bytes(size_t n);
int popart_denorm_launch(float* values, size_t n, const void* state, hipStream_t s);
int popart_scale_launch(float* dvalue, size_t n, const void* state, hipStream_t s);
int popart_update_launch(const float* vs, size_t n, void* state, float* w, size_t w_stride, int H, float* b, double beta,
                         double sigma_min, double sigma_max, const int* skip, void* ws, size_t ws_bytes, hipStream_t s);

// learner.cpp: a learner's PopArt block, made and freed by popart.hip, which hands its launchers in
// with it (as weights.hip hands in its ScaleFn): learner.cpp names nothing of popart.hip, so a
// library of the learner alone links. run_step calls the three launchers while the block is there
struct PopartBlock {
    void* state = nullptr;  // device, 32 bytes
    void* ws = nullptr;     // the moments workspace for T * B targets
    size_t ws_bytes = 0;
    double beta = 0.0, sigma_min = 0.0, sigma_max = 0.0;
    int (*denorm)(float*, size_t, const void*, hipStream_t) = nullptr;
    int (*scale)(float*, size_t, const void*, hipStream_t) = nullptr;
    int (*update)(const float*, size_t, void*, float*, size_t, int, float*, double, double, double, const int*, void*,
                  size_t, hipStream_t) = nullptr;
};
struct PopartView {
    int dev, TB, nranks;
    hipStream_t stream;
    PopartBlock* block;
};
int learner_popart_view(fi_learner* l, PopartView* out);
void learner_set_popart_block(fi_learner* l, PopartBlock* block, void (*free_fn)(void*));

// surrogate.hip: the clipped surrogate policy loss on V-trace targets (include/fi_surrogate.h, where the
// rule stands): rows, scan, loss and stats kernels in place of the V-trace launch. losses (nullable):
// 3 doubles, the partials summed by the stats kernel; stats (nullable): the 32-byte block; bad
// (nullable): as vtrace_launch's; tg (nullable): a tag around each launch, named after its kernel;
// *partials, *nblk_out (nullable): the [nblk][3] loss partials inside ws, what grad_sqnorm adds
struct KernelTagger;  // atari.h
size_t surrogate_workspace_bytes(int T, int B, int A);  // 0 for a refused shape
int surrogate_loss_blocks(int T, int B, int A);
int surrogate_check_params(const std::string& who, const fi_surrogate_params* p);  // FI_ERR_INVALID, `who` opens the message
int surrogate_launch(int T, int B, int A, const float* pi, const float* mu, const int32_t* act, const float* rew,
                     const float* disc, const float* val, const fi_vtrace_hparams& hp, const fi_surrogate_params& prm,
                     float* vs, float* adv, float* dlog, float* dval, double* losses, void* stats, void* ws, size_t ws_bytes,
                     int* bad, hipStream_t stream, KernelTagger* tg = nullptr, const double** partials = nullptr,
                     int* nblk_out = nullptr);

// the rows and scan kernels alone, on (some logits, mu): vs and adv are written, and *out names what they
// left in ws (a surrogate workspace) for a loss kernel of another file (target.hip): log rho per row, the
// advantage moments' partials and pivot, the word the bad actions were counted into (bad, or one inside
// ws, zeroed here) and the grid of the rows kernel, which a loss kernel over the same rows takes
struct SurrogateFront {
    const float* lr;      // [T * B]
    const double* mom;    // [nscan][2]
    const double* pivot;  // 1
    int* bad;
    int nscan, ct, slices, slice_len;
};
int surrogate_front_launch(int T, int B, int A, const float* pi, const float* mu, const int32_t* act, const float* rew,
                           const float* disc, const float* val, const fi_vtrace_hparams& hp, float* vs, float* adv, void* ws,
                           size_t ws_bytes, int* bad, hipStream_t stream, KernelTagger* tg, SurrogateFront* out);

// learner.cpp: a learner's surrogate block, made and freed by surrogate.hip, which hands its launcher
// in with it (as popart.hip does): learner.cpp names nothing of surrogate.hip, so a library of the
// learner alone links. While the block is there and `on`, run_step calls `launch` where it launches
// V-trace and hands *partials, *nblk to grad_sqnorm
struct SurrogateBlock {
    void* stats = nullptr;  // device, 32 bytes
    void* ws = nullptr;
    size_t ws_bytes = 0;
    bool on = false;
    float clip = 0.f, adv_eps = 0.f;
    uint32_t normalize = 0;
    int (*launch)(const SurrogateBlock*, int T, int B, int A, const float* pi, const float* mu, const int32_t* act,
                  const float* rew, const float* disc, const float* val, const fi_vtrace_hparams& hp, float* vs, float* adv,
                  float* dlog, float* dval, int* bad, hipStream_t stream, KernelTagger* tg, const double** partials,
                  int* nblk) = nullptr;
};
struct SurrogateView {
    int dev, T, B, A, nranks;
    hipStream_t stream;
    SurrogateBlock* block;
};
int learner_surrogate_view(fi_learner* l, SurrogateView* out);
void learner_set_surrogate_block(fi_learner* l, SurrogateBlock* block, void (*free_fn)(void*));

// learner.cpp: a learner's target-network block (include/fi_target.h, where the rule stands), made and freed
// by target.hip, which hands its launchers in with it: learner.cpp names nothing of target.hip, so a
// library of the learner alone links. While the block is `on`: a step with the surrogate objective on runs
// the target forward into tlogits / tvalues first and calls `launch` where it would call the surrogate's
// launcher; every step whose update number is a multiple of `period` calls `update` behind the optimiser
struct TargetBlock {
    float* theta = nullptr;    // the target parameters, nparams floats
    float* tlogits = nullptr;  // (T + 1, B, A)
    float* tvalues = nullptr;  // (T + 1, B): scratch, not used
    void* stats = nullptr;     // device, 32 bytes: uint64 updates, rows; double mean_log_r, mean_sq_log_r
    void* ws = nullptr;
    size_t ws_bytes = 0, nparams = 0;
    bool on = false;
    uint32_t period = 0;
    float tau = 0.f;
    int (*launch)(const TargetBlock*, const SurrogateBlock*, int T, int B, int A, const float* pi, const float* mu,
                  const int32_t* act, const float* rew, const float* disc, const float* val, const fi_vtrace_hparams& hp,
                  float* vs, float* adv, float* dlog, float* dval, int* bad, hipStream_t stream, KernelTagger* tg,
                  const double** partials, int* nblk) = nullptr;
    int (*update)(const TargetBlock*, const float* params, const int* skip, hipStream_t stream) = nullptr;
};
struct TargetView {
    int dev, T, B, A, nranks;
    size_t nparams;
    const float* params;
    hipStream_t stream;
    TargetBlock* block;
};
int learner_target_view(fi_learner* l, TargetView* out);
void learner_set_target_block(fi_learner* l, TargetBlock* block, void (*free_fn)(void*));

// learner.cpp: a learner's KL-penalty block (include/fi_kl.h, where the rule stands), made and freed by
// kl.hip, which hands its launchers in with it: learner.cpp names nothing of kl.hip, so a library of the
// learner alone links. While the block is `on` and the step has the reference's logits (mu always, tlogits
// after a target forward), run_step calls `penalty` directly behind the objective's launches and `adapt`
// behind the optimiser (and PopArt's and the target's updates)
struct KlBlock {
    void* state = nullptr;  // device, 48 bytes: fi_kl_stats
    void* ws = nullptr;     // one fp64 partial per workgroup of the penalty kernel
    size_t ws_bytes = 0;
    bool on = false;
    fi_kl_params prm{};  // by value into every later launch; prm.coeff: what fi_kl_enable was last given
    int (*penalty)(const KlBlock*, int T, int B, int A, const float* pi, const float* q, float* dlog,
                   hipStream_t stream) = nullptr;
    int (*adapt)(const KlBlock*, int T, int B, int A, const int* skip, hipStream_t stream) = nullptr;
};
struct KlView {
    int dev, T, B, A, nranks;
    bool has_target;  // fi_target_enable was called on the handle
    hipStream_t stream;
    KlBlock* block;
};
int learner_kl_view(fi_learner* l, KlView* out);
void learner_set_kl_block(fi_learner* l, KlBlock* block, void (*free_fn)(void*));

// actor.hip: what fi_ring_push_rollout (ring.hip) compares with the ring, what fi_env_rollout
// (env.hip) enqueues behind, and what fi_actor_set_params_dev (publish.hip) compares with the learner
struct ActorInfo {
    int dev, N;
    int arch;
    bool recording;
    hipStream_t stream;
    int A, D, H;
};
int actor_info(const fi_actor* a, ActorInfo* out);
// (the check of a caller's device pointers, check_dev_span, is host_util.h's)

// Exploration (include/fi_explore.h). explore.hip owns the kernel and the C entry points; an actor
// handle (actor.hip) carries this state and, while `active` in sample mode, calls `launch` where it
// launches the plain sampler and records `mu` in place of the policy's logits. actor.hip names
// nothing of explore.hip -- the launcher arrives with fi_explore_set -- so a library without
// explore.hip links. eps (N floats) and mu (N * A) are device memory made by the first
// fi_explore_set and freed with the handle; eps_host mirrors eps; mu_valid: the last act call ran
// `launch` and mu holds its rows. eps == nullptr in a launch: all 0.
typedef int (*BehaviourLaunchFn)(const float* logits, int N, int A, float tau, const float* eps, uint64_t seed,
                                 uint64_t draw, int32_t* actions, float* mu, int* nonfinite, hipStream_t s);
struct ExploreState {
    bool active = false;
    float tau = 1.f;
    std::vector<float> eps_host;
    float* eps = nullptr;
    float* mu = nullptr;
    bool mu_valid = false;
    BehaviourLaunchFn launch = nullptr;
};
ExploreState* actor_explore_state(fi_actor* a);  // actor.hip; nullptr for a null handle

}  // namespace fi
