/* fi_gather.h -- C ABI of a learner batch gathered from several device buffers (libfi_learner.so).
 *
 * fi_rollout.h steps a learner from one buffer of cfg.batch entries. Here the batch is a list of
 * segments: segment k holds n_k entries in device memory, entry_stride_k apart, and fills the
 * batch columns [c_k, c_k + n_k), c_k = n_0 + .. + n_(k-1); the n_k sum to cfg.batch. Segments may
 * lie in different allocations, have different strides and stand in any order. Several recording
 * actors (fi_rollout.h), each with its own num_envs, stream and parameter version, so feed one
 * learner step. The ingest kernels read every column's entry through a table of column base
 * addresses in device memory (csrc/gather.hip); the tensors they fill, and the step behind them,
 * are those of fi_learner_step_entries_dev. Status codes and fi_last_error() as fi_learner.h; one
 * thread at a time per handle.
 */
#ifndef FI_GATHER_H
#define FI_GATHER_H

#include <stddef.h>
#include <stdint.h>

#include "fi_actor.h"
#include "fi_learner.h"
#include "fi_rollout.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FI_MAX_SEGMENTS 64

typedef struct {
    const void* entries_dev; /* num_entries entries, entry i at entries_dev + i * entry_stride */
    size_t entry_stride;
    int32_t num_entries;
    void* ready_event;       /* hipEvent_t the learner's stream waits for, or NULL */
} fi_entry_segment;

/* The flags words (the parameter version the acting policy held, fi_rollout.h) of the T * B
 * records a step ingested; record T of an entry does not count. */
typedef struct {
    uint32_t min_version, max_version;
    uint64_t sum_versions, count; /* count = T * B */
} fi_batch_versions;

/* ---- the learner steps from segments -------------------------------------------------------- */
/* The learner's stream waits for every non-NULL ready_event, builds the column table, runs the
 * gathering ingest for the handle's record format, records the event
 * fi_learner_entries_consumed_event returns right behind it, and runs the unchanged step. The
 * column table and the version block (8 * batch + 16 bytes of device memory) are allocated on the
 * first call; no host-entry staging is allocated or touched. Returns when the step is done (the
 * _async form once it is enqueued: fi_learner_wait afterwards). FI_ERR_INVALID, naming the segment
 * and the numbers, before anything is enqueued: n_segs outside [1, FI_MAX_SEGMENTS]; a num_entries
 * below 1; num_entries that do not sum to cfg.batch; a segment whose entry_stride is below
 * fi_learner_entry_bytes(), whose stride or pointer is not 16-byte aligned, whose pointer is not
 * device memory of the handle's device or whose allocation ends before its last entry does; an
 * Atari handle in the stacked format.                                                          */
int fi_learner_step_segments_dev(fi_learner* l, const fi_entry_segment* segs, int32_t n_segs, fi_step_stats* out);
int fi_learner_step_segments_dev_async(fi_learner* l, const fi_entry_segment* segs, int32_t n_segs);
/* Waits for the handle's stream and returns the version block of the last step that came through
 * this header. FI_ERR_STATE before the first one.                                              */
int fi_learner_batch_versions(fi_learner* l, fi_batch_versions* out);

/* ---- acquire, step, release over several recording actors ---------------------------------- */
/* Actor k becomes segment k with num_entries = its num_envs. Every actor is checked as
 * fi_learner_step_rollout checks its one before any is acquired: FI_ERR_INVALID (with the actor's
 * index and the numbers) for another device, policy, num_actions, obs_dim or rollout T, for a
 * handle listed twice, and for num_envs that do not sum to the learner's batch; FI_ERR_STATE,
 * naming the index, when an actor has no completed unroll -- every ready unroll then still waits.
 * All unrolls are released with the learner's consumed event when the step returns FI_OK or
 * FI_ERR_NONFINITE; after any other status they all still wait. The _async form releases once the
 * step is enqueued (the event is recorded behind the ingest by then); fi_learner_wait afterwards. */
int fi_learner_step_rollouts(fi_learner* l, fi_actor* const* actors, int32_t n_actors, fi_step_stats* out);
int fi_learner_step_rollouts_async(fi_learner* l, fi_actor* const* actors, int32_t n_actors);

/* ---- standalone kernels on device pointers (stream: hipStream_t or NULL) ------------------- */
/* fi_ingest_atari_planes / fi_ingest_records (fi_learner.h) with column b's entry at cols_dev[b]:
 * a table of B device addresses in device memory, each 16-byte aligned and the base of an entry of
 * at least (T+1)*7168 + 21504 (records: (T+1)*1024) bytes. bad_dev (int, nullable) counts the
 * actions outside [0, A), which are stored clamped. versions_dev (nullable): 16 bytes, 8-byte
 * aligned, that end up holding the min (u32), max (u32) and sum (u64) of the T * B flags words;
 * the call initialises them on the stream first.                                               */
int fi_ingest_atari_planes_gather(const void* const* cols_dev, int T, int B, int A, uint8_t* frames, float* mu,
                                  int32_t* actions, float* rewards, float* discounts, int* bad_dev,
                                  void* versions_dev, void* stream);
int fi_ingest_records_gather(const void* const* cols_dev, int T, int B, int A, int D, float* obs, float* mu,
                             int32_t* actions, float* rewards, float* discounts, int* bad_dev, void* versions_dev,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif
