/* fi_rollout.h -- C ABI of rollouts recorded on the device (libfi_learner.so).
 *
 * Closes the loop between fi_actor.h and fi_learner.h without the host: a recording actor handle
 * writes, as it acts, the learner's own host-entry format into device memory, and a learner handle
 * on the same device steps straight from those entries (its ingest kernel reads them in place).
 * Only the rewards and discounts, 8 bytes per env-step, come from the host. Status codes and
 * fi_last_error() as fi_learner.h; one thread at a time per handle.
 *
 * Entry format. Atari handles: plane records (FI_RECORDS_PLANES),
 * (T+1) * 7168 + 21504 bytes per environment; MLP handles: (T+1) * 1024 bytes. The entry stride of
 * a rollout buffer is the entry size.
 *
 * Recording rule. Act call number j since fi_rollout_begin (fi_actor_act_planes on an Atari
 * handle, fi_actor_act_obs on an MLP handle) writes record t = j mod T of unroll j / T, from the
 * call's own device tensors: the plane (MLP: the obs_dim floats), mu = the policy's logits (A
 * floats, nothing beyond), the int32 action, episode_start (0 / 1; Atari), and in the flags word
 * the low 32 bits of the version given to the last fi_actor_set_params. fi_rollout_outcome fills
 * that record's reward and discount. Unrolls overlap by one step: call j = (k+1) T, the (T+1)-th
 * of unroll k, writes its plane and episode_start (MLP: its observation) into record T of unroll
 * k -- the rest of that record's header stays zero -- and the whole step into record 0 of the
 * other buffer, unroll k+1's first. A call that writes a record 0 also writes that buffer's
 * history block (Atari): channels 0, 1, 2 of the stack the policy just ran on, oldest first.
 * Unroll k is complete when that call returns. Reserved bytes and mu beyond A stay zero for the
 * buffers' life: with version 0 a completed unroll is byte-equal to what
 * pack_atari_plane_records / pack_records (freeimpala_amd/learner.py) build from the same steps.
 *
 * Refused with FI_ERR_STATE, before anything is enqueued or pushed: an act call when the previous
 * step's outcome was never supplied; the completing call of unroll k+1 while unroll k has not been
 * released (its buffer takes unroll k+2's record 0). fi_actor_act_frames on a recording handle is
 * FI_ERR_INVALID (stacked records are not produced), fi_actor_reset_stacks FI_ERR_STATE (it would
 * break the history the learner rebuilds). An act call that returns FI_ERR_NONFINITE has still
 * recorded its step. A handle that never began a rollout enqueues exactly what it did before.
 */
#ifndef FI_ROLLOUT_H
#define FI_ROLLOUT_H

#include <stddef.h>
#include <stdint.h>

#include "fi_actor.h"
#include "fi_learner.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the recorder on an actor handle ------------------------------------------------------ */
/* Allocates two zero-filled device buffers of num_envs entries each (2 * N * entry bytes;
 * FI_ERR_OOM carries the byte count) and starts recording. seq_len = T >= 1. FI_ERR_STATE when the
 * handle records already; FI_ERR_INVALID for an Atari handle with more than 18 actions.        */
int fi_rollout_begin(fi_actor* a, int32_t seq_len);
/* N rewards and N discounts (host) for the actions of the last act call. They pass through the
 * handle's pinned staging, one small H2D copy and a scatter kernel; the call returns once those
 * are enqueued. FI_ERR_STATE without an act call since the last outcome (or since begin).      */
int fi_rollout_outcome(fi_actor* a, const float* rewards, const float* discounts);
int fi_rollout_ready(const fi_actor* a); /* 1 when a completed unroll waits, else 0 */
size_t fi_rollout_entry_bytes(const fi_actor* a); /* 0 when not recording */
/* The completed unroll: its device buffer (N entries, entry i at entries_dev + i * entry_stride)
 * and ready_event, a hipEvent_t recorded on the actor's stream after the buffer's last write (the
 * handle owns it). Any of the outputs may be NULL. FI_ERR_STATE when no unroll waits.          */
int fi_rollout_acquire(fi_actor* a, const void** entries_dev, size_t* entry_stride, void** ready_event);
/* The consumer is done with the acquired buffer once consumed_event (a hipEvent_t; NULL: done
 * already) has completed: the actor's stream waits for it before its next write. FI_ERR_STATE
 * when no unroll waits.                                                                        */
int fi_rollout_release(fi_actor* a, void* consumed_event);
/* Copies the completed unroll's N entries to host memory (bytes == N * entry bytes); it does not
 * release. For tests and for a learner on another machine.                                     */
int fi_rollout_read(fi_actor* a, void* host_dst, size_t bytes);
int fi_rollout_end(fi_actor* a); /* stops recording, frees the buffers; FI_OK when not recording */

/* ---- the learner steps from device entries ------------------------------------------------- */
/* The learner's stream waits for ready_event (hipEvent_t or NULL), runs the handle's ingest kernel
 * for its record format straight from entries_dev (cfg.batch entries, entry_stride apart) and then
 * the unchanged step; no staging buffer is allocated or touched. Returns when the step is done
 * (the _async form once it is enqueued: fi_learner_wait as after fi_learner_step_async).
 * fi_learner_step_resident afterwards re-steps the same batch. FI_ERR_INVALID: entry_stride below
 * fi_learner_entry_bytes(); a stride or pointer that is not 16-byte aligned; a pointer that is not
 * device memory of the handle's device, or whose allocation ends before the last entry does; an
 * Atari handle in the stacked format (fi_learner_set_record_format(FI_RECORDS_PLANES) first).   */
int fi_learner_step_entries_dev(fi_learner* l, const void* entries_dev, size_t entry_stride, void* ready_event,
                                fi_step_stats* out);
int fi_learner_step_entries_dev_async(fi_learner* l, const void* entries_dev, size_t entry_stride,
                                      void* ready_event);
/* The hipEvent_t recorded on the learner's stream right after the last such ingest: what the
 * producer hands to fi_rollout_release. NULL before the first one.                             */
void* fi_learner_entries_consumed_event(fi_learner* l);
/* Pinned plus device bytes of the handle's host-entry staging buffers: 0 until a host batch came */
size_t fi_learner_staging_bytes(const fi_learner* l);
/* acquire, step, release in one call. FI_ERR_INVALID (with the numbers) unless actor and learner
 * share the device, the policy, num_actions and obs_dim, the actor's num_envs equals the learner's
 * batch and the rollout's T its seq_len; FI_ERR_STATE when no unroll is ready. The unroll is
 * released when the step returns FI_OK or FI_ERR_NONFINITE (it ran; the update was skipped); after
 * any other status it still waits, and fi_rollout_release(a, NULL) drops it.                   */
int fi_learner_step_rollout(fi_learner* l, fi_actor* a, fi_step_stats* out);

/* ---- standalone kernels on device pointers (stream: hipStream_t or NULL) ------------------- */
/* One step of N environments into plane-record entries: the plane (N, 7056) u8 and episode_start
 * (N) u8 into record t of entry i at entries_dev + i * entry_stride; with logits_dev != NULL also
 * mu = logits (N, A) fp32, the action (N) int32 and the flags word. Reward, discount and every
 * other byte are left as they are. entries_dev, entry_stride and planes_dev 16-byte aligned,
 * entry_stride >= (t+1) * 7168, 2 <= A <= 18.                                                  */
int fi_record_plane_step(void* entries_dev, size_t entry_stride, int32_t t, const uint8_t* planes_dev,
                         const uint8_t* episode_start_dev, const float* logits_dev, const int32_t* actions_dev,
                         uint32_t flags, int N, int A, void* stream);
/* Channels 0, 1, 2 of N stacks (N, 84, 84, 4) u8 as three planes, oldest first, at byte
 * history_offset of every entry (3 * 7056 bytes are written). entries_dev, entry_stride,
 * history_offset and stacks_dev 16-byte aligned, entry_stride >= history_offset + 21168.        */
int fi_extract_history(void* entries_dev, size_t entry_stride, size_t history_offset, const uint8_t* stacks_dev,
                       int N, void* stream);

#ifdef __cplusplus
}
#endif
#endif
