/* fi_ring.h -- C ABI of the device entry ring (libfi_learner.so).
 *
 * The reference's SharedBuffer in device memory: a ring of `capacity` entries of entry_bytes bytes
 * each, which recording actors (fi_rollout.h) push their completed unrolls into and from which a
 * learner handle on the same device steps. It stands between the two, so an actor no longer waits
 * for the learner (a pushed unroll is released at once), a batch no longer needs every actor
 * ready at the same moment, and an entry that was read once stays in its slot until a later push
 * overwrites it: a learner batch may mix fresh entries with replayed ones. The ring neither knows
 * nor cares about the record format. Status codes and fi_last_error() as fi_learner.h; one thread
 * at a time per handle.
 *
 * State. Two counters on the host, which issues every operation: head = entries ever pushed,
 * tail = entries ever taken as fresh. Entry e lives in slot e mod capacity. Unread = [tail, head);
 * replayable = [lo, tail) with lo = head > capacity ? head - capacity : 0: what was read once and
 * is still resident. A third counter, draw, counts the successful ring steps.
 *
 * The rule of a step with n_fresh fresh columns out of the learner's B, every number taken before
 * the call: column c < n_fresh takes entry tail + c (FIFO; n_fresh = B is the reference's
 * readBatch(B)); column c >= n_fresh takes entry lo + ((x_c * n_valid) >> 32) with
 * n_valid = tail - lo and x_c the first word of Philox4x32-10(key = seed, counter = draw * B + c,
 * stream 7): uniform, with replacement. Two columns may name one entry. Afterwards
 * tail += n_fresh and draw += 1.
 */
#ifndef FI_RING_H
#define FI_RING_H

#include <stddef.h>
#include <stdint.h>

#include "fi_actor.h"
#include "fi_gather.h"
#include "fi_learner.h"
#include "fi_rollout.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fi_ring fi_ring;

typedef struct {
    uint64_t capacity, entry_bytes;
    uint64_t head, tail; /* entries ever pushed / ever taken as fresh */
    uint64_t draw, seed;
} fi_ring_state;

/* ---- the handle --------------------------------------------------------------------------- */
/* One zero-filled device allocation of capacity * entry_bytes on `device` (FI_ERR_OOM carries the
 * byte count), a stream and a `pushed` event of the ring's own. FI_ERR_INVALID, with the number:
 * entry_bytes below 16 or no multiple of 16; capacity outside [1, 2^31 - 1].                   */
int fi_ring_create(int32_t device, size_t entry_bytes, int64_t capacity, uint64_t seed, fi_ring** out);
void fi_ring_destroy(fi_ring* r);
int fi_ring_info(const fi_ring* r, fi_ring_state* out);
/* The key and the counter of the replay draws (the next step uses `draw`). */
int fi_ring_seed(fi_ring* r, uint64_t seed, uint64_t draw);

/* n entries in device memory, entry i at entries_dev + i * entry_stride, become the entries head ..
 * head + n - 1: the ring's stream waits for ready_event (hipEvent_t or NULL), one kernel copies the
 * first entry_bytes bytes of each into its slot, and the `pushed` event is recorded behind it. The
 * call returns once that is enqueued. A push never overwrites an unread entry and never blocks:
 * FI_ERR_STATE ("full") when n > capacity - (head - tail), with nothing enqueued (the reference's
 * try_write). FI_ERR_INVALID as fi_learner_step_entries_dev: n below 1; entry_stride below
 * entry_bytes; a stride or pointer that is not 16-byte aligned; a pointer that is not device
 * memory of the ring's device, or whose allocation ends before the last entry does.            */
int fi_ring_push(fi_ring* r, const void* entries_dev, size_t entry_stride, int32_t n, void* ready_event);
/* The hipEvent_t recorded behind the last push's copy (the handle owns it); NULL before the first. */
void* fi_ring_pushed_event(fi_ring* r);
/* The ring's hipStream_t: pushes and read-backs run on it (for events around a push). */
void* fi_ring_stream(fi_ring* r);
/* Acquire the actor's completed unroll, push its num_envs entries, release it with the pushed
 * event: the actor may complete its next unroll without any learner having stepped.
 * FI_ERR_INVALID (with the numbers) for an actor on another device or whose
 * fi_rollout_entry_bytes() is not the ring's entry_bytes; FI_ERR_STATE when no unroll waits or the
 * ring is full -- the unroll then still waits.                                                 */
int fi_ring_push_rollout(fi_ring* r, fi_actor* a);

/* Both wait for the ring's stream; for tests and diagnostics. n slots from first_slot on (no wrap:
 * first_slot + n <= capacity) to host memory, bytes == n * entry_bytes.                        */
int fi_ring_read_slots(fi_ring* r, int64_t first_slot, int32_t n, void* host_dst, size_t bytes);
/* The entry indices the last ring step chose, column by column; n == that learner's batch.
 * FI_ERR_STATE before the first ring step.                                                     */
int fi_ring_last_entries(fi_ring* r, uint64_t* dst, int32_t n);

/* ---- the learner steps from a ring --------------------------------------------------------- */
/* One step whose batch is chosen by the rule above, 0 <= n_fresh <= cfg.batch. The learner's stream
 * waits for the `pushed` event; one kernel writes the column table (column c at base + slot *
 * entry_bytes), the neutral version block and the chosen entry indices (8 * batch bytes the ring
 * allocates on first use); the gathering ingest of fi_gather.h, the consumed event
 * (fi_learner_entries_consumed_event) and the unchanged step follow; the ring's stream is made to
 * wait for that event, so a later push that overwrites those slots is ordered behind the ingest.
 * Returns when the step is done (the _async form once it is enqueued: fi_learner_wait
 * afterwards). fi_learner_batch_versions works after it; no host-entry staging is touched. The
 * counters move when the step returns FI_OK or FI_ERR_NONFINITE (it ran; the update was skipped),
 * or, asynchronously, once it is enqueued; after any other status they stay -- a batch the learner
 * rejects for an action outside [0, A) is still unread.
 * Refused before anything is enqueued, every counter unchanged -- FI_ERR_STATE: fewer than n_fresh
 * entries unread; n_fresh < batch and nothing replayable. FI_ERR_INVALID, with the numbers: another
 * device; entry_bytes below fi_learner_entry_bytes(); n_fresh outside [0, batch]; an Atari handle
 * in the stacked format.                                                                       */
int fi_learner_step_ring(fi_learner* l, fi_ring* r, int32_t n_fresh, fi_step_stats* out);
int fi_learner_step_ring_async(fi_learner* l, fi_ring* r, int32_t n_fresh);

/* ---- standalone kernels on device pointers (stream: hipStream_t or NULL) ------------------- */
/* The push's copy: the first entry_bytes bytes of source entry i (src + i * src_stride) into slot
 * (first_entry + i) mod capacity of the ring at dst_base. 1 <= n <= capacity; dst_base, src and
 * src_stride 16-byte aligned, entry_bytes a multiple of 16, src_stride >= entry_bytes.          */
int fi_ring_copy_entries(void* dst_base, size_t entry_bytes, int64_t capacity, uint64_t first_entry, const void* src,
                         size_t src_stride, int32_t n, void* stream);
/* The rule on the device, one lane per column: cols_dev[c] = base + (e_c mod capacity) *
 * entry_bytes and entries_out_dev[c] = e_c (8 * B bytes each, 8-byte aligned; entries_out_dev
 * nullable), and versions_dev (nullable, 16 bytes) to its neutral state {min = ~0, max = 0,
 * sum = 0}. lo + n_valid == tail, n_valid <= capacity, 0 <= n_fresh <= B, and n_valid >= 1 when
 * n_fresh < B.                                                                                 */
int fi_ring_fill_columns(const void** cols_dev, uint64_t* entries_out_dev, void* versions_dev, const void* base,
                         size_t entry_bytes, int64_t capacity, int32_t B, int32_t n_fresh, uint64_t tail, uint64_t lo,
                         uint64_t n_valid, uint64_t seed, uint64_t draw, void* stream);

#ifdef __cplusplus
}
#endif
#endif
