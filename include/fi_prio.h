/* fi_prio.h -- C ABI of prioritised replay for the device entry ring (libfi_learner.so).
 *
 * fi_ring.h draws a step's replayed columns uniformly from the entries that were read before and
 * are still resident. Here they are drawn in proportion to a per-entry priority that the learner
 * refreshes from its own step: the TD magnitude |vs - V| of the column the entry filled. The rule
 * is integer arithmetic from the quantised priorities on, so a host reproduces every draw exactly
 * (freeimpala_amd/prio.py: prio_batch_entries). Nothing of fi_ring.h changes; its uniform step and
 * the prioritised one may alternate on one ring and share its `draw` counter. Status codes and
 * fi_last_error() as fi_learner.h; one thread at a time per handle.
 *
 * Priority of a column b, from the learner's vs (T, B) and values (T + 1, B), all in fp32:
 *   d_t = |vs[t, b] - values[t, b]|, t = 0 .. T-1
 *   p_b = eta * max_t d_t + (1 - eta) * (sum_t d_t) / T      (the sum over t ascending)
 * eta in [0, 1] is the ring's parameter, held as the fp32 number given at enable (R2D2: 0.9).
 *
 * Quantisation to u32: q = FI_PRIO_Q_MAX = 2^31 - 1 when p is NaN, Inf or >= 32768; otherwise
 * q = max(1, rint(p * 65536)), ties to even. q >= 1 always: every readable entry stays drawable
 * and a total is never 0.
 *
 * Table: one u32 per slot (4 * capacity bytes of device memory), touched only by kernels on the
 * learner's stream (and by fi_prio_set, which waits for them first). A prioritised ring needs
 * capacity <= 2^20; then a sum of priorities stays below 2^51 and is exact in u64.
 *
 * Which entries hold a priority: the ring keeps a host counter prio_hi; entries below it have a
 * table value. Before a prioritised step samples, it stores q_init (the quantised init_priority of
 * fi_prio_enable) to the slots of the entries [max(prio_hi, lo), tail + n_fresh) -- the range may
 * wrap -- and then prio_hi = tail + n_fresh. Entries that a uniform step took as fresh get q_init
 * this way.
 *
 * The draw of a step with n_fresh fresh columns out of B, every number taken before the call as
 * in fi_ring.h (lo, tail, n_valid = tail - lo, draw): column c < n_fresh takes entry tail + c.
 * For column c >= n_fresh let (w0, w1, ., .) = Philox4x32-10(key = seed, counter = draw * B + c,
 * stream 8), x = w0 * 2^32 + w1, Q = sum_{j < n_valid} q_j with q_j the priority of entry lo + j,
 * and r = (x * Q) >> 64. The column takes entry lo + min{ j : q_0 + ... + q_j > r }. With
 * replacement: two columns may name one entry. Afterwards tail += n_fresh and draw += 1.
 *
 * The refresh: after the step every column's entry e, fresh or replayed, gets
 * q[e mod capacity] = the maximum of quantise(p_b) over the columns b that name e, replacing the
 * old value; entries outside the batch keep theirs bit for bit. No floating-point atomics: one
 * pass stores 0 to every named slot, a second one folds with an integer atomic maximum.
 */
#ifndef FI_PRIO_H
#define FI_PRIO_H

#include <stddef.h>
#include <stdint.h>

#include "fi_ring.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FI_PRIO_Q_MAX 0x7fffffffu
#define FI_PRIO_MAX_CAPACITY (1 << 20)

typedef struct {
    uint32_t enabled; /* 0: every other field is 0 */
    float eta;
    uint32_t q_init;
    uint32_t reserved;
    uint64_t prio_hi;
    uint64_t table_bytes;
} fi_prio_state;

/* ---- the ring's priorities ---------------------------------------------------------------- */
/* Allocates the table (4 * capacity bytes) and the chunk sums of a draw (8 KiB); FI_ERR_OOM carries
 * the byte count. prio_hi = lo: no entry holds a priority yet. FI_ERR_INVALID, with the number: eta
 * outside [0, 1]; init_priority negative or not finite; capacity above 2^20. FI_ERR_STATE on a
 * second call.                                                                                 */
int fi_prio_enable(fi_ring* r, float eta, float init_priority);
int fi_prio_info(const fi_ring* r, fi_prio_state* out);
/* The priorities of the entries first_entry .. first_entry + n - 1, which must lie in [lo, tail)
 * (refused with the numbers otherwise; n >= 1). Both wait for the refresh of the ring's last
 * prioritised step. read: q_init for an entry at or above prio_hi. set: first stores q_init up to
 * tail as a prioritised step would (prio_hi = max(prio_hi, tail): never past an unread entry),
 * then src; a value of 0 or above FI_PRIO_Q_MAX is refused with nothing stored. For tests, and for
 * restoring priorities.                                                                         */
int fi_prio_read(fi_ring* r, uint64_t first_entry, int32_t n, uint32_t* dst);
int fi_prio_set(fi_ring* r, uint64_t first_entry, int32_t n, const uint32_t* src);

/* ---- the learner steps from a ring, replayed columns drawn by priority --------------------- */
/* fi_learner_step_ring with the draw above. On the learner's stream: the q_init fill, the chunk
 * sums of the window, one kernel that writes the column table, the neutral version block and the
 * chosen entry indices, then the gathering ingest and the unchanged step; behind the step the
 * refresh (priorities from vs / values, the two scatter passes). Every refusal of
 * fi_learner_step_ring applies with the same status, before anything is enqueued and with every
 * counter unchanged; in addition FI_ERR_STATE when priorities are not enabled and FI_ERR_INVALID
 * when a learner handle other than the first that took a prioritised step from this ring does.
 * Counters move as for fi_learner_step_ring. The refresh runs after FI_OK and after
 * FI_ERR_NONFINITE (NaN columns become FI_PRIO_Q_MAX, finite ones their value); on the _async
 * form once the step is enqueued; after any other status nothing is refreshed.
 * fi_ring_last_entries and fi_learner_batch_versions work after the call. fi_ring_destroy waits
 * for the last refresh.                                                                        */
int fi_learner_step_ring_prioritized(fi_learner* l, fi_ring* r, int32_t n_fresh, fi_step_stats* out);
int fi_learner_step_ring_prioritized_async(fi_learner* l, fi_ring* r, int32_t n_fresh);

/* ---- standalone kernels on device pointers (stream: hipStream_t or NULL) ------------------- */
/* q_out[b] = quantise(p_b), b < B, from vs (T, B) and the first T rows of values; T, B >= 1,
 * eta in [0, 1].                                                                               */
int fi_prio_from_td(const float* vs, const float* values, int32_t T, int32_t B, float eta, uint32_t* q_out,
                    void* stream);
/* The refresh on a table of `capacity` u32: the slots entries[b] mod capacity, b < B, get the
 * maximum of q_cols[b] over the columns that name them (q_cols[b] >= 1); no other slot is written. */
int fi_prio_scatter(uint32_t* table, int64_t capacity, const uint64_t* entries, const uint32_t* q_cols, int32_t B,
                    void* stream);
/* The draw on the device, as fi_ring_fill_columns: cols_dev, entries_out_dev (nullable) and
 * versions_dev (nullable) as there; table: `capacity` u32, entry e's priority at e mod capacity;
 * chunk_ws: 8 KiB of device scratch, 8-byte aligned. capacity <= 2^20, lo + n_valid == tail,
 * n_valid <= capacity, 0 <= n_fresh <= B, and n_valid >= 1 when n_fresh < B.                   */
int fi_prio_fill_columns(const void** cols_dev, uint64_t* entries_out_dev, void* versions_dev, const void* base,
                         size_t entry_bytes, int64_t capacity, int32_t B, int32_t n_fresh, uint64_t tail, uint64_t lo,
                         uint64_t n_valid, const uint32_t* table, void* chunk_ws, uint64_t seed, uint64_t draw,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif
