// ring_handle.h -- the entry ring's handle and what a step from it shares between ring.hip (the
// uniform rule, include/fi_ring.h) and prio.hip (the prioritised rule, include/fi_prio.h). Internal:
// not part of the C ABI. prio.hip builds on ring.hip; ring.hip names nothing of prio.hip, so a
// library without it still links.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "fi_ring.h"
#include "kernels.h"

struct fi_ring {
    int dev = 0;
    size_t entry = 0;
    int64_t C = 0;
    uint64_t seed = 0, draw = 0;
    uint64_t head = 0, tail = 0;
    char* base = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t pushed = nullptr;
    bool have_pushed = false;
    uint64_t* last = nullptr;  // the entries of the last ring step, 8 * last_cap bytes
    int last_cap = 0, last_n = 0;
    // ---- priorities (fi_prio.h); everything below stays as it is until fi_prio_enable
    bool prio_on = false;
    float eta = 0.f;
    uint32_t q_init = 0;
    uint64_t prio_hi = 0;           // entries below it hold a table value
    uint32_t* prio = nullptr;       // one u32 per slot
    uint64_t* prio_sums = nullptr;  // the chunk sums of one draw, 1024 u64
    uint32_t* prio_q = nullptr;     // the refresh's per-column priorities, 4 * prio_q_cap bytes
    int prio_q_cap = 0;
    const fi_learner* prio_owner = nullptr;  // the learner whose stream touches the table
    hipEvent_t prio_done = nullptr;          // behind the last prioritised step's refresh
    bool have_prio_done = false;
    // ---- exponents and importance weights (fi_weights.h); the values after fi_prio_enable
    float alpha = 1.f, beta = 0.f;
    float* is_w = nullptr;    // the weights of the last prioritised step that computed any, 4 * is_w_cap bytes
    int is_w_cap = 0;
    bool is_w_valid = false;  // the last prioritised step computed weights
};

namespace fi {

// the numbers of one batch, taken before the call (include/fi_ring.h)
struct RingBatch {
    const char* base;
    size_t entry_bytes;
    uint32_t C;
    int32_t n_fresh;
    uint64_t tail, lo, n_valid, seed, draw;
    uint64_t* entries_out;  // nullable
};

// ring.hip: every refusal of a step from a ring, before anything is enqueued or allocated; on FI_OK
// *li is the learner's shape and *rb the batch's numbers (entries_out still null)
int ring_step_check(fi_learner* l, fi_ring* r, int32_t n_fresh, const std::string& nm, LearnerInfo* li, RingBatch* rb);
// ring.hip: r->last for a batch of B columns
int ring_step_entries(fi_ring* r, int B, const std::string& nm);
// ring.hip: the hand-back of a step that ran or was enqueued (host_util.h: step_taken, finish_taken):
// the ring's stream waits for the consumed event, the counters move
int ring_step_taken(fi_learner* l, fi_ring* r, int32_t n_fresh, int B);
// weights.hip: the importance weights of a prioritised step (fi_weights.h), behind the draw that wrote
// `entries` and the chunk sums on the same stream
int prio_is_weights_launch(const uint64_t* entries, int B, int n_fresh, const uint32_t* table, int64_t C, uint64_t lo,
                           uint64_t n_valid, const uint64_t* sums, float beta, float* w_out, hipStream_t s);

}  // namespace fi
