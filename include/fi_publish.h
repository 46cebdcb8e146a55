/* fi_publish.h -- C ABI of parameter publication on the device (libfi_learner.so): the learner's
 * parameters reach its actors through stream order alone, with no host copy and no host wait.
 *
 * Nothing of the older headers changes: a handle that never calls a function of this header enqueues
 * exactly what it enqueued before and returns the same bits. Status codes and fi_last_error() as
 * fi_learner.h. One thread at a time per handle, with ONE exception: fi_actor_set_params_dev may be
 * called from the actor's thread while another thread uses the learner handle. It touches nothing of
 * the learner but the publication block, which a mutex of its own guards.
 *
 * Published parameters. The published form is fp32. With FI_PUBLISH_FP32 it is the learner's
 * parameters, bit for bit. With FI_PUBLISH_BF16 every parameter is rounded to bf16 and widened again:
 * round-to-nearest-even on the upper 16 bits; when all exponent bits are set the upper half is kept
 * and, if any of the lower 16 bits is set, its bit 6 is set (a NaN stays a NaN, +-Inf stays); the
 * result is the 16 bits shifted left by 16. Either way a snapshot holds exactly what
 * fi_actor_set_params of fi_learner_get_params' blob leaves in an actor: the two paths are
 * interchangeable bit for bit. The host form of the rule: freeimpala_amd/publish.py (round_params).
 *
 * The publication block. A learner gets one on its first fi_publish_params: two snapshot slots of a
 * 16-byte header {uint64 exact version, uint64 n} and param_count floats each, and a small host
 * record under a mutex. Publication k (k = 0, 1, ...) goes into slot k mod 2. fi_publish_params
 * enqueues on the learner's stream and returns without waiting: the stream waits for every reader
 * event recorded against that slot since the last publication into it; one kernel reads the
 * parameters once, rounds them when the dtype is bf16 and writes the slot; one lane writes the
 * header; the slot's event is recorded behind the kernel. *tag is the learner's version when the
 * publication is enqueued: the count of enqueued updates. The header's exact version is tag minus
 * the updates found skipped and not yet checked, read on the device: the number
 * fi_learner_get_params reports at that point of the stream. The two are equal unless an update
 * enqueued since the last check is skipped.
 *
 * Coupling. The learner's optimiser never waits for an actor. Only a publication into a slot waits
 * for that slot's readers, so a slow reader of publication k can delay publication k + 2 (and what
 * the learner's stream holds behind it) and nothing else.
 *
 * Reader events belong to the learner's block, so learner and actors may be destroyed in either
 * order. A slot takes at most 64 distinct readers (FI_MAX_SEGMENTS) between two publications into
 * it; an actor that reads a slot twice reuses its event; one more distinct reader is FI_ERR_STATE.
 */
#ifndef FI_PUBLISH_H
#define FI_PUBLISH_H

#include <stddef.h>
#include <stdint.h>

#include "fi_actor.h"
#include "fi_learner.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FI_PUBLISH_MAX_READERS 64 /* per slot: FI_MAX_SEGMENTS */

typedef struct {
    uint64_t publications;   /* publications enqueued so far; 0: the fields below are zero          */
    uint64_t tag;            /* the newest publication's tag                                        */
    uint64_t version;        /* its exact version, read from the slot's header (waits for it)       */
    uint32_t slot;           /* the slot that holds it                                              */
    uint32_t dtype;          /* the learner's publish_dtype                                       */
    uint32_t readers[2];     /* readers recorded against each slot since the last publication there */
} fi_publish_state;          /* 40 bytes; offsets 0, 8, 16, 24, 28, 32                              */

/* Publish the parameters as they are at this point of the learner's stream. tag may be NULL. */
int fi_publish_params(fi_learner* l, uint64_t* tag);
/* Waits for the newest publication and copies its snapshot (count == fi_learner_param_count floats)
 * and its exact version (nullable) to the host. FI_ERR_STATE before the first publication. */
int fi_publish_read(fi_learner* l, float* dst, size_t count, uint64_t* version);
int fi_publish_get_state(fi_learner* l, fi_publish_state* out);
/* The newest publication's event (hipEvent_t), NULL before the first. */
void* fi_publish_event(fi_learner* l);

/* The layer underneath, on any device pointer: the actor's stream waits for ready_event (hipEvent_t,
 * nullable), copies count floats from params_dev into the handle's parameters device to device,
 * rebuilds an Atari handle's operand images and records the handle's "params read" event
 * (*read_event_out, nullable) behind the copy. The handle's version becomes `version`. Nothing waits:
 * later act calls follow in stream order and the records they write carry the new version. A
 * recording handle may be given new parameters in the middle of an unroll. Checked before anything is
 * enqueued (FI_ERR_INVALID): count == fi_actor_param_count, 16-byte alignment, and params_dev is
 * device memory of the handle's device inside one allocation that holds count floats. */
int fi_actor_set_params_ptr(fi_actor* a, const float* params_dev, size_t count, uint64_t version, void* ready_event,
                            void** read_event_out);
/* The newest publication of l into a, by the layer above, and a reader event against its slot.
 * Refused with nothing enqueued and the handle unchanged: FI_ERR_STATE before the first publication
 * or for one distinct reader too many; FI_ERR_INVALID for another device, another policy or another
 * parameter count (num_actions, obs_dim, hidden). The handle's version becomes the publication's tag. */
int fi_actor_set_params_dev(fi_actor* a, fi_learner* l);
/* Waits for the actor's stream and copies its fp32 parameters out. FI_ERR_STATE before any were set. */
int fi_actor_read_params(fi_actor* a, float* dst, size_t count);

/* The kernel alone on device pointers (stream: hipStream_t or NULL): dst[i] = the published form of
 * src[i], i < n, dtype FI_PUBLISH_FP32 or FI_PUBLISH_BF16. Both pointers 16-byte aligned (FI_ERR_INVALID otherwise);
 * 16 bytes per lane and access, a scalar tail for n mod 4. */
int fi_publish_copy(float* dst_dev, const float* src_dev, size_t n, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif
