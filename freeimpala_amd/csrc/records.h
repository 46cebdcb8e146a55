// records.h -- the record schemas of a learner's entries, once: what the actor's recording kernels
// (rollout.hip) write and the ingest kernels (ingest_kernels.h, misc.hip, gather.hip) read. Byte
// offsets in a record; the public sizes are include/fi_learner.h's.
//
// MLP record (one 1 KiB ELEMENT per step, reference data_structures.h:35, agent.h:62):
//   [0,512) float obs[<=128] | [512,768) float mu_logits[<=64] | 768 int32 action |
//   772 float reward | 776 float discount | 780 uint32 flags | 784.. reserved.
// Stacked Atari record (28 ELEMENTs = 28,672 B per step, FI_ATARI_RECORD_BYTES):
//   [0,28224) u8 frame 84x84x4 NHWC | [28224,28480) float mu_logits[<=64] | 28480 int32 action |
//   28484 float reward | 28488 float discount | 28492 uint32 flags | 28496.. reserved.
// Atari plane record (7 ELEMENTs = 7,168 B per step, FI_ATARI_PLANE_RECORD_BYTES):
//   [0,7056) u8 plane 84x84 (the newest observation) | [7056,7128) float mu_logits[<=18] |
//   7128 int32 action | 7132 float reward | 7136 float discount | 7140 uint32 flags |
//   7144 uint32 episode_start | 7148.. reserved.
// In all three the header behind mu is action, reward, discount, flags: four consecutive dwords.
// An entry holds T+1 records (record T = bootstrap observation; of its header only a plane
// record's episode_start is read). A plane entry then holds, at (T+1)*7168, the history block: the
// three planes that precede record 0 in the actor's stack (oldest first, 3*7056 B, padded to
// FI_ATARI_HISTORY_BYTES).
#pragma once

#include <stddef.h>

#include "fi_learner.h"

namespace fi {

// the header behind a record's mu, relative to its action
constexpr int kHdrReward = 4, kHdrDiscount = 8, kHdrFlags = 12;

// ---------------------------------------------------------------- the MLP record
constexpr int kMlpRecBytes = FI_RECORD_BYTES;
constexpr int kMlpMaxObs = 128, kMlpMaxActions = 64;
constexpr int kMlpRecObs = 0;
constexpr int kMlpRecMu = kMlpRecObs + 4 * kMlpMaxObs;     // 512
constexpr int kMlpRecAct = kMlpRecMu + 4 * kMlpMaxActions;  // 768
constexpr int kMlpRecReward = kMlpRecAct + kHdrReward;      // 772, then the discount
constexpr int kMlpRecFlags = kMlpRecAct + kHdrFlags;        // 780
static_assert(kMlpRecReward == 772 && kMlpRecFlags + 4 <= kMlpRecBytes, "MLP record header");

// ---------------------------------------------------------------- the stacked Atari record
constexpr int kFrameBytes = 84 * 84 * 4;
constexpr int kFramePieces = kFrameBytes / 16;  // 1,764 16-byte pieces per frame
constexpr int kAtariRecBytes = FI_ATARI_RECORD_BYTES;
constexpr int kAtariRecMu = kFrameBytes;                        // 28224
constexpr int kAtariRecAct = kAtariRecMu + 4 * kMlpMaxActions;  // 28480
static_assert(kFramePieces * 16 == kFrameBytes, "a frame is a whole number of 16-byte pieces");
static_assert(kAtariRecAct + kHdrFlags + 4 <= kAtariRecBytes, "Atari record header");
static_assert(kAtariRecBytes == FI_ATARI_RECORD_ELEMENTS * FI_RECORD_BYTES, "Atari record size");

// ---------------------------------------------------------------- the plane record
constexpr int kPlaneBytes = 84 * 84;
constexpr int kPlanePieces = kPlaneBytes / 16;        // 441 16-byte pieces per plane
constexpr int kPlaneRuns = (kPlanePieces + 63) / 64;  // 7 runs of 64 pieces, the last of 57
constexpr int kPlaneMaxActions = 18;
constexpr int kPlaneRecBytes = FI_ATARI_PLANE_RECORD_BYTES;
constexpr int kPlaneRecMu = kPlaneBytes;                           // 7056
constexpr int kPlaneRecAct = kPlaneRecMu + 4 * kPlaneMaxActions;   // 7128: compact header, mu[18] then the action
constexpr int kPlaneRecReward = kPlaneRecAct + kHdrReward;         // 7132, then the discount
constexpr int kPlaneRecFlags = kPlaneRecAct + kHdrFlags;           // 7140
constexpr int kPlaneRecStart = kPlaneRecFlags + 4;                 // 7144: episode_start
static_assert(kPlanePieces * 16 == kPlaneBytes && kFramePieces == 4 * kPlanePieces, "whole 16-byte pieces");
static_assert(kPlaneRecReward == 7132 && kPlaneRecStart == 7144 && kPlaneRecStart + 4 <= kPlaneRecBytes,
              "plane record header");
static_assert(kPlaneRecBytes == FI_ATARI_PLANE_RECORD_ELEMENTS * FI_RECORD_BYTES && kPlaneRecBytes % 16 == 0,
              "plane record size");

// ---------------------------------------------------------------- the history block of a plane entry
constexpr int kHistoryPlanes = 3;
constexpr int kHistoryBytes = FI_ATARI_HISTORY_BYTES;
static_assert(kHistoryPlanes * kPlaneBytes <= kHistoryBytes &&
                  kHistoryBytes == FI_ATARI_HISTORY_ELEMENTS * FI_RECORD_BYTES, "history block");
constexpr size_t plane_history_offset(int T) { return (size_t)(T + 1) * kPlaneRecBytes; }

}  // namespace fi
