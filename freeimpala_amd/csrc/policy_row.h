// policy_row.h -- the one copy of the per-row arithmetic of the surrogate objectives and the KL penalty
// (surrogate.hip, target.hip, kl.hip). Internal, header-only; one lane works on one row of A logits in the
// wave's padded LDS rows (row_stream.h).
//   pair_log_prob    log-softmax at the action of two rows from one instruction sequence: bit-equal rows
//                    give bit-equal results, so their difference is exactly 0
//   pair_kl_grad     KL(q || p) of two rows and its gradient c (p - q), written over the p row
//   policy_row_grad  softmax, entropy and dlogits of one row, written over the row
//   adv_moments      m and s of the advantages from the scan's fp64 partials, in one fixed order
#pragma once

#include "row_stream.h"

namespace fi {

constexpr int kStatThreads = 64 * kWaves;  // the one-workgroup stats kernels; a loss workgroup has as many

// {log p(a), log q(a)}, p = softmax(zp), q = softmax(zm)
__device__ __forceinline__ f32x2 pair_log_prob(const float* __restrict__ zp, const float* __restrict__ zm, uint32_t A,
                                               uint32_t ai) {
    f32x2 mx = {zp[0], zm[0]};
    for (uint32_t i = 1; i < A; ++i) mx = __builtin_elementwise_max(mx, f32x2{zp[i], zm[i]});
    f32x2 se = {0.f, 0.f};
    for (uint32_t i = 0; i < A; ++i) {
        const f32x2 x = (f32x2{zp[i], zm[i]} - mx) * L2E;
        se += f32x2{__builtin_amdgcn_exp2f(x.x), __builtin_amdgcn_exp2f(x.y)};
    }
    const f32x2 lg = f32x2{__builtin_amdgcn_logf(se.x), __builtin_amdgcn_logf(se.y)} * LN2;
    return (f32x2{zp[ai], zm[ai]} - mx) - lg;
}

// zp[j] <- c (p_j - q_j), p = softmax(zp), q = softmax(zq); returns KL(q || p) = sum_j q_j (log q_j - log p_j).
// As in pair_log_prob both rows go through one instruction sequence: bit-equal rows give 0 everywhere, exactly
__device__ __forceinline__ float pair_kl_grad(float* __restrict__ zp, const float* __restrict__ zq, uint32_t A, float c) {
    f32x2 mx = {zp[0], zq[0]};
    for (uint32_t i = 1; i < A; ++i) mx = __builtin_elementwise_max(mx, f32x2{zp[i], zq[i]});
    f32x2 se = {0.f, 0.f};
    for (uint32_t i = 0; i < A; ++i) {
        const f32x2 x = (f32x2{zp[i], zq[i]} - mx) * L2E;
        se += f32x2{__builtin_amdgcn_exp2f(x.x), __builtin_amdgcn_exp2f(x.y)};
    }
    const f32x2 lg = f32x2{__builtin_amdgcn_logf(se.x), __builtin_amdgcn_logf(se.y)} * LN2;
    float kl = 0.f;
    for (uint32_t i = 0; i < A; ++i) {
        const f32x2 d = f32x2{zp[i], zq[i]} - mx, x = d * L2E;
        const f32x2 p = f32x2{__builtin_amdgcn_exp2f(x.x), __builtin_amdgcn_exp2f(x.y)} / se;
        const f32x2 l = d - lg;  // log p_i, log q_i
        kl += p.y * (l.y - l.x);
        zp[i] = c * (p.x - p.y);
    }
    return kl;
}

// z[j] <- g (1[j = ai] - p_j) + ec p_j (log p_j - sum_k p_k log p_k), p = softmax(z); returns sum_k p_k log p_k
__device__ __forceinline__ float policy_row_grad(float* __restrict__ z, uint32_t A, uint32_t ai, float g, float ec) {
    float mx = z[0];
    for (uint32_t i = 1; i < A; ++i) mx = fmaxf(mx, z[i]);
    float se = 0.f, sed = 0.f;
    for (uint32_t i = 0; i < A; ++i) {
        const float d = z[i] - mx, e = __builtin_amdgcn_exp2f(d * L2E);
        se += e;
        sed += e * d;
    }
    const float lg = __builtin_amdgcn_logf(se) * LN2;
    const float plogp = sed / se - lg;  // sum pi log pi
    for (uint32_t i = 0; i < A; ++i) {
        const float d = z[i] - mx, p = __builtin_amdgcn_exp2f(d * L2E) / se;
        z[i] = g * ((i == ai ? 1.f : 0.f) - p) + ec * p * ((d - lg) - plogp);
    }
    return plogp;
}

// m and s of A over n = T * B rows from the scan's partials mom[nscan][2] (sums of A - pivot and of its
// square): thread i adds the partials i, i + 256, ... in ascending order, then block_sums. Every
// workgroup of kStatThreads threads that runs this on the same numbers holds the same bits. n = 1
// gives s = 0 exactly: S2 / 1 and (S1 / 1)^2 are one product.
__device__ __forceinline__ void adv_moments(const double* mom, const double* pivot, int nscan, int T, int B, double* red,
                                            double& m, double& s) {
    double v[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < nscan; i += kStatThreads) {
        v[0] += mom[2 * i];
        v[1] += mom[2 * i + 1];
    }
    block_sums<2, kWaves>(v, red);
    const double n = (double)T * (double)B;
    const double m1 = v[0] / n, var = v[1] / n - m1 * m1;
    m = *pivot + m1;
    s = sqrt(var > 0.0 ? var : (var == var ? 0.0 : var));  // NaN stays NaN
}

}  // namespace fi
