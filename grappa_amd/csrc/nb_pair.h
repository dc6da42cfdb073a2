// One Lennard-Jones + Coulomb pair (fp32), shared by csrc/nonbonded.hip and csrc/relax.hip: the same arithmetic in both.
#pragma once
#include "common.h"

namespace {

constexpr float NB_K = (float)(138.93545764438198 * 10.0 / 4.184);      // kcal A / (mol e^2): OpenMM's ONE_4PI_EPS0

// one pair: d = x_i - x_j, sij / e4 / kqq = sigma, 4 eps, K q_i q_j of the pair.  v_rsq_f32 is good to 1 ulp and the twelfth power
// multiplies that by 12: one Newton step brings 1/r to half an ulp.
__device__ __forceinline__ void nb_pair(float dx, float dy, float dz, float sij, float e4, float kqq, float& elj, float& ec, float& gx,
                                        float& gy, float& gz) {
    const float r2 = dx * dx + dy * dy + dz * dz;
    float y = __builtin_amdgcn_rsqf(r2);
    y = __builtin_fmaf(0.5f * y, __builtin_fmaf(-r2 * y, y, 1.0f), y);
    const float y2 = y * y;
    const float sr2 = sij * sij * y2;
    const float sr6 = sr2 * sr2 * sr2;
    const float l6 = e4 * sr6, l12 = l6 * sr6;
    const float c = kqq * y;
    elj += l12 - l6;
    ec += c;
    const float f = (6.0f * l6 - 12.0f * l12 - c) * y2;      // (dE/dr) / r
    gx = __builtin_fmaf(f, dx, gx);
    gy = __builtin_fmaf(f, dy, gy);
    gz = __builtin_fmaf(f, dz, gz);
}

}  // namespace
