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

// The constants of a cutoff (include/grappa_hip.h grappa_nb_cut), each rounded once on the host: rc2 = rc^2; the switch S = 1 - 10 u^3 +
// 15 u^4 - 6 u^5, u = max(0, (r - rs) inv_w), inv_w = 1 / (rc - rs) (no switch: rs = rc, inv_w = 0, so u = 0 and S = 1 exactly); the
// reaction field k_rf = (eps - 1) / ((2 eps + 1) rc^3), c_rf = 3 eps / ((2 eps + 1) rc).
struct NbCutK {
    float rc2, rs, inv_w, krf, crf;
};

// one pair that is NOT an exception under a cutoff: nothing at all for r2 >= rc2 (a branch, so a NaN r2 is evaluated and is found as a
// non-finite gradient); else E_lj = S(r) 4 eps ((s/r)^12 - (s/r)^6), E_c = K q q (1/r + k_rf r^2 - c_rf) and their exact derivative.
__device__ __forceinline__ void nb_pair_cut(float dx, float dy, float dz, float sij, float e4, float kqq, const NbCutK& k, float& elj, float& ec,
                                            float& gx, float& gy, float& gz) {
    const float r2 = dx * dx + dy * dy + dz * dz;
    if (r2 >= k.rc2) return;
    float y = __builtin_amdgcn_rsqf(r2);
    y = __builtin_fmaf(0.5f * y, __builtin_fmaf(-r2 * y, y, 1.0f), y);
    const float y2 = y * y;
    const float sr2 = sij * sij * y2;
    const float sr6 = sr2 * sr2 * sr2;
    const float l6 = e4 * sr6, l12 = l6 * sr6;
    const float lj = l12 - l6;
    const float u = fmaxf((r2 * y - k.rs) * k.inv_w, 0.f), u2 = u * u, w = 1.0f - u;
    const float S = __builtin_fmaf(u2 * u, __builtin_fmaf(u, __builtin_fmaf(u, -6.0f, 15.0f), -10.0f), 1.0f);
    const float dS = -30.0f * u2 * w * w * k.inv_w * y;                               // (dS/dr) / r
    elj = __builtin_fmaf(S, lj, elj);
    ec = __builtin_fmaf(kqq, __builtin_fmaf(k.krf, r2, y) - k.crf, ec);
    const float fc = kqq * __builtin_fmaf(-y, y2, 2.0f * k.krf);                      // (dE_c/dr) / r
    const float f = __builtin_fmaf(S, (6.0f * l6 - 12.0f * l12) * y2, __builtin_fmaf(lj, dS, fc));
    gx = __builtin_fmaf(f, dx, gx);
    gy = __builtin_fmaf(f, dy, gy);
    gz = __builtin_fmaf(f, dz, gz);
}

}  // namespace
