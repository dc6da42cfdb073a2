// The X-H constraint solves that the two constrained dynamics kernels share, ONE copy each (csrc/dynamics_cons.hip: a molecule in a
// workgroup, the state in LDS; csrc/dynamics_steps.hip: a molecule over many workgroups, a cluster's state in registers): the cluster,
// the 4 x 4 elimination, P (the velocity projection), S (M-SHAKE) and the half drift that records S's reference bonds, as
// include/grappa_hip.h states them at grappa_md_langevin_cons_f32.
//   state  : the functions see a cluster's atoms through SLOTS -- 0 the centre, k + 1 the packed leaf k -- of a state St with
//            V3 x(slot), V3 v(slot), set_x(slot, V3), set_v(slot, V3).  Every slot is a compile-time constant once the loops are unrolled,
//            so a state held in registers is never indexed at run time.  An atom that is frozen (w == 0) is never written.
#pragma once
#include <float.h>
#include <math.h>

#include "common.h"
#include "mm_geom.h"

namespace {

constexpr int CL = GRAPPA_MD_CONS_MAX_LEAVES;

// a thread's cluster: the centre, the L constrained leaves (packed to the front) and their squared lengths
struct Cluster {
    int L, a0, al[CL];
    float w0, wl[CL], d2[CL];
};

// leaf `atom` with inverse mass wk and length d joins the cluster unless both of its ends are frozen (then it is no constraint)
__device__ __forceinline__ void cons_add_leaf(Cluster& cl, int atom, float wk, float d) {
    if (cl.w0 + wk > 0.f) {
#pragma unroll
        for (int j = 0; j < CL; ++j)          // (written out: cl.L is not a compile-time index)
            if (j == cl.L) cl.al[j] = atom, cl.wl[j] = wk, cl.d2[j] = d * d;
        ++cl.L;
    }
}

// M y = b for a 4 x 4 system whose unused rows are identity rows: elimination without pivoting, written out
__device__ __forceinline__ void solve4(float (&M)[CL][CL], float (&b)[CL], float (&y)[CL]) {
#pragma unroll
    for (int i = 0; i < CL; ++i) {
        const float inv = 1.0f / M[i][i];
#pragma unroll
        for (int j = i + 1; j < CL; ++j) {
            const float f = M[j][i] * inv;
#pragma unroll
            for (int c = i + 1; c < CL; ++c) M[j][c] -= f * M[i][c];
            b[j] -= f * b[i];
        }
    }
#pragma unroll
    for (int i = CL - 1; i >= 0; --i) {
        float s = b[i];
#pragma unroll
        for (int c = i + 1; c < CL; ++c) s -= M[i][c] * y[c];
        y[i] = s / M[i][i];
    }
}

// P: the cluster's velocities projected onto r_k . (v_k - v_0) = 0, one direct solve
template <class St>
__device__ __forceinline__ void cons_project(const Cluster& c, St& st) {
    const V3 x0 = st.x(0);
    V3 v0 = st.v(0);
    V3 r[CL];
    float M[CL][CL], b[CL], mu[CL];
#pragma unroll
    for (int k = 0; k < CL; ++k) {
        r[k] = {0.f, 0.f, 0.f}, b[k] = 0.f;
        if (k < c.L) {
            r[k] = st.x(k + 1) - x0;
            b[k] = dot(r[k], st.v(k + 1) - v0);
        }
    }
#pragma unroll
    for (int k = 0; k < CL; ++k)
#pragma unroll
        for (int l = 0; l < CL; ++l) {
            M[k][l] = k == l ? 1.f : 0.f;
            if (k < c.L && l < c.L) M[k][l] = c.w0 * dot(r[k], r[l]) + (k == l ? c.wl[k] * dot(r[k], r[k]) : 0.f);
        }
    solve4(M, b, mu);
    V3 s = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < CL; ++k)
        if (k < c.L) {
            s = s + mu[k] * r[k];
            if (c.wl[k] > 0.f) st.set_v(k + 1, st.v(k + 1) - (c.wl[k] * mu[k]) * r[k]);
        }
    if (c.w0 > 0.f) st.set_v(0, v0 + c.w0 * s);
}

// S: the cluster's coordinates brought back to its lengths along the bonds of the reference coordinates rref (relative to the centre),
// the velocities corrected by the same displacement / (dt / 2) if `vel`.  false: not converged within the cap.
template <class St>
__device__ __forceinline__ bool cons_shake(const Cluster& c, const V3 (&rref)[CL], St& st, float tol2, float ih2, bool vel) {
    V3 x0 = st.x(0);
    V3 rt[CL], r[CL];
    float lam[CL], sig[CL];
#pragma unroll
    for (int k = 0; k < CL; ++k) {
        rt[k] = {0.f, 0.f, 0.f}, r[k] = {0.f, 0.f, 0.f}, lam[k] = 0.f, sig[k] = 0.f;
        if (k < c.L) rt[k] = st.x(k + 1) - x0;
    }
    V3 s = {0.f, 0.f, 0.f};
    bool ok = false;
    for (int it = 0; it <= GRAPPA_MD_CONS_MAX_ITER; ++it) {
        s = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < CL; ++k)
            if (k < c.L) s = s + lam[k] * rref[k];
        ok = true;
#pragma unroll
        for (int k = 0; k < CL; ++k)
            if (k < c.L) {
                r[k] = rt[k] - (c.wl[k] * lam[k]) * rref[k] - c.w0 * s;
                sig[k] = dot(r[k], r[k]) - c.d2[k];
                if (!(fabsf(sig[k]) <= tol2 * c.d2[k])) ok = false;          // (a sigma that is not finite: not converged)
            }
        if (ok || it == GRAPPA_MD_CONS_MAX_ITER) break;
        float J[CL][CL], dl[CL];
#pragma unroll
        for (int k = 0; k < CL; ++k)
#pragma unroll
            for (int l = 0; l < CL; ++l) {
                J[k][l] = k == l ? 1.f : 0.f;
                if (k < c.L && l < c.L) J[k][l] = -2.0f * (c.w0 * dot(r[k], rref[l]) + (k == l ? c.wl[k] * dot(r[k], rref[k]) : 0.f));
            }
        solve4(J, sig, dl);
#pragma unroll
        for (int k = 0; k < CL; ++k)
            if (k < c.L) lam[k] -= dl[k];
    }
    bool finite = true;
#pragma unroll
    for (int k = 0; k < CL; ++k)
        if (k < c.L && !(fabsf(lam[k]) <= FLT_MAX)) finite = false;
    if (!finite) return false;          // nothing to apply
    if (c.w0 > 0.f) {
        x0 = x0 + c.w0 * s;
        st.set_x(0, x0);
        if (vel) st.set_v(0, st.v(0) + ih2 * (c.w0 * s));
    }
#pragma unroll
    for (int k = 0; k < CL; ++k)
        if (k < c.L && c.wl[k] > 0.f) {          // (a frozen leaf keeps its bits: its bond is held by the centre alone)
            st.set_x(k + 1, x0 + r[k]);
            if (vel) st.set_v(k + 1, st.v(k + 1) - (c.wl[k] * lam[k] * ih2) * rref[k]);
        }
    return ok;
}

// the reference bonds of the coordinates held
template <class St>
__device__ __forceinline__ void cons_bonds(const Cluster& c, V3 (&rref)[CL], const St& st) {
    const V3 x0 = st.x(0);
#pragma unroll
    for (int k = 0; k < CL; ++k) {
        rref[k] = {0.f, 0.f, 0.f};
        if (k < c.L) rref[k] = st.x(k + 1) - x0;
    }
}

// the reference bonds of the coordinates held, then a half drift of the cluster's moving atoms
template <class St>
__device__ __forceinline__ void cons_drift(const Cluster& c, V3 (&rref)[CL], St& st, float h2) {
    cons_bonds(c, rref, st);
#pragma unroll
    for (int k = 0; k < CL; ++k)
        if (k < c.L && c.wl[k] > 0.f) st.set_x(k + 1, st.x(k + 1) + h2 * st.v(k + 1));
    if (c.w0 > 0.f) st.set_x(0, st.x(0) + h2 * st.v(0));
}

}  // namespace
