// The three passes of the GB/SA implicit solvent (include/grappa_hip.h grappa_gb_desc) over a work item, as the energy entry
// (csrc/gb_obc.hip) and the stepwise dynamics (csrc/dynamics_steps.hip) run them: ONE text for both, what one of them evaluates or
// rounds the other does.  A thread owns one (i-atom, conformation) and one of JS slices of the j loop (gb_tile_loop of csrc/gb_loop.h);
// the slices are added in slice order through LDS.  No Newton's third law and no atomics.
//   born   : I_i = sum_j H(r, o_i, s_j) -> B_i and dB_i/dI_i
//   pair   : sum_j q_j / f_ij -> the gradient at fixed B, dE/dB_i -- complete in the thread of i, which visits every j -- plus the
//            surface-area term and its dE/dB_i, w_i = dE/dB_i dB_i/dI_i, and (E) the block's energies in double
//   chain  : for atom i over all j, (w_i dH(r, o_i, s_j)/dr + w_j dH(r, o_j, s_i)/dr) / r along x_i - x_j; what becomes of the sum is
//            the caller's epilogue
// pair reads B of every j and chain reads w of every j, which other workgroups write: each pass boundary is a launch boundary.
// MD (the dynamics): a conformation that has stopped (status != running) is neither loaded nor evaluated nor written, as in rs_force.
// Cut (csrc/gb_loop.h; GbNoCut, the default, is the text as it was): under GbCut a pair with gb_r2 >= rc2 adds nothing to any of the
// three sums -- the same fp32 r2 and the same test in all three, before any reciprocal or transcendental -- and a far tile is skipped.
#pragma once
#include <math.h>

#include "common.h"
#include "gb_loop.h"
#include "nb_plan.h"

namespace {

struct GbK {                  // the options as the kernels use them, each rounded once on the host
    float offset, alpha, beta, gamma;
    float kt;                 // K (1/eps_in - 1/eps_out)
    float sa;                 // 4 pi surface_tension
    float probe;
};

struct GbArgs {
    RsGeom q;
    const float* x;           // [N,C,3]
    const float *charge, *radius, *scale;
    GbK k;
    float *B, *dBdI, *w;      // [N,C] in the workspace
    float* gdir;              // [N,C,3]: the gradient at fixed B, written by the pair pass (G), or NULL
    double* part;             // [blocks][C][2]: polar, SA energy of the block's i-atoms (E)
    float* born;              // [N,C] or NULL
    const int* status;        // [B,C] (MD)
};

struct GbShared {
    float4 xs[NB_TJ * NB_CW];      // j coordinates and B_j or w_j: [jj][conformation of the item]
    float4 ps[NB_TJ];              // j parameters: q, o, s
    float red[5][NB_NT];
    int run[NB_CW];
};

struct GbLane {
    RsItem r;
    int JS, NL, s, l, cl, il, i, c;
    bool active, owner;
};

// the thread's place in the workgroup's item, as nb_pairs_kernel and rs_force deal it out; false: the table's item is refused or (MD)
// all of its conformations have stopped.  Every thread of the workgroup calls it (MD: one barrier).
template <bool MD>
__device__ inline bool gb_lane(const GbArgs& a, GbShared& sh, GbLane& w) {
    if (!rs_item(a.q, w.r)) return false;
    if constexpr (MD)
        if (!rs_running(w.r, a.q.C, a.status, sh.run)) return false;
    w.NL = w.r.ni * w.r.nc;
    w.JS = NB_NT / w.NL < NB_JS ? NB_NT / w.NL : NB_JS;
    const int t = threadIdx.x;
    w.s = t / w.NL, w.l = t - w.s * w.NL;
    w.cl = w.l / w.r.ni, w.il = w.l - w.cl * w.r.ni;      // i is the fast index (l < NL: cl < nc)
    w.i = w.r.i0 + w.il, w.c = w.r.c0 + w.cl;
    w.active = w.s < w.JS;
    if constexpr (MD) w.active = w.active && sh.run[w.cl] != 0;
    w.owner = w.active && w.s == 0;
    return true;
}

__device__ __forceinline__ float gb_cut_rc2(const GbNoCut&) { return 0.f; }
__device__ __forceinline__ float gb_cut_rc2(const GbCut& cut) { return cut.c.rc2; }

template <bool MD, class Pass, class Cut>
__device__ __forceinline__ void gb_pass_loop(const GbArgs& a, const GbLane& w, GbShared& sh, Pass& pass, Cut& cut) {
    if constexpr (MD) gb_tile_loop(a.x, w.r, a.q.C, w.s, w.JS, w.i, w.c, w.cl, w.active, sh.run, sh.xs, sh.ps, pass, cut);
    else gb_tile_loop(a.x, w.r, a.q.C, w.s, w.JS, w.i, w.c, w.cl, w.active, nullptr, sh.xs, sh.ps, pass, cut);
}

// r2 of a pair and whether the pair is inside: without a cutoff the expression as it always stood (the compiler contracts it as it
// likes), under one gb_r2 and the test of grappa_gb_cut (a NaN r2 is inside, and is found as a non-finite result)
template <bool CUT>
__device__ __forceinline__ bool gb_inside(float dx, float dy, float dz, float rc2, float& r2) {
    if constexpr (CUT) {
        r2 = gb_r2(dx, dy, dz);
        return !(r2 >= rc2);
    } else {
        r2 = dx * dx + dy * dy + dz * dz;
        return true;
    }
}

// the slices of NV values of one (atom, conformation), added in slice order by the owner (one barrier)
template <int NV>
__device__ inline void gb_slices(const GbLane& w, GbShared& sh, float (&v)[NV]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < NV; ++k) sh.red[k][t] = v[k];
    __syncthreads();
    if (w.owner)
        for (int q = 1; q < w.JS; ++q)
#pragma unroll
            for (int k = 0; k < NV; ++k) v[k] += sh.red[k][q * w.NL + w.l];
}

// ------------------------------------------------------------------------------------------------ born
template <bool CUT>
struct GbBornPass {
    const GbArgs& a;
    float oi, ioi, I;
    float rc2;                    // (CUT)
    __device__ __forceinline__ float4 jatom(int j) const {
        const float o = a.radius[j] - a.k.offset;
        return make_float4(0.f, o, a.scale[j] * o, 0.f);
    }
    __device__ __forceinline__ float jconf(int, int) const { return 0.f; }
    __device__ __forceinline__ void pair(float dx, float dy, float dz, const float4& pj, float) {
        float r2;
        if (!gb_inside<CUT>(dx, dy, dz, rc2, r2)) return;
        const float ir = gb_rsqrt(r2);
        I += gb_h(r2 * ir, ir, oi, ioi, pj.z);
    }
};

// tiles (Cut only): [n_items] or NULL, the tiles the item evaluated -- the same in all three passes, written here
template <bool MD, class Cut = GbNoCut>
__device__ __forceinline__ void gb_born_body(const GbArgs& a, GbShared& sh, Cut cut = Cut{}, int* tiles = nullptr) {
    GbLane w;
    if (!gb_lane<MD>(a, sh, w)) return;
    if constexpr (Cut::on)
        if (!nb_cut_blocks_ok(w.r, a.q.n_blocks)) return;
    const int C = a.q.C;
    const float R = a.radius[w.i], S = a.scale[w.i];
    const float o = R - a.k.offset;
    GbBornPass<Cut::on> pass{a, o, gb_rcp(o), 0.f, gb_cut_rc2(cut)};
    gb_pass_loop<MD>(a, w, sh, pass, cut);
    if constexpr (Cut::on)
        if (tiles && threadIdx.x == 0) tiles[blockIdx.x] = cut.count;
    float v[1] = {pass.I};
    gb_slices(w, sh, v);
    if (w.owner) {
        const GbK& k = a.k;
        const float psi = 0.5f * o * v[0];
        const float P = psi * __builtin_fmaf(psi, __builtin_fmaf(k.gamma, psi, -k.beta), k.alpha);
        const float dP = __builtin_fmaf(psi, __builtin_fmaf(3.0f * k.gamma, psi, -2.0f * k.beta), k.alpha);
        // tanh P and 1 - tanh^2 P from one exponential: the second keeps its relative accuracy where the first saturates
        const float e = expf(-2.0f * fabsf(P));
        const float den = gb_rcp(1.0f + e);
        const float th = copysignf((1.0f - e) * den, P);
        const float sech2 = 4.0f * e * den * den;
        const float iR = gb_rcp(R);
        float B = gb_rcp(pass.ioi - th * iR);
        if (!(o > 0.f && S > 0.f)) B = __builtin_nanf("");      // parameters outside the model: the molecule's results are NaN
        const size_t at = (size_t)w.i * C + w.c;
        a.B[at] = B;
        a.dBdI[at] = B * B * sech2 * dP * (0.5f * o) * iR;
        if (a.born) a.born[at] = B;
    }
}

// ------------------------------------------------------------------------------------------------ pair
template <bool G, bool CUT>
struct GbPairPass {
    const GbArgs& a;
    float qi, Bi;
    float rc2;                    // (CUT)
    float e, db, gx, gy, gz;      // sum q_j / f, sum q_j B_j exp(-D) (1 + D) / f^3, sum q_j (1 - exp(-D)/4) / f^3 (x_i - x_j)
    __device__ __forceinline__ float4 jatom(int j) const { return make_float4(a.charge[j], 0.f, 0.f, 0.f); }
    __device__ __forceinline__ float jconf(int j, int c) const { return a.B[(size_t)j * a.q.C + c]; }
    __device__ __forceinline__ void pair(float dx, float dy, float dz, const float4& pj, float Bj) {
        float r2;
        if (!gb_inside<CUT>(dx, dy, dz, rc2, r2)) return;
        const float P = Bi * Bj;
        const float D = 0.25f * r2 * gb_rcp(P);
        const float ex = expf(-D);
        const float y = gb_rsqrt(__builtin_fmaf(P, ex, r2));      // 1 / f
        const float y3 = y * y * y;
        e = __builtin_fmaf(pj.x, y, e);
        db = __builtin_fmaf(pj.x * Bj, ex * (1.0f + D) * y3, db);
        if constexpr (G) {
            const float f = pj.x * __builtin_fmaf(-0.25f, ex, 1.0f) * y3;
            gx = __builtin_fmaf(f, dx, gx);
            gy = __builtin_fmaf(f, dy, gy);
            gz = __builtin_fmaf(f, dz, gz);
        }
    }
};

// G: the gradient at fixed B -> a.gdir; E: the block's energies -> a.part
template <bool G, bool E, bool MD, class Cut = GbNoCut>
__device__ __forceinline__ void gb_pair_body(const GbArgs& a, GbShared& sh, Cut cut = Cut{}) {
    GbLane w;
    if (!gb_lane<MD>(a, sh, w)) return;
    if constexpr (Cut::on)
        if (!nb_cut_blocks_ok(w.r, a.q.n_blocks)) return;
    const int C = a.q.C;
    const size_t at = (size_t)w.i * C + w.c;
    const float qi = a.charge[w.i], Bi = a.B[at];
    GbPairPass<G, Cut::on> pass{a, qi, Bi, gb_cut_rc2(cut), 0.f, 0.f, 0.f, 0.f, 0.f};
    gb_pass_loop<MD>(a, w, sh, pass, cut);
    float v[5] = {pass.e, pass.db, pass.gx, pass.gy, pass.gz};
    gb_slices(w, sh, v);
    float epol = 0.f, esa = 0.f;
    if (w.owner) {
        const GbK& k = a.k;
        const float R = a.radius[w.i];
        const float iB = gb_rcp(Bi);
        const float kq = k.kt * qi;
        epol = -0.5f * kq * __builtin_fmaf(qi, iB, v[0]);                 // the self term: f_ii = B_i
        const float rb = R * iB, rb2 = rb * rb, rp = R + k.probe;
        esa = k.sa * rp * rp * (rb2 * rb2 * rb2);
        const float dEdB = 0.5f * kq * __builtin_fmaf(qi, iB * iB, v[1]) - 6.0f * esa * iB;
        a.w[at] = dEdB * a.dBdI[at];
        if constexpr (G) {
            float* g = a.gdir + at * 3;
            g[0] = kq * v[2], g[1] = kq * v[3], g[2] = kq * v[4];
        }
    }
    if constexpr (E) {
        __syncthreads();
        if (w.owner) sh.red[0][w.l] = epol, sh.red[1][w.l] = esa;
        __syncthreads();
        if (w.owner && w.il == 0) {
            double sp = 0.0, ss = 0.0;
            for (int k = 0; k < w.r.ni; ++k) {
                sp += (double)sh.red[0][w.cl * w.r.ni + k];
                ss += (double)sh.red[1][w.cl * w.r.ni + k];
            }
            double* o = a.part + ((size_t)w.r.blk * C + w.c) * 2;
            o[0] = sp, o[1] = ss;
        }
    }
}

// ------------------------------------------------------------------------------------------------ chain
template <bool CUT>
struct GbChainPass {
    const GbArgs& a;
    float oi, si, wi;
    float gx, gy, gz;
    float rc2;                    // (CUT)
    __device__ __forceinline__ float4 jatom(int j) const {
        const float o = a.radius[j] - a.k.offset;
        return make_float4(0.f, o, a.scale[j] * o, 0.f);
    }
    __device__ __forceinline__ float jconf(int j, int c) const { return a.w[(size_t)j * a.q.C + c]; }
    __device__ __forceinline__ void pair(float dx, float dy, float dz, const float4& pj, float wj) {
        float r2;
        if (!gb_inside<CUT>(dx, dy, dz, rc2, r2)) return;
        const float ir = gb_rsqrt(r2);
        const float r = r2 * ir, ir2 = ir * ir;
        const float f = __builtin_fmaf(wi, gb_dh(r, ir2, oi, pj.z), wj * gb_dh(r, ir2, pj.y, si)) * ir;
        gx = __builtin_fmaf(f, dx, gx);
        gy = __builtin_fmaf(f, dy, gy);
        gz = __builtin_fmaf(f, dz, gz);
    }
};

// epi(w, gx, gy, gz) runs in EVERY thread of an item that was not refused, after the barrier that follows the slices' words in sh.red
// (the sums are the chain gradient only where w.owner); it may use barriers, and must pass one before it writes sh.red
template <bool MD, class Cut = GbNoCut, class Epi>
__device__ __forceinline__ void gb_chain_body(const GbArgs& a, GbShared& sh, Epi epi, Cut cut = Cut{}) {
    GbLane w;
    if (!gb_lane<MD>(a, sh, w)) return;
    if constexpr (Cut::on)
        if (!nb_cut_blocks_ok(w.r, a.q.n_blocks)) return;
    const size_t at = (size_t)w.i * a.q.C + w.c;
    const float o = a.radius[w.i] - a.k.offset;
    GbChainPass<Cut::on> pass{a, o, a.scale[w.i] * o, a.w[at], 0.f, 0.f, 0.f, gb_cut_rc2(cut)};
    gb_pass_loop<MD>(a, w, sh, pass, cut);
    float v[3] = {pass.gx, pass.gy, pass.gz};
    gb_slices(w, sh, v);
    epi(w, v[0], v[1], v[2]);
}

// ------------------------------------------------------------------------------------------------ host
// the pass workspace: B, dBdI, w [N,C]
struct GbPassWs {
    float *B, *dBdI, *w;
};
inline GbPassWs gb_pass_ws(WsCarve& k, int N, int C) {
    const size_t nc = (size_t)N * (size_t)C;
    GbPassWs p;
    p.B = k.take<float>(nc), p.dBdI = k.take<float>(nc), p.w = k.take<float>(nc);
    return p;
}

// false: the options are refused
inline bool gb_consts(const grappa_gb_desc* gb, GbK& k) {
    if (!gb) return false;
    const float v[8] = {gb->offset, gb->alpha, gb->beta, gb->gamma, gb->eps_in, gb->eps_out, gb->surface_tension, gb->probe};
    for (float f : v)
        if (!isfinite(f)) return false;
    if (!(gb->eps_in > 0.f) || !(gb->eps_out > 0.f) || gb->surface_tension < 0.f || gb->probe < 0.f) return false;
    k.offset = gb->offset, k.alpha = gb->alpha, k.beta = gb->beta, k.gamma = gb->gamma, k.probe = gb->probe;
    k.kt = (float)((138.93545764438198 * 10.0 / 4.184) * (1.0 / (double)gb->eps_in - 1.0 / (double)gb->eps_out));
    k.sa = (float)(4.0 * 3.14159265358979323846 * (double)gb->surface_tension);
    return true;
}

}  // namespace
