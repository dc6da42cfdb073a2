// The tiled all-pairs loop of a work item (csrc/nb_plan.h) for the implicit solvent (include/grappa_hip.h grappa_gb_desc): the tile
// load, the barriers, the slice split and the stopped-conformation mask of nb_pair_loop (csrc/nb_loop.h) without the exception walk --
// GB knows no exceptions -- written ONCE, with the pass (born, pair, chain of csrc/gb_obc.hip) as a policy:
//   float4 P::jatom(j)                       what LDS holds of j-atom j for all conformations
//   float  P::jconf(j, c)                    what it holds of (j, conformation c) beside the coordinates (B_j or w_j; xs[..].w)
//   void   P::pair(dx, dy, dz, pj, wj)       one ordered pair i != j: d = x_i - x_j, pj = jatom(j), wj = jconf(j, c)
// and the formulas every pass shares (gb_lu, gb_h, gb_dh).
// Under a cutoff (include/grappa_hip.h grappa_gb_cut) the loop takes a cut policy, a compile-time choice as nb_pair_loop's is: GbCut
// asks for the verdicts of the item's tiles NB_NT at a time (nb_cut_decide<false> of csrc/nb_cut.h: the boxes alone, GB has no exception range)
// and skips a far tile without loading it or passing its barriers; the pass then drops each pair with gb_r2 >= rc2.  GbNoCut compiles to
// the loop as it was.
#pragma once
#include <type_traits>

#include "common.h"
#include "nb_cut.h"
#include "nb_plan.h"

namespace {

// 1/x and 1/sqrt(x): v_rcp_f32 / v_rsq_f32 are good to 1 ulp; one Newton step brings them to half an ulp (as nb_pair does for 1/r)
__device__ __forceinline__ float gb_rcp(float x) {
    const float y = __builtin_amdgcn_rcpf(x);
    return __builtin_fmaf(__builtin_fmaf(-x, y, 1.0f), y, y);
}
__device__ __forceinline__ float gb_rsqrt(float x) {
    const float y = __builtin_amdgcn_rsqf(x);
    return __builtin_fmaf(0.5f * y, __builtin_fmaf(-x * y, y, 1.0f), y);
}

// the integration limits of H(r, o_i, s_j) as l = 1/L, u = 1/(r + s_j); false: j's sphere lies inside atom i, H = 0 (a NaN r is
// evaluated and comes out as NaN)
__device__ __forceinline__ bool gb_lu(float r, float oi, float sj, float& L, float& l, float& u) {
    const float rs = r + sj;
    if (oi >= rs) return false;
    L = fmaxf(oi, fabsf(r - sj));
    l = gb_rcp(L);
    u = gb_rcp(rs);
    return true;
}

// H(r, o_i, s_j) with ir = 1/r; ioi = 1/o_i
__device__ __forceinline__ float gb_h(float r, float ir, float oi, float ioi, float sj) {
    float L, l, u;
    if (!gb_lu(r, oi, sj, L, l, u)) return 0.f;
    const float d2 = (l - u) * (l + u);      // l^2 - u^2
    float h = (l - u) - 0.25f * r * d2 + 0.5f * ir * logf(L * u) + 0.25f * sj * sj * ir * d2;
    if (oi < sj - r) h += 2.0f * (ioi - l);
    return h;
}

// dH(r, o_i, s_j)/dr with ir2 = 1/r^2
__device__ __forceinline__ float gb_dh(float r, float ir2, float oi, float sj) {
    float L, l, u;
    if (!gb_lu(r, oi, sj, L, l, u)) return 0.f;
    const float d2 = (l - u) * (l + u);
    return -0.25f * d2 * __builtin_fmaf(sj * sj, ir2, 1.0f) - 0.5f * ir2 * logf(L * u);
}

// ------------------------------------------------------------------------------------------------ the cutoff
// r2 of a pair as ALL THREE passes form it under a cutoff, products and sums rounded one by one in this order (no contraction: the
// compiler may not fuse these), so that born, pair and chain agree on which pairs are inside: r2 serves the test and the pair's arithmetic
__device__ __forceinline__ float gb_r2(float dx, float dy, float dz) {
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

struct GbCutDev {
    float rc2;               // (float)((double)rc * rc): a pair is inside unless r2 >= rc2
    float thr;               // rc2 (1 + 2^-18), as nb_cut_consts forms it
    int prune;
    const float4* box;       // [n_blocks][C][2], written by the launch before the first pass (gb_cut_boxes)
};

struct GbNoCut {
    static constexpr bool on = false;
};
struct GbCut {
    static constexpr bool on = true;
    GbCutDev c;
    unsigned char* near;      // NB_NT bytes of LDS for the verdicts
    int count;                // tiles evaluated (the same in every thread of the workgroup)
};

// the options as the ABI states them (comparisons written so that a NaN is refused) -> the constants, each rounded once from double
inline bool gb_cut_consts(const grappa_gb_cut* o, GbCutDev& c) {
    if (!o) return false;
    const double rc = o->cutoff;
    if (!(rc > 0.0 && rc <= FLT_MAX) || (o->prune != 0 && o->prune != 1)) return false;
    c.rc2 = (float)(rc * rc);
    if (!(c.rc2 <= FLT_MAX)) return false;
    c.thr = (float)((double)c.rc2 * (1.0 + 1.0 / 262144.0));
    c.prune = o->prune;
    c.box = nullptr;
    return true;
}

// The box half of nb_cut_box_range: the boxes of the item's (block, conformations) at x [N,C,3].  Every thread of the item's workgroup
// calls it.
__device__ inline void gb_cut_boxes(const RsItem& r, int C, const float* __restrict__ x, float4* box) {
    __shared__ float bx[NB_NT * 3];
    const int t = threadIdx.x;
    if (t < r.ni * r.nc) {
        const int cl = t / r.ni, il = t - cl * r.ni;
        const float* p = x + ((size_t)(r.i0 + il) * C + r.c0 + cl) * 3;
        bx[3 * t] = p[0], bx[3 * t + 1] = p[1], bx[3 * t + 2] = p[2];
    }
    nb_cut_box_write(bx, nullptr, r.ni, r.nc, r.blk, C, r.c0, box);
}

// Every thread of the item's workgroup calls it (barriers inside); the thread is slice s of JS of (atom i, conformation c = r.c0 + cl)
// and takes part in the pairs iff `active`.  x: the coordinates [N,C,3]; run: as in nb_pair_loop (an int array in LDS, or the literal
// nullptr: all conformations run).  xs, ps: NB_TJ * NB_CW and NB_TJ float4 of LDS.  The pairs of the thread's slice reach pass.pair in
// ascending j.  Cut: GbNoCut, or GbCut with its block numbers checked by nb_cut_blocks_ok before the call; cut.count gains the tiles
// evaluated.
template <class Pass, class Run, class Cut>
__device__ __forceinline__ void gb_tile_loop(const float* __restrict__ x, const RsItem& r, int C, int s, int JS, int i, int c, int cl, bool active,
                                             Run run, float4* xs, float4* ps, Pass& pass, Cut& cut) {
    constexpr bool masked = !std::is_null_pointer<Run>::value;
    const int t = threadIdx.x, m0 = r.m0, m1 = r.m1, c0 = r.c0, nc = r.nc;
    float xi = 0.f, yi = 0.f, zi = 0.f;
    if (active) {
        const float* p = x + ((size_t)i * C + c) * 3;
        xi = p[0], yi = p[1], zi = p[2];
    }
    [[maybe_unused]] const int ntiles = nb_tiles(r), kb0 = nb_first_block(r);      // (read by the cut policy only)
    for (int j0 = m0; j0 < m1; j0 += NB_TJ) {
        if constexpr (Cut::on) {      // NB_NT verdicts at a time; a far tile loads nothing and passes no barrier of the tile
            const int jt = (j0 - m0) / NB_TJ, k = jt & (NB_NT - 1);
            if (k == 0) {
                if constexpr (masked) nb_cut_decide<false>(cut.c, C, r.blk, kb0, ntiles, jt, c0, nc, run, cut.near);
                else nb_cut_decide<false>(cut.c, C, r.blk, kb0, ntiles, jt, c0, nc, nullptr, cut.near);
            }
            if (!cut.near[k]) continue;
            ++cut.count;
        }
        const int nj = m1 - j0 < NB_TJ ? m1 - j0 : NB_TJ;
        __syncthreads();
        for (int idx = t; idx < nj * nc; idx += NB_NT) {
            const int jj = idx / nc, cc = idx - jj * nc;
            if constexpr (masked)
                if (!run[cc]) continue;
            const float* p = x + ((size_t)(j0 + jj) * C + c0 + cc) * 3;
            xs[jj * NB_CW + cc] = make_float4(p[0], p[1], p[2], pass.jconf(j0 + jj, c0 + cc));
        }
        if (t < nj) ps[t] = pass.jatom(j0 + t);
        __syncthreads();
        if (active) {
            for (int jj = s; jj < nj; jj += JS) {
                if (j0 + jj == i) continue;
                const float4 xj = xs[jj * NB_CW + cl];
                pass.pair(xi - xj.x, yi - xj.y, zi - xj.z, ps[jj], xj.w);
            }
        }
    }
}

}  // namespace
