// The tiled all-pairs loop of a work item (csrc/nb_plan.h) for the implicit solvent (include/grappa_hip.h grappa_gb_desc): the tile
// load, the barriers, the slice split and the stopped-conformation mask of nb_pair_loop (csrc/nb_loop.h) without the exception walk --
// GB knows no exceptions -- written ONCE, with the pass (born, pair, chain of csrc/gb_obc.hip) as a policy:
//   float4 P::jatom(j)                       what LDS holds of j-atom j for all conformations
//   float  P::jconf(j, c)                    what it holds of (j, conformation c) beside the coordinates (B_j or w_j; xs[..].w)
//   void   P::pair(dx, dy, dz, pj, wj)       one ordered pair i != j: d = x_i - x_j, pj = jatom(j), wj = jconf(j, c)
// and the formulas every pass shares (gb_lu, gb_h, gb_dh).
#pragma once
#include <type_traits>

#include "common.h"
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

// Every thread of the item's workgroup calls it (barriers inside); the thread is slice s of JS of (atom i, conformation c = r.c0 + cl)
// and takes part in the pairs iff `active`.  x: the coordinates [N,C,3]; run: as in nb_pair_loop (an int array in LDS, or the literal
// nullptr: all conformations run).  xs, ps: NB_TJ * NB_CW and NB_TJ float4 of LDS.  The pairs of the thread's slice reach pass.pair in
// ascending j.
template <class Pass, class Run>
__device__ __forceinline__ void gb_tile_loop(const float* __restrict__ x, const RsItem& r, int C, int s, int JS, int i, int c, int cl, bool active,
                                             Run run, float4* xs, float4* ps, Pass& pass) {
    constexpr bool masked = !std::is_null_pointer<Run>::value;
    const int t = threadIdx.x, m0 = r.m0, m1 = r.m1, c0 = r.c0, nc = r.nc;
    float xi = 0.f, yi = 0.f, zi = 0.f;
    if (active) {
        const float* p = x + ((size_t)i * C + c) * 3;
        xi = p[0], yi = p[1], zi = p[2];
    }
    for (int j0 = m0; j0 < m1; j0 += NB_TJ) {
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
