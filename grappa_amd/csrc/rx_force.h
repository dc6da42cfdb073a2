// The force evaluation of the fused kernels that keep one molecule in one workgroup (csrc/relax.hip, csrc/dynamics.hip): the LDS image of
// a molecule, the bonded gather and the pair loop of one (atom, slice), and the fixed-order workgroup reductions.
#pragma once
#include <limits.h>

#include "common.h"
#include "mm_geom.h"
#include "nb_pair.h"

namespace {

constexpr int RX_MAX = 512;               // atoms per molecule at most
constexpr int RX_NT = 256;                // threads per workgroup
constexpr int RX_JS = 16;                 // slices per atom at most
constexpr int RX_APT = RX_MAX / RX_NT;    // atoms per owner thread at most
constexpr int RX_NW = RX_NT / GRAPPA_WAVE;
constexpr int RX_STEP_CAP = 1000000;

struct RxShared {
    float4 xs[RX_MAX];              // x, y, z, q
    float2 ps[RX_MAX];              // sigma / 2, sqrt(eps)
    float part[3 * RX_MAX];         // partial gradients [xyz][slice * n + atom]; at the end: energy partials [6][RX_NT]
    float wred[5][RX_NW];
    float wmax[RX_NW];
    double esum[6];
};

__device__ inline int rx_clamp(int v, int N) { return v < 0 ? 0 : (v > N ? N : v); }

// an atom of the molecule by its batch-global index (an index outside the molecule -- a table of another batch -- reads atom 0)
__device__ inline V3 rx_ld(const RxShared& sh, int atom, int m0, int n) {
    const unsigned a = (unsigned)(atom - m0);
    const float4 p = sh.xs[a < (unsigned)n ? a : 0u];
    return {p.x, p.y, p.z};
}

// slice s of the bonded gradient of atom i
__device__ inline V3 rx_bonded(const grappa_mm_desc& d, const RxShared& sh, int i, int s, int JS, int m0, int n) {
    V3 g = {0.f, 0.f, 0.f};
    const int i0 = d.inc_ptr[i], i1 = d.inc_ptr[i + 1];
    for (int q = i0 + s; q < i1; q += JS) {
        const int code = d.inc_code[q];
        const int pos = code & 3, l = (code >> 2) & 3, t = code >> 4;
        if (l == 0) {
            V3 u;
            const float r = bond_geom(rx_ld(sh, d.idx[0][2 * t], m0, n), rx_ld(sh, d.idx[0][2 * t + 1], m0, n), u);
            const float coef = d.k[0][t] * (r - d.eq[0][t]);
            g = g + (pos == 0 ? coef : -coef) * u;
        } else if (l == 1) {
            V3 e0, e2;
            const float th = angle_geom(rx_ld(sh, d.idx[1][3 * t], m0, n), rx_ld(sh, d.idx[1][3 * t + 1], m0, n),
                                        rx_ld(sh, d.idx[1][3 * t + 2], m0, n), e0, e2);
            const float coef = d.k[1][t] * (th - d.eq[1][t]);
            const V3 dv = pos == 0 ? e0 : (pos == 2 ? e2 : (-1.0f) * (e0 + e2));
            g = g + coef * dv;
        } else {
            V3 d0, d1, d2, d3;
            const int* id = d.idx[l] + 4 * (size_t)t;
            const float phi = dihedral_geom(rx_ld(sh, id[0], m0, n), rx_ld(sh, id[1], m0, n), rx_ld(sh, id[2], m0, n), rx_ld(sh, id[3], m0, n),
                                            d0, d1, d2, d3);
            const float coef = torsion_dcoef(d.k[l] + (size_t)t * d.n_per[l], d.n_per[l], phi);
            const V3 dv = pos == 0 ? d0 : (pos == 1 ? d1 : (pos == 2 ? d2 : d3));
            g = g + coef * dv;
        }
    }
    return g;
}

// slice s of the pair sums of atom i = m0 + il: j = m0 + s, m0 + s + JS, .. ascending
__device__ inline void rx_pairs(const grappa_nb_desc& d, const RxShared& sh, int il, int s, int JS, int m0, int n, float& elj, float& ec,
                                float& gx, float& gy, float& gz) {
    const int i = m0 + il;
    const float4 pi = sh.xs[il];
    const float2 qi = sh.ps[il];
    const float kq = NB_K * pi.w, hs = qi.x, se = 4.0f * qi.y;
    int ep = d.exc_ptr[i];
    const int ee = d.exc_ptr[i + 1];
    int nx = ep < ee ? d.exc_atom[ep] : INT_MAX;
    for (int jl = s; jl < n; jl += JS) {
        const int j = m0 + jl;
        while (nx < j) {
            ++ep;
            nx = ep < ee ? d.exc_atom[ep] : INT_MAX;
        }
        const float4 pj = sh.xs[jl];
        const float2 qj = sh.ps[jl];
        float sij = hs + qj.x, e4 = se * qj.y, kqq = kq * pj.w;
        bool skip = j == i;
        if (nx == j) {
            const float q = d.exc_qq[ep], e = d.exc_eps[ep];
            sij = d.exc_sigma[ep];
            e4 = 4.0f * e;
            kqq = NB_K * q;
            skip = skip || (q == 0.f && e == 0.f);
        }
        if (!skip) nb_pair(pi.x - pj.x, pi.y - pj.y, pi.z - pj.z, sij, e4, kqq, elj, ec, gx, gy, gz);
    }
}

// two maxima and three sums over the workgroup, in a fixed order; every thread gets the same bits.  One barrier.
__device__ inline void rx_reduce(float& m0, float& m1, float& s0, float& s1, float& s2, float (*w)[RX_NW]) {
#pragma unroll
    for (int o = GRAPPA_WAVE / 2; o > 0; o >>= 1) {
        m0 = fmaxf(m0, __shfl_xor(m0, o, GRAPPA_WAVE));
        m1 = fmaxf(m1, __shfl_xor(m1, o, GRAPPA_WAVE));
        s0 += __shfl_xor(s0, o, GRAPPA_WAVE);
        s1 += __shfl_xor(s1, o, GRAPPA_WAVE);
        s2 += __shfl_xor(s2, o, GRAPPA_WAVE);
    }
    const int wave = threadIdx.x / GRAPPA_WAVE;
    if ((threadIdx.x & (GRAPPA_WAVE - 1)) == 0) w[0][wave] = m0, w[1][wave] = m1, w[2][wave] = s0, w[3][wave] = s1, w[4][wave] = s2;
    __syncthreads();
    m0 = w[0][0], m1 = w[1][0], s0 = w[2][0], s1 = w[3][0], s2 = w[4][0];
#pragma unroll
    for (int k = 1; k < RX_NW; ++k) {
        m0 = fmaxf(m0, w[0][k]);
        m1 = fmaxf(m1, w[1][k]);
        s0 += w[2][k];
        s1 += w[3][k];
        s2 += w[4][k];
    }
}

// one maximum over the workgroup, the same way.  One barrier.
__device__ inline float rx_reduce_max(float m, float* w) {
#pragma unroll
    for (int o = GRAPPA_WAVE / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, GRAPPA_WAVE));
    if ((threadIdx.x & (GRAPPA_WAVE - 1)) == 0) w[threadIdx.x / GRAPPA_WAVE] = m;
    __syncthreads();
    m = w[0];
#pragma unroll
    for (int k = 1; k < RX_NW; ++k) m = fmaxf(m, w[k]);
    return m;
}

}  // namespace
