// The core of the fused kernels that keep one molecule in one workgroup (csrc/relax.hip, csrc/dynamics.hip): the LDS image of a molecule
// and the workgroup's item, the gradient of the coordinates held (the bonded gather and the pair loop of one (atom, slice), the owner's
// sum over the slices), the six energy terms, and the fixed-order workgroup reductions.
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
    return bonded_gather(d, d.inc_ptr[i] + s, d.inc_ptr[i + 1], JS, [&](int atom) { return rx_ld(sh, atom, m0, n); });
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

// the workgroup's item: molecule b in conformation c, its atoms m0 .. m0 + n, and the thread's (atom, slice): up to 256 atoms one unit
// per thread in JS slices (thread t: slice s of atom il0, active if s < JS), above that one slice and RX_APT atoms per thread
struct RxItem {
    int b, c;
    size_t item;
    int m0, n, JS, s, il0;
    bool active;
};

// fills w and loads the molecule into sh.xs / sh.ps (no barrier: the caller's comes before the first read).  false: nothing to run --
// a molecule without atoms, or one above the size limit (status 3 and nothing else)
__device__ inline bool rx_begin(const grappa_mm_desc& d, const grappa_nb_desc& nb, int has_nb, int* status, RxShared& sh, RxItem& w) {
    const int C = d.C, t = threadIdx.x;
    w.b = (int)(blockIdx.x / (unsigned)C), w.c = (int)(blockIdx.x - (unsigned)w.b * (unsigned)C);
    w.item = (size_t)w.b * C + w.c;
    w.m0 = rx_clamp(d.atom_molptr[w.b], d.N);
    const int n = rx_clamp(d.atom_molptr[w.b + 1], d.N) - w.m0, m0 = w.m0;
    w.n = n;
    if (n <= 0) return false;
    if (n > RX_MAX) {
        if (t == 0) status[w.item] = 3;
        return false;
    }
    for (int il = t; il < n; il += RX_NT) {
        const float* p = d.xyz + ((size_t)(m0 + il) * C + w.c) * 3;
        sh.xs[il] = make_float4(p[0], p[1], p[2], has_nb ? nb.charge[m0 + il] : 0.f);
        sh.ps[il] = has_nb ? make_float2(0.5f * nb.sigma[m0 + il], sqrtf(nb.epsilon[m0 + il])) : make_float2(0.f, 0.f);
    }
    w.JS = n > RX_NT ? 1 : (RX_NT / n < RX_JS ? RX_NT / n : RX_JS);
    w.s = n > RX_NT ? 0 : t / n;
    w.il0 = t - w.s * n;
    w.active = w.s < w.JS;
    return true;
}

// g = grad E at the coordinates in LDS, into the owners' registers: the partial gradient of every (atom, slice), a barrier, the owner adds
// the slices in slice order and hands each of its atoms' gradients to each(k, g[k]) (what a caller tests or accumulates per atom, in
// the same pass).  One barrier; sh.part is read after it, so another must pass before it is written again.
template <class Each>
__device__ __forceinline__ void rx_gradient(const grappa_mm_desc& d, const grappa_nb_desc& nb, int has_nb, RxShared& sh, const RxItem& w,
                                            V3 (&g)[RX_APT], Each each) {
    const int t = threadIdx.x, n = w.n;
    if (w.active)
        for (int il = w.il0; il < n; il += RX_NT) {
            V3 p = rx_bonded(d, sh, w.m0 + il, w.s, w.JS, w.m0, n);
            if (has_nb) {
                float elj = 0.f, ec = 0.f;
                rx_pairs(nb, sh, il, w.s, w.JS, w.m0, n, elj, ec, p.x, p.y, p.z);
            }
            const int u = w.s * n + il;
            sh.part[u] = p.x, sh.part[RX_MAX + u] = p.y, sh.part[2 * RX_MAX + u] = p.z;
        }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RX_APT; ++k) {
        const int il = t + k * RX_NT;
        if (il < n) {
            V3 gi = {sh.part[il], sh.part[RX_MAX + il], sh.part[2 * RX_MAX + il]};
            for (int q = 1; q < w.JS; ++q) {
                const int u = q * n + il;
                gi.x += sh.part[u], gi.y += sh.part[RX_MAX + u], gi.z += sh.part[2 * RX_MAX + u];
            }
            g[k] = gi;
            each(k, gi);
        }
    }
}

// The potential energy at the coordinates in LDS: the six terms as thread partials in fp32 (a thread's tuples t, t + 256, .. and the pairs
// of its (atom, slice)), added in double in thread order -> sh.esum (every pair was counted from both of its atoms); their sum in thread 0.
// A caller with one more sum to form hands it to the same two barriers: its thread partial `extra` goes through extra_part[RX_NT] and
// thread 6 adds them the same way into *extra_sum (extra_part = NULL: none).
// (Thread 6 because threads 0 .. 5 each add one of the six terms; *extra_sum holds the plain sum, any scaling is the caller's, and it
// may be read only after this function returns, that is after the second barrier.)
// sh.part must be free: every reader of the last partial gradients has passed a barrier.  Two barriers.
__device__ __forceinline__ double rx_energies(const grappa_mm_desc& d, const grappa_nb_desc& nb, int has_nb, RxShared& sh, const RxItem& w,
                                              float extra = 0.f, float* extra_part = nullptr, double* extra_sum = nullptr) {
    const int t = threadIdx.x, b = w.b, n = w.n;
    const auto ld = [&](int atom) { return rx_ld(sh, atom, w.m0, n); };
    float e[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, x;
    for (int tt = d.mol_ptr[0][b] + t; tt < d.mol_ptr[0][b + 1]; tt += RX_NT) e[0] += bonded_tuple_energy(d, 0, tt, ld, x);
    for (int tt = d.mol_ptr[1][b] + t; tt < d.mol_ptr[1][b + 1]; tt += RX_NT) e[1] += bonded_tuple_energy(d, 1, tt, ld, x);
    for (int l = 2; l < 4; ++l)
        for (int tt = d.mol_ptr[l][b] + t; tt < d.mol_ptr[l][b + 1]; tt += RX_NT) e[l] += bonded_tuple_energy(d, l, tt, ld, x);
    if (has_nb && w.active)
        for (int il = w.il0; il < n; il += RX_NT) {
            float gx = 0.f, gy = 0.f, gz = 0.f;
            rx_pairs(nb, sh, il, w.s, w.JS, w.m0, n, e[4], e[5], gx, gy, gz);
        }
#pragma unroll
    for (int q = 0; q < 6; ++q) sh.part[q * RX_NT + t] = e[q];
    if (extra_part) extra_part[t] = extra;
    __syncthreads();
    if (t < 6) {
        double sum = 0.0;
        for (int k = 0; k < RX_NT; ++k) sum += (double)sh.part[t * RX_NT + k];
        sh.esum[t] = t < 4 ? sum : 0.5 * sum;
    } else if (t == 6 && extra_part) {
        double sum = 0.0;
        for (int k = 0; k < RX_NT; ++k) sum += (double)extra_part[k];
        *extra_sum = sum;
    }
    __syncthreads();
    double tot = 0.0;
    if (t == 0)
        for (int q = 0; q < 6; ++q) tot += sh.esum[q];
    return tot;
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
