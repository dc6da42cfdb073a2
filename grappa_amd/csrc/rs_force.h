// A molecule spread over many workgroups: the work items of the nonbonded plan (csrc/nb_plan.h) as csrc/relax_steps.hip and
// csrc/dynamics_steps.hip walk them, and the one-launch force of that decomposition, shared by both.
//   item   : (molecule, block of ni <= 64 i-atoms, nc conformations), one workgroup of NB_NT threads; rs_item refuses a table made for
//            another batch.
//   force  : rs_force computes g = grad E(x) of the item's (atom, conformation) pairs: bonded_gather of csrc/mm_geom.h, as in
//            mm_gradient_kernel (the thread's slice of the atom's incidences, neighbours read from global memory) plus the j loop of
//            nb_pairs_kernel (j-atoms through LDS in ascending blocks of 64, the sorted exception row walked in step with j, an exception
//            replaces the pair, an exclusion or j == i is skipped, no pair energy kept), slices added in slice order.  What a kernel does
//            with the gradient of an (atom, conformation) -- the minimiser's partials, the integrator's closing kick -- is its epilogue,
//            a functor, the way rx_gradient of csrc/rx_force.h takes one.  A compile-time cut policy (csrc/nb_cut.h) chooses between
//            all pairs and a cutoff with tile pruning; there is one definition of the loop for both.
// The workgroup reads x of the whole molecule and the status of its own conformations; it writes nothing itself.
#pragma once
#include <limits.h>

#include "common.h"
#include "mm_geom.h"
#include "nb_cut.h"
#include "nb_pair.h"
#include "nb_plan.h"

namespace {

constexpr int RS_RUNNING = -1;           // status in the workspace while an item runs

struct RsGeom {                          // what every per-block kernel needs of the batch
    int N, C, B, n_blocks;
    const int* atom_molptr;
    const int* blk_ptr;                  // [B+1]
    const int4* items;
};

struct RsItem {
    int mol, i0, blk, c0, m0, m1, ni, nc;
};

// the workgroup's item, checked as nb_pairs_kernel checks it (a table made for another batch is walked away from, not followed)
__device__ inline bool rs_item(const RsGeom& q, RsItem& r) {
    const int4 it = q.items[blockIdx.x];
    r.mol = it.x, r.i0 = it.y, r.blk = it.z, r.c0 = it.w;
    if (r.mol < 0 || r.mol >= q.B || r.blk < 0 || r.blk >= q.n_blocks || r.c0 < 0 || r.c0 >= q.C) return false;
    r.m0 = nb_clamp(q.atom_molptr[r.mol], q.N), r.m1 = nb_clamp(q.atom_molptr[r.mol + 1], q.N);
    if (r.i0 < r.m0 || r.i0 >= r.m1) return false;
    r.ni = r.m1 - r.i0 < NB_T ? r.m1 - r.i0 : NB_T;
    int nch, ncb;
    nb_chunks(r.ni, q.C, nch, ncb);
    r.nc = q.C - r.c0 < ncb ? q.C - r.c0 : ncb;      // (ni * nc <= NB_NT and nc <= NB_CW by nb_chunks)
    return true;
}

// which of the item's conformations still run -> run[0 .. nc); false if none does.  One barrier.
__device__ inline bool rs_running(const RsItem& r, int C, const int* __restrict__ status, int* run) {
    if ((int)threadIdx.x < r.nc) run[threadIdx.x] = status[(size_t)r.mol * C + r.c0 + threadIdx.x] == RS_RUNNING;
    __syncthreads();
    int any = 0;
    for (int cc = 0; cc < r.nc; ++cc) any |= run[cc];
    return any != 0;
}

inline RsGeom rs_geom(const grappa_mm_desc* mm, const int* table_dev, int n_blocks) {
    RsGeom q;
    q.N = mm->N, q.C = mm->C, q.B = mm->B, q.n_blocks = n_blocks;
    q.atom_molptr = mm->atom_molptr;
    q.blk_ptr = table_dev + 4;
    q.items = (const int4*)(table_dev + 4 + (((size_t)mm->B + 1 + 3) & ~(size_t)3));
    return q;
}

struct RsForceIn {
    grappa_mm_desc mm;       // tables only: mm.xyz is not read
    grappa_nb_desc nb;       // tables only
    int has_nb;
    RsGeom q;
    const float* x;          // [N,C,3]
    const int* status;       // [B,C]
};

inline RsForceIn rs_force_in(const grappa_mm_desc* mm, const grappa_nb_desc* nb, const RsGeom& q, const float* x, const int* status) {
    RsForceIn f;
    f.mm = *mm;
    f.mm.xyz = nullptr;
    f.has_nb = nb != nullptr;
    if (nb) f.nb = *nb; else f.nb = grappa_nb_desc{};
    f.nb.xyz = nullptr;
    f.q = q;
    f.x = x, f.status = status;
    return f;
}

struct RsShared {
    float4 xs[NB_TJ * NB_CW];      // j coordinates: [jj][conformation of the item]
    float4 ps[NB_TJ];              // j parameters: q, sigma / 2, sqrt(eps)
    float red[4][NB_NT];
    int run[NB_CW];
};

struct RsLane {                    // the thread's (atom, conformation) of the item
    int l, il, cl, i, c;           // l = cl * ni + il; atom i = i0 + il, conformation c = c0 + cl
    bool owner;                    // the thread that holds the gradient of (i, c); false for a conformation that has stopped
};

__device__ inline V3 rs_ld(const float* __restrict__ x, int atom, int N, int C, int c) {      // (an index outside the batch reads atom 0)
    return ldv(x, (unsigned)atom < (unsigned)N ? atom : 0, C, c);
}

// slice s of the bonded gradient of atom i in conformation c
__device__ inline V3 rs_bonded(const grappa_mm_desc& d, const float* __restrict__ x, int i, int s, int JS, int c) {
    return bonded_gather(d, d.inc_ptr[i] + s, d.inc_ptr[i + 1], JS, [&](int atom) { return rs_ld(x, atom, d.N, d.C, c); });
}

// The item's force.  Cut is the compile-time cut policy of csrc/nb_cut.h: NbNoCut is the all-pairs force; NbCut evaluates a pair that is
// no exception with nb_pair_cut and skips the tiles the rule of csrc/nb_cut.h calls far.  Every thread of the workgroup calls it; false: the table's item was refused or all of its conformations have
// stopped, nothing was done and epi was not called.  Otherwise epi(r, w, g) runs in EVERY thread after the barrier that follows the slices' words in
// sh.red (g is the gradient only where w.owner); it may use barriers, and must pass one before it writes sh.red.
template <class Cut, class Epi>
__device__ __forceinline__ bool rs_force(const RsForceIn& a, RsShared& sh, const Cut& cut, Epi epi) {
    RsItem r;
    if (!rs_item(a.q, r)) return false;
    const int C = a.q.C;
    if (!rs_running(r, C, a.status, sh.run)) return false;      // every conformation of the item has stopped: nothing of it is touched
    if constexpr (Cut::on) {      // the boxes of the molecule's blocks are read: a table whose block numbers do not fit is walked away from
        const int kb0 = r.blk - (r.i0 - r.m0) / NB_T;
        if (kb0 < 0 || kb0 + (r.m1 - r.m0 + NB_TJ - 1) / NB_TJ > a.q.n_blocks) return false;
    }
    const int ni = r.ni, nc = r.nc, i0 = r.i0, c0 = r.c0, m0 = r.m0, m1 = r.m1;
    const int NL = ni * nc;
    const int JS = NB_NT / NL < NB_JS ? NB_NT / NL : NB_JS;
    const int t = threadIdx.x, s = t / NL, l = t - s * NL;
    const int cl = l / ni, il = l - cl * ni;      // (l < NL: cl < nc)
    const int i = i0 + il, c = c0 + cl;
    const bool active = s < JS && sh.run[cl] != 0;

    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (active) {
        const V3 p = rs_bonded(a.mm, a.x, i, s, JS, c);
        gx = p.x, gy = p.y, gz = p.z;
    }
    if (a.has_nb) {
        const grappa_nb_desc& d = a.nb;
        float xi = 0.f, yi = 0.f, zi = 0.f, kq = 0.f, hs = 0.f, se = 0.f;
        int ep = 0, ee = 0, nx = INT_MAX;
        if (active) {
            const float* p = a.x + ((size_t)i * C + c) * 3;
            xi = p[0], yi = p[1], zi = p[2];
            kq = NB_K * d.charge[i];
            hs = 0.5f * d.sigma[i];
            se = 4.0f * sqrtf(d.epsilon[i]);
            ep = d.exc_ptr[i];
            ee = d.exc_ptr[i + 1];
            nx = ep < ee ? d.exc_atom[ep] : INT_MAX;
        }
        float elj = 0.f, ec = 0.f;      // (no pair energy is kept: dead code to the compiler)
        [[maybe_unused]] const int ntiles = (m1 - m0 + NB_TJ - 1) / NB_TJ, kb0 = r.blk - (i0 - m0) / NB_T;      // (read by the cut policy only)
        for (int j0 = m0; j0 < m1; j0 += NB_TJ) {
            if constexpr (Cut::on) {      // NB_NT verdicts at a time; a far tile loads nothing and passes no barrier of the tile
                const int jt = (j0 - m0) / NB_TJ, k = jt & (NB_NT - 1);
                if (k == 0) nb_cut_decide(cut.c, C, r.blk, kb0, ntiles, jt, c0, nc, sh.run, cut.near);
                if (!cut.near[k]) continue;
            }
            const int nj = m1 - j0 < NB_TJ ? m1 - j0 : NB_TJ;
            __syncthreads();
            for (int idx = t; idx < nj * nc; idx += NB_NT) {
                const int jj = idx / nc, cc = idx - jj * nc;
                if (sh.run[cc]) {
                    const float* p = a.x + ((size_t)(j0 + jj) * C + c0 + cc) * 3;
                    sh.xs[jj * NB_CW + cc] = make_float4(p[0], p[1], p[2], 0.f);
                }
            }
            if (t < nj) sh.ps[t] = make_float4(d.charge[j0 + t], 0.5f * d.sigma[j0 + t], sqrtf(d.epsilon[j0 + t]), 0.f);
            __syncthreads();
            const bool lookup = active && ((i >= j0 && i < j0 + nj) || nx < j0 + nj);
            if (__builtin_amdgcn_ballot_w64(lookup) != 0) {
                if (active) {
                    for (int jj = s; jj < nj; jj += JS) {
                        const int j = j0 + jj;
                        const float4 p = sh.ps[jj];
                        float sij = hs + p.y, e4 = se * p.z, kqq = kq * p.x;
                        bool skip = j == i;
                        while (nx < j) {
                            ++ep;
                            nx = ep < ee ? d.exc_atom[ep] : INT_MAX;
                        }
                        bool exc = false;      // (read by the cut policy only)
                        if (nx == j) {
                            const float q = d.exc_qq[ep], e = d.exc_eps[ep];
                            exc = true;
                            sij = d.exc_sigma[ep];
                            e4 = 4.0f * e;
                            kqq = NB_K * q;
                            skip = skip || (q == 0.f && e == 0.f);
                            ++ep;
                            nx = ep < ee ? d.exc_atom[ep] : INT_MAX;
                        }
                        if (!skip) {
                            const float4 x = sh.xs[jj * NB_CW + cl];
                            if constexpr (Cut::on) {      // an exception is not cut
                                if (exc) nb_pair(xi - x.x, yi - x.y, zi - x.z, sij, e4, kqq, elj, ec, gx, gy, gz);
                                else nb_pair_cut(xi - x.x, yi - x.y, zi - x.z, sij, e4, kqq, cut.c.k, elj, ec, gx, gy, gz);
                            } else {
                                nb_pair(xi - x.x, yi - x.y, zi - x.z, sij, e4, kqq, elj, ec, gx, gy, gz);
                            }
                        }
                    }
                    while (nx < j0 + nj) {      // partners that belong to other slices
                        ++ep;
                        nx = ep < ee ? d.exc_atom[ep] : INT_MAX;
                    }
                }
            } else if (active) {
#pragma unroll 4
                for (int jj = s; jj < nj; jj += JS) {
                    const float4 p = sh.ps[jj];
                    const float4 x = sh.xs[jj * NB_CW + cl];
                    if constexpr (Cut::on) nb_pair_cut(xi - x.x, yi - x.y, zi - x.z, hs + p.y, se * p.z, kq * p.x, cut.c.k, elj, ec, gx, gy, gz);
                    else nb_pair(xi - x.x, yi - x.y, zi - x.z, hs + p.y, se * p.z, kq * p.x, elj, ec, gx, gy, gz);
                }
            }
        }
    }
    // the slices of one (atom, conformation), added in slice order
    sh.red[0][t] = gx, sh.red[1][t] = gy, sh.red[2][t] = gz;
    __syncthreads();
    const RsLane w = {l, il, cl, i, c, active && s == 0};
    if (w.owner) {
        for (int q = 1; q < JS; ++q) {
            const int o = q * NL + l;
            gx += sh.red[0][o], gy += sh.red[1][o], gz += sh.red[2][o];
        }
    }
    epi(r, w, V3{gx, gy, gz});
    return true;
}

}  // namespace
