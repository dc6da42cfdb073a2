// The nonbonded cutoff (include/grappa_hip.h grappa_nb_cut), shared by csrc/nonbonded.hip and csrc/rs_force.h: ONE definition of the
// constants the host derives from the options, of a block's bounding box and exception range, and of the rule by which a work item skips
// a tile (i-block I, j-block J) -- so that the energy kernel and the force of the stepwise dynamics skip the same tiles.
//   box    : per (block, conformation) the exact fp32 minimum and maximum of the block's coordinates, two float4 (lo, hi).  A NaN
//            coordinate makes its axis NaN in both.  One writer: the work item that owns (block, conformation).
//   range  : per block the first and last TILE of its molecule (tile = j-block counted from the molecule's first atom) that holds an
//            exception partner of one of the block's atoms, from the first and last partner of each atom (ascending per atom), partners
//            clamped into the molecule; {INT_MAX, -1} if the block has none.
//   rule   : tile (I, J) is evaluated iff prune == 0, or J lies in the range of I, or for a running conformation of the item
//            NOT d2 > thr, d2 = sum over x, y, z of max(0, lo_I - hi_J, lo_J - hi_I)^2 in fp32 (products and sums rounded one by one, in
//            that order), thr = rc2 (1 + 2^-18) rounded once on the host.  Written so that a NaN counts as near.
// A decision is taken by ONE thread per tile from words an earlier launch wrote, and read by the whole workgroup from LDS after a barrier:
// it is uniform, so a skipped tile passes none of the tile's barriers.
#pragma once
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"
#include "nb_pair.h"
#include "nb_plan.h"

namespace {

static_assert(NB_T == NB_TJ, "a block's box serves as i-block and as j-block");

struct NbCutDev {
    NbCutK k;                // the pair's constants (csrc/nb_pair.h)
    float thr;               // rc2 (1 + 2^-18)
    int prune;
    const float4* box;       // [n_blocks][C][2]
    const int2* er;          // [n_blocks]
};

// The cut policy of the pair loop (nb_pair_loop of csrc/nb_loop.h, called by nb_pairs_kernel of csrc/nonbonded.hip and by rs_force of
// csrc/rs_force.h), a compile-time choice.
struct NbNoCut {
    static constexpr bool on = false;
};
struct NbCut {
    static constexpr bool on = true;
    NbCutDev c;
    unsigned char* near;      // NB_NT bytes of LDS for the verdicts
};

// the options as the ABI states them (comparisons written so that a NaN is refused) -> the constants, every one rounded once from double
inline bool nb_cut_consts(const grappa_nb_cut* o, NbCutK& k, float& thr) {
    if (!o) return false;
    const double rc = o->cutoff, rs = o->switch_distance, eps = o->rf_dielectric;
    if (!(rc > 0.0 && rc <= FLT_MAX) || !(eps >= 1.0 && eps <= FLT_MAX) || !(rs == 0.0 || (rs > 0.0 && rs < rc))) return false;
    if (o->prune != 0 && o->prune != 1) return false;
    k.rc2 = (float)(rc * rc);
    if (!(k.rc2 <= FLT_MAX)) return false;
    k.rs = rs > 0.0 ? (float)rs : (float)rc;                    // no switch: u = 0 everywhere below rc
    k.inv_w = rs > 0.0 ? (float)(1.0 / (rc - rs)) : 0.f;
    k.krf = (float)((eps - 1.0) / ((2.0 * eps + 1.0) * rc * rc * rc));
    k.crf = (float)(3.0 * eps / ((2.0 * eps + 1.0) * rc));
    thr = (float)((double)k.rc2 * (1.0 + 1.0 / 262144.0));
    return k.inv_w <= FLT_MAX;
}

// ------------------------------------------------------------------------------------------------ boxes and ranges
// Every thread of the workgroup calls it.  bx[3 * l .. ] holds the coordinates of lane l = cl * ni + il of the item (written before the
// call, no barrier yet); thread (cl, k), k = 0..5, folds axis k % 3 of conformation c0 + cl over the block's atoms -- min for k < 3 --
// and, where keep[cl] == 0 (NULL: everywhere), writes the word.  One barrier.
__device__ inline void nb_cut_box_write(const float* bx, const int* keep, int ni, int nc, int blk, int C, int c0, float4* box) {
    __syncthreads();
    const int t = threadIdx.x, cl = t / 6, k = t - cl * 6;
    if (cl >= nc || (keep && keep[cl])) return;
    const int ax = k < 3 ? k : k - 3;
    float m = bx[3 * (cl * ni) + ax];
    for (int il = 1; il < ni; ++il) {
        const float v = bx[3 * (cl * ni + il) + ax];
        const bool take = k < 3 ? v < m : v > m;
        m = (take || !(v == v)) ? v : m;      // (a NaN is taken and then stays)
    }
    float* o = (float*)(box + ((size_t)blk * C + c0 + cl) * 2 + (k < 3 ? 0 : 1));
    o[ax] = m;
    if (ax == 0) o[3] = 0.f;
}

// the block's exception range; threads il < ni look at their atom, thread 0 folds and writes.  er_s: NB_T int2 of LDS.  One barrier.
__device__ inline void nb_cut_range_write(const int* __restrict__ exc_ptr, const int* __restrict__ exc_atom, int i0, int ni, int m0, int m1, int blk,
                                          int2* er_s, int2* er) {
    const int t = threadIdx.x;
    if (t < ni) {
        const int ep = exc_ptr[i0 + t], ee = exc_ptr[i0 + t + 1];
        int2 r = make_int2(INT_MAX, -1);
        if (ep < ee) {
            int a = exc_atom[ep], b = exc_atom[ee - 1];
            a = a < m0 ? m0 : (a >= m1 ? m1 - 1 : a);
            b = b < m0 ? m0 : (b >= m1 ? m1 - 1 : b);
            r = make_int2((a - m0) / NB_TJ, (b - m0) / NB_TJ);
        }
        er_s[t] = r;
    }
    __syncthreads();
    if (t == 0) {
        int2 r = er_s[0];
        for (int k = 1; k < ni; ++k) {
            r.x = er_s[k].x < r.x ? er_s[k].x : r.x;
            r.y = er_s[k].y > r.y ? er_s[k].y : r.y;
        }
        er[blk] = r;
    }
}

// The launch before the first pair loop under the cut policy: the boxes of the item's (block, conformations) at x [N,C,3] and, by the
// item of the block's first conformations, the block's exception range.  Every thread of the item's workgroup calls it.
__device__ inline void nb_cut_box_range(const RsItem& r, int C, const float* __restrict__ x, const int* __restrict__ exc_ptr,
                                        const int* __restrict__ exc_atom, float4* box, int2* er) {
    __shared__ float bx[NB_NT * 3];
    __shared__ int2 er_s[NB_T];
    const int t = threadIdx.x;
    if (t < r.ni * r.nc) {
        const int cl = t / r.ni, il = t - cl * r.ni;
        const float* p = x + ((size_t)(r.i0 + il) * C + r.c0 + cl) * 3;
        bx[3 * t] = p[0], bx[3 * t + 1] = p[1], bx[3 * t + 2] = p[2];
    }
    if (r.c0 == 0) nb_cut_range_write(exc_ptr, exc_atom, r.i0, r.ni, r.m0, r.m1, r.blk, er_s, er);
    nb_cut_box_write(bx, nullptr, r.ni, r.nc, r.blk, C, r.c0, box);
}

// ------------------------------------------------------------------------------------------------ the skip rule
// the boxes of all blocks of the item's molecule are read: false for a table whose block numbers do not fit, which is walked away from
__device__ inline bool nb_cut_blocks_ok(const RsItem& r, int n_blocks) {
    const int kb0 = nb_first_block(r);
    return kb0 >= 0 && kb0 + nb_tiles(r) <= n_blocks;
}

__device__ inline float nb_cut_gap2(const float4 lo_i, const float4 hi_i, const float4 lo_j, const float4 hi_j) {
    auto gap = [](float a, float b) {          // max(0, a, b); a NaN gives 0
        float d = a > b ? a : b;
        return d > 0.f ? d : 0.f;
    };
    const float dx = gap(lo_i.x - hi_j.x, lo_j.x - hi_i.x), dy = gap(lo_i.y - hi_j.y, lo_j.y - hi_i.y), dz = gap(lo_i.z - hi_j.z, lo_j.z - hi_i.z);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// The verdicts of the item's tiles jt0 .. jt0 + NB_NT - 1 (those below ntiles) -> near[0 .. NB_NT): thread t takes tile jt0 + t.  Every
// thread of the workgroup calls it; two barriers (the first lets the readers of the previous verdicts finish).  blk: the item's block,
// kb0: the first block of its molecule, run: which of its nc conformations still run (NULL: all).  ER = false: the boxes alone decide (the
// implicit solvent of csrc/gb_loop.h, which knows no exceptions; Dev then needs thr, prune and box only).
template <bool ER = true, class Dev>
__device__ inline void nb_cut_decide(const Dev& c, int C, int blk, int kb0, int ntiles, int jt0, int c0, int nc, const int* run,
                                     unsigned char* near) {
    const int t = threadIdx.x, jt = jt0 + t;
    __syncthreads();
    if (jt < ntiles) {
        bool ev = c.prune == 0;
        if constexpr (ER) {
            if (!ev) {
                const int2 e = c.er[blk];
                ev = jt >= e.x && jt <= e.y;
            }
        }
        for (int cc = 0; cc < nc && !ev; ++cc) {
            if (run && !run[cc]) continue;
            const float4* bi = c.box + ((size_t)blk * C + c0 + cc) * 2;
            const float4* bj = c.box + ((size_t)(kb0 + jt) * C + c0 + cc) * 2;
            ev = !(nb_cut_gap2(bi[0], bi[1], bj[0], bj[1]) > c.thr);
        }
        near[t] = ev ? 1 : 0;
    }
    __syncthreads();
}

}  // namespace
