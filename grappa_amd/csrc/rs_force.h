// A molecule spread over many workgroups: the work items of the nonbonded plan (csrc/nb_plan.h) as csrc/relax_steps.hip and
// csrc/dynamics_steps.hip walk them, and the one-launch force of that decomposition, shared by both.
//   item   : (molecule, block of ni <= 64 i-atoms, nc conformations), one workgroup of NB_NT threads; rs_item of csrc/nb_plan.h decodes
//            it and refuses a table made for another batch.
//   force  : rs_force computes g = grad E(x) of the item's (atom, conformation) pairs: bonded_gather of csrc/mm_geom.h, as in
//            mm_gradient_kernel (the thread's slice of the atom's incidences, neighbours read from global memory) plus the pair loop of
//            the nonbonded energy kernel itself (nb_pair_loop of csrc/nb_loop.h, described at the head of csrc/nonbonded.hip; no pair
//            energy kept), slices added in slice order.  What a kernel does with the gradient of an (atom, conformation) -- the
//            minimiser's partials, the integrator's closing kick -- is its epilogue, a functor, the way rx_gradient of csrc/rx_force.h
//            takes one.  A compile-time cut policy (csrc/nb_cut.h) chooses between all pairs and a cutoff with tile pruning.
// The workgroup reads x of the whole molecule and the status of its own conformations; it writes nothing itself.
#pragma once
#include "common.h"
#include "mm_geom.h"
#include "nb_cut.h"
#include "nb_loop.h"
#include "nb_plan.h"

namespace {

// (RS_RUNNING and rs_running, the stopped-conformation mask of an item: csrc/nb_plan.h)

inline RsGeom rs_geom(const grappa_mm_desc* mm, const int* table_dev, int n_blocks) {
    RsGeom q;
    q.N = mm->N, q.C = mm->C, q.B = mm->B, q.n_blocks = n_blocks;
    q.atom_molptr = mm->atom_molptr;
    const NbTableView tv = nb_table_view(table_dev, mm->B);
    q.blk_ptr = tv.blk_ptr, q.items = tv.items;
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
    if (Cut::on && !nb_cut_blocks_ok(r, a.q.n_blocks)) return false;
    const int ni = r.ni;
    const int NL = ni * r.nc;
    const int JS = NB_NT / NL < NB_JS ? NB_NT / NL : NB_JS;
    const int t = threadIdx.x, s = t / NL, l = t - s * NL;
    const int cl = l / ni, il = l - cl * ni;      // (l < NL: cl < nc)
    const int i = r.i0 + il, c = r.c0 + cl;
    const bool active = s < JS && sh.run[cl] != 0;

    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (active) {
        const V3 p = rs_bonded(a.mm, a.x, i, s, JS, c);
        gx = p.x, gy = p.y, gz = p.z;
    }
    if (a.has_nb) {
        // (no pair energy is kept: dead code to the compiler)
        const NbSums sum = nb_pair_loop(a.nb, a.x, r, C, s, JS, i, c, cl, active, sh.run, cut, sh.xs, sh.ps, NbSums{0.f, 0.f, gx, gy, gz, 0});
        gx = sum.gx, gy = sum.gy, gz = sum.gz;
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

// The six potential terms at the held coordinates x by the library's own energy kernels: the bits of grappa_mm_energy_fwd_f32 and
// grappa_nonbonded_fwd_planned_f32 (cut given: grappa_nonbonded_fwd_cut_f32, in the workspace nbws) there.  terms [6,B,C] (rows 4, 5
// only with nb), e_mm and e_nb [B,C]; nbws: the nonbonded call's workspace.
inline int steps_terms_at(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut, const int* table_dev,
                          int n_items, int n_blocks, const float* x, float* e_mm, float* e_nb, float* terms, void* nbws, size_t nbws_bytes) {
    grappa_mm_desc me = *mm;
    me.xyz = x;
    const int rc = grappa_mm_energy_fwd_f32(stream, &me, e_mm, terms, nullptr, nullptr);
    if (rc != GRAPPA_OK || !nb) return rc;
    grappa_nb_desc ne = *nb;
    ne.xyz = x;
    ne.atom_molptr = mm->atom_molptr;
    float* te = terms + 4 * (size_t)mm->B * mm->C;
    if (cut) return grappa_nonbonded_fwd_cut_f32(stream, &ne, cut, table_dev, n_items, n_blocks, e_nb, te, nullptr, nullptr, nbws, nbws_bytes);
    return grappa_nonbonded_fwd_planned_f32(stream, &ne, table_dev, n_items, n_blocks, e_nb, te, nullptr, nbws, nbws_bytes);
}

// The two terms of the GB/SA implicit solvent at the held coordinates x by the library's own entry: the bits of grappa_gb_obc_fwd_f32
// there.  e_gb [B,C], terms_gb [2,B,C] (polar, surface area); gbws: that call's workspace, a region of its own.
inline int steps_gb_terms_at(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_gb_desc* gb, const int* table_dev,
                             int n_items, int n_blocks, const float* x, float* e_gb, float* terms_gb, void* gbws, size_t gbws_bytes) {
    grappa_nb_desc ne = *nb;
    ne.xyz = x;
    ne.atom_molptr = mm->atom_molptr;
    return grappa_gb_obc_fwd_f32(stream, &ne, gb, table_dev, n_items, n_blocks, e_gb, terms_gb, nullptr, nullptr, gbws, gbws_bytes);
}

// ... under the solvent's cutoff (gbcut == NULL: the call above): grappa_gb_obc_fwd_cut_f32 itself, no second energy path
inline int steps_gb_cut_terms_at(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_gb_desc* gb,
                                 const grappa_gb_cut* gbcut, const int* table_dev, int n_items, int n_blocks, const float* x, float* e_gb,
                                 float* terms_gb, void* gbws, size_t gbws_bytes) {
    if (!gbcut) return steps_gb_terms_at(stream, mm, nb, gb, table_dev, n_items, n_blocks, x, e_gb, terms_gb, gbws, gbws_bytes);
    grappa_nb_desc ne = *nb;
    ne.xyz = x;
    ne.atom_molptr = mm->atom_molptr;
    return grappa_gb_obc_fwd_cut_f32(stream, &ne, gb, gbcut, table_dev, n_items, n_blocks, e_gb, terms_gb, nullptr, nullptr, nullptr, gbws,
                                     gbws_bytes);
}

// ------------------------------------------------------------------------------------------------ a cutoff on the stepwise paths
// a cutoff as the three calls of a stepwise path carry it: the caller's options and the device constants made of them
struct RsCut {
    const grappa_nb_cut* opts;
    NbCutDev dev;
};

// cut given: false if its options are refused or nb is missing; else the constants (box and er are set once the workspace is laid out)
inline bool rs_cut_make(const grappa_nb_cut* cut, const grappa_nb_desc* nb, RsCut& c) {
    c.opts = cut;
    c.dev = NbCutDev{};
    if (!nb || !nb_cut_consts(cut, c.dev.k, c.dev.thr)) return false;
    c.dev.prune = cut->prune;
    return true;
}

// with a cutoff, the launch of init between the init kernel and the first force: the boxes and exception ranges at x (csrc/nb_cut.h)
struct RsBoxArgs {
    RsGeom q;
    const float* x;
    const int *exc_ptr, *exc_atom;
    float4* box;
    int2* er;
};

__global__ __launch_bounds__(NB_NT) void rs_box_kernel(RsBoxArgs a) {
    RsItem r;
    if (rs_item(a.q, r)) nb_cut_box_range(r, a.q.C, a.x, a.exc_ptr, a.exc_atom, a.box, a.er);
}

}  // namespace
