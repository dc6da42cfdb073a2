// Nonbonded energy and gradient (Lennard-Jones + Coulomb, no cutoff: OpenMM's NonbondedForce with NoCutoff) over all atom pairs of
// every molecule of a batch, fp32, xyz[N,C,3] (include/grappa_hip.h grappa_nb_desc).
//   table  : the work-item list.  A work item is (molecule, block of ni <= NB_T i-atoms, nc conformations); it depends on the molecule's
//            size and on C only, never on the molecule's place in the batch.  grappa_nonbonded_plan builds the list on the HOST from a
//            host copy of atom_molptr, once per (batch, C); the caller keeps it in device memory and grappa_nonbonded_fwd_planned_f32
//            launches exactly one workgroup per item.  A caller that holds atom_molptr in device memory only calls
//            grappa_nonbonded_fwd_f32: one workgroup (nb_setup_kernel) builds the same list in the workspace first, and the pairs grid
//            is its upper bound.  Both paths run the same items in the same way: the same bits.
//   pairs  : one workgroup of 256 threads per work item.  A thread owns one (i-atom, conformation) and one of JS slices of the j loop
//            (JS = 256 / (ni * nc): one 50,000-atom molecule with C = 1 keeps all four wavefronts busy, slice s takes j = s, s + JS, ..).
//            The molecule's j-atoms pass through LDS in ascending blocks of NB_TJ: coordinates per conformation, parameters once for all
//            conformations.  (With ni * nc < 64 the lanes of one wavefront belong to several slices and read several rows of the LDS
//            block at once: those reads are not broadcasts.)  A thread walks its atom's sorted exception list in step with j: an
//            exception REPLACES the pair's parameters, an exclusion (eps = 0 and qq = 0) or j == i is not evaluated at all.  Blocks
//            in which no thread of a wavefront has an exception or its own atom take a loop without the lookup.  (The text of this
//            loop is nb_pair_loop of csrc/nb_loop.h; the force of the stepwise minimiser and dynamics, csrc/rs_force.h, calls it too.)
//            No Newton's third law and no atomics: an atom's gradient is summed by its owner in a fixed j order, the slices are added
//            in a fixed order through LDS, and the block's half-energies sum_i 1/2 sum_j e_ij are added over i in double.
//   reduce : one workgroup per molecule adds the blocks' partial energies in double in a fixed order.
//   cutoff : grappa_nonbonded_fwd_cut_f32 runs the same pairs kernel under the cut policy of csrc/nb_cut.h (OpenMM's CutoffNonPeriodic:
//            reaction field, switch, exceptions uncut; nb_pair_cut of csrc/nb_pair.h) after one launch that writes the blocks' bounding
//            boxes and exception ranges; the item then skips the j-blocks the rule of csrc/nb_cut.h calls far -- no neighbour list, no
//            sort, no atomics, and the same bits as with every tile evaluated.
// Same input, same bits.  A non-excluded pair at zero distance gives inf / NaN, as in OpenMM.
#include <limits.h>

#include "common.h"
#include "nb_cut.h"
#include "nb_loop.h"
#include "nb_pair.h"
#include "nb_plan.h"
#include "nb_reduce.h"

namespace {

// ------------------------------------------------------------------------------------------------ setup
// hdr[0] = number of work items; blk_ptr[b] = first i-block of molecule b (blocks number the rows of the partial energies);
// items[k] = {molecule, first i-atom, i-block, first conformation}
__global__ __launch_bounds__(NB_NT) void nb_setup_kernel(int N, int C, int B, const int* __restrict__ molptr, int* __restrict__ hdr,
                                                         int* __restrict__ blk_ptr, int4* __restrict__ items, int max_blk, int max_items) {
    __shared__ int sblk[NB_NT], sitem[NB_NT];
    const int t = threadIdx.x;
    const int per = (B + NB_NT - 1) / NB_NT;
    const int b0 = t * per < B ? t * per : B, b1 = b0 + per < B ? b0 + per : B;
    int nblk = 0, nitem = 0, cf, ncb;
    nb_chunks(NB_T, C, cf, ncb);
    for (int b = b0; b < b1; ++b) {
        const int n = nb_clamp(molptr[b + 1], N) - nb_clamp(molptr[b], N);
        const int full = n > 0 ? n / NB_T : 0, rem = n > 0 ? n - full * NB_T : 0;
        int cr = 0;
        if (rem) nb_chunks(rem, C, cr, ncb);
        nblk += full + (rem ? 1 : 0);
        nitem += full * cf + cr;
    }
    sblk[t] = nblk;
    sitem[t] = nitem;
    __syncthreads();
    if (t == 0) {
        int ab = 0, ai = 0;
        for (int k = 0; k < NB_NT; ++k) {
            const int vb = sblk[k], vi = sitem[k];
            sblk[k] = ab;
            sitem[k] = ai;
            ab += vb;
            ai += vi;
        }
        hdr[0] = ai < max_items ? ai : max_items;
        blk_ptr[B] = ab < max_blk ? ab : max_blk;
    }
    __syncthreads();
    int blk = sblk[t], item = sitem[t];
    for (int b = b0; b < b1; ++b) {
        blk_ptr[b] = blk < max_blk ? blk : max_blk;
        const int a0 = nb_clamp(molptr[b], N), a1 = nb_clamp(molptr[b + 1], N);
        for (int i0 = a0; i0 < a1; i0 += NB_T, ++blk) {
            const int ni = a1 - i0 < NB_T ? a1 - i0 : NB_T;
            int nch;
            nb_chunks(ni, C, nch, ncb);
            for (int k = 0; k < nch; ++k, ++item)
                if (item < max_items && blk < max_blk) items[item] = make_int4(b, i0, blk, k * ncb);
        }
    }
}

// ------------------------------------------------------------------------------------------------ pairs
struct NbArgs {
    grappa_nb_desc d;
    const int* hdr;        // hdr[0] = number of work items (the grid is an upper bound), or NULL (the grid is exact)
    const int4* items;
    double* part;      // [blocks][C][2]: LJ, Coulomb half-energies of the block's i-atoms
    float* grad;
    int max_blk;       // rows of `part`
};
__device__ inline RsGeom nb_geom(const NbArgs& a) { return {a.d.N, a.d.C, a.d.B, a.max_blk, a.d.atom_molptr, nullptr, a.items}; }

// Cut: the compile-time cut policy of csrc/nb_cut.h (NbNoCut: all pairs; NbCut: nb_pair_cut for a pair that is no exception, far tiles
// skipped, tiles[item] = the tiles evaluated)
template <class Cut>
__global__ __launch_bounds__(NB_NT) void nb_pairs_kernel(NbArgs a, Cut cut, int* tiles) {
    __shared__ float4 xs[NB_TJ * NB_CW];      // j coordinates: [jj][conformation of the item]
    __shared__ float4 ps[NB_TJ];              // j parameters: q, sigma / 2, sqrt(eps)
    __shared__ float red[5][NB_NT];
    if constexpr (Cut::on) {
        __shared__ unsigned char near[NB_NT];
        cut.near = near;
    }
    if (a.hdr && (int)blockIdx.x >= a.hdr[0]) return;
    const grappa_nb_desc& d = a.d;
    const int C = d.C;
    RsItem r;
    if (!rs_item(nb_geom(a), r)) return;
    if (Cut::on && !nb_cut_blocks_ok(r, a.max_blk)) return;
    const int ni = r.ni, blk = r.blk;
    const int NL = ni * r.nc;
    const int JS = NB_NT / NL < NB_JS ? NB_NT / NL : NB_JS;
    const int t = threadIdx.x, s = t / NL, l = t - s * NL;
    const bool active = s < JS;
    const int cl = l / ni, il = l - cl * ni;      // i is the fast index: the lanes of a wavefront share few conformations (LDS broadcasts)
    const int i = r.i0 + il, c = r.c0 + cl;

    const NbSums sum = nb_pair_loop(d, d.xyz, r, C, s, JS, i, c, cl, active, nullptr, cut, xs, ps, NbSums{0.f, 0.f, 0.f, 0.f, 0.f, 0});
    float elj = sum.elj, ec = sum.ec, gx = sum.gx, gy = sum.gy, gz = sum.gz;
    if constexpr (Cut::on)
        if (tiles && t == 0) tiles[blockIdx.x] = sum.tiles;
    // the slices of one (atom, conformation), added in slice order
    red[0][t] = elj, red[1][t] = ec, red[2][t] = gx, red[3][t] = gy, red[4][t] = gz;
    __syncthreads();
    const bool owner = active && s == 0;
    if (owner) {
        for (int q = 1; q < JS; ++q) {
            const int o = q * NL + l;
            elj += red[0][o], ec += red[1][o], gx += red[2][o], gy += red[3][o], gz += red[4][o];
        }
        if (a.grad) {
            float* g = a.grad + ((size_t)i * C + c) * 3;
            g[0] = gx, g[1] = gy, g[2] = gz;
        }
    }
    __syncthreads();
    if (owner) red[0][l] = elj, red[1][l] = ec;
    __syncthreads();
    if (owner && il == 0) {
        double slj = 0.0, sc = 0.0;
        for (int k = 0; k < ni; ++k) {
            slj += (double)red[0][cl * ni + k];
            sc += (double)red[1][cl * ni + k];
        }
        double* o = a.part + ((size_t)blk * C + c) * 2;
        o[0] = 0.5 * slj, o[1] = 0.5 * sc;
    }
}

// the boxes of the item's (block, conformations) at d.xyz and, by the item of the block's first conformations, the block's exception
// range (csrc/nb_cut.h): the launch before nb_pairs_kernel<NbCut>
__global__ __launch_bounds__(NB_NT) void nb_box_kernel(NbArgs a, float4* box, int2* er) {
    RsItem r;
    if (rs_item(nb_geom(a), r)) nb_cut_box_range(r, a.d.C, a.d.xyz, a.d.exc_ptr, a.d.exc_atom, box, er);
}

struct NbLayout {
    size_t blk_ptr, items, part, total;
    long long max_blk, max_items;
};
NbLayout nb_layout(int N, int C, int B) {
    NbLayout L;
    WsCarve w{nullptr};
    // every molecule ends in at most one short block; a block of ni <= NB_T atoms takes at most ceil(C / (NB_NT / NB_T)) work items
    L.max_blk = (long long)N / NB_T + B;
    L.max_items = L.max_blk * ((C + NB_NT / NB_T - 1) / (NB_NT / NB_T));
    w.skip(256);      // hdr
    L.blk_ptr = w.skip(sizeof(int) * ((size_t)B + 1));
    L.items = w.skip(sizeof(int4) * (size_t)L.max_items);
    L.part = w.skip(sizeof(double) * 2 * (size_t)L.max_blk * (size_t)C);
    L.total = w.off;
    return L;
}

}  // namespace

extern "C" int grappa_nonbonded_iblock(void) { return NB_T; }

extern "C" size_t grappa_nonbonded_workspace_bytes(int N, int C, int B) {
    if (N <= 0 || C <= 0 || B <= 0) return 0;
    return nb_layout(N, C, B).total;
}

static int nb_check(const grappa_nb_desc* d, const float* energy) {
    if (!d->xyz || !d->atom_molptr || !d->charge || !d->sigma || !d->epsilon || !d->exc_ptr || !d->exc_atom || !d->exc_qq || !d->exc_sigma ||
        !d->exc_eps || !energy)
        return GRAPPA_ERR_ARG;
    return GRAPPA_OK;
}

extern "C" int grappa_nonbonded_fwd_f32(void* stream, const grappa_nb_desc* d, float* energy, float* term_energy, float* grad, void* ws,
                                        size_t ws_bytes) {
    if (!d || d->N < 0 || d->C < 0 || d->B < 0) return GRAPPA_ERR_ARG;
    if (d->N == 0 || d->C == 0 || d->B == 0) return GRAPPA_OK;
    if (nb_check(d, energy) != GRAPPA_OK || !ws) return GRAPPA_ERR_ARG;
    const NbLayout L = nb_layout(d->N, d->C, d->B);
    if (L.max_items > INT_MAX) return GRAPPA_ERR_ARG;
    if (ws_bytes < L.total) return GRAPPA_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    int* hdr = (int*)w;
    int* blk_ptr = (int*)(w + L.blk_ptr);
    int4* items = (int4*)(w + L.items);
    double* part = (double*)(w + L.part);
    GRAPPA_LAUNCH(nb_setup_kernel, dim3(1), dim3(NB_NT), 0, st, d->N, d->C, d->B, d->atom_molptr, hdr, blk_ptr, items, (int)L.max_blk,
                  (int)L.max_items);
    NbArgs a{*d, hdr, items, part, grad, (int)L.max_blk};
    GRAPPA_LAUNCH(nb_pairs_kernel<NbNoCut>, dim3((unsigned)L.max_items), dim3(NB_NT), 0, st, a, NbNoCut{}, (int*)nullptr);
    GRAPPA_LAUNCH(nb_reduce_kernel, dim3(d->B), dim3(NB_NT), 0, st, d->C, d->B, blk_ptr, part, energy, term_energy);
    return grappa_launch_status();
}

// the table of the planned path (csrc/nb_plan.h states its layout, nb_table_view reads it)
extern "C" long long grappa_nonbonded_plan(int N, int C, int B, const int* atom_molptr_host, int* table, long long table_ints) {
    if (N < 0 || C < 1 || B < 1 || !atom_molptr_host) return GRAPPA_ERR_ARG;
    const long long items0 = nb_table_items0(B);
    long long blk = 0, item = 0;
    for (int pass = 0; pass < (table ? 2 : 1); ++pass) {      // count, then (with a table of the counted size) fill
        if (pass == 1) {
            if (table_ints < items0 + 4 * item) return GRAPPA_ERR_WORKSPACE;
            table[0] = (int)item, table[1] = (int)blk, table[2] = table[3] = 0;
            for (long long k = 4 + B + 1; k < items0; ++k) table[k] = 0;
            blk = item = 0;
        }
        for (int b = 0; b < B; ++b) {
            const int a0 = atom_molptr_host[b], a1 = atom_molptr_host[b + 1];
            if (a0 < 0 || a1 < a0 || a1 > N) return GRAPPA_ERR_ARG;
            if (pass == 1) table[4 + b] = (int)blk;
            for (int i0 = a0; i0 < a1; i0 += NB_T, ++blk) {
                int nch, ncb;
                nb_chunks(a1 - i0 < NB_T ? a1 - i0 : NB_T, C, nch, ncb);
                if (pass == 1)
                    for (int k = 0; k < nch; ++k) {
                        int* it = table + items0 + 4 * (item + k);
                        it[0] = b, it[1] = i0, it[2] = (int)blk, it[3] = k * ncb;
                    }
                item += nch;
            }
        }
        if (item > INT_MAX / 4 || blk > INT_MAX) return GRAPPA_ERR_ARG;
        if (pass == 1) table[4 + B] = (int)blk;
    }
    return items0 + 4 * item;
}

extern "C" int grappa_nonbonded_fwd_planned_f32(void* stream, const grappa_nb_desc* d, const int* table_dev, int n_items, int n_blocks,
                                                float* energy, float* term_energy, float* grad, void* ws, size_t ws_bytes) {
    if (!d || d->N < 0 || d->C < 0 || d->B < 0 || n_items < 0 || n_blocks < 0) return GRAPPA_ERR_ARG;
    if (d->N == 0 || d->C == 0 || d->B == 0) return GRAPPA_OK;
    if (nb_check(d, energy) != GRAPPA_OK || !table_dev || (n_blocks > 0 && !ws)) return GRAPPA_ERR_ARG;
    if (n_blocks > (long long)d->N / NB_T + d->B) return GRAPPA_ERR_ARG;
    if (ws_bytes < sizeof(double) * 2 * (size_t)n_blocks * (size_t)d->C) return GRAPPA_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const NbTableView tv = nb_table_view(table_dev, d->B);
    NbArgs a{*d, nullptr, tv.items, (double*)ws, grad, n_blocks};
    if (n_items > 0) GRAPPA_LAUNCH(nb_pairs_kernel<NbNoCut>, dim3((unsigned)n_items), dim3(NB_NT), 0, st, a, NbNoCut{}, (int*)nullptr);
    GRAPPA_LAUNCH(nb_reduce_kernel, dim3(d->B), dim3(NB_NT), 0, st, d->C, d->B, tv.blk_ptr, (const double*)ws, energy, term_energy);
    return grappa_launch_status();
}

// ------------------------------------------------------------------------------------------------ with a cutoff
namespace {

struct NbCutLayout {
    size_t part, box, er, total;
};
NbCutLayout nb_cut_layout(int C, int n_blocks) {
    const size_t kc = (size_t)n_blocks * (size_t)C;
    NbCutLayout L;
    WsCarve w{nullptr};
    L.part = w.skip(sizeof(double) * 2 * kc);
    L.box = w.skip(sizeof(float4) * 2 * kc);
    L.er = w.skip(sizeof(int2) * (size_t)n_blocks);
    L.total = w.off;
    return L;
}

}  // namespace

extern "C" size_t grappa_nonbonded_cut_workspace_bytes(int C, int n_blocks) {
    if (C <= 0 || n_blocks <= 0) return 0;
    return nb_cut_layout(C, n_blocks).total;
}

extern "C" int grappa_nonbonded_fwd_cut_f32(void* stream, const grappa_nb_desc* d, const grappa_nb_cut* cut, const int* table_dev, int n_items,
                                            int n_blocks, float* energy, float* term_energy, float* grad, int* tiles, void* ws, size_t ws_bytes) {
    NbCutDev c;
    if (!d || d->N < 0 || d->C < 0 || d->B < 0 || n_items < 0 || n_blocks < 0 || !nb_cut_consts(cut, c.k, c.thr)) return GRAPPA_ERR_ARG;
    if (d->N == 0 || d->C == 0 || d->B == 0) return GRAPPA_OK;
    if (nb_check(d, energy) != GRAPPA_OK || !table_dev || (n_blocks > 0 && !ws)) return GRAPPA_ERR_ARG;
    if ((((uintptr_t)ws | (uintptr_t)table_dev) & 15) != 0) return GRAPPA_ERR_ARG;      // (float4 boxes, int4 items)
    if (n_blocks > (long long)d->N / NB_T + d->B || (long long)n_blocks * d->C > INT_MAX) return GRAPPA_ERR_ARG;
    const NbCutLayout L = nb_cut_layout(d->C, n_blocks);
    if (n_blocks > 0 && ws_bytes < L.total) return GRAPPA_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    const NbTableView tv = nb_table_view(table_dev, d->B);
    NbArgs a{*d, nullptr, tv.items, (double*)(w + L.part), grad, n_blocks};
    c.prune = cut->prune;
    c.box = (const float4*)(w + L.box), c.er = (const int2*)(w + L.er);
    if (n_items > 0) {
        GRAPPA_LAUNCH(nb_box_kernel, dim3((unsigned)n_items), dim3(NB_NT), 0, st, a, (float4*)(w + L.box), (int2*)(w + L.er));
        GRAPPA_LAUNCH(nb_pairs_kernel<NbCut>, dim3((unsigned)n_items), dim3(NB_NT), 0, st, a, NbCut{c, nullptr}, tiles);
    }
    GRAPPA_LAUNCH(nb_reduce_kernel, dim3(d->B), dim3(NB_NT), 0, st, d->C, d->B, tv.blk_ptr, (const double*)(w + L.part), energy, term_energy);
    return grappa_launch_status();
}
