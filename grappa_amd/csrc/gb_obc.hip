// GB/SA implicit solvent in the Onufriev-Bashford-Case form (include/grappa_hip.h grappa_gb_desc states the energy in full), fp32,
// xyz[N,C,3], over the work items of the nonbonded plan (csrc/nb_plan.h): one workgroup of 256 threads per item.  The three passes are
// csrc/gb_pass.h's (born, pair, chain; the stepwise dynamics of csrc/dynamics_steps.hip runs the same text); here
//   born   : B, dBdI [N,C] -> the workspace (and `born`)
//   pair   : the gradient at fixed B -> grad, w [N,C] -> the workspace, the block's energies in double -> the workspace
//   chain  : both chain parts, added to grad by the owner of the (atom, conformation): the word the pair pass wrote for it
//   reduce : nb_reduce_kernel of csrc/nb_reduce.h adds the blocks' energies per molecule
// Each pass boundary is a launch boundary.  Same input, same bits.
#include <limits.h>

#include "common.h"
#include "gb_pass.h"
#include "nb_plan.h"
#include "nb_reduce.h"

namespace {

__global__ __launch_bounds__(NB_NT) void gb_born_kernel(GbArgs a) {
    __shared__ GbShared sh;
    gb_born_body<false>(a, sh);
}

template <bool G>
__global__ __launch_bounds__(NB_NT) void gb_pair_kernel(GbArgs a) {
    __shared__ GbShared sh;
    gb_pair_body<G, true, false>(a, sh);
}

__global__ __launch_bounds__(NB_NT) void gb_chain_kernel(GbArgs a) {
    __shared__ GbShared sh;
    gb_chain_body<false>(a, sh, [&](const GbLane& w, float gx, float gy, float gz) {
        if (!w.owner) return;      // one writer per word and launch
        float* g = a.gdir + ((size_t)w.i * a.q.C + w.c) * 3;
        g[0] += gx, g[1] += gy, g[2] += gz;
    });
}

// ---- under a cutoff (grappa_gb_cut): the same bodies under the GbCut policy of csrc/gb_loop.h, behind one launch that writes the boxes
__global__ __launch_bounds__(NB_NT) void gb_boxes_kernel(GbArgs a, float4* box) {
    RsItem r;
    if (rs_item(a.q, r)) gb_cut_boxes(r, a.q.C, a.x, box);
}

__global__ __launch_bounds__(NB_NT) void gb_born_cut_kernel(GbArgs a, GbCutDev c, int* tiles) {
    __shared__ GbShared sh;
    __shared__ unsigned char near[NB_NT];
    gb_born_body<false, GbCut>(a, sh, GbCut{c, near, 0}, tiles);
}

template <bool G>
__global__ __launch_bounds__(NB_NT) void gb_pair_cut_kernel(GbArgs a, GbCutDev c) {
    __shared__ GbShared sh;
    __shared__ unsigned char near[NB_NT];
    gb_pair_body<G, true, false, GbCut>(a, sh, GbCut{c, near, 0});
}

__global__ __launch_bounds__(NB_NT) void gb_chain_cut_kernel(GbArgs a, GbCutDev c) {
    __shared__ GbShared sh;
    __shared__ unsigned char near[NB_NT];
    gb_chain_body<false, GbCut>(
        a, sh,
        [&](const GbLane& w, float gx, float gy, float gz) {
            if (!w.owner) return;      // one writer per word and launch
            float* g = a.gdir + ((size_t)w.i * a.q.C + w.c) * 3;
            g[0] += gx, g[1] += gy, g[2] += gz;
        },
        GbCut{c, near, 0});
}

struct GbLayout {
    GbPassWs p;
    double* part;
    size_t total;
};
GbLayout gb_layout(char* base, int N, int C, int n_blocks) {
    GbLayout L;
    WsCarve k{base};
    L.p = gb_pass_ws(k, N, C);
    L.part = k.take<double>(2 * (size_t)n_blocks * (size_t)C);
    L.total = k.off;
    return L;
}

// (the boxes lie behind the words of the all-pairs call)
struct GbCutLayout {
    GbLayout g;
    float4* box;
    size_t total;
};
GbCutLayout gb_cut_layout(char* base, int N, int C, int n_blocks) {
    GbCutLayout L;
    L.g = gb_layout(base, N, C, n_blocks);
    WsCarve k{base};
    k.off = L.g.total;
    L.box = k.take<float4>(2 * (size_t)n_blocks * (size_t)C);
    L.total = k.off;
    return L;
}

}  // namespace

extern "C" size_t grappa_gb_obc_workspace_bytes(int N, int C, int n_blocks) {
    if (N <= 0 || C <= 0 || n_blocks <= 0) return 0;
    return gb_layout(nullptr, N, C, n_blocks).total;
}

extern "C" int grappa_gb_obc_fwd_f32(void* stream, const grappa_nb_desc* nb, const grappa_gb_desc* gb, const int* table_dev, int n_items,
                                     int n_blocks, float* energy, float* term_energy, float* grad, float* born, void* ws, size_t ws_bytes) {
    GbK k;
    if (!nb || nb->N < 0 || nb->C < 0 || nb->B < 0 || n_items < 0 || n_blocks < 0 || !gb_consts(gb, k)) return GRAPPA_ERR_ARG;
    if (nb->N == 0 || nb->C == 0 || nb->B == 0) return GRAPPA_OK;
    if (!nb->xyz || !nb->charge || !nb->atom_molptr || !gb->radius || !gb->scale || !energy || !table_dev || !ws) return GRAPPA_ERR_ARG;
    if ((((uintptr_t)ws | (uintptr_t)table_dev) & 15) != 0) return GRAPPA_ERR_ARG;
    if (n_blocks > (long long)nb->N / NB_T + nb->B || (long long)n_blocks * nb->C > INT_MAX || (long long)nb->N * nb->C * 3 > INT_MAX)
        return GRAPPA_ERR_ARG;
    const GbLayout L = gb_layout((char*)ws, nb->N, nb->C, n_blocks);
    if (ws_bytes < L.total) return GRAPPA_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const NbTableView tv = nb_table_view(table_dev, nb->B);
    GbArgs a = {};
    a.q = RsGeom{nb->N, nb->C, nb->B, n_blocks, nb->atom_molptr, tv.blk_ptr, tv.items};
    a.x = nb->xyz, a.charge = nb->charge, a.radius = gb->radius, a.scale = gb->scale, a.k = k;
    a.B = L.p.B, a.dBdI = L.p.dBdI, a.w = L.p.w, a.part = L.part;
    a.gdir = grad, a.born = born;
    if (n_items > 0) {
        const dim3 grid((unsigned)n_items), block(NB_NT);
        GRAPPA_LAUNCH(gb_born_kernel, grid, block, 0, st, a);
        if (grad) {
            GRAPPA_LAUNCH(gb_pair_kernel<true>, grid, block, 0, st, a);
            GRAPPA_LAUNCH(gb_chain_kernel, grid, block, 0, st, a);
        } else {
            GRAPPA_LAUNCH(gb_pair_kernel<false>, grid, block, 0, st, a);
        }
    }
    GRAPPA_LAUNCH(nb_reduce_kernel, dim3(nb->B), dim3(NB_NT), 0, st, nb->C, nb->B, tv.blk_ptr, (const double*)L.part, energy, term_energy);
    return grappa_launch_status();
}

extern "C" size_t grappa_gb_obc_cut_workspace_bytes(int N, int C, int n_blocks) {
    if (N <= 0 || C <= 0 || n_blocks <= 0) return 0;
    return gb_cut_layout(nullptr, N, C, n_blocks).total;
}

// box (every (block, conformation) of the table's items), born, pair, chain, reduce: 5 launches, 4 with grad == NULL
extern "C" int grappa_gb_obc_fwd_cut_f32(void* stream, const grappa_nb_desc* nb, const grappa_gb_desc* gb, const grappa_gb_cut* gbcut,
                                         const int* table_dev, int n_items, int n_blocks, float* energy, float* term_energy, float* grad,
                                         float* born, int* tiles, void* ws, size_t ws_bytes) {
    GbK k;
    GbCutDev c;
    if (!nb || nb->N < 0 || nb->C < 0 || nb->B < 0 || n_items < 0 || n_blocks < 0 || !gb_consts(gb, k) || !gb_cut_consts(gbcut, c))
        return GRAPPA_ERR_ARG;
    if (nb->N == 0 || nb->C == 0 || nb->B == 0) return GRAPPA_OK;
    if (!nb->xyz || !nb->charge || !nb->atom_molptr || !gb->radius || !gb->scale || !energy || !table_dev || !ws) return GRAPPA_ERR_ARG;
    if ((((uintptr_t)ws | (uintptr_t)table_dev) & 15) != 0) return GRAPPA_ERR_ARG;
    if (n_blocks > (long long)nb->N / NB_T + nb->B || (long long)n_blocks * nb->C > INT_MAX || (long long)nb->N * nb->C * 3 > INT_MAX)
        return GRAPPA_ERR_ARG;
    const GbCutLayout L = gb_cut_layout((char*)ws, nb->N, nb->C, n_blocks);
    if (ws_bytes < L.total) return GRAPPA_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const NbTableView tv = nb_table_view(table_dev, nb->B);
    GbArgs a = {};
    a.q = RsGeom{nb->N, nb->C, nb->B, n_blocks, nb->atom_molptr, tv.blk_ptr, tv.items};
    a.x = nb->xyz, a.charge = nb->charge, a.radius = gb->radius, a.scale = gb->scale, a.k = k;
    a.B = L.g.p.B, a.dBdI = L.g.p.dBdI, a.w = L.g.p.w, a.part = L.g.part;
    a.gdir = grad, a.born = born;
    c.box = L.box;
    if (n_items > 0) {
        const dim3 grid((unsigned)n_items), block(NB_NT);
        GRAPPA_LAUNCH(gb_boxes_kernel, grid, block, 0, st, a, L.box);
        GRAPPA_LAUNCH(gb_born_cut_kernel, grid, block, 0, st, a, c, tiles);
        if (grad) {
            GRAPPA_LAUNCH(gb_pair_cut_kernel<true>, grid, block, 0, st, a, c);
            GRAPPA_LAUNCH(gb_chain_cut_kernel, grid, block, 0, st, a, c);
        } else {
            GRAPPA_LAUNCH(gb_pair_cut_kernel<false>, grid, block, 0, st, a, c);
        }
    }
    GRAPPA_LAUNCH(nb_reduce_kernel, dim3(nb->B), dim3(NB_NT), 0, st, nb->C, nb->B, tv.blk_ptr, (const double*)L.g.part, energy, term_energy);
    return grappa_launch_status();
}
