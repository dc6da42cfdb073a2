// The work-item decomposition of the nonbonded plan (include/grappa_hip.h grappa_nonbonded_plan), shared by csrc/nonbonded.hip and the
// stepwise kernels (csrc/rs_force.h, csrc/relax_steps.hip, csrc/dynamics_steps.hip): ONE definition of the block sizes, of how a block's
// conformations are dealt out, of the plan table's layout and of how a workgroup decodes its item, so that all read the same table the
// same way.
#pragma once
#include "common.h"

namespace {

constexpr int NB_T = GRAPPA_NB_IBLOCK;      // i-atoms per work item
constexpr int NB_TJ = 64;                   // j-atoms per LDS block
constexpr int NB_NT = 256;                  // threads per workgroup
constexpr int NB_CW = 16;                   // conformations per work item at most (LDS: NB_TJ * NB_CW float4)
constexpr int NB_JS = 16;                   // j slices at most

// conformations of a block of ni i-atoms are dealt out in nchunks work items of at most ncb
__host__ __device__ inline void nb_chunks(int ni, int C, int& nchunks, int& ncb) {
    int cpw = NB_NT / ni;
    if (cpw > NB_CW) cpw = NB_CW;
    nchunks = (C + cpw - 1) / cpw;
    ncb = (C + nchunks - 1) / nchunks;
}

__device__ inline int nb_clamp(int v, int N) { return v < 0 ? 0 : (v > N ? N : v); }

// the plan table as ints: [n_items, n_blocks, 0, 0 | blk_ptr[B+1], padded to a multiple of 4 | items: 4 per item]
inline long long nb_table_items0(long long B) { return 4 + ((B + 1 + 3) & ~3LL); }

struct NbTableView {
    const int* blk_ptr;                  // [B+1]: the first i-block of each molecule
    const int4* items;                   // {molecule, first i-atom, i-block, first conformation}
};
inline NbTableView nb_table_view(const int* table_dev, int B) { return {table_dev + 4, (const int4*)(table_dev + nb_table_items0(B))}; }

struct RsGeom {                          // what every per-item kernel needs of the batch
    int N, C, B, n_blocks;
    const int* atom_molptr;
    const int* blk_ptr;                  // [B+1]
    const int4* items;
};

struct RsItem {
    int mol, i0, blk, c0, m0, m1, ni, nc;
};

// the workgroup's item; false: a table made for another batch, which is walked away from, not followed
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

constexpr int RS_RUNNING = -1;           // status in the workspace of a stepwise path while an item runs

// which of the item's conformations still run -> run[0 .. nc); false if none does.  One barrier.
__device__ inline bool rs_running(const RsItem& r, int C, const int* __restrict__ status, int* run) {
    if ((int)threadIdx.x < r.nc) run[threadIdx.x] = status[(size_t)r.mol * C + r.c0 + threadIdx.x] == RS_RUNNING;
    __syncthreads();
    int any = 0;
    for (int cc = 0; cc < r.nc; ++cc) any |= run[cc];
    return any != 0;
}

// the j-tiles of the item's molecule, and the molecule's first block (tile jt of the molecule is the atoms of block nb_first_block + jt)
__device__ inline int nb_tiles(const RsItem& r) { return (r.m1 - r.m0 + NB_TJ - 1) / NB_TJ; }
__device__ inline int nb_first_block(const RsItem& r) { return r.blk - (r.i0 - r.m0) / NB_T; }

// a workspace dealt out front to back in pieces that start on 256-byte boundaries: the layouts of nonbonded.hip, relax_steps.hip and
// dynamics_steps.hip (base == NULL: sizes only)
struct WsCarve {
    char* base;
    size_t off = 0;
    size_t skip(size_t bytes) {          // -> the piece's offset
        const size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    }
    template <class T>
    T* take(size_t count) {
        return (T*)(base + skip(sizeof(T) * count));
    }
};

}  // namespace
