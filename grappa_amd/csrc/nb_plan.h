// The work-item decomposition of the nonbonded plan (include/grappa_hip.h grappa_nonbonded_plan), shared by csrc/nonbonded.hip and
// csrc/relax_steps.hip: ONE definition of the block sizes and of how a block's conformations are dealt out, so that both read the same
// table the same way.
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

}  // namespace
