// The energy reduction of the tiled pair kernels: the partial energies a work item's workgroup leaves per (i-block, conformation), added
// per molecule -- ONE text for the nonbonded kernel (csrc/nonbonded.hip) and the implicit solvent (csrc/gb_obc.hip), whose two terms
// (polar, surface area) take the places of Lennard-Jones and Coulomb.
#pragma once
#include "common.h"
#include "nb_plan.h"

namespace {

// ------------------------------------------------------------------------------------------------ reduce
// one workgroup per molecule; thread (r, conformation) adds the blocks r, r + R, .. and the R rows are added in order
__global__ __launch_bounds__(NB_NT) void nb_reduce_kernel(int C, int B, const int* __restrict__ blk_ptr, const double* __restrict__ part,
                                                          float* __restrict__ energy, float* __restrict__ term_energy) {
    __shared__ double red[2][NB_NT];
    const int b = blockIdx.x, t = threadIdx.x;
    const int k0 = blk_ptr[b], k1 = blk_ptr[b + 1];
    const int cs = C < NB_NT ? C : NB_NT, R = NB_NT / cs;
    const int r = t / cs, cl = t - r * cs;
    for (int cb = 0; cb < C; cb += cs) {
        const int c = cb + cl;
        const bool ok = r < R && c < C;
        double slj = 0.0, sc = 0.0;
        if (ok)
            for (int k = k0 + r; k < k1; k += R) {
                const double* p = part + ((size_t)k * C + c) * 2;
                slj += p[0], sc += p[1];
            }
        red[0][t] = slj, red[1][t] = sc;
        __syncthreads();
        if (ok && r == 0) {
            for (int q = 1; q < R; ++q) slj += red[0][q * cs + cl], sc += red[1][q * cs + cl];
            energy[(size_t)b * C + c] = (float)(slj + sc);
            if (term_energy) {
                term_energy[(size_t)b * C + c] = (float)slj;
                term_energy[((size_t)B + b) * C + c] = (float)sc;
            }
        }
        __syncthreads();
    }
}

}  // namespace
