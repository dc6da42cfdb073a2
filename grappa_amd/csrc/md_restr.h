// Restraints on the stepwise dynamics (include/grappa_hip.h grappa_md_restr; csrc/dynamics_steps.hip): harmonic tethers to a
// reference structure and periodic dihedral restraints with one target per conformation,
//   E_r(b,c) = sum_r dih_k_r (1 - cos(phi_r - dih_target_{r,c})) + sum_i 0.5 pos_k_i |x_{i,c} - ref_{i,c}|^2,
// phi from dihedral_geom of csrc/mm_geom.h.  Three pieces:
//   gradient : in the force launch's epilogue (ms_force_body<.., RESTR = true> of csrc/dynamics_steps.hip, written into that kernel's
//              text): the owner of (atom, conformation) adds to the force field's gradient the molecule's rows that name its atom in
//              ascending r, then its tether.  The row range and the rows are workgroup-uniform loads; a row's four atoms are read from
//              x in global memory (they may lie in other blocks: x is only read in the force launch), so a row's geometry is computed by
//              up to four threads and no thread waits for another.
//   vet      : mr_vet_kernel at init, shaped like msc_vet_kernel.  Per (molecule, conformation): indices in [0, n), the four atoms of a
//              row distinct, dih_k finite and >= 0, the conformation's targets finite, pos_k finite and >= 0, at most
//              GRAPPA_RELAX_MAX_DIHEDRALS rows, dih_molptr monotone and within [0, R].  A refused item: status 5 and bit 2 of every
//              block's flag word, so it never runs.  A NaN target refuses its conformation only.  The epilogue and the energy kernel clamp
//              all the same (tables other than the ones init saw): no index of a table becomes an access out of range.
//              A non-finite pos_ref under a positive pos_k has no check of its own: it makes the gradient non-finite, which is status 2
//              by the force launch's own test.
//   energy   : mr_energy_kernel, one workgroup per (molecule, conformation) at the held coordinates: thread t adds the tethers of atoms
//              t, t + 256, .. in ascending order in double, the 256 rows are added in order (the scheme of nb_reduce_kernel), then the
//              dihedral rows in ascending r.
// Same input, same bits; no atomics.
#pragma once
#include <float.h>

#include "common.h"
#include "mm_geom.h"
#include "nb_plan.h"

namespace {

constexpr int MR_MAX = GRAPPA_RELAX_MAX_DIHEDRALS;
constexpr int MR_NT = 256;

struct MrDev {
    const float* pos_k;          // [N] or NULL
    const float* ref;            // [N,C,3]: the workspace's copy of the reference (read only with pos_k)
    const int* molptr;           // [B+1], NULL iff R == 0
    const int* atoms;            // [R,4] within the molecule
    const float* k;              // [R]
    const float* target;         // [R,C]
    int R;
};

// the rows of molecule mol, clamped: k0 .. k0 + nr with 0 <= nr <= MR_MAX inside [0, R]
__device__ __forceinline__ void mr_rows(const MrDev& m, int mol, int& k0, int& nr) {
    k0 = 0, nr = 0;
    if (m.R <= 0) return;
    k0 = nb_clamp(m.molptr[mol], m.R);
    const int k1 = nb_clamp(m.molptr[mol + 1], m.R);
    nr = k1 - k0 < 0 ? 0 : (k1 - k0 > MR_MAX ? MR_MAX : k1 - k0);
}

// row k of a molecule of n atoms: its atoms, false if one lies outside the molecule (such a row is not followed)
__device__ __forceinline__ bool mr_row(const MrDev& m, int k, int n, int4& at) {
    const int* p = m.atoms + 4 * (size_t)k;
    at = {p[0], p[1], p[2], p[3]};
    return (unsigned)at.x < (unsigned)n && (unsigned)at.y < (unsigned)n && (unsigned)at.z < (unsigned)n && (unsigned)at.w < (unsigned)n;
}

// ---- init: the reference into the workspace
__global__ __launch_bounds__(256) void mr_ref_kernel(size_t n3, const float* __restrict__ src, float* __restrict__ ref) {
    const size_t u = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (u < n3) ref[u] = src[u];
}

// ---- init: the tables vetted (the items of the molecule's first block, one per chunk of conformations, each decide the same for their
// own conformations from the same words)
__global__ __launch_bounds__(NB_NT) void mr_vet_kernel(RsGeom q, MrDev m, int* status, int* bad) {
    __shared__ int inv[NB_CW + 1];          // [0 .. nc): the conformation; [NB_CW]: the molecule
    RsItem r;
    if (!rs_item(q, r)) return;
    const int b0 = nb_clamp(q.blk_ptr[r.mol], q.n_blocks), b1 = nb_clamp(q.blk_ptr[r.mol + 1], q.n_blocks);
    if (r.blk != b0) return;
    const int C = q.C, t = threadIdx.x, n = r.m1 - r.m0;
    if (t <= NB_CW) inv[t] = 0;
    __syncthreads();
    int k0 = 0, nr = 0;
    if (m.R > 0) {
        const int p0 = m.molptr[r.mol], p1 = m.molptr[r.mol + 1];
        if (p0 < 0 || p1 < p0 || p1 > m.R || p1 - p0 > MR_MAX) {
            if (t == 0) inv[NB_CW] = 1;
        } else {
            k0 = p0, nr = p1 - p0;
        }
    }
    if (t < nr) {
        int4 at;
        bool ok = mr_row(m, k0 + t, n, at);
        if (at.x == at.y || at.x == at.z || at.x == at.w || at.y == at.z || at.y == at.w || at.z == at.w) ok = false;
        const float kr = m.k[k0 + t];
        if (!(kr >= 0.f && kr <= FLT_MAX)) ok = false;          // (a NaN is refused)
        if (!ok) inv[NB_CW] = 1;
        for (int cc = 0; cc < r.nc; ++cc)
            if (!(fabsf(m.target[(size_t)(k0 + t) * C + r.c0 + cc]) <= FLT_MAX)) inv[cc] = 1;
    }
    if (m.pos_k)
        for (int il = t; il < n; il += NB_NT) {
            const float pk = m.pos_k[r.m0 + il];
            if (!(pk >= 0.f && pk <= FLT_MAX)) inv[NB_CW] = 1;
        }
    __syncthreads();
    const int all = inv[NB_CW];
    if (t < r.nc && (all || inv[t])) status[(size_t)r.mol * C + r.c0 + t] = 5;
    for (int u = t; u < (b1 - b0) * r.nc; u += NB_NT) {
        const int cc = u % r.nc;
        if (all || inv[cc]) bad[(size_t)(b0 + u / r.nc) * C + r.c0 + cc] = 4;
    }
}

// ---- frames and finish: E_r and the restrained dihedrals at the held coordinates; one workgroup per (molecule, conformation)
struct MrEnergyArgs {
    int N, C, B;
    int final;               // 1: the finish (every item with atoms but a refused one); 0: a frame (running items only)
    const int* atom_molptr;
    const float* x;
    const int* status;
    MrDev m;
    float *erestr, *phi;     // [B,C], [R,C]; either may be NULL
};

__global__ __launch_bounds__(MR_NT) void mr_energy_kernel(MrEnergyArgs a) {
    __shared__ double part[MR_NT];
    __shared__ float erow[MR_MAX];
    const int C = a.C, t = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)C), c = (int)(blockIdx.x - (unsigned)b * (unsigned)C);
    if (b >= a.B) return;
    const int m0 = nb_clamp(a.atom_molptr[b], a.N), m1 = nb_clamp(a.atom_molptr[b + 1], a.N), n = m1 - m0;
    if (n <= 0) return;                                  // a molecule without atoms writes nothing
    const int st = a.status[(size_t)b * C + c];
    if (st == 5 || (!a.final && st != RS_RUNNING)) return;
    int k0, nr;
    mr_rows(a.m, b, k0, nr);
    double s = 0.0;
    if (a.m.pos_k)
        for (int il = t; il < n; il += MR_NT) {
            const float pk = a.m.pos_k[m0 + il];
            if (pk != 0.f) {
                const V3 dx = ldv(a.x, m0 + il, C, c) - ldv(a.m.ref, m0 + il, C, c);
                s += (double)(0.5f * pk * dot(dx, dx));
            }
        }
    part[t] = s;
    if (t < nr) {
        int4 at;
        float e = 0.f, phi = 0.f;
        if (mr_row(a.m, k0 + t, n, at)) {
            V3 d0, d1, d2, d3;
            phi = dihedral_geom(ldv(a.x, m0 + at.x, C, c), ldv(a.x, m0 + at.y, C, c), ldv(a.x, m0 + at.z, C, c), ldv(a.x, m0 + at.w, C, c), d0, d1,
                                d2, d3);
            e = a.m.k[k0 + t] * (1.0f - cosf(phi - a.m.target[(size_t)(k0 + t) * C + c]));
        }
        erow[t] = e;
        if (a.phi) a.phi[(size_t)(k0 + t) * C + c] = phi;
    }
    __syncthreads();
    if (t == 0 && a.erestr) {
        double tot = 0.0;
        for (int k = 0; k < MR_NT; ++k) tot += part[k];
        for (int k = 0; k < nr; ++k) tot += (double)erow[k];
        a.erestr[(size_t)b * C + c] = (float)tot;
    }
}

// no restraints at all: E_r = 0 for every molecule that has atoms
__global__ __launch_bounds__(256) void mr_zero_kernel(const int* __restrict__ atom_molptr, int N, int B, int C, float* __restrict__ erestr) {
    const size_t u = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= (size_t)B * C) return;
    const int b = (int)(u / (unsigned)C);
    if (nb_clamp(atom_molptr[b + 1], N) > nb_clamp(atom_molptr[b], N)) erestr[u] = 0.f;
}

}  // namespace
