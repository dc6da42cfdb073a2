// Temperature ladders and replica exchange on the stepwise dynamics (include/grappa_hip.h grappa_md_remd; csrc/dynamics_steps.hip).
// Every (molecule b, conformation c) is a replica: it keeps its coordinates, its noise stream and its index c; what moves is the SLOT of
// the ladder temperatures[C] it holds.  Per item the workspace keeps slot[b,c], its inverse who[b,s], kt_item[b,c] = ACC kB T_slot (what
// the thermostat step reads) and scale[b,c], the factor the last attempt left for the replica's velocities.  Four pieces:
//   init     : mx_init_kernel, one workgroup per molecule: the temperatures and the caller's slots_in row vetted (a bad one: status 5 and
//              bit 2 of every block's flag word, as refused restraint tables), then slot, who, kt_item and scale = 1.
//   exchange : ms_exchange_kernel, one workgroup per molecule, a thread per slot of the ladder (looping: C is not bounded by NB_CW).  The
//              thread of slot s = a (mod 2) with s + 1 < C decides the pair (s, s + 1) in double and, on acceptance, swaps slot, who and
//              kt_item of the two replicas and leaves their velocity factors in scale; the thread of a slot outside every pair writes
//              scale = 1.  Pairs of one attempt are disjoint, so every word has one writer.
//   rescale  : ms_rescale_kernel, one workgroup per work item: the owner of (atom, conformation) multiplies v by the replica's factor,
//              one thread per conformation the block's kinetic partial by its square in double.  Nothing is written where scale == 1.
//   finish   : mx_slots_out_kernel: the slots of every item that ran -> slots_out.
// Same input, same bits; no atomics; workgroups exchange data across launch boundaries only.
#pragma once
#include <float.h>
#include <math.h>

#include "common.h"
#include "md_noise.h"
#include "nb_plan.h"

namespace {

// ACC kB T as md_consts forms it: in double, rounded once
__host__ __device__ inline float mx_kt(float T) { return (float)(MD_ACC * MD_KB * (double)T); }

struct MxDev {
    const float* temperatures;   // [C], the caller's
    int *slot, *who;             // [B,C]: the slot replica c holds; the replica that holds slot s
    float *kt_item, *scale;      // [B,C]
    float *epot, *erestr;        // [B,C]: the energies of an attempt that no frame of the same step holds
};

// ---- init
struct MxInitArgs {
    int N, C, B, n_blocks;
    const int *atom_molptr, *blk_ptr;
    const int* slots_in;         // [B,C] or NULL: slot = c
    int exchanging;              // exchange_every > 0: a temperature of 0 is refused too
    MxDev x;
    int *status, *bad;
};

__global__ __launch_bounds__(256) void mx_init_kernel(MxInitArgs a) {
    const int b = (int)blockIdx.x, C = a.C, t = threadIdx.x;
    if (b >= a.B) return;
    const size_t row = (size_t)b * C;
    int invalid = 0;
    for (int c = t; c < C; c += 256) {
        const float T = a.x.temperatures[c];
        if (!(T >= 0.f && T <= FLT_MAX) || (a.exchanging && !(T > 0.f))) invalid = 1;      // (a NaN is refused)
        if (a.slots_in) {          // in range and met by no earlier conformation: C such values are a permutation
            const int s = a.slots_in[row + c];
            if ((unsigned)s >= (unsigned)C) invalid = 1;
            else
                for (int d = 0; d < c; ++d)
                    if (a.slots_in[row + d] == s) invalid = 1;
        }
    }
    invalid = __syncthreads_or(invalid);
    const bool some = nb_clamp(a.atom_molptr[b + 1], a.N) > nb_clamp(a.atom_molptr[b], a.N);
    const int k0 = nb_clamp(a.blk_ptr[b], a.n_blocks), k1 = nb_clamp(a.blk_ptr[b + 1], a.n_blocks);
    for (int c = t; c < C; c += 256) {
        const int s = invalid || !a.slots_in ? c : a.slots_in[row + c];      // (a refused row never runs: the identity keeps its words in range)
        a.x.slot[row + c] = s, a.x.who[row + s] = c;
        a.x.kt_item[row + c] = mx_kt(a.x.temperatures[s]), a.x.scale[row + c] = 1.0f;
        if (invalid && some) {
            a.status[row + c] = 5;
            for (int k = k0; k < k1; ++k) a.bad[(size_t)k * C + c] = 4;
        }
    }
}

// ---- an attempt
struct MxExchArgs {
    int N, C, B, n_blocks;
    const int *atom_molptr, *blk_ptr;
    const unsigned long long* mol_key;
    const int *status, *bad;
    MxDev x;
    const float *epot, *erestr;  // [B,C] at this step; erestr NULL: 0
    unsigned g;                  // the global index of the step behind which the attempt comes; the attempt's number is g / K
    int parity;                  // (g / K) & 1
    int* log_slot;               // the attempt's rows of the logs [B,C], or NULL
    float *log_epot, *log_erestr;
};

// does replica c of molecule b still run (status, and no flag on any of its blocks)?  -> its energies too
__device__ __forceinline__ bool mx_live(const MxExchArgs& a, size_t row, int c, int k0, int k1, float& ep, float& er) {
    ep = a.epot[row + c], er = a.erestr ? a.erestr[row + c] : 0.f;
    if (a.status[row + c] != RS_RUNNING) return false;
    int f = 0;
    for (int k = k0; k < k1; ++k) f |= a.bad[(size_t)k * a.C + c];
    return f == 0;
}

// the rows of the logs of replica c: its slot behind the attempt, and the energies the decision read (NaN for a replica that no longer
// runs; a refused one, status 5, is not written at all)
__device__ __forceinline__ void mx_log(const MxExchArgs& a, size_t row, int c, int s, bool live, float ep, float er) {
    if (a.status[row + c] == 5) return;
    if (a.log_slot) a.log_slot[row + c] = s;
    if (a.log_epot) a.log_epot[row + c] = live ? ep : NAN;
    if (a.log_erestr) a.log_erestr[row + c] = live ? er : NAN;
}

__global__ __launch_bounds__(256) void ms_exchange_kernel(MxExchArgs a) {
    const int b = (int)blockIdx.x, C = a.C;
    if (b >= a.B) return;
    if (nb_clamp(a.atom_molptr[b + 1], a.N) <= nb_clamp(a.atom_molptr[b], a.N)) return;      // a molecule without atoms has no replicas
    const size_t row = (size_t)b * C;
    const int k0 = nb_clamp(a.blk_ptr[b], a.n_blocks), k1 = nb_clamp(a.blk_ptr[b + 1], a.n_blocks);
    const unsigned long long key = a.mol_key[b];
    for (int s = (int)threadIdx.x; s < C; s += 256) {
        const bool even = ((s ^ a.parity) & 1) == 0;
        if (!even && s >= 1) continue;                       // the upper slot of a pair: its lower slot's thread writes for it
        const int lo = a.x.who[row + s];
        if ((unsigned)lo >= (unsigned)C) continue;           // (a workspace that init did not write is not followed)
        float ep_lo, er_lo, ep_hi, er_hi;
        const bool live_lo = mx_live(a, row, lo, k0, k1, ep_lo, er_lo);
        if (!even || s + 1 >= C) {                           // a slot outside every pair of this attempt
            a.x.scale[row + lo] = 1.0f;
            mx_log(a, row, lo, s, live_lo, ep_lo, er_lo);
            continue;
        }
        const int hi = a.x.who[row + s + 1];
        if ((unsigned)hi >= (unsigned)C) continue;
        const bool live_hi = mx_live(a, row, hi, k0, k1, ep_hi, er_hi);
        const double u_lo = (double)ep_lo + (double)er_lo, u_hi = (double)ep_hi + (double)er_hi;
        const float t_s = a.x.temperatures[s], t_h = a.x.temperatures[s + 1];
        bool accept = false;
        if (live_lo && live_hi && fabs(u_lo) <= DBL_MAX && fabs(u_hi) <= DBL_MAX) {      // (a NaN is not attempted)
            const double d = (1.0 / (MD_KB * (double)t_s) - 1.0 / (MD_KB * (double)t_h)) * (u_lo - u_hi);
            uint32_t w[4];
            grappa_philox4x32_10((uint32_t)key, (uint32_t)(key >> 32), (uint32_t)s, 0u, a.g, 2u, w);
            const double u = ((double)w[0] + 0.5) * 0x1p-32;
            accept = d >= 0.0 || u < exp(d);
        }
        if (accept) {
            a.x.slot[row + lo] = s + 1, a.x.slot[row + hi] = s;
            a.x.who[row + s] = hi, a.x.who[row + s + 1] = lo;
            a.x.kt_item[row + lo] = mx_kt(t_h), a.x.kt_item[row + hi] = mx_kt(t_s);
            a.x.scale[row + lo] = (float)sqrt((double)t_h / (double)t_s), a.x.scale[row + hi] = (float)sqrt((double)t_s / (double)t_h);
        } else {
            a.x.scale[row + lo] = 1.0f, a.x.scale[row + hi] = 1.0f;
        }
        mx_log(a, row, lo, accept ? s + 1 : s, live_lo, ep_lo, er_lo);
        mx_log(a, row, hi, accept ? s : s + 1, live_hi, ep_hi, er_hi);
    }
}

// ---- the velocities and the kinetic partials of the replicas an attempt swapped
struct MxRescaleArgs {
    RsGeom q;
    float* v;
    double* kpart;
    const float* scale;
};

__global__ __launch_bounds__(NB_NT) void ms_rescale_kernel(MxRescaleArgs a) {
    RsItem r;
    if (!rs_item(a.q, r)) return;
    const int C = a.q.C, t = threadIdx.x;
    if (t >= r.ni * r.nc) return;
    const int cl = t / r.ni, il = t - cl * r.ni, c = r.c0 + cl;
    const float f = a.scale[(size_t)r.mol * C + c];
    if (f == 1.0f) return;
    const size_t off = ((size_t)(r.i0 + il) * C + c) * 3;
    a.v[off] *= f, a.v[off + 1] *= f, a.v[off + 2] *= f;
    if (il == 0) a.kpart[(size_t)r.blk * C + c] *= (double)f * f;
}

// ---- finish: the slot of every item of a molecule with atoms but a refused one (slot == NULL: no ladder, c)
__global__ __launch_bounds__(256) void mx_slots_out_kernel(const int* __restrict__ atom_molptr, int N, int B, int C, const int* __restrict__ status,
                                                           const int* __restrict__ slot, int* __restrict__ out) {
    const size_t u = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= (size_t)B * C) return;
    const int b = (int)(u / (unsigned)C);
    if (nb_clamp(atom_molptr[b + 1], N) <= nb_clamp(atom_molptr[b], N) || status[u] == 5) return;
    out[u] = slot ? slot[u] : (int)(u - (size_t)b * C);
}

}  // namespace
