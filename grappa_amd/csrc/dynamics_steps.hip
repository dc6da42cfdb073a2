// Stepwise Langevin dynamics (BAOAB) for molecules of any size under the full MM force field, fp32 (include/grappa_hip.h
// grappa_md_steps_*_f32): the loop of csrc/dynamics.hip with a molecule spread over many workgroups and a step made of two launches.
//   items  : the nonbonded plan's (csrc/nb_plan.h, walked as csrc/rs_force.h walks them): (molecule, block of ni <= 64 i-atoms, nc
//            conformations), one workgroup of 256 threads each; the plan is about atoms, so it also serves a call without nonbonded parameters.
//   state  : in the caller's workspace: x, v, g [N,C,3]; per (molecule, conformation) status (running / 2) and steps; per (block,
//            conformation) the flag of a non-finite gradient and the kinetic partial sum m v^2 (double); the scratch of the energy kernels.
//   step   : move   a thread per (atom, conformation) of the item.  Every workgroup of a molecule ORs the flags of ALL the molecule's
//                   blocks (written by the force launch before it) and leaves a flagged conformation untouched; otherwise B, A, O, A
//                   on its own atoms.  The workgroup of the molecule's FIRST block is the one writer of status and steps.
//            force  g at the new x (rs_force of csrc/rs_force.h, the force of the stepwise minimiser), then per owner thread the closing
//                   kick, the non-finite test, the frame's coordinates on a frame step, and per (block, conformation) the flag and the
//                   kinetic partial over the block's atoms in ascending order in double.  It reads status, which the move launch wrote.
//            Launch boundaries are the only synchronisation between workgroups: no cooperative launch, no flag that is waited on, no
//            atomics.  Every word has one writer per launch, and no workgroup reads in a launch what a sibling writes in it: move reads
//            flags and writes status, force reads status and writes flags.
//   stopped: a flag, once set, stays: the force launch leaves a stopped conformation alone, so its flags, x, v, g and partials keep the
//            values of the step that found the non-finite gradient, whatever is enqueued afterwards.
//   frames : coordinates by the force launch of a frame step; energies, if asked for, by the library's own energy kernels at the held
//   and end  coordinates (mm_energy_kernel, nb_pairs_kernel + nb_reduce_kernel through their entry points: no second energy code path)
//            and one small launch that adds the six terms in double in term order and the kinetic partials in ascending block order.
//   noise  : csrc/md_noise.h, keyed by (mol_key, atom WITHIN the molecule, conformation, global step, purpose): the fused kernel's stream.
//   options: a run may have a nonbonded cutoff, X-H constraints, an implicit solvent (with or without a cutoff of its own) and
//            restraints.  Every entry resolves the optional pointers it takes into ONE plan (MsPlan, ms_plan: the section "the run plan"
//            below) -- what the run has, every refusal, the derived flags -- and ms_init / ms_run / ms_finish act on that plan with the
//            workspace carved for it in one place (ms_carve).  The six families of entries (plain, _cut_, _cons_, _gb_, _gbcut_,
//            _restr_) differ in the pointers they take and in nothing else: a family is the widest call with the others NULL, and an
//            option that is absent (NULL; K == 0; R == 0 without tethers) launches what the family without it launches.
//   cutoff : the force launch is rs_force under the cut policy of csrc/nb_cut.h; the move launch's item writes the box of its own
//            (block, conformations) after moving -- the box's only writer -- and the force launch reads all boxes across the launch
//            boundary: a step stays two launches, init gains one (boxes and exception ranges).  Energies by
//            grappa_nonbonded_fwd_cut_f32 at the held coordinates.
//   constraints: X-H star clusters under g-BAOAB with P and S of csrc/md_cons.h; a cluster is integrated by the thread of its centre,
//            and a step becomes move, boxes (with a cutoff), force, close: the section "X-H constraints" below states the
//            decomposition, the launches and the hazards.
//   solvent: the section "implicit solvent" below: the force launch as it is, without its closing kick, then born, pair and chain of
//            csrc/gb_pass.h; the chain launch's epilogue closes the step.
//   restraints: tethers and dihedral restraints of csrc/md_restr.h: their gradient is added to the owner's gi at the head of the force
//            launch's epilogue, the one place every Hamiltonian above passes through (the section "restraints" below); a step gains
//            no launch, init gains two.
//   ladders: a temperature per conformation and replica exchange between neighbouring slots (csrc/md_remd.h, the section "ladders"
//            below; the entries grappa_md_remd_*_f32): the move launch reads kt of the item's slot, and behind every K-th step an
//            exchange launch and a rescale launch follow the energy launches of a frame; a step gains no launch.
// Same input, same bits; a molecule's bits depend neither on its place in the batch nor on how the steps are dealt out to run calls.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"
#include "desc_check.h"
#include "gb_pass.h"
#include "md_cons.h"
#include "md_noise.h"
#include "md_remd.h"
#include "md_restr.h"
#include "rs_force.h"

namespace {

constexpr int MS_NW = NB_NT / GRAPPA_WAVE;

struct MsWs {
    float *x, *v, *g;                    // [N,C,3]
    int *status, *steps;                 // [B,C]
    int* bad;                            // [n_blocks][C]: the block holds a non-finite gradient
    double* kpart;                       // [n_blocks][C]: sum m v^2 over the block's atoms
    float *e_mm, *e_nb, *terms;          // frames and finish: [B,C], [B,C], [6,B,C]
    double* nbpart;                      // frames and finish: the nonbonded kernel's partial energies [n_blocks][C][2]
    float4* box;                         // with a cutoff: the blocks' boxes [n_blocks][C][2] and exception ranges [n_blocks] (csrc/nb_cut.h)
    int2* er;
    char* nbcut;                         // with a cutoff, frames and finish: the workspace of grappa_nonbonded_fwd_cut_f32
    size_t nbcut_bytes;
    int* claim;                          // with constraints: per atom the cluster that holds it, -1: none [N]
    int* cfail;                          // with constraints: a cluster owned by the block did not converge [n_blocks][C]
    size_t total;
};

// (the words of a cutoff lie behind the others, those of constraints behind both: without either the layout is the one it was)
MsWs ms_layout(char* base, int N, int C, int B, int n_blocks, bool cut, bool cons) {
    MsWs w;
    WsCarve k{base};
    const size_t n3 = (size_t)N * C * 3, bc = (size_t)B * C, kc = (size_t)n_blocks * C;
    w.x = k.take<float>(n3), w.v = k.take<float>(n3), w.g = k.take<float>(n3);
    w.status = k.take<int>(bc), w.steps = k.take<int>(bc);
    w.bad = k.take<int>(kc);
    w.kpart = k.take<double>(kc);
    w.e_mm = k.take<float>(bc), w.e_nb = k.take<float>(bc), w.terms = k.take<float>(6 * bc);
    w.nbpart = k.take<double>(2 * kc);
    w.box = nullptr, w.er = nullptr, w.nbcut = nullptr, w.nbcut_bytes = 0;
    if (cut) {
        w.box = k.take<float4>(2 * kc), w.er = k.take<int2>((size_t)n_blocks);
        w.nbcut_bytes = grappa_nonbonded_cut_workspace_bytes(C, n_blocks);
        w.nbcut = k.take<char>(w.nbcut_bytes);
    }
    w.claim = nullptr, w.cfail = nullptr;
    if (cons) w.claim = k.take<int>((size_t)N), w.cfail = k.take<int>(kc);
    w.total = k.off;
    return w;
}

// ------------------------------------------------------------------------------------------------ init
struct MsInitArgs {
    int N, C, B, n_blocks;
    const int* atom_molptr;
    const float *start, *vel_in, *mass;
    const unsigned long long* mol_key;
    float kt0;
    unsigned first_step;
    MsWs w;
    const float* lad_t;      // the ladder form: temperatures[C], the start velocities drawn at the replica's slot temperature
    const int* lad_slots;    // ... the caller's slots_in [B,C], or NULL: slot = c
};

// a thread per (atom, conformation): x = start, v = vel_in (a frozen atom: 0) or the draw at init_temperature; the first B * C threads
// also set the items' state, the first n_blocks * C the blocks' words
// LADDER: kt0 per conformation, ACC kB T of the slot the replica starts in (a slot out of range, which mx_init_kernel refuses, is clamped)
template <bool LADDER>
__device__ __forceinline__ void ms_init_body(const MsInitArgs& a) {
    const size_t u = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int N = a.N, C = a.C, B = a.B;
    if (u < (size_t)N * C) {
        const int atom = (int)(u / (unsigned)C), c = (int)(u - (size_t)atom * C);
        V3 v = {0.f, 0.f, 0.f};
        const float m = a.mass[atom];
        if (m > 0.f) {          // (a mass that is zero, negative or NaN: a frozen atom, v = 0)
            if (a.vel_in) {
                v = {a.vel_in[3 * u], a.vel_in[3 * u + 1], a.vel_in[3 * u + 2]};
            } else if (LADDER || a.kt0 > 0.f) {
                int lo = 0, hi = B - 1;          // the last molecule that starts at or before the atom
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (nb_clamp(a.atom_molptr[mid], N) <= atom) lo = mid; else hi = mid - 1;
                }
                const int m0 = nb_clamp(a.atom_molptr[lo], N), m1 = nb_clamp(a.atom_molptr[lo + 1], N);
                float kt0 = a.kt0;
                if constexpr (LADDER) {
                    const int s = a.lad_slots ? a.lad_slots[(size_t)lo * C + c] : c;
                    kt0 = mx_kt(a.lad_t[s < 0 ? 0 : (s >= C ? C - 1 : s)]);
                }
                if (atom >= m0 && atom < m1 && (!LADDER || kt0 > 0.f))          // (an atom that no molecule holds keeps v = 0)
                    v = sqrtf(kt0 * (1.0f / m)) * md_normal3(a.mol_key[lo], (unsigned)(atom - m0), (unsigned)c, a.first_step, 1u);
            }
        }
        a.w.x[3 * u] = a.start[3 * u], a.w.x[3 * u + 1] = a.start[3 * u + 1], a.w.x[3 * u + 2] = a.start[3 * u + 2];
        a.w.v[3 * u] = v.x, a.w.v[3 * u + 1] = v.y, a.w.v[3 * u + 2] = v.z;
        a.w.g[3 * u] = 0.f, a.w.g[3 * u + 1] = 0.f, a.w.g[3 * u + 2] = 0.f;
    }
    if (u < (size_t)B * C) {
        const int b = (int)(u / (unsigned)C);
        const bool some = nb_clamp(a.atom_molptr[b + 1], N) > nb_clamp(a.atom_molptr[b], N);
        a.w.status[u] = some ? RS_RUNNING : 0;      // a molecule without atoms never runs (and the finish writes nothing for it)
        a.w.steps[u] = 0;
    }
    if (u < (size_t)a.n_blocks * C) a.w.bad[u] = 0, a.w.kpart[u] = 0.0;
}

__global__ __launch_bounds__(256) void ms_init_kernel(MsInitArgs a) { ms_init_body<false>(a); }
__global__ __launch_bounds__(256) void ms_init_ladder_kernel(MsInitArgs a) { ms_init_body<true>(a); }

// ------------------------------------------------------------------------------------------------ move
struct MsMoveArgs {
    RsGeom q;
    float *x, *v;
    const float *g, *mass;
    const unsigned long long* mol_key;
    const int* bad;
    int *status, *steps;
    MdConsts k;
    unsigned step;           // the global index of the step: the random stream's position
    const float* kt_item;    // the ladder form: ACC kB T of the slot each item holds [B,C] (csrc/md_remd.h), read in place of k.kt
};

// ACC kB T of the thermostat step: the call's, or on a ladder (csrc/md_remd.h) that of the slot the item holds
template <bool LADDER>
__device__ __forceinline__ float ms_kt(const MsMoveArgs& a, size_t item) {
    if constexpr (LADDER) return a.kt_item[item];
    else return a.k.kt;
}

// B, A, O, A on atom i of conformation c (a frozen atom is not touched); CUT: the coordinates it leaves -> bxl[0..3)
template <bool CUT, bool LADDER = false>
__device__ __forceinline__ void ms_move_atom(const MsMoveArgs& a, const RsItem& r, int i, int c, float* bxl) {
    const int C = a.q.C;
    const float m = a.mass[i];
    if (m > 0.f) {                                   // (a frozen atom is not touched)
        const size_t off = ((size_t)i * C + c) * 3;
        const float im = 1.0f / m, kw = a.k.hk * im;
        const V3 gi = {a.g[off], a.g[off + 1], a.g[off + 2]};
        V3 vk = {a.v[off], a.v[off + 1], a.v[off + 2]};
        vk = vk - kw * gi;
        float xx = a.x[off], xy = a.x[off + 1], xz = a.x[off + 2];
        xx += a.k.h2 * vk.x, xy += a.k.h2 * vk.y, xz += a.k.h2 * vk.z;
        if (a.k.thermostat)
            vk = a.k.c1 * vk + (a.k.c2 * sqrtf(ms_kt<LADDER>(a, (size_t)r.mol * C + c) * im)) * md_normal3(a.mol_key[r.mol], (unsigned)(i - r.m0), (unsigned)c, a.step, 0u);
        xx += a.k.h2 * vk.x, xy += a.k.h2 * vk.y, xz += a.k.h2 * vk.z;
        a.x[off] = xx, a.x[off + 1] = xy, a.x[off + 2] = xz;
        a.v[off] = vk.x, a.v[off + 1] = vk.y, a.v[off + 2] = vk.z;
        if constexpr (CUT) bxl[0] = xx, bxl[1] = xy, bxl[2] = xz;
    } else if constexpr (CUT) {
        const size_t off = ((size_t)i * C + c) * 3;
        bxl[0] = a.x[off], bxl[1] = a.x[off + 1], bxl[2] = a.x[off + 2];
    }
}

// the thread's (atom, conformation) of the item; CUT: the coordinates it leaves -> bxl[0..3) (not for a stopped conformation)
// KEEP (with restraints): a stopped item that no longer runs keeps the status it has (5: its tables were refused)
template <bool CUT, bool KEEP = false, bool LADDER = false>
__device__ __forceinline__ void ms_move_lane(const MsMoveArgs& a, const RsItem& r, int k0, const int* stop, float* bxl) {
    const int C = a.q.C, t = threadIdx.x, ni = r.ni;
    const int cl = t / ni, il = t - cl * ni;
    const int i = r.i0 + il, c = r.c0 + cl;
    const size_t item = (size_t)r.mol * C + c;
    const bool writer = r.blk == k0 && il == 0;      // the molecule's first block: the one writer of the item's status and steps
    if (stop[cl]) {                                  // a non-finite gradient: the item keeps the x and v it holds
        if constexpr (KEEP) {
            if (writer && a.status[item] == RS_RUNNING) a.status[item] = 2;
        } else {
            if (writer) a.status[item] = 2;
        }
        return;
    }
    ms_move_atom<CUT, LADDER>(a, r, i, c, bxl);
    if (writer) a.steps[item] += 1;
}

// Has a block of the molecule flagged the conformation?  -> stop[0 .. nc), then a barrier.  Every workgroup of the molecule forms the same
// OR from the same words, which the force launch before this one wrote: wavefront w takes the conformations w, w + 4, .., its lanes the
// blocks.  BITS: the OR of the words themselves (with constraints a word holds more than one flag), else 1.
template <bool BITS>
__device__ __forceinline__ void ms_stop_flags(const int* bad, const RsItem& r, int C, int k0, int k1, int* stop) {
    const int t = threadIdx.x, wave = t / GRAPPA_WAVE, lane = t & (GRAPPA_WAVE - 1);
    for (int cc = wave; cc < r.nc; cc += MS_NW) {
        int f = 0;
        for (int k = k0 + lane; k < k1; k += GRAPPA_WAVE) f |= bad[(size_t)k * C + r.c0 + cc];
        if constexpr (BITS) {
            int code = 0;
            for (int bit = 1; bit <= 4; bit <<= 1) code |= __builtin_amdgcn_ballot_w64((f & bit) != 0) != 0 ? bit : 0;
            if (lane == 0) stop[cc] = code;
        } else {
            const bool any = __builtin_amdgcn_ballot_w64(f != 0) != 0;
            if (lane == 0) stop[cc] = any ? 1 : 0;
        }
    }
    __syncthreads();
}

// CUT: the item also writes the box of its own (block, conformations) at the coordinates it leaves (csrc/nb_cut.h): it is the box's only
// writer, the force launch after it the reader.  A stopped conformation keeps its box, as it keeps its x.
template <bool CUT, bool KEEP = false, bool LADDER = false>
__device__ __forceinline__ void ms_move_body(const MsMoveArgs& a, float4* box) {
    __shared__ int stop[NB_CW];
    RsItem r;
    if (!rs_item(a.q, r)) return;
    const int C = a.q.C, t = threadIdx.x, ni = r.ni;
    const int k0 = nb_clamp(a.q.blk_ptr[r.mol], a.q.n_blocks), k1 = nb_clamp(a.q.blk_ptr[r.mol + 1], a.q.n_blocks);
    ms_stop_flags<false>(a.bad, r, C, k0, k1, stop);
    if constexpr (CUT) {
        __shared__ float bx[NB_NT * 3];
        if (t < ni * r.nc) ms_move_lane<true, KEEP, LADDER>(a, r, k0, stop, bx + 3 * t);
        nb_cut_box_write(bx, stop, ni, r.nc, r.blk, C, r.c0, box);
    } else {
        if (t < ni * r.nc) ms_move_lane<false, KEEP, LADDER>(a, r, k0, stop, nullptr);
    }
}

__global__ __launch_bounds__(NB_NT) void ms_move_kernel(MsMoveArgs a) { ms_move_body<false>(a, nullptr); }
__global__ __launch_bounds__(NB_NT) void ms_move_cut_kernel(MsMoveArgs a, float4* box) { ms_move_body<true>(a, box); }
__global__ __launch_bounds__(NB_NT) void ms_move_restr_kernel(MsMoveArgs a) { ms_move_body<false, true>(a, nullptr); }
__global__ __launch_bounds__(NB_NT) void ms_move_restr_cut_kernel(MsMoveArgs a, float4* box) { ms_move_body<true, true>(a, box); }
// on a ladder (csrc/md_remd.h): new kernels, the four above are what they were.  The ladder's vet may refuse an item (5), so both are KEEP
__global__ __launch_bounds__(NB_NT) void ms_move_ladder_kernel(MsMoveArgs a) { ms_move_body<false, true, true>(a, nullptr); }
__global__ __launch_bounds__(NB_NT) void ms_move_cut_ladder_kernel(MsMoveArgs a, float4* box) { ms_move_body<true, true, true>(a, box); }

// ------------------------------------------------------------------------------------------------ force
struct MsForceArgs {
    RsForceIn f;             // the force of csrc/rs_force.h
    float *v, *g;
    const float* mass;
    int* bad;
    double* kpart;
    float hk;                // dt / 2 ACC; 0: no closing kick (the gradient of init)
    float* frame_xyz;        // the frame this step writes, or NULL
};

// CONS (with constraints): the block's flag word also takes, as bit 1, the constraint-failure word that the launch before this one left for
// the block (cfail), and the kinetic partial is left to the close launch, which follows the closing P
// RESTR (with restraints, csrc/md_restr.h): the owner adds to gi -- before g is written, before the closing kick and before the
// non-finite test -- the molecule's restrained dihedrals that name its atom in ascending r, then its tether.  The row range and the rows
// are workgroup-uniform loads; the rows' atoms are read from x in global memory, which no launch writes while the force launch runs.
template <bool CONS = false, bool RESTR = false, class Cut>
__device__ __forceinline__ void ms_force_body(const MsForceArgs& a, const Cut& cut, const int* cfail = nullptr, const MrDev& mr = MrDev{}) {
    __shared__ RsShared sh;
    rs_force(a.f, sh, cut, [&](const RsItem& r, const RsLane& w, V3 gi) {
        const int C = a.f.q.C, ni = r.ni;
        float mv2 = 0.f, bad = 0.f;
        if constexpr (RESTR) {
            int k0, nr;
            mr_rows(mr, r.mol, k0, nr);
            if (w.owner) {
                const int n = r.m1 - r.m0, il = w.i - r.m0;
                for (int k = k0; k < k0 + nr; ++k) {
                    int4 at;
                    if (!mr_row(mr, k, n, at)) continue;
                    const int p = at.x == il ? 0 : (at.y == il ? 1 : (at.z == il ? 2 : (at.w == il ? 3 : -1)));
                    if (p >= 0) {
                        V3 d0, d1, d2, d3;
                        const float phi = dihedral_geom(ldv(a.f.x, r.m0 + at.x, C, w.c), ldv(a.f.x, r.m0 + at.y, C, w.c),
                                                        ldv(a.f.x, r.m0 + at.z, C, w.c), ldv(a.f.x, r.m0 + at.w, C, w.c), d0, d1, d2, d3);
                        const float coef = mr.k[k] * sinf(phi - mr.target[(size_t)k * C + w.c]);
                        gi = gi + coef * (p == 0 ? d0 : (p == 1 ? d1 : (p == 2 ? d2 : d3)));
                    }
                }
                if (mr.pos_k) {
                    const float pk = mr.pos_k[w.i];
                    if (pk != 0.f) gi = gi + pk * (ldv(a.f.x, w.i, C, w.c) - ldv(mr.ref, w.i, C, w.c));
                }
            }
        }
        if (w.owner) {
            const size_t off = ((size_t)w.i * C + w.c) * 3;
            a.g[off] = gi.x, a.g[off + 1] = gi.y, a.g[off + 2] = gi.z;
            const float m = a.mass[w.i];
            V3 vi = {a.v[off], a.v[off + 1], a.v[off + 2]};
            if (m > 0.f) {
                if (a.hk > 0.f) {          // the closing B of the step
                    vi = vi - (a.hk * (1.0f / m)) * gi;
                    a.v[off] = vi.x, a.v[off + 1] = vi.y, a.v[off + 2] = vi.z;
                }
                mv2 = m * dot(vi, vi);
            }
            if (!(sqrtf(dot(gi, gi)) <= FLT_MAX)) bad = 1.f;      // (written so that a NaN counts as non-finite)
            if (a.frame_xyz) {
                const float* p = a.f.x + off;
                a.frame_xyz[off] = p[0], a.frame_xyz[off + 1] = p[1], a.frame_xyz[off + 2] = p[2];
            }
        }
        __syncthreads();
        if (w.owner) sh.red[0][w.l] = mv2, sh.red[1][w.l] = bad;
        __syncthreads();
        if (w.owner && w.il == 0) {      // the block's words of one conformation: over its atoms in ascending order, in double
            double sk = 0.0;
            float fb = 0.f;
            for (int k = 0; k < ni; ++k) {
                const int o = w.cl * ni + k;
                sk += (double)sh.red[0][o];
                fb = fmaxf(fb, sh.red[1][o]);
            }
            const size_t o = (size_t)r.blk * C + w.c;
            if constexpr (CONS) {
                a.bad[o] = (fb != 0.f ? 1 : 0) | (cfail[o] != 0 ? 2 : 0);
            } else {
                a.kpart[o] = sk;
                a.bad[o] = fb != 0.f ? 1 : 0;
            }
        }
    });
}

__global__ __launch_bounds__(NB_NT) void ms_force_kernel(MsForceArgs a) { ms_force_body(a, NbNoCut{}); }

__global__ __launch_bounds__(NB_NT) void ms_force_cut_kernel(MsForceArgs a, NbCutDev c) {
    __shared__ unsigned char near[NB_NT];
    ms_force_body(a, NbCut{c, near});
}

__global__ __launch_bounds__(NB_NT) void ms_force_cons_kernel(MsForceArgs a, const int* cfail) { ms_force_body<true>(a, NbNoCut{}, cfail); }

__global__ __launch_bounds__(NB_NT) void ms_force_cons_cut_kernel(MsForceArgs a, NbCutDev c, const int* cfail) {
    __shared__ unsigned char near[NB_NT];
    ms_force_body<true>(a, NbCut{c, near}, cfail);
}

// the four with restraints: new kernels, the four above are what they were
__global__ __launch_bounds__(NB_NT) void ms_force_restr_kernel(MsForceArgs a, MrDev m) { ms_force_body<false, true>(a, NbNoCut{}, nullptr, m); }

__global__ __launch_bounds__(NB_NT) void ms_force_restr_cut_kernel(MsForceArgs a, NbCutDev c, MrDev m) {
    __shared__ unsigned char near[NB_NT];
    ms_force_body<false, true>(a, NbCut{c, near}, nullptr, m);
}

__global__ __launch_bounds__(NB_NT) void ms_force_restr_cons_kernel(MsForceArgs a, const int* cfail, MrDev m) {
    ms_force_body<true, true>(a, NbNoCut{}, cfail, m);
}

__global__ __launch_bounds__(NB_NT) void ms_force_restr_cons_cut_kernel(MsForceArgs a, NbCutDev c, const int* cfail, MrDev m) {
    __shared__ unsigned char near[NB_NT];
    ms_force_body<true, true>(a, NbCut{c, near}, cfail, m);
}

// ------------------------------------------------------------------------------------------------ X-H constraints (grappa_md_steps_*_cons_f32)
// g-BAOAB with the star clusters, P and S of csrc/md_cons.h, stated in include/grappa_hip.h at grappa_md_langevin_cons_f32.
//   owner  : a cluster is integrated, all its atoms together, by the thread of its CENTRE -- the lane that the centre atom has in the
//            work item of its block -- with the cluster's coordinates and velocities in registers; its leaves may lie in any block of
//            the molecule.  A clustered atom is skipped by its ordinary owner; a free atom moves exactly as in ms_move_kernel.
//   claim  : one word per atom, written during init: the cluster that holds the atom, -1 for a free atom.  It vets "no atom in two
//            clusters" across workgroups (a launch stores, the next reads back) and then IS the ownership list: lane il of a block owns
//            the cluster claim[i0 + il] if that atom is its centre, so a block's clusters are walked in ascending order of their centres
//            with no list to build.
//   step   : move (clusters: B P | A S P | O P | A S P, free atoms: B A O A; the block's constraint-failure word, fresh each launch),
//            boxes (with a cutoff: rs_box_kernel, since a block's atoms may be moved by a sibling), force (the kick of every atom by
//            its owner; the block's flag word takes the failure word as bit 1), close (clusters: P; the block's kinetic partial):
//            three launches, four under a cutoff.
//   hazards: as above, every word has one writer per launch and no workgroup reads what a sibling writes in the same launch.  x and v of
//            a clustered atom are read and written by the centre's thread alone in move and close, by the atom's owner alone in
//            force; cfail is written by move (its block) and read by force (its block); the flags are written by force and read by
//            move; status and steps are written and read by the first block's move alone, and read by the later launches of the step.
//   flags  : a block's word: bit 0 a non-finite gradient, bit 1 a constraint that did not converge (status 4), bit 2 the item's tables
//            were refused (status 5; set once by the vet launch in every block of the molecule).  All are sticky.
struct MscDev {
    const int *molptr, *atoms;           // the caller's tables: [B+1], [K, CL+1]
    const float* d;                      // [K, CL]
    int K;
    int *claim, *cfail;                  // the workspace's words
    float tol2, ih2;                     // 2 tolerance, 2 / dt
};

// a cluster's state in registers as the slots of csrc/md_cons.h
struct RegCluster {
    V3 xs[CL + 1], vs[CL + 1];
    __device__ __forceinline__ V3 x(int s) const { return xs[s]; }
    __device__ __forceinline__ V3 v(int s) const { return vs[s]; }
    __device__ __forceinline__ void set_x(int s, V3 p) { xs[s] = p; }
    __device__ __forceinline__ void set_v(int s, V3 p) { vs[s] = p; }
};

// the checks a cluster passes by itself in a molecule of n atoms -> its atoms as the table holds them; false: refused
__device__ __forceinline__ bool msc_cluster_ok(const MscDev& cn, int k, int n, int (&at)[CL + 1]) {
    const int* p = cn.atoms + (size_t)k * (CL + 1);
    const float* q = cn.d + (size_t)k * CL;
#pragma unroll
    for (int j = 0; j <= CL; ++j) at[j] = p[j];
    bool ok = (unsigned)at[0] < (unsigned)n, leaf = false;
#pragma unroll
    for (int j = 1; j <= CL; ++j)
        if (at[j] != -1) {
            leaf = true;
            const float dj = q[j - 1];
            if ((unsigned)at[j] >= (unsigned)n || !(dj > 0.f && dj <= FLT_MAX)) ok = false;
#pragma unroll
            for (int l = 0; l < j; ++l)
                if (at[l] == at[j]) ok = false;
        }
    return ok && leaf;          // a cluster has at least one leaf
}

// is atom i (of the item's molecule) the centre of a cluster?  -> that cluster with GLOBAL atom indices and its leaves packed (a leaf
// whose two ends are frozen is no constraint); false: a free atom or a leaf.  The tables were vetted by init; an index that is out of
// range all the same (other tables than init saw) is not followed.
__device__ __forceinline__ bool msc_cluster_of(const MscDev& cn, const RsItem& r, int i, const float* __restrict__ mass, Cluster& cl) {
    const int k = cn.claim[i];
    if ((unsigned)k >= (unsigned)cn.K) return false;
    const int* p = cn.atoms + (size_t)k * (CL + 1);
    if (p[0] != i - r.m0) return false;
    const float m = mass[i];
    cl.L = 0, cl.a0 = i, cl.w0 = m > 0.f ? 1.0f / m : 0.f;
#pragma unroll
    for (int j = 0; j < CL; ++j) cl.al[j] = i, cl.wl[j] = 0.f, cl.d2[j] = 1.f;
#pragma unroll
    for (int j = 1; j <= CL; ++j) {
        const int at = p[j];
        if ((unsigned)at < (unsigned)(r.m1 - r.m0)) {
            const float mk = mass[r.m0 + at];
            cons_add_leaf(cl, r.m0 + at, mk > 0.f ? 1.0f / mk : 0.f, cn.d[(size_t)k * CL + j - 1]);
        }
    }
    return true;
}

__device__ __forceinline__ V3 msc_ld3(const float* p, size_t off) { return {p[off], p[off + 1], p[off + 2]}; }
__device__ __forceinline__ void msc_st3(float* p, size_t off, V3 a) { p[off] = a.x, p[off + 1] = a.y, p[off + 2] = a.z; }
__device__ __forceinline__ int msc_slot_atom(const Cluster& cl, int s) { return s == 0 ? cl.a0 : cl.al[s - 1]; }
__device__ __forceinline__ float msc_slot_w(const Cluster& cl, int s) { return s == 0 ? cl.w0 : cl.wl[s - 1]; }

// the cluster's coordinates and velocities of conformation c: global memory -> registers, and back for its moving atoms
__device__ __forceinline__ void msc_load(const Cluster& cl, int C, int c, const float* x, const float* v, RegCluster& st) {
#pragma unroll
    for (int s = 0; s <= CL; ++s) {
        st.xs[s] = {0.f, 0.f, 0.f}, st.vs[s] = {0.f, 0.f, 0.f};
        if (s <= cl.L) {
            const size_t off = ((size_t)msc_slot_atom(cl, s) * C + c) * 3;
            st.xs[s] = msc_ld3(x, off), st.vs[s] = msc_ld3(v, off);
        }
    }
}
__device__ __forceinline__ void msc_store(const Cluster& cl, int C, int c, float* x, float* v, const RegCluster& st) {
#pragma unroll
    for (int s = 0; s <= CL; ++s)
        if (s <= cl.L && msc_slot_w(cl, s) > 0.f) {          // (a frozen atom keeps its bits)
            const size_t off = ((size_t)msc_slot_atom(cl, s) * C + c) * 3;
            if (x) msc_st3(x, off, st.xs[s]);
            msc_st3(v, off, st.vs[s]);
        }
}

// ---- init: the claim words and the failure words cleared
__global__ __launch_bounds__(256) void msc_clear_kernel(int N, size_t kc, int* claim, int* cfail) {
    const size_t u = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (u < (size_t)N) claim[u] = -1;
    if (u < kc) cfail[u] = 0;
}

// ---- init: every cluster that passes its own checks stores its index to its atoms' claim words (plain stores; the item of the
// molecule's first block and first conformations walks the molecule's clusters)
__global__ __launch_bounds__(NB_NT) void msc_claim_kernel(RsGeom q, MscDev cn) {
    RsItem r;
    if (!rs_item(q, r) || r.blk != nb_clamp(q.blk_ptr[r.mol], q.n_blocks) || r.c0 != 0) return;
    const int n = r.m1 - r.m0, k0 = nb_clamp(cn.molptr[r.mol], cn.K), k1 = nb_clamp(cn.molptr[r.mol + 1], cn.K);
    for (int k = k0 + (int)threadIdx.x; k < k1; k += NB_NT) {
        int at[CL + 1];
        if (!msc_cluster_ok(cn, k, n, at)) continue;
#pragma unroll
        for (int j = 0; j <= CL; ++j)
            if (at[j] != -1) cn.claim[r.m0 + at[j]] = k;
    }
}

// ---- init: every cluster reads its claims back: of two clusters that hold one atom at least one finds the other's index.  A molecule
// with a refused cluster: status 5 and bit 2 in every block's flag word, for the conformations of this item (the items of the molecule's
// first block, one per chunk of conformations, each decide the same from the same words).
__global__ __launch_bounds__(NB_NT) void msc_vet_kernel(RsGeom q, MscDev cn, int* status, int* bad) {
    RsItem r;
    if (!rs_item(q, r)) return;
    const int b0 = nb_clamp(q.blk_ptr[r.mol], q.n_blocks), b1 = nb_clamp(q.blk_ptr[r.mol + 1], q.n_blocks);
    if (r.blk != b0) return;
    const int n = r.m1 - r.m0, k0 = nb_clamp(cn.molptr[r.mol], cn.K), k1 = nb_clamp(cn.molptr[r.mol + 1], cn.K);
    int invalid = 0;
    for (int k = k0 + (int)threadIdx.x; k < k1; k += NB_NT) {
        int at[CL + 1];
        if (!msc_cluster_ok(cn, k, n, at)) {
            invalid = 1;
            continue;
        }
#pragma unroll
        for (int j = 0; j <= CL; ++j)
            if (at[j] != -1 && cn.claim[r.m0 + at[j]] != k) invalid = 1;          // another cluster claimed the atom too
    }
    if (!__syncthreads_or(invalid)) return;
    const int C = q.C, t = threadIdx.x;
    if (t < r.nc) status[(size_t)r.mol * C + r.c0 + t] = 5;
    for (int u = t; u < (b1 - b0) * r.nc; u += NB_NT) bad[(size_t)(b0 + u / r.nc) * C + r.c0 + u % r.nc] = 4;
}

// the block's constraint-failure word of every conformation of the item: the OR over the block's cluster threads (fail: this thread's)
__device__ __forceinline__ void msc_write_fail(const RsItem& r, int C, bool lane, bool fail, const int* live, int* cfail) {
    __shared__ int cf[NB_CW];
    const int t = threadIdx.x;
    if (t < NB_CW) cf[t] = 0;
    __syncthreads();
    if (lane && fail) cf[t / r.ni] = 1;
    __syncthreads();
    if (t < r.nc && live[t]) cfail[(size_t)r.blk * C + r.c0 + t] = cf[t];
}

// ---- init: the start's S and P (after the init kernel, the claims and the vet; before the boxes and the first force)
struct MscStartArgs {
    RsGeom q;
    float *x, *v;
    const float* mass;
    const int* status;
    MscDev cn;
    int constrain_start;
};

__global__ __launch_bounds__(NB_NT) void msc_start_kernel(MscStartArgs a) {
    __shared__ int run[NB_CW];
    RsItem r;
    if (!rs_item(a.q, r)) return;
    const int C = a.q.C, t = threadIdx.x;
    if (!rs_running(r, C, a.status, run)) return;      // (a refused item: nothing of it is touched)
    const bool lane = t < r.ni * r.nc;
    bool fail = false;
    Cluster cl;
    if (lane && run[t / r.ni] && msc_cluster_of(a.cn, r, r.i0 + t % r.ni, a.mass, cl) && cl.L > 0) {
        const int c = r.c0 + t / r.ni;
        RegCluster st;
        msc_load(cl, C, c, a.x, a.v, st);
        if (a.constrain_start) {
            V3 rref[CL];
            cons_bonds(cl, rref, st);
            fail = !cons_shake(cl, rref, st, a.cn.tol2, a.cn.ih2, false);
        }
        cons_project(cl, st);
        msc_store(cl, C, c, a.constrain_start ? a.x : nullptr, a.v, st);
    }
    msc_write_fail(r, C, lane, fail, run, a.cn.cfail);
}

// ---- move
// the thread's (atom, conformation) of the item: a free atom as ms_move_lane moves it, a centre its whole cluster, a leaf nothing;
// true: an S of the thread's cluster did not converge
template <bool LADDER = false>
__device__ __forceinline__ bool msc_move_lane(const MsMoveArgs& a, const MscDev& cn, const RsItem& r, int k0, const int* stop) {
    const int C = a.q.C, t = threadIdx.x, ni = r.ni;
    const int cc = t / ni, il = t - cc * ni;
    const int i = r.i0 + il, c = r.c0 + cc;
    const size_t item = (size_t)r.mol * C + c;
    const bool writer = r.blk == k0 && il == 0;      // the molecule's first block: the one writer (and reader) of the item's status and steps
    if (stop[cc]) {
        // a flag the force launch left: the item keeps the x and v it holds.  A constraint failure (it wins over a non-finite gradient)
        // also takes back the count of the step that failed; the start's S failing leaves 0.  Once: the status is then final.
        if (writer && a.status[item] == RS_RUNNING) {
            const bool cfail = (stop[cc] & 2) != 0;
            a.status[item] = cfail ? 4 : 2;
            if (cfail && a.steps[item] > 0) a.steps[item] -= 1;
        }
        return false;
    }
    if (writer) a.steps[item] += 1;
    if (cn.claim[i] < 0) {
        ms_move_atom<false, LADDER>(a, r, i, c, nullptr);
        return false;
    }
    Cluster cl;
    if (!msc_cluster_of(cn, r, i, a.mass, cl) || cl.L == 0) return false;
    RegCluster st;
    msc_load(cl, C, c, a.x, a.v, st);
    const unsigned long long key = a.mol_key[r.mol];
    // B P
#pragma unroll
    for (int s = 0; s <= CL; ++s)
        if (s <= cl.L && msc_slot_w(cl, s) > 0.f)
            st.vs[s] = st.vs[s] - (a.k.hk * msc_slot_w(cl, s)) * msc_ld3(a.g, ((size_t)msc_slot_atom(cl, s) * C + c) * 3);
    cons_project(cl, st);
    // A S P
    V3 rref[CL];
    bool fail = false;
    cons_drift(cl, rref, st, a.k.h2);
    if (!cons_shake(cl, rref, st, cn.tol2, cn.ih2, true)) fail = true;
    cons_project(cl, st);
    // O P
    if (a.k.thermostat) {
#pragma unroll
        for (int s = 0; s <= CL; ++s)
            if (s <= cl.L && msc_slot_w(cl, s) > 0.f) {
                const float w = msc_slot_w(cl, s);
                st.vs[s] = a.k.c1 * st.vs[s] + (a.k.c2 * sqrtf(ms_kt<LADDER>(a, item) * w)) * md_normal3(key, (unsigned)(msc_slot_atom(cl, s) - r.m0), (unsigned)c, a.step, 0u);
            }
        cons_project(cl, st);
    }
    // A S P
    cons_drift(cl, rref, st, a.k.h2);
    if (!cons_shake(cl, rref, st, cn.tol2, cn.ih2, true)) fail = true;
    cons_project(cl, st);
    msc_store(cl, C, c, a.x, a.v, st);
    return fail;
}

__global__ __launch_bounds__(NB_NT) void ms_move_cons_kernel(MsMoveArgs a, MscDev cn) {
    __shared__ int stop[NB_CW];
    __shared__ int live[NB_CW];
    RsItem r;
    if (!rs_item(a.q, r)) return;
    const int C = a.q.C, t = threadIdx.x;
    const int k0 = nb_clamp(a.q.blk_ptr[r.mol], a.q.n_blocks), k1 = nb_clamp(a.q.blk_ptr[r.mol + 1], a.q.n_blocks);
    ms_stop_flags<true>(a.bad, r, C, k0, k1, stop);
    const bool lane = t < r.ni * r.nc;
    const bool fail = lane && msc_move_lane(a, cn, r, k0, stop);
    if (t < r.nc) live[t] = stop[t] == 0;          // (a stopped conformation keeps its failure word, as it keeps its x)
    msc_write_fail(r, C, lane, fail, live, cn.cfail);
}

// on a ladder (csrc/md_remd.h): the kernel above with msc_move_lane<true>.  A kernel of its own text, not a shared body: moved into a
// function the compiler schedules the unladdered kernel differently, and that kernel is to stay the code it was
__global__ __launch_bounds__(NB_NT) void ms_move_cons_ladder_kernel(MsMoveArgs a, MscDev cn) {
    __shared__ int stop[NB_CW];
    __shared__ int live[NB_CW];
    RsItem r;
    if (!rs_item(a.q, r)) return;
    const int C = a.q.C, t = threadIdx.x;
    const int k0 = nb_clamp(a.q.blk_ptr[r.mol], a.q.n_blocks), k1 = nb_clamp(a.q.blk_ptr[r.mol + 1], a.q.n_blocks);
    ms_stop_flags<true>(a.bad, r, C, k0, k1, stop);
    const bool lane = t < r.ni * r.nc;
    const bool fail = lane && msc_move_lane<true>(a, cn, r, k0, stop);
    if (t < r.nc) live[t] = stop[t] == 0;
    msc_write_fail(r, C, lane, fail, live, cn.cfail);
}

// ---- close: the closing P of the block's clusters, then the block's kinetic partial: over the block's atoms in ascending order, in
// double, where a free atom gives m v^2, a centre the sum of its cluster's moving atoms (centre, then leaves in table order) and a leaf
// nothing.  project == 0 (init): the partial alone.
struct MscCloseArgs {
    RsGeom q;
    const float* x;
    float* v;
    const float* mass;
    const int* status;
    MscDev cn;
    double* kpart;
    int project;
};

__global__ __launch_bounds__(NB_NT) void msc_close_kernel(MscCloseArgs a) {
    __shared__ int run[NB_CW];
    __shared__ double kin[NB_NT];
    RsItem r;
    if (!rs_item(a.q, r)) return;
    const int C = a.q.C, t = threadIdx.x, ni = r.ni;
    if (!rs_running(r, C, a.status, run)) return;
    const int cc = t / ni, il = t - cc * ni;
    const bool lane = t < ni * r.nc && run[cc] != 0;
    double mv2 = 0.0;
    if (lane) {
        const int i = r.i0 + il, c = r.c0 + cc;
        Cluster cl;
        if (a.cn.claim[i] < 0) {
            const float m = a.mass[i];
            if (m > 0.f) {
                const V3 vi = msc_ld3(a.v, ((size_t)i * C + c) * 3);
                mv2 = (double)(m * dot(vi, vi));
            }
        } else if (msc_cluster_of(a.cn, r, i, a.mass, cl)) {
            RegCluster st;
            msc_load(cl, C, c, a.x, a.v, st);
            if (a.project && cl.L > 0) {
                cons_project(cl, st);
                msc_store(cl, C, c, nullptr, a.v, st);
            }
#pragma unroll
            for (int s = 0; s <= CL; ++s)
                if (s <= cl.L && msc_slot_w(cl, s) > 0.f) mv2 += (double)(a.mass[msc_slot_atom(cl, s)] * dot(st.vs[s], st.vs[s]));
        }
    }
    kin[t] = mv2;
    __syncthreads();
    if (lane && il == 0) {
        double sk = 0.0;
        for (int k = 0; k < ni; ++k) sk += kin[cc * ni + k];
        a.kpart[(size_t)r.blk * C + r.c0 + cc] = sk;
    }
}

// ---- finish: x and v of every item but a refused one -> xyz_out, vel_out (a thread per (atom, conformation) of the item)
__global__ __launch_bounds__(NB_NT) void msc_copy_kernel(RsGeom q, const float* x, const float* v, const int* status, float* xyz_out, float* vel_out) {
    RsItem r;
    if (!rs_item(q, r)) return;
    const int t = threadIdx.x;
    if (t >= r.ni * r.nc) return;
    const int cc = t / r.ni, i = r.i0 + t % r.ni, c = r.c0 + cc;
    if (status[(size_t)r.mol * q.C + c] == 5) return;
    const size_t off = ((size_t)i * q.C + c) * 3;
    msc_st3(xyz_out, off, msc_ld3(x, off)), msc_st3(vel_out, off, msc_ld3(v, off));
}

// ------------------------------------------------------------------------------------------------ energies and outputs
struct MsOutArgs {
    int N, C, B, n_blocks, has_nb;
    int final;               // 1: the finish (every item with atoms; x, v, steps and status too); 0: a frame (running items only)
    int with_epot;           // 0: the six terms were not computed (a frame that asks for the kinetic energy alone)
    const int *atom_molptr, *blk_ptr;
    const float *x, *v, *terms;      // terms [6,B,C] in the workspace (rows 4, 5 only with has_nb)
    const double* kpart;
    const int *bad, *status_ws, *steps_ws;
    float *xyz_out, *vel_out, *epot, *ekin;
    int *steps, *status;
};

// CONS (with constraints): x and v are copied per item by msc_copy_kernel, an item whose tables were refused (5) gets its status and
// nothing else, and a set constraint flag (bit 1 of a block's word) ends a running item with 4 and takes the failing step back
template <bool CONS>
__global__ __launch_bounds__(256) void ms_out_kernel(MsOutArgs a) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (!CONS && a.final && gid < (size_t)a.N * a.C * 3) {
        a.xyz_out[gid] = a.x[gid];
        a.vel_out[gid] = a.v[gid];
    }
    const size_t bc = (size_t)a.B * a.C;
    if (gid >= bc) return;
    const int b = (int)(gid / (unsigned)a.C), c = (int)(gid - (size_t)b * a.C);
    if (nb_clamp(a.atom_molptr[b + 1], a.N) <= nb_clamp(a.atom_molptr[b], a.N)) return;      // a molecule without atoms writes nothing
    const int st = a.status_ws[gid];
    if (!a.final && st != RS_RUNNING) return;       // a stopped item's later frames are not written
    if (CONS && st == 5) {
        a.status[gid] = 5;
        return;
    }
    // the kinetic partials and the flags of the item's blocks, in ascending block order
    const int k0 = nb_clamp(a.blk_ptr[b], a.n_blocks), k1 = nb_clamp(a.blk_ptr[b + 1], a.n_blocks);
    double ks = 0.0;
    int flagged = 0;
    for (int k = k0; k < k1; ++k) {
        ks += a.kpart[(size_t)k * a.C + c];
        flagged |= a.bad[(size_t)k * a.C + c];
    }
    if (a.epot && a.with_epot) {
        double tot = 0.0;
        for (int q = 0; q < 6; ++q) tot += (double)((q < 4 || a.has_nb) ? a.terms[q * bc + gid] : 0.f);
        a.epot[gid] = (float)tot;
    }
    if (a.ekin) a.ekin[gid] = (float)((0.5 / MD_ACC) * ks);
    if (a.final && CONS) {
        const bool failed = st == RS_RUNNING && (flagged & 2) != 0;      // (the move launch that would have taken the step back never came)
        const int n = a.steps_ws[gid];
        a.steps[gid] = failed && n > 0 ? n - 1 : n;
        a.status[gid] = st == RS_RUNNING ? ((flagged & 2) ? 4 : (flagged ? 2 : 0)) : st;
    } else if (a.final) {
        a.steps[gid] = a.steps_ws[gid];
        a.status[gid] = st == RS_RUNNING ? (flagged ? 2 : 0) : st;      // (the gradient that closed the last step is tested here)
    }
}

// ------------------------------------------------------------------------------------------------ implicit solvent (grappa_md_steps_*_gb_f32)
// GB/SA (include/grappa_hip.h grappa_gb_desc) as a term of the force: the three passes of csrc/gb_pass.h under the stopped-conformation
// mask, behind the force launch, which runs AS IT IS with hk = 0 (no closing kick: the form init has always used) -- so the kernels of a
// run without solvent are not touched by this section, and a run with it launches the very same force kernels.
//   step   : move, force (g = bonded + nonbonded, the frame's coordinates, the flag), born, pair (the gradient at fixed B -> ggb), chain:
//            its epilogue adds g + ggb + the chain sum in that order, writes g, gives the closing kick, ORs the non-finite test of the sum
//            into the block's flag word and (without constraints) rewrites the block's kinetic partial.  5 launches; with constraints
//            move, force, born, pair, chain, close: 6.  init gains the same three launches behind its force launch.
//   hazards: born writes B, dBdI of its own (atom, conformation)s, pair reads B of every j and writes w and ggb of its own, chain reads w
//            of every j and writes g, v of its own and the flag and partial of its own block: every word has one writer per launch and
//            is read only across a launch boundary.  The flag word is the block's own, written by the force launch before.
//   energies: grappa_gb_obc_fwd_f32 itself at the held coordinates, in a workspace region of its own (steps_gb_terms_at of
//            csrc/rs_force.h), and one small launch that adds the eight terms in double in term order.
//   cutoff  : grappa_md_steps_*_gbcut_f32 (include/grappa_hip.h grappa_gb_cut).  The three passes run under the GbCut policy of
//            csrc/gb_loop.h -- the text the energy entry instantiates -- and read the boxes that the launches of a nonbonded cutoff
//            write: rs_box_kernel in init and behind a constrained move, the move launch itself otherwise.  ONE set of boxes serves
//            both cutoffs; the nonbonded cutoff may be given beside the solvent's (the force launch is then its NbCut instantiation,
//            untouched) or not.  A step gains no launch over the all-pairs solvent step except the box launch behind a constrained
//            move, which a nonbonded cutoff adds as well.  Energies: grappa_gb_obc_fwd_cut_f32 itself (steps_gb_cut_terms_at).
struct MsGb {
    const grappa_gb_desc* opts;
    GbK k;
    const grappa_gb_cut* cut;            // NULL: all pairs
    GbCutDev cdev;                       // (box is set once the workspace is laid out)
};

struct MsGbWs {
    GbPassWs p;
    float* ggb;                          // [N,C,3]: the gradient at fixed B
    float *e_gb, *terms_gb;              // frames and finish: [B,C], [2,B,C]
    char* fwd;                           // frames and finish: the workspace of grappa_gb_obc_fwd_f32
    size_t fwd_bytes;
    size_t total;
};

// (the words of the solvent lie behind all others: `off` = the total of ms_layout)
MsGbWs ms_gb_layout(char* base, size_t off, int N, int C, int B, int n_blocks, bool gbcut) {
    MsGbWs g;
    WsCarve k{base};
    k.off = off;
    g.p = gb_pass_ws(k, N, C);
    g.ggb = k.take<float>((size_t)N * C * 3);
    g.e_gb = k.take<float>((size_t)B * C), g.terms_gb = k.take<float>(2 * (size_t)B * C);
    g.fwd_bytes = gbcut ? grappa_gb_obc_cut_workspace_bytes(N, C, n_blocks > 0 ? n_blocks : 1)
                        : grappa_gb_obc_workspace_bytes(N, C, n_blocks > 0 ? n_blocks : 1);
    g.fwd = k.take<char>(g.fwd_bytes);
    g.total = k.off;
    return g;
}

__global__ __launch_bounds__(NB_NT) void ms_gb_born_kernel(GbArgs a) {
    __shared__ GbShared sh;
    gb_born_body<true>(a, sh);
}

__global__ __launch_bounds__(NB_NT) void ms_gb_pair_kernel(GbArgs a) {
    __shared__ GbShared sh;
    gb_pair_body<true, false, true>(a, sh);
}

struct MsGbCloseArgs {
    GbArgs a;
    float *v, *g;
    const float* mass;
    int* bad;
    double* kpart;
    float hk;                // dt / 2 ACC; 0: no closing kick (init)
};

// the chain launch's epilogue (gb_chain_body's epi); CONS: the kinetic partial is left to the close launch, which follows the closing P
template <bool CONS>
__device__ __forceinline__ void ms_gb_close(const MsGbCloseArgs& c, GbShared& sh, const GbLane& w, float cx, float cy, float cz) {
    const int C = c.a.q.C, ni = w.r.ni;
    float mv2 = 0.f, bad = 0.f;
    if (w.owner) {
        const size_t off = ((size_t)w.i * C + w.c) * 3;
        const V3 gi = {(c.g[off] + c.a.gdir[off]) + cx, (c.g[off + 1] + c.a.gdir[off + 1]) + cy, (c.g[off + 2] + c.a.gdir[off + 2]) + cz};
        c.g[off] = gi.x, c.g[off + 1] = gi.y, c.g[off + 2] = gi.z;
        const float m = c.mass[w.i];
        V3 vi = {c.v[off], c.v[off + 1], c.v[off + 2]};
        if (m > 0.f) {
            if (c.hk > 0.f) {          // the closing B of the step
                vi = vi - (c.hk * (1.0f / m)) * gi;
                c.v[off] = vi.x, c.v[off + 1] = vi.y, c.v[off + 2] = vi.z;
            }
            mv2 = m * dot(vi, vi);
        }
        if (!(sqrtf(dot(gi, gi)) <= FLT_MAX)) bad = 1.f;      // (written so that a NaN counts as non-finite)
    }
    __syncthreads();
    if (w.owner) sh.red[0][w.l] = mv2, sh.red[1][w.l] = bad;
    __syncthreads();
    if (w.owner && w.il == 0) {      // the block's words of one conformation: over its atoms in ascending order, in double
        double sk = 0.0;
        float fb = 0.f;
        for (int k = 0; k < ni; ++k) {
            const int o = w.cl * ni + k;
            sk += (double)sh.red[0][o];
            fb = fmaxf(fb, sh.red[1][o]);
        }
        const size_t o = (size_t)w.r.blk * C + w.c;
        if constexpr (!CONS) c.kpart[o] = sk;
        if (fb != 0.f) c.bad[o] |= 1;          // (the block's own word, which the force launch before this one wrote)
    }
}

template <bool CONS>
__global__ __launch_bounds__(NB_NT) void ms_gb_chain_kernel(MsGbCloseArgs c) {
    __shared__ GbShared sh;
    gb_chain_body<true>(c.a, sh, [&](const GbLane& w, float cx, float cy, float cz) { ms_gb_close<CONS>(c, sh, w, cx, cy, cz); });
}

// the three passes under the solvent's cutoff: the bodies of the energy entry's cut kernels under the stopped-conformation mask
__global__ __launch_bounds__(NB_NT) void ms_gb_born_cut_kernel(GbArgs a, GbCutDev d) {
    __shared__ GbShared sh;
    __shared__ unsigned char near[NB_NT];
    gb_born_body<true, GbCut>(a, sh, GbCut{d, near, 0});
}

__global__ __launch_bounds__(NB_NT) void ms_gb_pair_cut_kernel(GbArgs a, GbCutDev d) {
    __shared__ GbShared sh;
    __shared__ unsigned char near[NB_NT];
    gb_pair_body<true, false, true, GbCut>(a, sh, GbCut{d, near, 0});
}

template <bool CONS>
__global__ __launch_bounds__(NB_NT) void ms_gb_chain_cut_kernel(MsGbCloseArgs c, GbCutDev d) {
    __shared__ GbShared sh;
    __shared__ unsigned char near[NB_NT];
    gb_chain_body<true, GbCut>(
        c.a, sh, [&](const GbLane& w, float cx, float cy, float cz) { ms_gb_close<CONS>(c, sh, w, cx, cy, cz); }, GbCut{d, near, 0});
}

// the three solvent launches behind a force launch that gave no closing kick
void ms_launch_gb(hipStream_t st, const grappa_nb_desc* nb, const MsGb& gb, const RsGeom& q, const MsWs& w, const MsGbWs& gw, const float* mass,
                  float hk, int n_items, bool cons) {
    MsGbCloseArgs c = {};
    c.a.q = q, c.a.x = w.x, c.a.charge = nb->charge, c.a.radius = gb.opts->radius, c.a.scale = gb.opts->scale, c.a.k = gb.k;
    c.a.B = gw.p.B, c.a.dBdI = gw.p.dBdI, c.a.w = gw.p.w, c.a.gdir = gw.ggb, c.a.part = nullptr, c.a.born = nullptr, c.a.status = w.status;
    c.v = w.v, c.g = w.g, c.mass = mass, c.bad = w.bad, c.kpart = w.kpart, c.hk = hk;
    const dim3 grid((unsigned)n_items), block(NB_NT);
    if (gb.cut) {
        GbCutDev d = gb.cdev;
        d.box = w.box;
        GRAPPA_LAUNCH(ms_gb_born_cut_kernel, grid, block, 0, st, c.a, d);
        GRAPPA_LAUNCH(ms_gb_pair_cut_kernel, grid, block, 0, st, c.a, d);
        if (cons) GRAPPA_LAUNCH(ms_gb_chain_cut_kernel<true>, grid, block, 0, st, c, d);
        else GRAPPA_LAUNCH(ms_gb_chain_cut_kernel<false>, grid, block, 0, st, c, d);
        return;
    }
    GRAPPA_LAUNCH(ms_gb_born_kernel, grid, block, 0, st, c.a);
    GRAPPA_LAUNCH(ms_gb_pair_kernel, grid, block, 0, st, c.a);
    if (cons) GRAPPA_LAUNCH(ms_gb_chain_kernel<true>, grid, block, 0, st, c);
    else GRAPPA_LAUNCH(ms_gb_chain_kernel<false>, grid, block, 0, st, c);
}

// epot with the solvent's two terms, and esolv: the conditions of ms_out_kernel, which ran before it and left epot without them
template <bool CONS>
__global__ __launch_bounds__(256) void ms_out_gb_kernel(MsOutArgs a, const float* terms_gb, float* esolv) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, bc = (size_t)a.B * a.C;
    if (gid >= bc) return;
    const int b = (int)(gid / (unsigned)a.C);
    if (nb_clamp(a.atom_molptr[b + 1], a.N) <= nb_clamp(a.atom_molptr[b], a.N)) return;
    const int st = a.status_ws[gid];
    if (!a.final && st != RS_RUNNING) return;
    if (CONS && st == 5) return;
    const double es = (double)terms_gb[gid] + (double)terms_gb[bc + gid];
    if (a.epot) {
        double tot = 0.0;
        for (int q = 0; q < 6; ++q) tot += (double)((q < 4 || a.has_nb) ? a.terms[q * bc + gid] : 0.f);
        a.epot[gid] = (float)(tot + es);
    }
    if (esolv) esolv[gid] = (float)es;
}

// ------------------------------------------------------------------------------------------------ host
// (the argument checks the three calls share: steps_seam_check of csrc/desc_check.h; GRAPPA_SEAM_EMPTY: nothing to do)

// ------------------------------------------------------------------------------------------------ restraints (grappa_md_steps_*_restr_f32)
// Tethers and dihedral restraints of csrc/md_restr.h on every Hamiltonian above.
//   gradient: every variant launches ms_force_body, whose epilogue holds the owner's gi before g is written, before the closing kick and
//            before the non-finite test; the restrained instantiations add the restraint gradient there.  What follows reads that g and
//            recomputes nothing: the next move launch (with constraints ms_move_cons_kernel, B P) reads g; msc_close_kernel reads x and v
//            only (the closing P and the kinetic partial), no gradient; in solvent the force launch runs with hk == 0 and the chain
//            launch's epilogue (ms_gb_close) reads g, adds ggb and the chain sum, writes g, kicks and tests the sum.  So no launch per
//            step is added and no word has a second writer.
//   hazards : x is written by move alone and read by force (its own and, for a row's atoms, other blocks': across the launch
//            boundary); the reference is written once by init; g is written by the owner in force (and chain), read by the next move;
//            status 5 and bit 2 of the flag words are written by the vet launch of init, before the first force launch reads status.
//   status 5: as with constraints, a refused item never runs and its outputs are not touched: the move launches of a restrained run
//            leave a status that is not RS_RUNNING alone (KEEP), and the finish copies x and v item by item (msc_copy_kernel,
//            ms_out_kernel<true>).
//   energies: mr_energy_kernel at the held coordinates, where the six terms are evaluated: on frame steps and at finish.  epot stays
//            the force field's (plus the solvent's); E_r is reported beside it.
//   workspace: the reference [N,C,3], behind every other word.
struct MsRestr {
    MrDev dev;                           // (dev.ref is set once the workspace is laid out)
    const float* ref_src;                // the caller's pos_ref, or NULL: mm->xyz as init receives it
};

float* ms_restr_ref(char* base, size_t off, int N, int C, size_t& total) {
    WsCarve k{base};
    k.off = off;
    float* ref = k.take<float>((size_t)N * C * 3);
    total = k.off;
    return ref;
}

// ------------------------------------------------------------------------------------------------ ladders (grappa_md_remd_*_f32)
// A temperature ladder over the C conformations of a call, with or without exchanges between neighbouring slots: csrc/md_remd.h states
// the replicas, the slots and the kernels.
//   move    : the LADDER instantiations of the move launches read kt of the item's slot from kt_item; everything else of a step stays.
//   attempt : behind the step whose global index g is a multiple of exchange_every, after that step's own frame outputs: the energies
//            by the launches a frame uses (ms_launch_terms, ms_launch_out, mr_energy_kernel) into workspace scratch -- or, where the
//            frame of this very step asked for them, the frame's own rows: nothing is evaluated twice -- then ms_exchange_kernel (one
//            workgroup per molecule) and ms_rescale_kernel (one per item).  x and g are untouched, so no force is recomputed.
//   hazards : slot, who, kt_item and scale are written by the exchange launch alone (init apart) and read by the rescale launch and the
//            next move launch; v and the kinetic partials are written by the rescale launch between a step's last launch and the next
//            step's move.  The exchange launch reads status and the flag words, which the step's launches wrote.
//   status 5: a slots_in row that is no permutation, or a temperature the ladder refuses: mx_init_kernel, as the restraints' vet.  A
//            run on a ladder is therefore item-wise like a restrained one (the KEEP moves, the item-wise finish).
//   workspace: the ladder's words behind every other word.
struct MsRemd {
    const float* temperatures;
    const int* slots_in;
    int every, init_at_ladder;
};

MxDev ms_remd_layout(char* base, size_t off, int B, int C, size_t& total) {
    WsCarve k{base};
    k.off = off;
    const size_t bc = (size_t)B * C;
    MxDev x = {};
    x.slot = k.take<int>(bc), x.who = k.take<int>(bc);
    x.kt_item = k.take<float>(bc), x.scale = k.take<float>(bc);
    x.epot = k.take<float>(bc), x.erestr = k.take<float>(bc);
    total = k.off;
    return x;
}

// ------------------------------------------------------------------------------------------------ the run plan
// What a run has, resolved ONCE per call from the optional pointers of its entry: a family of entries is the widest call with the
// pointers it does not take NULL, and what a plan without an option launches is what the narrower family launches.  The plan lives on
// the caller's stack and is rebuilt by every call, as RsCut and MsGb always were.
struct MsHas {                           // what lays claim to words of the workspace
    bool cut, cons, gb, gbcut, restr;    // the nonbonded cutoff, constraints, the solvent, the solvent's own cutoff, restraints
    bool remd;                           // a temperature ladder
    bool boxes() const { return cut || gbcut; }          // either cutoff reads the blocks' boxes
};

struct MsPlan {
    MsHas has;
    RsCut cut;                           // has.cut: RsCut / rs_cut_make of csrc/rs_force.h
    const grappa_md_cons* cons;          // has.cons: the caller's tables (K > 0), else NULL
    MsGb gb;                             // has.gb; gb.cut is the solvent's cutoff (has.gbcut) or NULL
    MsRestr restr;                       // has.restr
    MsRemd remd;                         // has.remd
    const RsCut* c() const { return has.cut ? &cut : nullptr; }
    bool keep() const { return has.restr || has.remd; }      // an item may be refused (5) by a vet of init other than the constraints'
};

// Every refusal an option can meet, in one place: GRAPPA_ERR_ARG, else GRAPPA_OK with p filled.  An entry asks this before it looks at
// anything else, so a refused option is refused for an empty batch too.
//   cut   : bad options, or no nb
//   cons  : K < 0; with K > 0 a NULL table or a tolerance outside [2^-20, 2^-7] (a NaN is refused).  NULL or K == 0: none
//   gb    : no nb or no charges (the solvent reads them), NULL radius / scale, bad options; cut beside a solvent that has no cutoff of
//           its own; gbcut without gb, or with bad options
//   r     : R < 0, a NULL dihedral table with R > 0, R * C >= 2^31, pos_ref without pos_k.  NULL, or R == 0 with pos_k == NULL: none
//   x     : a NULL ladder, exchange_every < 0, exchanges without a thermostat (o: friction > 0 is asked of it).  NULL: none
int ms_plan(const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut, const grappa_md_cons* cons, const grappa_gb_desc* gb,
            const grappa_gb_cut* gbcut, const grappa_md_restr* r, MsPlan& p, const grappa_md_remd* x = nullptr,
            const grappa_md_opts* o = nullptr) {
    p = MsPlan{};
    if (cut) {
        if (!rs_cut_make(cut, nb, p.cut)) return GRAPPA_ERR_ARG;
        p.has.cut = true;
    }
    if (cons && cons->K != 0) {
        if (cons->K < 0 || !cons->cluster_molptr || !cons->cluster_atoms || !cons->cluster_d) return GRAPPA_ERR_ARG;
        if (!(cons->tolerance >= 0x1p-20f && cons->tolerance <= 0x1p-7f)) return GRAPPA_ERR_ARG;
        p.cons = cons, p.has.cons = true;
    }
    if (gb || gbcut) {
        if (!gb || (cut && !gbcut) || !nb || !nb->charge || !gb->radius || !gb->scale || !gb_consts(gb, p.gb.k)) return GRAPPA_ERR_ARG;
        if (gbcut && !gb_cut_consts(gbcut, p.gb.cdev)) return GRAPPA_ERR_ARG;
        p.gb.opts = gb, p.gb.cut = gbcut;
        p.has.gb = true, p.has.gbcut = gbcut != nullptr;
    }
    if (r) {
        if (r->R < 0 || (r->R > 0 && (!r->dih_molptr || !r->dih_atoms || !r->dih_k || !r->dih_target)) || (r->pos_ref && !r->pos_k))
            return GRAPPA_ERR_ARG;
        if (r->R > 0 && mm && mm->C > 0 && (long long)r->R * mm->C >= (1LL << 31)) return GRAPPA_ERR_ARG;
        if (r->R > 0 || r->pos_k) {
            p.has.restr = true;
            p.restr.dev.pos_k = r->pos_k, p.restr.dev.R = r->R, p.restr.ref_src = r->pos_ref;
            if (r->R > 0) p.restr.dev.molptr = r->dih_molptr, p.restr.dev.atoms = r->dih_atoms, p.restr.dev.k = r->dih_k, p.restr.dev.target = r->dih_target;
        }
    }
    if (x) {
        if (!x->temperatures || x->exchange_every < 0 || (x->exchange_every > 0 && !(o && o->friction > 0.f))) return GRAPPA_ERR_ARG;
        p.has.remd = true;
        p.remd = MsRemd{x->temperatures, x->slots_in, x->exchange_every, x->init_at_ladder};
    }
    return GRAPPA_OK;
}

// A plan's words in the workspace (base == NULL: sizes only).  The cut's words lie behind the base's, those of constraints behind both
// (ms_layout), the solvent's behind those, the restraints' reference behind those, the ladder's words last: a narrower plan's layout is a
// prefix of a wider one's.
struct MsCarve {
    MsWs w;
    MsGbWs gw;                           // has.gb
    float* ref;                          // has.restr
    MxDev x;                             // has.remd (x.temperatures is set by ms_remd_dev)
    size_t total;
};

MsCarve ms_carve(char* base, int N, int C, int B, int n_blocks, const MsHas& h) {
    MsCarve k = {};
    k.w = ms_layout(base, N, C, B, n_blocks, h.boxes(), h.cons);
    k.total = k.w.total;
    if (h.gb) k.gw = ms_gb_layout(base, k.total, N, C, B, n_blocks, h.gbcut), k.total = k.gw.total;
    if (h.restr) k.ref = ms_restr_ref(base, k.total, N, C, k.total);
    if (h.remd) k.x = ms_remd_layout(base, k.total, B, C, k.total);
    return k;
}

// (the *_workspace_bytes entries: constraints count with K > 0)
size_t ms_bytes(int N, int C, int B, int n_blocks, int K, MsHas h) {
    if (N <= 0 || C <= 0 || B <= 0 || n_blocks < 0 || K < 0) return 0;
    h.cons = K > 0;
    return ms_carve(nullptr, N, C, B, n_blocks, h).total;
}

// the restraints as the kernels take them, their reference where the workspace holds it
MrDev ms_restr_dev(const MsPlan& p, const MsCarve& k) {
    MrDev m = p.restr.dev;
    m.ref = k.ref;
    return m;
}

// the ladder as the kernels take it: the caller's temperatures and the workspace's words
MxDev ms_remd_dev(const MsPlan& p, const MsCarve& k) {
    MxDev x = k.x;
    x.temperatures = p.remd.temperatures;
    return x;
}

// ------------------------------------------------------------------------------------------------ launches
// the force launch: restraints x constraints (cfail != NULL) x cutoff, chosen here and nowhere else.  hk == 0: no closing kick
void ms_launch_force(hipStream_t st, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const RsCut* c, const RsGeom& q, const MsWs& w,
                     const float* mass, float hk, float* frame_xyz, int n_items, const int* cfail, const MrDev* mr) {
    MsForceArgs f;
    f.f = rs_force_in(mm, nb, q, w.x, w.status);
    f.v = w.v, f.g = w.g, f.mass = mass, f.bad = w.bad, f.kpart = w.kpart;
    f.hk = hk, f.frame_xyz = frame_xyz;
    const dim3 grid((unsigned)n_items), block(NB_NT);
    NbCutDev d = {};
    if (c) d = c->dev, d.box = w.box, d.er = w.er;
    if (mr) {
        if (c && cfail) GRAPPA_LAUNCH(ms_force_restr_cons_cut_kernel, grid, block, 0, st, f, d, cfail, *mr);
        else if (c) GRAPPA_LAUNCH(ms_force_restr_cut_kernel, grid, block, 0, st, f, d, *mr);
        else if (cfail) GRAPPA_LAUNCH(ms_force_restr_cons_kernel, grid, block, 0, st, f, cfail, *mr);
        else GRAPPA_LAUNCH(ms_force_restr_kernel, grid, block, 0, st, f, *mr);
    } else {
        if (c && cfail) GRAPPA_LAUNCH(ms_force_cons_cut_kernel, grid, block, 0, st, f, d, cfail);
        else if (c) GRAPPA_LAUNCH(ms_force_cut_kernel, grid, block, 0, st, f, d);
        else if (cfail) GRAPPA_LAUNCH(ms_force_cons_kernel, grid, block, 0, st, f, cfail);
        else GRAPPA_LAUNCH(ms_force_kernel, grid, block, 0, st, f);
    }
}

// the move launch: the ladder x (constraints, else refusable items x boxes), chosen here and nowhere else (on a ladder every item is refusable)
void ms_launch_move(hipStream_t st, const MsPlan& p, const MsMoveArgs& mv, const MscDev& cn, const MsWs& w, int n_items) {
    const dim3 grid((unsigned)n_items), block(NB_NT);
    if (p.has.remd) {
        if (p.has.cons) GRAPPA_LAUNCH(ms_move_cons_ladder_kernel, grid, block, 0, st, mv, cn);
        else if (p.has.boxes()) GRAPPA_LAUNCH(ms_move_cut_ladder_kernel, grid, block, 0, st, mv, w.box);
        else GRAPPA_LAUNCH(ms_move_ladder_kernel, grid, block, 0, st, mv);
        return;
    }
    if (p.has.cons) GRAPPA_LAUNCH(ms_move_cons_kernel, grid, block, 0, st, mv, cn);
    else if (p.has.restr && p.has.boxes()) GRAPPA_LAUNCH(ms_move_restr_cut_kernel, grid, block, 0, st, mv, w.box);
    else if (p.has.restr) GRAPPA_LAUNCH(ms_move_restr_kernel, grid, block, 0, st, mv);
    else if (p.has.boxes()) GRAPPA_LAUNCH(ms_move_cut_kernel, grid, block, 0, st, mv, w.box);
    else GRAPPA_LAUNCH(ms_move_kernel, grid, block, 0, st, mv);
}

// The energy terms at w.x, by the library's own entries.  six: the six of steps_terms_at (csrc/rs_force.h), in the part of this workspace
// that the cut or the planned nonbonded call takes (a frame that asks for the solvent's energy alone does not need them); with a
// solvent its two terms, in a region of their own.
int ms_launch_terms(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const MsPlan& p, const int* table_dev, int n_items,
                    int n_blocks, const MsCarve& k, bool six) {
    const MsWs& w = k.w;
    int rc = GRAPPA_OK;
    if (six && p.has.cut)
        rc = steps_terms_at(stream, mm, nb, p.cut.opts, table_dev, n_items, n_blocks, w.x, w.e_mm, w.e_nb, w.terms, w.nbcut, w.nbcut_bytes);
    else if (six)
        rc = steps_terms_at(stream, mm, nb, nullptr, table_dev, n_items, n_blocks, w.x, w.e_mm, w.e_nb, w.terms, w.nbpart,
                            sizeof(double) * 2 * (size_t)n_blocks * (size_t)mm->C);
    if (rc == GRAPPA_OK && p.has.gb)
        rc = steps_gb_cut_terms_at(stream, mm, nb, p.gb.opts, p.gb.cut, table_dev, n_items, n_blocks, w.x, k.gw.e_gb, k.gw.terms_gb, k.gw.fwd,
                                   k.gw.fwd_bytes);
    return rc;
}

MsOutArgs ms_out_args(const grappa_mm_desc* mm, const grappa_nb_desc* nb, const RsGeom& q, const MsWs& w) {
    MsOutArgs a = {};
    a.N = mm->N, a.C = mm->C, a.B = mm->B, a.n_blocks = q.n_blocks, a.has_nb = nb != nullptr;
    a.atom_molptr = mm->atom_molptr, a.blk_ptr = q.blk_ptr;
    a.x = w.x, a.v = w.v, a.terms = w.terms, a.kpart = w.kpart, a.bad = w.bad, a.status_ws = w.status, a.steps_ws = w.steps;
    return a;
}

// ms_out_kernel over `threads` threads and, with the solvent's terms, ms_out_gb_kernel behind it.  item_wise (constraints or restraints):
// a refused item's outputs are not touched
void ms_launch_out(hipStream_t st, const MsOutArgs& a, bool item_wise, size_t threads, const float* terms_gb, float* esolv) {
    const dim3 grid((unsigned)((threads + 255) / 256)), grid_bc((unsigned)(((size_t)a.B * a.C + 255) / 256)), block(256);
    if (item_wise) GRAPPA_LAUNCH(ms_out_kernel<true>, grid, block, 0, st, a);
    else GRAPPA_LAUNCH(ms_out_kernel<false>, grid, block, 0, st, a);
    if (!terms_gb) return;
    if (item_wise) GRAPPA_LAUNCH(ms_out_gb_kernel<true>, grid_bc, block, 0, st, a, terms_gb, esolv);
    else GRAPPA_LAUNCH(ms_out_gb_kernel<false>, grid_bc, block, 0, st, a, terms_gb, esolv);
}

// constraints as the three calls carry them: the caller's tables (cons->K > 0, checked), the step's constants and the workspace's words
MscDev msc_dev(const grappa_md_cons* cons, const grappa_md_opts* o, const MsWs& w) {
    MscDev d = {};
    d.molptr = cons->cluster_molptr, d.atoms = cons->cluster_atoms, d.d = cons->cluster_d, d.K = cons->K;
    d.claim = w.claim, d.cfail = w.cfail;
    d.tol2 = 2.0f * cons->tolerance;
    d.ih2 = 1.0f / md_consts(o).h2;
    return d;
}

void ms_launch_boxes(hipStream_t st, const grappa_nb_desc* nb, const RsGeom& q, const MsWs& w, int n_items) {
    const RsBoxArgs b = {q, w.x, nb->exc_ptr, nb->exc_atom, w.box, w.er};
    GRAPPA_LAUNCH(rs_box_kernel, dim3((unsigned)n_items), dim3(NB_NT), 0, st, b);
}

void msc_launch_close(hipStream_t st, const RsGeom& q, const MsWs& w, const MscDev& cn, const float* mass, int project, int n_items) {
    const MscCloseArgs a = {q, w.x, w.v, mass, w.status, cn, w.kpart, project};
    GRAPPA_LAUNCH(msc_close_kernel, dim3((unsigned)n_items), dim3(NB_NT), 0, st, a);
}

MrEnergyArgs mr_energy_args(const grappa_mm_desc* mm, const MsWs& w, const MrDev& m, int final, float* erestr, float* phi) {
    MrEnergyArgs a = {};
    a.N = mm->N, a.C = mm->C, a.B = mm->B, a.final = final;
    a.atom_molptr = mm->atom_molptr, a.x = w.x, a.status = w.status, a.m = m, a.erestr = erestr, a.phi = phi;
    return a;
}

// ------------------------------------------------------------------------------------------------ the three calls
// what an entry may be asked to write beyond the state: NULL where it is not asked for or its family has no such output
struct MsFrames {
    float *xyz, *epot, *ekin, *esolv, *erestr, *phi;
};

struct MsExch {                          // the logs of a run's attempts [X,B,C], each NULL where it is not asked for
    int* slot;
    float *epot, *erestr;
};

struct MsEnds {
    float *xyz, *vel, *epot, *ekin;      // required, as steps and status are
    int *steps, *status;
    float *esolv, *erestr, *phi;
    int* slots;                          // the ladder's entries: required there
};

int ms_init(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_md_opts* o, const MsPlan& p, const float* mass,
            const unsigned long long* mol_key, const float* vel_in, const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes) {
    const int rc = steps_seam_check(mm, nb, o && md_opts_ok(o), table_dev, n_items, n_blocks, ws);
    if (rc != GRAPPA_OK) return rc < 0 ? rc : GRAPPA_OK;
    if (!mass || !mol_key) return GRAPPA_ERR_ARG;
    const MsCarve cv = ms_carve((char*)ws, mm->N, mm->C, mm->B, n_blocks, p.has);
    if (ws_bytes < cv.total) return GRAPPA_ERR_WORKSPACE;
    const MsWs& w = cv.w;
    const MrDev mrd = ms_restr_dev(p, cv);
    const MrDev* mr = p.has.restr ? &mrd : nullptr;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    MsInitArgs a;
    a.N = mm->N, a.C = mm->C, a.B = mm->B, a.n_blocks = n_blocks;
    a.atom_molptr = mm->atom_molptr, a.start = mm->xyz, a.vel_in = vel_in, a.mass = mass, a.mol_key = mol_key;
    a.kt0 = md_consts(o).kt0, a.first_step = o->first_step;
    a.w = w;
    const bool at_ladder = p.has.remd && p.remd.init_at_ladder != 0;
    a.lad_t = at_ladder ? p.remd.temperatures : nullptr, a.lad_slots = at_ladder ? p.remd.slots_in : nullptr;
    size_t n = (size_t)mm->N * mm->C;
    const size_t bc = (size_t)mm->B * mm->C, kc = (size_t)n_blocks * mm->C;
    n = n > bc ? n : bc;
    n = n > kc ? n : kc;
    if (at_ladder) GRAPPA_LAUNCH(ms_init_ladder_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    else GRAPPA_LAUNCH(ms_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    const RsGeom q = rs_geom(mm, table_dev, n_blocks);
    if (p.has.remd) {          // the ladder vetted and its words set, behind the init kernel and in front of everything that reads status
        const MxInitArgs xa = {mm->N, mm->C, mm->B, n_blocks, mm->atom_molptr, q.blk_ptr, p.remd.slots_in, p.remd.every > 0, ms_remd_dev(p, cv),
                               w.status, w.bad};
        GRAPPA_LAUNCH(mx_init_kernel, dim3((unsigned)mm->B), dim3(256), 0, st, xa);
    }
    const dim3 grid((unsigned)n_items), block(NB_NT);
    MscDev cn = {};
    if (p.cons) {          // the tables vetted: clear, claim, read back
        cn = msc_dev(p.cons, o, w);
        const size_t nk = (size_t)mm->N > kc ? (size_t)mm->N : kc;
        GRAPPA_LAUNCH(msc_clear_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st, mm->N, kc, w.claim, w.cfail);
        if (n_items == 0) return grappa_launch_status();
        GRAPPA_LAUNCH(msc_claim_kernel, grid, block, 0, st, q, cn);
        GRAPPA_LAUNCH(msc_vet_kernel, grid, block, 0, st, q, cn, w.status, w.bad);
    }
    // with restraints: the reference into the workspace and the tables vetted, behind the init kernel (and the constraints' vet) and in
    // front of everything that reads status
    if (mr && mr->pos_k) {
        const size_t n3 = (size_t)mm->N * mm->C * 3;
        GRAPPA_LAUNCH(mr_ref_kernel, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, st, n3, p.restr.ref_src ? p.restr.ref_src : mm->xyz, cv.ref);
    }
    if (n_items == 0) return grappa_launch_status();
    if (mr) GRAPPA_LAUNCH(mr_vet_kernel, grid, block, 0, st, q, *mr, w.status, w.bad);
    // the start's S and P (with constraints), the boxes (with either cutoff), the gradient at the start without a kick, the solvent's
    // share of it, and with constraints the kinetic partials
    if (p.cons && (p.cons->constrain_start || !vel_in)) {
        const MscStartArgs sa = {q, w.x, w.v, mass, w.status, cn, p.cons->constrain_start != 0};
        GRAPPA_LAUNCH(msc_start_kernel, grid, block, 0, st, sa);
    }
    if (p.has.boxes()) ms_launch_boxes(st, nb, q, w, n_items);
    ms_launch_force(st, mm, nb, p.c(), q, w, mass, 0.f, nullptr, n_items, w.cfail, mr);
    if (p.has.gb) ms_launch_gb(st, nb, p.gb, q, w, cv.gw, mass, 0.f, n_items, p.has.cons);
    if (p.cons) msc_launch_close(st, q, w, cn, mass, 0, n_items);
    return grappa_launch_status();
}

int ms_run(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_md_opts* o, const MsPlan& p, const float* mass,
           const unsigned long long* mol_key, const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes, int step0, int n_steps,
           MsFrames fr, MsExch ex = MsExch{}) {
    // an output of an option the plan lacks is no output of this run: dropped before anything asks whether the run writes frames
    if (!p.has.gb) fr.esolv = nullptr;
    if (!p.has.restr) fr.erestr = fr.phi = nullptr;
    const int rc = steps_seam_check(mm, nb, o && md_opts_ok(o), table_dev, n_items, n_blocks, ws);
    if (rc < 0) return rc;
    if (n_steps < 1 || step0 < 0 || (long long)step0 + n_steps > o->n_steps) return GRAPPA_ERR_ARG;
    const bool frames_e = fr.epot || fr.ekin || fr.esolv, frames_r = fr.erestr || fr.phi;
    const bool frames = o->save_every > 0 && (fr.xyz || frames_e || frames_r);
    if (frames && step0 % o->save_every != 0) return GRAPPA_ERR_ARG;
    // a ladder with exchanges: K; its logs ask that the call begin on an attempt's boundary, so that row i is attempt base / K + 1 + i
    const unsigned K = p.has.remd ? (unsigned)p.remd.every : 0u, base = o->first_step + (unsigned)step0;
    if (K == 0) ex = MsExch{};
    if ((ex.slot || ex.epot || ex.erestr) && base % K != 0) return GRAPPA_ERR_ARG;
    if (rc != GRAPPA_OK) return GRAPPA_OK;
    if (!mass || !mol_key) return GRAPPA_ERR_ARG;
    const MsCarve cv = ms_carve((char*)ws, mm->N, mm->C, mm->B, n_blocks, p.has);
    if (ws_bytes < cv.total) return GRAPPA_ERR_WORKSPACE;
    const MsWs& w = cv.w;
    const MrDev mrd = ms_restr_dev(p, cv);
    const MrDev* mr = p.has.restr ? &mrd : nullptr;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const RsGeom q = rs_geom(mm, table_dev, n_blocks);
    const MdConsts k = md_consts(o);
    const float hkf = p.has.gb ? 0.f : k.hk;          // with the solvent the chain launch gives the closing kick
    const bool item_wise = p.has.cons || p.keep();
    const MxDev xd = ms_remd_dev(p, cv);
    MscDev cn = {};
    if (p.cons) cn = msc_dev(p.cons, o, w);
    MsMoveArgs mv;
    mv.kt_item = p.has.remd ? xd.kt_item : nullptr;
    mv.q = q, mv.x = w.x, mv.v = w.v, mv.g = w.g, mv.mass = mass, mv.mol_key = mol_key;
    mv.bad = w.bad, mv.status = w.status, mv.steps = w.steps, mv.k = k;
    const size_t n3 = (size_t)mm->N * mm->C * 3, bc = (size_t)mm->B * mm->C;
    const int frame0 = frames ? step0 / o->save_every : 0;
    for (int s = 0; s < n_steps; ++s) {
        const int done = step0 + s + 1;                                   // steps of the run completed by this one
        const bool due = frames && done % o->save_every == 0;
        const size_t f = due ? (size_t)(done / o->save_every - 1 - frame0) : 0;
        if (n_items > 0) {
            // move, force: 2 launches; with constraints move, boxes (with either cutoff), force, close: 3 or 4; the solvent's three
            // behind the force launch
            mv.step = o->first_step + (unsigned)(step0 + s);
            ms_launch_move(st, p, mv, cn, w, n_items);
            if (p.has.cons && p.has.boxes()) ms_launch_boxes(st, nb, q, w, n_items);
            ms_launch_force(st, mm, nb, p.c(), q, w, mass, hkf, due && fr.xyz ? fr.xyz + f * n3 : nullptr, n_items, w.cfail, mr);
            if (p.has.gb) ms_launch_gb(st, nb, p.gb, q, w, cv.gw, mass, k.hk, n_items, p.has.cons);
            if (p.has.cons) msc_launch_close(st, q, w, cn, mass, 1, n_items);
        }
        // the energy terms at the coordinates the step left: for the frame, for the attempt, once for both
        const bool exch = K > 0 && (base + (unsigned)s + 1u) % K == 0;
        const bool six = (due && fr.epot) || exch, terms = six || (due && fr.esolv);
        if (terms) {
            const int erc = ms_launch_terms(stream, mm, nb, p, table_dev, n_items, n_blocks, cv, six);
            if (erc != GRAPPA_OK) return erc;
        }
        if (due && frames_e) {
            MsOutArgs a = ms_out_args(mm, nb, q, w);
            a.final = 0, a.with_epot = fr.epot != nullptr;
            a.epot = fr.epot ? fr.epot + f * bc : nullptr, a.ekin = fr.ekin ? fr.ekin + f * bc : nullptr;
            ms_launch_out(st, a, item_wise, bc, p.has.gb && terms ? cv.gw.terms_gb : nullptr, fr.esolv ? fr.esolv + f * bc : nullptr);
        }
        if (due && frames_r) {          // E_r and the restrained dihedrals of the frame, at the coordinates the step left
            const MrEnergyArgs e = mr_energy_args(mm, w, *mr, 0, fr.erestr ? fr.erestr + f * bc : nullptr,
                                                  fr.phi ? fr.phi + f * (size_t)mr->R * mm->C : nullptr);
            GRAPPA_LAUNCH(mr_energy_kernel, dim3((unsigned)bc), dim3(MR_NT), 0, st, e);
        }
        if (exch) {
            // the attempt behind this step: epot and E_r as a frame at this step reports them -- the frame's own rows where it has them,
            // else the same launches into the ladder's scratch -- then the decisions, then the swapped replicas' velocities
            const unsigned g = base + (unsigned)s + 1u;
            const float *ue = due && fr.epot ? fr.epot + f * bc : nullptr, *ur = due && mr && fr.erestr ? fr.erestr + f * bc : nullptr;
            if (!ue) {
                MsOutArgs a = ms_out_args(mm, nb, q, w);
                a.final = 0, a.with_epot = 1, a.epot = xd.epot;
                ms_launch_out(st, a, item_wise, bc, p.has.gb ? cv.gw.terms_gb : nullptr, nullptr);
                ue = xd.epot;
            }
            if (mr && !ur) {
                const MrEnergyArgs e = mr_energy_args(mm, w, *mr, 0, xd.erestr, nullptr);
                GRAPPA_LAUNCH(mr_energy_kernel, dim3((unsigned)bc), dim3(MR_NT), 0, st, e);
                ur = xd.erestr;
            }
            const size_t row = (size_t)(g / K - base / K - 1u) * bc;
            const MxExchArgs xa = {mm->N, mm->C, mm->B, n_blocks, mm->atom_molptr, q.blk_ptr, mol_key, w.status, w.bad, xd, ue, ur, g,
                                   (int)((g / K) & 1u), ex.slot ? ex.slot + row : nullptr, ex.epot ? ex.epot + row : nullptr,
                                   ex.erestr ? ex.erestr + row : nullptr};
            GRAPPA_LAUNCH(ms_exchange_kernel, dim3((unsigned)mm->B), dim3(256), 0, st, xa);
            if (n_items > 0) {
                const MxRescaleArgs ra = {q, w.v, w.kpart, xd.scale};
                GRAPPA_LAUNCH(ms_rescale_kernel, dim3((unsigned)n_items), dim3(NB_NT), 0, st, ra);
            }
        }
    }
    return grappa_launch_status();
}

int ms_finish(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_md_opts* o, const MsPlan& p, const int* table_dev,
              int n_items, int n_blocks, void* ws, size_t ws_bytes, const MsEnds& e) {
    const int rc = steps_seam_check(mm, nb, o && md_opts_ok(o), table_dev, n_items, n_blocks, ws);
    if (rc != GRAPPA_OK) return rc < 0 ? rc : GRAPPA_OK;
    if (!e.xyz || !e.vel || !e.epot || !e.ekin || !e.steps || !e.status) return GRAPPA_ERR_ARG;
    const MsCarve cv = ms_carve((char*)ws, mm->N, mm->C, mm->B, n_blocks, p.has);
    if (ws_bytes < cv.total) return GRAPPA_ERR_WORKSPACE;
    const MsWs& w = cv.w;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int erc = ms_launch_terms(stream, mm, nb, p, table_dev, n_items, n_blocks, cv, true);
    if (erc != GRAPPA_OK) return erc;
    const RsGeom q = rs_geom(mm, table_dev, n_blocks);
    MsOutArgs a = ms_out_args(mm, nb, q, w);
    a.final = 1, a.with_epot = 1;
    a.xyz_out = e.xyz, a.vel_out = e.vel, a.epot = e.epot, a.ekin = e.ekin, a.steps = e.steps, a.status = e.status;
    const size_t n3 = (size_t)mm->N * mm->C * 3, bc = (size_t)mm->B * mm->C;
    const bool item_wise = p.has.cons || p.keep();          // a refused item's outputs are not touched: x and v item by item
    if (item_wise && n_items > 0) GRAPPA_LAUNCH(msc_copy_kernel, dim3((unsigned)n_items), dim3(NB_NT), 0, st, q, w.x, w.v, w.status, e.xyz, e.vel);
    ms_launch_out(st, a, item_wise, item_wise || n3 < bc ? bc : n3, p.has.gb ? cv.gw.terms_gb : nullptr, e.esolv);
    if (p.has.restr) {
        const MrEnergyArgs ea = mr_energy_args(mm, w, ms_restr_dev(p, cv), 1, e.erestr, e.phi);
        GRAPPA_LAUNCH(mr_energy_kernel, dim3((unsigned)bc), dim3(MR_NT), 0, st, ea);
    }
    if (e.slots)          // the ladder's entries: the slot every item holds (no ladder: c)
        GRAPPA_LAUNCH(mx_slots_out_kernel, dim3((unsigned)((bc + 255) / 256)), dim3(256), 0, st, mm->atom_molptr, mm->N, mm->B, mm->C, w.status,
                      p.has.remd ? cv.x.slot : nullptr, e.slots);
    return grappa_launch_status();
}

// without restraints the _restr_ finish still owes its caller erestr: 0 for the molecules that have atoms, behind a finish that succeeded
int ms_zero_erestr(void* stream, const grappa_mm_desc* mm, float* erestr) {
    if (!mm || mm->N <= 0 || mm->C <= 0 || mm->B <= 0 || !mm->atom_molptr) return GRAPPA_OK;
    const size_t bc = (size_t)mm->B * mm->C;
    GRAPPA_LAUNCH(mr_zero_kernel, dim3((unsigned)((bc + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), mm->atom_molptr, mm->N,
                  mm->B, mm->C, erestr);
    return grappa_launch_status();
}

}  // namespace

// ------------------------------------------------------------------------------------------------ the entries
// Seven families of four (the seventh, grappa_md_remd_*, at the end of the file): each takes the optional pointers of the one before it plus one, builds the plan from those it takes (the
// others NULL), returns GRAPPA_ERR_ARG if the plan is refused, and makes the call.  None calls another.
extern "C" size_t grappa_md_steps_workspace_bytes(int N, int C, int B, int n_blocks) { return ms_bytes(N, C, B, n_blocks, 0, MsHas{}); }

extern "C" int grappa_md_steps_init_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_md_opts* o,
                                        const float* mass, const unsigned long long* mol_key, const float* vel_in, const int* table_dev,
                                        int n_items, int n_blocks, void* ws, size_t ws_bytes) {
    MsPlan p;
    if (ms_plan(mm, nb, nullptr, nullptr, nullptr, nullptr, nullptr, p) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    return ms_init(stream, mm, nb, o, p, mass, mol_key, vel_in, table_dev, n_items, n_blocks, ws, ws_bytes);
}

extern "C" int grappa_md_steps_run_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_md_opts* o,
                                       const float* mass, const unsigned long long* mol_key, const int* table_dev, int n_items, int n_blocks,
                                       void* ws, size_t ws_bytes, int step0, int n_steps, float* frames_xyz, float* frames_epot,
                                       float* frames_ekin) {
    MsPlan p;
    if (ms_plan(mm, nb, nullptr, nullptr, nullptr, nullptr, nullptr, p) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    return ms_run(stream, mm, nb, o, p, mass, mol_key, table_dev, n_items, n_blocks, ws, ws_bytes, step0, n_steps,
                  MsFrames{frames_xyz, frames_epot, frames_ekin});
}

extern "C" int grappa_md_steps_finish_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_md_opts* o,
                                          const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes, float* xyz_out,
                                          float* vel_out, float* epot, float* ekin, int* steps, int* status) {
    MsPlan p;
    if (ms_plan(mm, nb, nullptr, nullptr, nullptr, nullptr, nullptr, p) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    return ms_finish(stream, mm, nb, o, p, table_dev, n_items, n_blocks, ws, ws_bytes, MsEnds{xyz_out, vel_out, epot, ekin, steps, status});
}

// with a nonbonded cutoff (cut)
extern "C" size_t grappa_md_steps_cut_workspace_bytes(int N, int C, int B, int n_blocks) {
    MsHas h = {};
    h.cut = true;
    return ms_bytes(N, C, B, n_blocks, 0, h);
}

extern "C" int grappa_md_steps_init_cut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                            const grappa_md_opts* o, const float* mass, const unsigned long long* mol_key, const float* vel_in,
                                            const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes) {
    MsPlan p;
    if (ms_plan(mm, nb, cut, nullptr, nullptr, nullptr, nullptr, p) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    return ms_init(stream, mm, nb, o, p, mass, mol_key, vel_in, table_dev, n_items, n_blocks, ws, ws_bytes);
}

extern "C" int grappa_md_steps_run_cut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                           const grappa_md_opts* o, const float* mass, const unsigned long long* mol_key, const int* table_dev,
                                           int n_items, int n_blocks, void* ws, size_t ws_bytes, int step0, int n_steps, float* frames_xyz,
                                           float* frames_epot, float* frames_ekin) {
    MsPlan p;
    if (ms_plan(mm, nb, cut, nullptr, nullptr, nullptr, nullptr, p) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    return ms_run(stream, mm, nb, o, p, mass, mol_key, table_dev, n_items, n_blocks, ws, ws_bytes, step0, n_steps,
                  MsFrames{frames_xyz, frames_epot, frames_ekin});
}

extern "C" int grappa_md_steps_finish_cut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                              const grappa_md_opts* o, const int* table_dev, int n_items, int n_blocks, void* ws,
                                              size_t ws_bytes, float* xyz_out, float* vel_out, float* epot, float* ekin, int* steps,
                                              int* status) {
    MsPlan p;
    if (ms_plan(mm, nb, cut, nullptr, nullptr, nullptr, nullptr, p) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    return ms_finish(stream, mm, nb, o, p, table_dev, n_items, n_blocks, ws, ws_bytes, MsEnds{xyz_out, vel_out, epot, ekin, steps, status});
}

// with X-H constraints (cons)
extern "C" size_t grappa_md_steps_cons_workspace_bytes(int N, int C, int B, int n_blocks, int K, int with_cut) {
    MsHas h = {};
    h.cut = with_cut != 0;
    return ms_bytes(N, C, B, n_blocks, K, h);
}

extern "C" int grappa_md_steps_init_cons_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                             const grappa_md_opts* o, const grappa_md_cons* cons, const float* mass,
                                             const unsigned long long* mol_key, const float* vel_in, const int* table_dev, int n_items,
                                             int n_blocks, void* ws, size_t ws_bytes) {
    MsPlan p;
    if (ms_plan(mm, nb, cut, cons, nullptr, nullptr, nullptr, p) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    return ms_init(stream, mm, nb, o, p, mass, mol_key, vel_in, table_dev, n_items, n_blocks, ws, ws_bytes);
}

extern "C" int grappa_md_steps_run_cons_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                            const grappa_md_opts* o, const grappa_md_cons* cons, const float* mass,
                                            const unsigned long long* mol_key, const int* table_dev, int n_items, int n_blocks, void* ws,
                                            size_t ws_bytes, int step0, int n_steps, float* frames_xyz, float* frames_epot, float* frames_ekin) {
    MsPlan p;
    if (ms_plan(mm, nb, cut, cons, nullptr, nullptr, nullptr, p) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    return ms_run(stream, mm, nb, o, p, mass, mol_key, table_dev, n_items, n_blocks, ws, ws_bytes, step0, n_steps,
                  MsFrames{frames_xyz, frames_epot, frames_ekin});
}

extern "C" int grappa_md_steps_finish_cons_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                               const grappa_md_opts* o, const grappa_md_cons* cons, const int* table_dev, int n_items,
                                               int n_blocks, void* ws, size_t ws_bytes, float* xyz_out, float* vel_out, float* epot, float* ekin,
                                               int* steps, int* status) {
    MsPlan p;
    if (ms_plan(mm, nb, cut, cons, nullptr, nullptr, nullptr, p) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    return ms_finish(stream, mm, nb, o, p, table_dev, n_items, n_blocks, ws, ws_bytes, MsEnds{xyz_out, vel_out, epot, ekin, steps, status});
}

// with the GB/SA implicit solvent (gb): no nonbonded cutoff beside it in this family
extern "C" size_t grappa_md_steps_gb_workspace_bytes(int N, int C, int B, int n_blocks, int K) {
    MsHas h = {};
    h.gb = true;
    return ms_bytes(N, C, B, n_blocks, K, h);
}

extern "C" int grappa_md_steps_init_gb_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                           const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb, const float* mass,
                                           const unsigned long long* mol_key, const float* vel_in, const int* table_dev, int n_items,
                                           int n_blocks, void* ws, size_t ws_bytes) {
    MsPlan p;
    if (ms_plan(mm, nb, cut, cons, gb, nullptr, nullptr, p) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    return ms_init(stream, mm, nb, o, p, mass, mol_key, vel_in, table_dev, n_items, n_blocks, ws, ws_bytes);
}

extern "C" int grappa_md_steps_run_gb_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                          const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb, const float* mass,
                                          const unsigned long long* mol_key, const int* table_dev, int n_items, int n_blocks, void* ws,
                                          size_t ws_bytes, int step0, int n_steps, float* frames_xyz, float* frames_epot, float* frames_ekin,
                                          float* frames_esolv) {
    MsPlan p;
    if (ms_plan(mm, nb, cut, cons, gb, nullptr, nullptr, p) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    return ms_run(stream, mm, nb, o, p, mass, mol_key, table_dev, n_items, n_blocks, ws, ws_bytes, step0, n_steps,
                  MsFrames{frames_xyz, frames_epot, frames_ekin, frames_esolv});
}

extern "C" int grappa_md_steps_finish_gb_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                             const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb, const int* table_dev,
                                             int n_items, int n_blocks, void* ws, size_t ws_bytes, float* xyz_out, float* vel_out, float* epot,
                                             float* ekin, int* steps, int* status, float* esolv) {
    MsPlan p;
    if (ms_plan(mm, nb, cut, cons, gb, nullptr, nullptr, p) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    return ms_finish(stream, mm, nb, o, p, table_dev, n_items, n_blocks, ws, ws_bytes,
                     MsEnds{xyz_out, vel_out, epot, ekin, steps, status, esolv});
}

// with the solvent under its own cutoff (gbcut, include/grappa_hip.h grappa_gb_cut): gb is then required, and cut may be given beside it
extern "C" size_t grappa_md_steps_gbcut_workspace_bytes(int N, int C, int B, int n_blocks, int K) {
    MsHas h = {};
    h.gb = h.gbcut = true;
    return ms_bytes(N, C, B, n_blocks, K, h);
}

extern "C" int grappa_md_steps_init_gbcut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                              const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb,
                                              const grappa_gb_cut* gbcut, const float* mass, const unsigned long long* mol_key,
                                              const float* vel_in, const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes) {
    MsPlan p;
    if (ms_plan(mm, nb, cut, cons, gb, gbcut, nullptr, p) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    return ms_init(stream, mm, nb, o, p, mass, mol_key, vel_in, table_dev, n_items, n_blocks, ws, ws_bytes);
}

extern "C" int grappa_md_steps_run_gbcut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                             const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb,
                                             const grappa_gb_cut* gbcut, const float* mass, const unsigned long long* mol_key,
                                             const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes, int step0, int n_steps,
                                             float* frames_xyz, float* frames_epot, float* frames_ekin, float* frames_esolv) {
    MsPlan p;
    if (ms_plan(mm, nb, cut, cons, gb, gbcut, nullptr, p) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    return ms_run(stream, mm, nb, o, p, mass, mol_key, table_dev, n_items, n_blocks, ws, ws_bytes, step0, n_steps,
                  MsFrames{frames_xyz, frames_epot, frames_ekin, frames_esolv});
}

extern "C" int grappa_md_steps_finish_gbcut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                                const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb,
                                                const grappa_gb_cut* gbcut, const int* table_dev, int n_items, int n_blocks, void* ws,
                                                size_t ws_bytes, float* xyz_out, float* vel_out, float* epot, float* ekin, int* steps, int* status,
                                                float* esolv) {
    MsPlan p;
    if (ms_plan(mm, nb, cut, cons, gb, gbcut, nullptr, p) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    return ms_finish(stream, mm, nb, o, p, table_dev, n_items, n_blocks, ws, ws_bytes,
                     MsEnds{xyz_out, vel_out, epot, ekin, steps, status, esolv});
}

// with restraints (r, include/grappa_hip.h grappa_md_restr).  The finish requires erestr whatever the plan holds; without restraints it is
// written as 0 for molecules that have atoms, and the frames' restraint outputs are not written.
extern "C" size_t grappa_md_steps_restr_workspace_bytes(int N, int C, int B, int n_blocks, int K, int with_cut, int with_gb, int with_gbcut) {
    MsHas h = {};
    h.cut = with_cut != 0, h.gbcut = with_gbcut != 0, h.gb = with_gb != 0 || h.gbcut, h.restr = true;
    return ms_bytes(N, C, B, n_blocks, K, h);
}

extern "C" int grappa_md_steps_init_restr_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                              const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb,
                                              const grappa_gb_cut* gbcut, const grappa_md_restr* r, const float* mass,
                                              const unsigned long long* mol_key, const float* vel_in, const int* table_dev, int n_items,
                                              int n_blocks, void* ws, size_t ws_bytes) {
    MsPlan p;
    if (ms_plan(mm, nb, cut, cons, gb, gbcut, r, p) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    return ms_init(stream, mm, nb, o, p, mass, mol_key, vel_in, table_dev, n_items, n_blocks, ws, ws_bytes);
}

extern "C" int grappa_md_steps_run_restr_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                             const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb,
                                             const grappa_gb_cut* gbcut, const grappa_md_restr* r, const float* mass,
                                             const unsigned long long* mol_key, const int* table_dev, int n_items, int n_blocks, void* ws,
                                             size_t ws_bytes, int step0, int n_steps, float* frames_xyz, float* frames_epot, float* frames_ekin,
                                             float* frames_esolv, float* frames_erestr, float* frames_phi) {
    MsPlan p;
    if (ms_plan(mm, nb, cut, cons, gb, gbcut, r, p) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    return ms_run(stream, mm, nb, o, p, mass, mol_key, table_dev, n_items, n_blocks, ws, ws_bytes, step0, n_steps,
                  MsFrames{frames_xyz, frames_epot, frames_ekin, frames_esolv, frames_erestr, frames_phi});
}

extern "C" int grappa_md_steps_finish_restr_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                                const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb,
                                                const grappa_gb_cut* gbcut, const grappa_md_restr* r, const int* table_dev, int n_items,
                                                int n_blocks, void* ws, size_t ws_bytes, float* xyz_out, float* vel_out, float* epot, float* ekin,
                                                int* steps, int* status, float* esolv, float* erestr, float* dih_phi) {
    MsPlan p;
    if (!erestr || ms_plan(mm, nb, cut, cons, gb, gbcut, r, p) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    const int fc = ms_finish(stream, mm, nb, o, p, table_dev, n_items, n_blocks, ws, ws_bytes,
                             MsEnds{xyz_out, vel_out, epot, ekin, steps, status, esolv, erestr, dih_phi});
    return fc != GRAPPA_OK || p.has.restr ? fc : ms_zero_erestr(stream, mm, erestr);
}

// on a temperature ladder, with or without exchanges (x, include/grappa_hip.h grappa_md_remd): the _restr_ calls with x directly after r.
// x == NULL is the _restr_ call itself; the finish then writes slots_out as c.
extern "C" size_t grappa_md_remd_workspace_bytes(int N, int C, int B, int n_blocks, int K, int with_cut, int with_gb, int with_gbcut,
                                                 int with_restr) {
    MsHas h = {};
    h.cut = with_cut != 0, h.gbcut = with_gbcut != 0, h.gb = with_gb != 0 || h.gbcut, h.restr = with_restr != 0, h.remd = true;
    return ms_bytes(N, C, B, n_blocks, K, h);
}

extern "C" int grappa_md_remd_init_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                       const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb, const grappa_gb_cut* gbcut,
                                       const grappa_md_restr* r, const grappa_md_remd* x, const float* mass, const unsigned long long* mol_key,
                                       const float* vel_in, const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes) {
    MsPlan p;
    if (ms_plan(mm, nb, cut, cons, gb, gbcut, r, p, x, o) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    return ms_init(stream, mm, nb, o, p, mass, mol_key, vel_in, table_dev, n_items, n_blocks, ws, ws_bytes);
}

extern "C" int grappa_md_remd_run_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                      const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb, const grappa_gb_cut* gbcut,
                                      const grappa_md_restr* r, const grappa_md_remd* x, const float* mass, const unsigned long long* mol_key,
                                      const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes, int step0, int n_steps,
                                      float* frames_xyz, float* frames_epot, float* frames_ekin, float* frames_esolv, float* frames_erestr,
                                      float* frames_phi, int* exch_slot, float* exch_epot, float* exch_erestr) {
    MsPlan p;
    if (ms_plan(mm, nb, cut, cons, gb, gbcut, r, p, x, o) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    return ms_run(stream, mm, nb, o, p, mass, mol_key, table_dev, n_items, n_blocks, ws, ws_bytes, step0, n_steps,
                  MsFrames{frames_xyz, frames_epot, frames_ekin, frames_esolv, frames_erestr, frames_phi}, MsExch{exch_slot, exch_epot, exch_erestr});
}

extern "C" int grappa_md_remd_finish_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                         const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb, const grappa_gb_cut* gbcut,
                                         const grappa_md_restr* r, const grappa_md_remd* x, const int* table_dev, int n_items, int n_blocks,
                                         void* ws, size_t ws_bytes, float* xyz_out, float* vel_out, float* epot, float* ekin, int* steps,
                                         int* status, float* esolv, float* erestr, float* dih_phi, int* slots_out) {
    MsPlan p;
    if (!erestr || !slots_out || ms_plan(mm, nb, cut, cons, gb, gbcut, r, p, x, o) != GRAPPA_OK) return GRAPPA_ERR_ARG;
    const int fc = ms_finish(stream, mm, nb, o, p, table_dev, n_items, n_blocks, ws, ws_bytes,
                             MsEnds{xyz_out, vel_out, epot, ekin, steps, status, esolv, erestr, dih_phi, slots_out});
    return fc != GRAPPA_OK || p.has.restr ? fc : ms_zero_erestr(stream, mm, erestr);
}
