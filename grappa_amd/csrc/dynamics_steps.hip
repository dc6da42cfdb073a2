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
//   cutoff : grappa_md_steps_*_cut_f32 (cut == NULL: the calls without).  The force launch is rs_force under the cut policy of
//            csrc/nb_cut.h; the move launch's item writes the box of its own (block, conformations) after moving -- the box's only
//            writer -- and the force launch reads all boxes across the launch boundary: a step stays two launches, init gains one (boxes
//            and exception ranges).  Energies by grappa_nonbonded_fwd_cut_f32 at the held coordinates.
// Same input, same bits; a molecule's bits depend neither on its place in the batch nor on how the steps are dealt out to run calls.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"
#include "desc_check.h"
#include "md_noise.h"
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
    size_t total;
};

// (the words of a cutoff lie behind the others: without one the layout is the one it was)
MsWs ms_layout(char* base, int N, int C, int B, int n_blocks, bool cut = false) {
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
};

// a thread per (atom, conformation): x = start, v = vel_in (a frozen atom: 0) or the draw at init_temperature; the first B * C threads
// also set the items' state, the first n_blocks * C the blocks' words
__global__ __launch_bounds__(256) void ms_init_kernel(MsInitArgs a) {
    const size_t u = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int N = a.N, C = a.C, B = a.B;
    if (u < (size_t)N * C) {
        const int atom = (int)(u / (unsigned)C), c = (int)(u - (size_t)atom * C);
        V3 v = {0.f, 0.f, 0.f};
        const float m = a.mass[atom];
        if (m > 0.f) {          // (a mass that is zero, negative or NaN: a frozen atom, v = 0)
            if (a.vel_in) {
                v = {a.vel_in[3 * u], a.vel_in[3 * u + 1], a.vel_in[3 * u + 2]};
            } else if (a.kt0 > 0.f) {
                int lo = 0, hi = B - 1;          // the last molecule that starts at or before the atom
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (nb_clamp(a.atom_molptr[mid], N) <= atom) lo = mid; else hi = mid - 1;
                }
                const int m0 = nb_clamp(a.atom_molptr[lo], N), m1 = nb_clamp(a.atom_molptr[lo + 1], N);
                if (atom >= m0 && atom < m1)          // (an atom that no molecule holds keeps v = 0)
                    v = sqrtf(a.kt0 * (1.0f / m)) * md_normal3(a.mol_key[lo], (unsigned)(atom - m0), (unsigned)c, a.first_step, 1u);
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
};

// the thread's (atom, conformation) of the item; CUT: the coordinates it leaves -> bxl[0..3) (not for a stopped conformation)
template <bool CUT>
__device__ __forceinline__ void ms_move_lane(const MsMoveArgs& a, const RsItem& r, int k0, const int* stop, float* bxl) {
    const int C = a.q.C, t = threadIdx.x, ni = r.ni;
    const int cl = t / ni, il = t - cl * ni;
    const int i = r.i0 + il, c = r.c0 + cl;
    const size_t item = (size_t)r.mol * C + c;
    const bool writer = r.blk == k0 && il == 0;      // the molecule's first block: the one writer of the item's status and steps
    if (stop[cl]) {                                  // a non-finite gradient: the item keeps the x and v it holds
        if (writer) a.status[item] = 2;
        return;
    }
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
            vk = a.k.c1 * vk + (a.k.c2 * sqrtf(a.k.kt * im)) * md_normal3(a.mol_key[r.mol], (unsigned)(i - r.m0), (unsigned)c, a.step, 0u);
        xx += a.k.h2 * vk.x, xy += a.k.h2 * vk.y, xz += a.k.h2 * vk.z;
        a.x[off] = xx, a.x[off + 1] = xy, a.x[off + 2] = xz;
        a.v[off] = vk.x, a.v[off + 1] = vk.y, a.v[off + 2] = vk.z;
        if constexpr (CUT) bxl[0] = xx, bxl[1] = xy, bxl[2] = xz;
    } else if constexpr (CUT) {
        const size_t off = ((size_t)i * C + c) * 3;
        bxl[0] = a.x[off], bxl[1] = a.x[off + 1], bxl[2] = a.x[off + 2];
    }
    if (writer) a.steps[item] += 1;
}

// CUT: the item also writes the box of its own (block, conformations) at the coordinates it leaves (csrc/nb_cut.h): it is the box's only
// writer, the force launch after it the reader.  A stopped conformation keeps its box, as it keeps its x.
template <bool CUT>
__device__ __forceinline__ void ms_move_body(const MsMoveArgs& a, float4* box) {
    __shared__ int stop[NB_CW];
    RsItem r;
    if (!rs_item(a.q, r)) return;
    const int C = a.q.C, t = threadIdx.x, ni = r.ni;
    // has a block of the molecule flagged the conformation?  Every workgroup of the molecule forms the same OR from the same words, which
    // the force launch before this one wrote: wavefront w takes the conformations w, w + 4, .., its lanes the blocks
    const int k0 = nb_clamp(a.q.blk_ptr[r.mol], a.q.n_blocks), k1 = nb_clamp(a.q.blk_ptr[r.mol + 1], a.q.n_blocks);
    const int wave = t / GRAPPA_WAVE, lane = t & (GRAPPA_WAVE - 1);
    for (int cc = wave; cc < r.nc; cc += MS_NW) {
        int f = 0;
        for (int k = k0 + lane; k < k1; k += GRAPPA_WAVE) f |= a.bad[(size_t)k * C + r.c0 + cc];
        const bool any = __builtin_amdgcn_ballot_w64(f != 0) != 0;
        if (lane == 0) stop[cc] = any ? 1 : 0;
    }
    __syncthreads();
    if constexpr (CUT) {
        __shared__ float bx[NB_NT * 3];
        if (t < ni * r.nc) ms_move_lane<true>(a, r, k0, stop, bx + 3 * t);
        nb_cut_box_write(bx, stop, ni, r.nc, r.blk, C, r.c0, box);
    } else {
        if (t < ni * r.nc) ms_move_lane<false>(a, r, k0, stop, nullptr);
    }
}

__global__ __launch_bounds__(NB_NT) void ms_move_kernel(MsMoveArgs a) { ms_move_body<false>(a, nullptr); }
__global__ __launch_bounds__(NB_NT) void ms_move_cut_kernel(MsMoveArgs a, float4* box) { ms_move_body<true>(a, box); }

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

template <class Cut>
__device__ __forceinline__ void ms_force_body(const MsForceArgs& a, const Cut& cut) {
    __shared__ RsShared sh;
    rs_force(a.f, sh, cut, [&](const RsItem& r, const RsLane& w, V3 gi) {
        const int C = a.f.q.C, ni = r.ni;
        float mv2 = 0.f, bad = 0.f;
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
            a.kpart[o] = sk;
            a.bad[o] = fb != 0.f ? 1 : 0;
        }
    });
}

__global__ __launch_bounds__(NB_NT) void ms_force_kernel(MsForceArgs a) { ms_force_body(a, NbNoCut{}); }

__global__ __launch_bounds__(NB_NT) void ms_force_cut_kernel(MsForceArgs a, NbCutDev c) {
    __shared__ unsigned char near[NB_NT];
    ms_force_body(a, NbCut{c, near});
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

__global__ __launch_bounds__(256) void ms_out_kernel(MsOutArgs a) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (a.final && gid < (size_t)a.N * a.C * 3) {
        a.xyz_out[gid] = a.x[gid];
        a.vel_out[gid] = a.v[gid];
    }
    const size_t bc = (size_t)a.B * a.C;
    if (gid >= bc) return;
    const int b = (int)(gid / (unsigned)a.C), c = (int)(gid - (size_t)b * a.C);
    if (nb_clamp(a.atom_molptr[b + 1], a.N) <= nb_clamp(a.atom_molptr[b], a.N)) return;      // a molecule without atoms writes nothing
    const int st = a.status_ws[gid];
    if (!a.final && st != RS_RUNNING) return;       // a stopped item's later frames are not written
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
    if (a.final) {
        a.steps[gid] = a.steps_ws[gid];
        a.status[gid] = st == RS_RUNNING ? (flagged ? 2 : 0) : st;      // (the gradient that closed the last step is tested here)
    }
}

// ------------------------------------------------------------------------------------------------ host
// (the argument checks the three calls share: steps_seam_check of csrc/desc_check.h; GRAPPA_SEAM_EMPTY: nothing to do)

// (a cutoff as the three calls carry it: RsCut / rs_cut_make of csrc/rs_force.h; c == NULL: none)
void ms_launch_force(hipStream_t st, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const RsCut* c, const RsGeom& q, const MsWs& w,
                     const float* mass, float hk, float* frame_xyz, int n_items) {
    MsForceArgs f;
    f.f = rs_force_in(mm, nb, q, w.x, w.status);
    f.v = w.v, f.g = w.g, f.mass = mass, f.bad = w.bad, f.kpart = w.kpart;
    f.hk = hk, f.frame_xyz = frame_xyz;
    if (c) {
        NbCutDev d = c->dev;
        d.box = w.box, d.er = w.er;
        GRAPPA_LAUNCH(ms_force_cut_kernel, dim3((unsigned)n_items), dim3(NB_NT), 0, st, f, d);
    } else {
        GRAPPA_LAUNCH(ms_force_kernel, dim3((unsigned)n_items), dim3(NB_NT), 0, st, f);
    }
}

// steps_terms_at of csrc/rs_force.h at w.x, in the part of this workspace that the cut or the planned nonbonded call takes
int ms_launch_terms(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const RsCut* c, const int* table_dev, int n_items,
                    int n_blocks, const MsWs& w) {
    if (c) return steps_terms_at(stream, mm, nb, c->opts, table_dev, n_items, n_blocks, w.x, w.e_mm, w.e_nb, w.terms, w.nbcut, w.nbcut_bytes);
    return steps_terms_at(stream, mm, nb, nullptr, table_dev, n_items, n_blocks, w.x, w.e_mm, w.e_nb, w.terms, w.nbpart,
                          sizeof(double) * 2 * (size_t)n_blocks * (size_t)mm->C);
}

MsOutArgs ms_out_args(const grappa_mm_desc* mm, const grappa_nb_desc* nb, const RsGeom& q, const MsWs& w) {
    MsOutArgs a = {};
    a.N = mm->N, a.C = mm->C, a.B = mm->B, a.n_blocks = q.n_blocks, a.has_nb = nb != nullptr;
    a.atom_molptr = mm->atom_molptr, a.blk_ptr = q.blk_ptr;
    a.x = w.x, a.v = w.v, a.terms = w.terms, a.kpart = w.kpart, a.bad = w.bad, a.status_ws = w.status, a.steps_ws = w.steps;
    return a;
}

// the three calls, with and without a cutoff (c == NULL: none)
int ms_init(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const RsCut* c, const grappa_md_opts* o, const float* mass,
            const unsigned long long* mol_key, const float* vel_in, const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes) {
    const int rc = steps_seam_check(mm, nb, o && md_opts_ok(o), table_dev, n_items, n_blocks, ws);
    if (rc != GRAPPA_OK) return rc < 0 ? rc : GRAPPA_OK;
    if (!mass || !mol_key) return GRAPPA_ERR_ARG;
    const MsWs w = ms_layout((char*)ws, mm->N, mm->C, mm->B, n_blocks, c != nullptr);
    if (ws_bytes < w.total) return GRAPPA_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    MsInitArgs a;
    a.N = mm->N, a.C = mm->C, a.B = mm->B, a.n_blocks = n_blocks;
    a.atom_molptr = mm->atom_molptr, a.start = mm->xyz, a.vel_in = vel_in, a.mass = mass, a.mol_key = mol_key;
    a.kt0 = md_consts(o).kt0, a.first_step = o->first_step;
    a.w = w;
    size_t n = (size_t)mm->N * mm->C;
    const size_t bc = (size_t)mm->B * mm->C, kc = (size_t)n_blocks * mm->C;
    n = n > bc ? n : bc;
    n = n > kc ? n : kc;
    GRAPPA_LAUNCH(ms_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    const RsGeom q = rs_geom(mm, table_dev, n_blocks);
    if (c && n_items > 0) {
        const RsBoxArgs b = {q, w.x, nb->exc_ptr, nb->exc_atom, w.box, w.er};
        GRAPPA_LAUNCH(rs_box_kernel, dim3((unsigned)n_items), dim3(NB_NT), 0, st, b);
    }
    if (n_items > 0) ms_launch_force(st, mm, nb, c, q, w, mass, 0.f, nullptr, n_items);
    return grappa_launch_status();
}

int ms_run(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const RsCut* c, const grappa_md_opts* o, const float* mass,
           const unsigned long long* mol_key, const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes, int step0, int n_steps,
           float* frames_xyz, float* frames_epot, float* frames_ekin) {
    const int rc = steps_seam_check(mm, nb, o && md_opts_ok(o), table_dev, n_items, n_blocks, ws);
    if (rc < 0) return rc;
    if (n_steps < 1 || step0 < 0 || (long long)step0 + n_steps > o->n_steps) return GRAPPA_ERR_ARG;
    const bool frames = o->save_every > 0 && (frames_xyz || frames_epot || frames_ekin);
    if (frames && step0 % o->save_every != 0) return GRAPPA_ERR_ARG;
    if (rc != GRAPPA_OK) return GRAPPA_OK;
    if (!mass || !mol_key) return GRAPPA_ERR_ARG;
    const MsWs w = ms_layout((char*)ws, mm->N, mm->C, mm->B, n_blocks, c != nullptr);
    if (ws_bytes < w.total) return GRAPPA_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const RsGeom q = rs_geom(mm, table_dev, n_blocks);
    const MdConsts k = md_consts(o);
    MsMoveArgs mv;
    mv.q = q, mv.x = w.x, mv.v = w.v, mv.g = w.g, mv.mass = mass, mv.mol_key = mol_key;
    mv.bad = w.bad, mv.status = w.status, mv.steps = w.steps, mv.k = k;
    const size_t n3 = (size_t)mm->N * mm->C * 3, bc = (size_t)mm->B * mm->C;
    const int frame0 = frames ? step0 / o->save_every : 0;
    for (int s = 0; s < n_steps; ++s) {
        const int done = step0 + s + 1;                                   // steps of the run completed by this one
        const bool due = frames && done % o->save_every == 0;
        const size_t f = due ? (size_t)(done / o->save_every - 1 - frame0) : 0;
        if (n_items > 0) {
            mv.step = o->first_step + (unsigned)(step0 + s);
            if (c) GRAPPA_LAUNCH(ms_move_cut_kernel, dim3((unsigned)n_items), dim3(NB_NT), 0, st, mv, w.box);
            else GRAPPA_LAUNCH(ms_move_kernel, dim3((unsigned)n_items), dim3(NB_NT), 0, st, mv);
            ms_launch_force(st, mm, nb, c, q, w, mass, k.hk, due && frames_xyz ? frames_xyz + f * n3 : nullptr, n_items);
        }
        if (due && (frames_epot || frames_ekin)) {
            if (frames_epot) {
                const int erc = ms_launch_terms(stream, mm, nb, c, table_dev, n_items, n_blocks, w);
                if (erc != GRAPPA_OK) return erc;
            }
            MsOutArgs a = ms_out_args(mm, nb, q, w);
            a.final = 0, a.with_epot = frames_epot != nullptr;
            a.epot = frames_epot ? frames_epot + f * bc : nullptr, a.ekin = frames_ekin ? frames_ekin + f * bc : nullptr;
            GRAPPA_LAUNCH(ms_out_kernel, dim3((unsigned)((bc + 255) / 256)), dim3(256), 0, st, a);
        }
    }
    return grappa_launch_status();
}

int ms_finish(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const RsCut* c, const grappa_md_opts* o, const int* table_dev,
              int n_items, int n_blocks, void* ws, size_t ws_bytes, float* xyz_out, float* vel_out, float* epot, float* ekin, int* steps,
              int* status) {
    const int rc = steps_seam_check(mm, nb, o && md_opts_ok(o), table_dev, n_items, n_blocks, ws);
    if (rc != GRAPPA_OK) return rc < 0 ? rc : GRAPPA_OK;
    if (!xyz_out || !vel_out || !epot || !ekin || !steps || !status) return GRAPPA_ERR_ARG;
    const MsWs w = ms_layout((char*)ws, mm->N, mm->C, mm->B, n_blocks, c != nullptr);
    if (ws_bytes < w.total) return GRAPPA_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int erc = ms_launch_terms(stream, mm, nb, c, table_dev, n_items, n_blocks, w);
    if (erc != GRAPPA_OK) return erc;
    MsOutArgs a = ms_out_args(mm, nb, rs_geom(mm, table_dev, n_blocks), w);
    a.final = 1, a.with_epot = 1;
    a.xyz_out = xyz_out, a.vel_out = vel_out, a.epot = epot, a.ekin = ekin, a.steps = steps, a.status = status;
    const size_t n3 = (size_t)mm->N * mm->C * 3, bc = (size_t)mm->B * mm->C, n = n3 > bc ? n3 : bc;
    GRAPPA_LAUNCH(ms_out_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    return grappa_launch_status();
}

}  // namespace

extern "C" size_t grappa_md_steps_workspace_bytes(int N, int C, int B, int n_blocks) {
    if (N <= 0 || C <= 0 || B <= 0 || n_blocks < 0) return 0;
    return ms_layout(nullptr, N, C, B, n_blocks).total;
}

extern "C" int grappa_md_steps_init_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_md_opts* o,
                                        const float* mass, const unsigned long long* mol_key, const float* vel_in, const int* table_dev,
                                        int n_items, int n_blocks, void* ws, size_t ws_bytes) {
    return ms_init(stream, mm, nb, nullptr, o, mass, mol_key, vel_in, table_dev, n_items, n_blocks, ws, ws_bytes);
}

extern "C" int grappa_md_steps_run_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_md_opts* o,
                                       const float* mass, const unsigned long long* mol_key, const int* table_dev, int n_items, int n_blocks,
                                       void* ws, size_t ws_bytes, int step0, int n_steps, float* frames_xyz, float* frames_epot,
                                       float* frames_ekin) {
    return ms_run(stream, mm, nb, nullptr, o, mass, mol_key, table_dev, n_items, n_blocks, ws, ws_bytes, step0, n_steps, frames_xyz, frames_epot,
                  frames_ekin);
}

extern "C" int grappa_md_steps_finish_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_md_opts* o,
                                          const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes, float* xyz_out,
                                          float* vel_out, float* epot, float* ekin, int* steps, int* status) {
    return ms_finish(stream, mm, nb, nullptr, o, table_dev, n_items, n_blocks, ws, ws_bytes, xyz_out, vel_out, epot, ekin, steps, status);
}

// with a cutoff: cut == NULL is the call above; bad options in cut, or a cut without nb, are refused before anything else is looked at
extern "C" size_t grappa_md_steps_cut_workspace_bytes(int N, int C, int B, int n_blocks) {
    if (N <= 0 || C <= 0 || B <= 0 || n_blocks < 0) return 0;
    return ms_layout(nullptr, N, C, B, n_blocks, true).total;
}

extern "C" int grappa_md_steps_init_cut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                            const grappa_md_opts* o, const float* mass, const unsigned long long* mol_key, const float* vel_in,
                                            const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes) {
    RsCut c;
    if (cut && !rs_cut_make(cut, nb, c)) return GRAPPA_ERR_ARG;
    return ms_init(stream, mm, nb, cut ? &c : nullptr, o, mass, mol_key, vel_in, table_dev, n_items, n_blocks, ws, ws_bytes);
}

extern "C" int grappa_md_steps_run_cut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                           const grappa_md_opts* o, const float* mass, const unsigned long long* mol_key, const int* table_dev,
                                           int n_items, int n_blocks, void* ws, size_t ws_bytes, int step0, int n_steps, float* frames_xyz,
                                           float* frames_epot, float* frames_ekin) {
    RsCut c;
    if (cut && !rs_cut_make(cut, nb, c)) return GRAPPA_ERR_ARG;
    return ms_run(stream, mm, nb, cut ? &c : nullptr, o, mass, mol_key, table_dev, n_items, n_blocks, ws, ws_bytes, step0, n_steps, frames_xyz,
                  frames_epot, frames_ekin);
}

extern "C" int grappa_md_steps_finish_cut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                              const grappa_md_opts* o, const int* table_dev, int n_items, int n_blocks, void* ws,
                                              size_t ws_bytes, float* xyz_out, float* vel_out, float* epot, float* ekin, int* steps,
                                              int* status) {
    RsCut c;
    if (cut && !rs_cut_make(cut, nb, c)) return GRAPPA_ERR_ARG;
    return ms_finish(stream, mm, nb, cut ? &c : nullptr, o, table_dev, n_items, n_blocks, ws, ws_bytes, xyz_out, vel_out, epot, ekin, steps, status);
}
