// Stepwise FIRE minimiser for molecules of any size under the full MM force field, fp32 (include/grappa_hip.h
// grappa_relax_steps_*_f32): the loop of csrc/relax.hip with a molecule spread over many workgroups and a step made of four launches.
//   items  : the nonbonded plan's (csrc/nb_plan.h): (molecule, block of ni <= 64 i-atoms, nc conformations), one workgroup of 256 threads
//            each; the plan is about atoms, so it also serves a call without nonbonded parameters.
//   state  : in the caller's workspace: x, v, g [N,C,3]; per (molecule, conformation) h, a, npos, steps, status and the scalars of the
//            step in flight (mix, keep, downhill, gmax); per (block, conformation) the partials P, |F|^2, |v|^2, max |g_i| (double) and
//            max |d_i| (float).
//   step   : decide  one workgroup of 64 threads per (molecule, conformation): adds the item's block partials in ascending block
//                    order in double (as nb_reduce_kernel does), applies the loop's stop tests and FIRE's decisions (csrc/fire.h) and
//                    writes the item's new scalars.  It is the ONLY writer of the per-item state, and it runs in a launch of its own: no workgroup
//                    reads a scalar that a sibling writes in the same launch.
//            vel     v = keep v + mix F + h F per atom, the block's max |h v_i|
//            move    max over the item's blocks, s = min(1, max_disp / max), x += s h v, v = s v
//            force   g at the new x (rs_force of csrc/rs_force.h: the bonded gradient plus the pair loop of nb_pairs_kernel itself,
//                    slices added in slice order); then the block's partials.
//            Launch boundaries are the only synchronisation between workgroups: no cooperative launch, no flag, no float atomics.
//            The one atomic is the integer decrement of the count of running items by the thread that stops an item.
//   stopped: every launch leaves a (molecule, conformation) whose status is final alone, so the result depends neither on the number of
//            steps enqueued after it stopped nor on the chunk size.
//   finish : one more decide (stop tests only), the six energy terms by the library's own energy kernels (mm_energy_kernel,
//            nb_pairs_kernel + nb_reduce_kernel through their entry points: no second energy code path) at the held coordinates, and a
//            copy kernel.
//   cutoff : grappa_relax_steps_*_cut_f32 (cut == NULL: the calls without).  The force launch is rs_force under the cut policy of
//            csrc/nb_cut.h; the move launch's item writes the box of its own (block, conformations) after moving -- the box's only
//            writer -- and the force launch reads all boxes across the launch boundary: a step stays four launches, init gains one (boxes
//            and exception ranges).  The finish's nonbonded energy by grappa_nonbonded_fwd_cut_f32 at the held coordinates.
//   solvent: grappa_relax_steps_*_gb_f32 (gb == NULL: the calls without).  The section "implicit solvent" below: the force launch as it
//            is, then born, pair and chain of csrc/gb_pass.h; the chain launch's epilogue completes g and rewrites the block's partials.
// Same input, same bits; a molecule's bits do not depend on its place in the batch.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"
#include "desc_check.h"
#include "fire.h"
#include "gb_pass.h"
#include "rs_force.h"

namespace {

constexpr int RS_DNT = 64;               // threads of a decide workgroup
constexpr int RS_NW = NB_NT / GRAPPA_WAVE;

struct RsState {                         // per (molecule, conformation): [B*C] each
    float *h, *al, *mix, *keep, *gmax;
    int *npos, *steps, *status, *downhill;
};

struct RsWs {
    float *x, *v, *g;                    // [N,C,3]
    RsState s;
    double* part;                        // [n_blocks][C][4]: P, |F|^2, |v|^2, max |g_i| (inf: a non-finite gradient)
    float* dpart;                        // [n_blocks][C]: max |h v_i|
    float *e_mm, *e_nb, *terms;          // finish: [B,C], [B,C], [6,B,C]
    double* nbpart;                      // finish: the nonbonded kernel's partial energies [n_blocks][C][2]
    float4* box;                         // with a cutoff: the blocks' boxes [n_blocks][C][2] and exception ranges [n_blocks] (csrc/nb_cut.h)
    int2* er;
    char* nbcut;                         // with a cutoff, finish: the workspace of grappa_nonbonded_fwd_cut_f32
    size_t nbcut_bytes;
    size_t total;
};

// (the words of a cutoff lie behind the others: without one the layout is the one it was)
RsWs rs_layout(char* base, int N, int C, int B, int n_blocks, bool cut = false) {
    RsWs w;
    WsCarve k{base};
    const size_t n3 = (size_t)N * C * 3, bc = (size_t)B * C, kc = (size_t)n_blocks * C;
    w.x = k.take<float>(n3), w.v = k.take<float>(n3), w.g = k.take<float>(n3);
    w.s.h = k.take<float>(bc), w.s.al = k.take<float>(bc), w.s.mix = k.take<float>(bc), w.s.keep = k.take<float>(bc);
    w.s.gmax = k.take<float>(bc);
    w.s.npos = k.take<int>(bc), w.s.steps = k.take<int>(bc), w.s.status = k.take<int>(bc), w.s.downhill = k.take<int>(bc);
    w.part = k.take<double>(4 * kc);
    w.dpart = k.take<float>(kc);
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
struct RsInitArgs {
    int N, C, B;
    const int* atom_molptr;
    const float* start;
    float *x, *v;
    RsState s;
    float dt_start, alpha_start;
    int* n_running;
};

__global__ __launch_bounds__(256) void rs_init_kernel(RsInitArgs a) {
    __shared__ int cnt[256];
    const int t = threadIdx.x;
    const size_t gid = (size_t)blockIdx.x * 256 + t;
    if (gid < (size_t)a.N * a.C * 3) {
        a.x[gid] = a.start[gid];
        a.v[gid] = 0.f;
    }
    if (gid < (size_t)a.B * a.C) {
        const int b = (int)(gid / a.C);
        const bool some = nb_clamp(a.atom_molptr[b + 1], a.N) > nb_clamp(a.atom_molptr[b], a.N);
        a.s.h[gid] = a.dt_start, a.s.al[gid] = a.alpha_start, a.s.mix[gid] = 0.f, a.s.keep[gid] = 0.f, a.s.gmax[gid] = 0.f;
        a.s.npos[gid] = 0, a.s.steps[gid] = 0, a.s.downhill[gid] = 0;
        a.s.status[gid] = some ? RS_RUNNING : 0;      // a molecule without atoms never runs (and the finish writes nothing for it)
    }
    if (blockIdx.x == 0) {      // the count of running items: molecules with atoms, times C (integers: any order gives the same number)
        int n = 0;
        for (int b = t; b < a.B; b += 256) n += nb_clamp(a.atom_molptr[b + 1], a.N) > nb_clamp(a.atom_molptr[b], a.N) ? 1 : 0;
        cnt[t] = n;
        __syncthreads();
        if (t == 0) {
            long long sum = 0;
            for (int k = 0; k < 256; ++k) sum += cnt[k];
            a.n_running[0] = (int)(sum * a.C);
        }
    }
}

// ------------------------------------------------------------------------------------------------ force
struct RsForceArgs {
    RsForceIn f;             // the force of csrc/rs_force.h
    const float* v;
    float* g;
    double* part;
};

template <class Cut>
__device__ __forceinline__ void rs_force_body(const RsForceArgs& a, const Cut& cut) {
    __shared__ RsShared sh;
    rs_force(a.f, sh, cut, [&](const RsItem& r, const RsLane& w, V3 gi) {
        const int C = a.f.q.C, ni = r.ni;
        float pP = 0.f, pF = 0.f, pv = 0.f, pg = 0.f;
        if (w.owner) {
            const size_t off = ((size_t)w.i * C + w.c) * 3;
            a.g[off] = gi.x, a.g[off + 1] = gi.y, a.g[off + 2] = gi.z;
            const V3 vi = {a.v[off], a.v[off + 1], a.v[off + 2]};
            const float g2 = dot(gi, gi), gn = sqrtf(g2);
            pP = -dot(gi, vi);          // F = -g
            pF = g2;
            pv = dot(vi, vi);
            pg = gn <= FLT_MAX ? gn : INFINITY;      // (written so that a NaN counts as non-finite)
        }
        __syncthreads();
        if (w.owner) sh.red[0][w.l] = pP, sh.red[1][w.l] = pF, sh.red[2][w.l] = pv, sh.red[3][w.l] = pg;
        __syncthreads();
        if (w.owner && w.il == 0) {      // the block's partials of one conformation: over its atoms in ascending order, in double
            double sP = 0.0, sF = 0.0, sv = 0.0;
            float mg = 0.f;
            for (int k = 0; k < ni; ++k) {
                const int o = w.cl * ni + k;
                sP += (double)sh.red[0][o], sF += (double)sh.red[1][o], sv += (double)sh.red[2][o];
                mg = fmaxf(mg, sh.red[3][o]);
            }
            double* o = a.part + ((size_t)r.blk * C + w.c) * 4;
            o[0] = sP, o[1] = sF, o[2] = sv, o[3] = (double)mg;
        }
    });
}

__global__ __launch_bounds__(NB_NT) void rs_force_kernel(RsForceArgs a) { rs_force_body(a, NbNoCut{}); }

// (the rule looks only at the item's running conformations: a.f.status is the minimiser's, RS_RUNNING while an item runs)
__global__ __launch_bounds__(NB_NT) void rs_force_cut_kernel(RsForceArgs a, NbCutDev c) {
    __shared__ unsigned char near[NB_NT];
    rs_force_body(a, NbCut{c, near});
}

// ------------------------------------------------------------------------------------------------ decide
struct RsDecideArgs {
    grappa_relax_opts o;
    int C, n_blocks;
    const int* blk_ptr;
    const double* part;
    RsState s;
    int* n_running;      // NULL: not counted (the finish)
    int final;           // the finish: stop tests only, a running item ends with status 0
};

__global__ __launch_bounds__(RS_DNT) void rs_decide_kernel(RsDecideArgs a) {
    __shared__ double red[4][RS_DNT];
    const size_t item = blockIdx.x;
    if (a.s.status[item] != RS_RUNNING) return;
    const int C = a.C, t = threadIdx.x;
    const int b = (int)(item / (unsigned)C), c = (int)(item - (size_t)b * C);
    const int k0 = nb_clamp(a.blk_ptr[b], a.n_blocks), k1 = nb_clamp(a.blk_ptr[b + 1], a.n_blocks);
    double P = 0.0, F2 = 0.0, v2 = 0.0, gm = 0.0;
    for (int k = k0 + t; k < k1; k += RS_DNT) {      // thread t adds the blocks t, t + 64, .. ascending; the 64 rows are added in order
        const double* p = a.part + ((size_t)k * C + c) * 4;
        P += p[0], F2 += p[1], v2 += p[2];
        gm = fmax(gm, p[3]);
    }
    red[0][t] = P, red[1][t] = F2, red[2][t] = v2, red[3][t] = gm;
    __syncthreads();
    if (t != 0) return;
#pragma unroll 4
    for (int q = 1; q < RS_DNT; ++q) {
        P += red[0][q], F2 += red[1][q], v2 += red[2][q];
        gm = fmax(gm, red[3][q]);
    }
    const grappa_relax_opts& o = a.o;
    float gmf = (float)gm;
    const int steps = a.s.steps[item];
    int status = RS_RUNNING;
    if (!(gmf <= FLT_MAX)) {
        gmf = INFINITY;
        status = 2;
    } else if (gmf <= o.tolerance) {
        status = 1;
    } else if (steps >= o.max_steps || a.final) {
        status = 0;
    }
    if (status != RS_RUNNING) {
        a.s.gmax[item] = gmf;
        a.s.status[item] = status;
        if (a.n_running) atomicSub(a.n_running, 1);
        return;
    }
    // FIRE: mix the velocity towards the force (or stop it); the new time step
    const float Pf = (float)P, F2f = (float)F2, v2f = (float)v2;
    float h = a.s.h[item], al = a.s.al[item];
    int npos = a.s.npos[item];
    float mix, keep;
    const bool downhill = fire_decide(o, Pf, F2f, v2f, h, al, npos, mix, keep);
    a.s.h[item] = h, a.s.al[item] = al, a.s.mix[item] = mix, a.s.keep[item] = keep;
    a.s.npos[item] = npos, a.s.downhill[item] = downhill ? 1 : 0, a.s.steps[item] = steps + 1;
}

// ------------------------------------------------------------------------------------------------ vel, move
struct RsUpdArgs {
    RsGeom q;
    float *x, *v;
    const float* g;
    RsState s;
    float* dpart;
    float max_disp;
};

__global__ __launch_bounds__(NB_NT) void rs_vel_kernel(RsUpdArgs a) {
    __shared__ float red[NB_NT];
    RsItem r;
    if (!rs_item(a.q, r)) return;
    const int C = a.q.C, t = threadIdx.x, ni = r.ni;
    const bool in = t < ni * r.nc;
    const int cl = in ? t / ni : 0, il = in ? t - cl * ni : 0;
    const int c = r.c0 + cl;
    const size_t item = (size_t)r.mol * C + c;
    const bool on = in && a.s.status[item] == RS_RUNNING;
    float dm = 0.f;
    if (on) {
        const size_t off = ((size_t)(r.i0 + il) * C + c) * 3;
        const float h = a.s.h[item];
        const V3 gi = {a.g[off], a.g[off + 1], a.g[off + 2]};
        V3 vk = {0.f, 0.f, 0.f};                   // P <= 0: the velocity is dropped, whatever it held
        if (a.s.downhill[item]) {
            const V3 vi = {a.v[off], a.v[off + 1], a.v[off + 2]};
            vk = a.s.keep[item] * vi - a.s.mix[item] * gi;      // F = -g
        }
        vk = vk - h * gi;
        a.v[off] = vk.x, a.v[off + 1] = vk.y, a.v[off + 2] = vk.z;
        dm = h * sqrtf(dot(vk, vk));
    }
    red[t] = dm;
    __syncthreads();
    if (on && il == 0) {
        for (int k = 1; k < ni; ++k) dm = fmaxf(dm, red[cl * ni + k]);
        a.dpart[(size_t)r.blk * C + c] = dm;
    }
}

// the thread's (atom, conformation) of the item, t < ni * nc; CUT: the coordinates it leaves -> bxl[0..3) (not for a stopped conformation)
template <bool CUT>
__device__ __forceinline__ void rs_move_lane(const RsUpdArgs& a, const RsItem& r, int C, int t, int ni, const float* sdm, const int* run,
                                             float* bxl) {
    const int cl = t / ni, il = t - cl * ni;
    if (!run[cl]) return;
    const int c = r.c0 + cl;
    const float dm = sdm[cl], h = a.s.h[(size_t)r.mol * C + c];
    const float sc = dm > 0.f ? fminf(1.0f, a.max_disp / dm) : 1.0f;
    const float hs = sc * h;
    const size_t off = ((size_t)(r.i0 + il) * C + c) * 3;
    const V3 vk = {a.v[off], a.v[off + 1], a.v[off + 2]};
    const float xx = a.x[off] + hs * vk.x, xy = a.x[off + 1] + hs * vk.y, xz = a.x[off + 2] + hs * vk.z;
    a.x[off] = xx, a.x[off + 1] = xy, a.x[off + 2] = xz;
    a.v[off] = sc * vk.x, a.v[off + 1] = sc * vk.y, a.v[off + 2] = sc * vk.z;
    if constexpr (CUT) bxl[0] = xx, bxl[1] = xy, bxl[2] = xz;
}

// CUT: the item also writes the box of its own (block, conformations) at the coordinates it leaves (csrc/nb_cut.h): it is the box's only
// writer, the force launch after it the reader.  A stopped conformation keeps its box, as it keeps its x.  Only the uniform returns of
// rs_item and rs_running come before the barriers of nb_cut_box_write: the whole workgroup reaches them.  (a by value: through a reference
// the all-pairs instantiation's index arithmetic compiles to other instructions than rs_move_kernel had.)
template <bool CUT>
__device__ __forceinline__ void rs_move_body(const RsUpdArgs a, float4* box) {
    __shared__ float sdm[NB_CW];
    __shared__ int run[NB_CW];
    RsItem r;
    if (!rs_item(a.q, r)) return;
    const int C = a.q.C, t = threadIdx.x, ni = r.ni;
    if (!rs_running(r, C, a.s.status, run)) return;
    // the largest displacement of each running conformation over ALL blocks of the molecule (every workgroup of the molecule forms the
    // same maximum from the same partials): wavefront w takes the conformations w, w + 4, .., its lanes the blocks
    const int k0 = nb_clamp(a.q.blk_ptr[r.mol], a.q.n_blocks), k1 = nb_clamp(a.q.blk_ptr[r.mol + 1], a.q.n_blocks);
    const int wave = t / GRAPPA_WAVE, lane = t & (GRAPPA_WAVE - 1);
    for (int cc = wave; cc < r.nc; cc += RS_NW) {
        if (!run[cc]) continue;
        float m = 0.f;
        for (int k = k0 + lane; k < k1; k += GRAPPA_WAVE) m = fmaxf(m, a.dpart[(size_t)k * C + r.c0 + cc]);
#pragma unroll
        for (int o = GRAPPA_WAVE / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, GRAPPA_WAVE));
        if (lane == 0) sdm[cc] = m;
    }
    if constexpr (CUT) {
        __shared__ float bx[NB_NT * 3];
        __shared__ int keep[NB_CW];
        if (t < r.nc) keep[t] = !run[t];
        __syncthreads();
        if (t < ni * r.nc) rs_move_lane<true>(a, r, C, t, ni, sdm, run, bx + 3 * t);
        nb_cut_box_write(bx, keep, ni, r.nc, r.blk, C, r.c0, box);
    } else {
        __syncthreads();
        if (t < ni * r.nc) rs_move_lane<false>(a, r, C, t, ni, sdm, run, nullptr);
    }
}

__global__ __launch_bounds__(NB_NT) void rs_move_kernel(RsUpdArgs a) { rs_move_body<false>(a, nullptr); }
__global__ __launch_bounds__(NB_NT) void rs_move_cut_kernel(RsUpdArgs a, float4* box) { rs_move_body<true>(a, box); }

// ------------------------------------------------------------------------------------------------ finish
struct RsOutArgs {
    int N, C, B, has_nb;
    const int* atom_molptr;
    const float *x, *g, *terms;      // terms [6,B,C] in the workspace (rows 4, 5 only with has_nb)
    RsState s;
    float *xyz_out, *energy, *term_energy, *grad, *gmax;
    int *steps, *status;
};

__global__ __launch_bounds__(256) void rs_out_kernel(RsOutArgs a) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gid < (size_t)a.N * a.C * 3) {
        a.xyz_out[gid] = a.x[gid];
        if (a.grad) a.grad[gid] = a.g[gid];
    }
    const size_t bc = (size_t)a.B * a.C;
    if (gid < bc) {
        const int b = (int)(gid / a.C);
        if (nb_clamp(a.atom_molptr[b + 1], a.N) <= nb_clamp(a.atom_molptr[b], a.N)) return;      // a molecule without atoms writes nothing
        double tot = 0.0;
        for (int q = 0; q < 6; ++q) {
            const float e = (q < 4 || a.has_nb) ? a.terms[q * bc + gid] : 0.f;
            if (a.term_energy) a.term_energy[q * bc + gid] = e;
            tot += (double)e;
        }
        a.energy[gid] = (float)tot;
        a.gmax[gid] = a.s.gmax[gid];
        a.steps[gid] = a.s.steps[gid];
        a.status[gid] = a.s.status[gid];
    }
}

// ------------------------------------------------------------------------------------------------ implicit solvent (grappa_relax_steps_*_gb_f32)
// GB/SA (include/grappa_hip.h grappa_gb_desc) as a term of the minimised energy: the three passes of csrc/gb_pass.h under the
// stopped-conformation mask, behind the force launch, which runs AS IT IS -- so the kernels of a call without solvent are not touched by
// this section, and a call with it launches the very same decide, vel, move and force kernels.
//   step   : decide, vel, move, force (g = bonded + nonbonded and the partials of THAT gradient), born, pair (the gradient at fixed B ->
//            ggb), chain: its epilogue adds g + ggb + the chain sum in that order, writes g and rewrites the block's four partials from
//            the total gradient and the unchanged v.  7 launches.  init gains the same three launches behind its force launch.
//   hazards: born writes B, dBdI of its own (atom, conformation)s, pair reads B of every j and writes w and ggb of its own, chain reads w
//            of every j and writes g and the partials of its own block: every word has one writer per launch and is read only across a
//            launch boundary.  The force launch's partials are overwritten before the next decide reads them; decide stays the only
//            writer of the per-item state, and a non-finite total gradient reaches it as max |g_i| = inf: status 2 by the path it has.
//   energies: grappa_gb_obc_fwd_f32 itself at the held coordinates, in a workspace region of its own (steps_gb_terms_at of
//            csrc/rs_force.h), and one small launch that adds the eight terms in double in term order.
struct RsGb {
    const grappa_gb_desc* opts;
    GbK k;
};

struct RsGbWs {
    GbPassWs p;
    float* ggb;                          // [N,C,3]: the gradient at fixed B
    float *e_gb, *terms_gb;              // finish: [B,C], [2,B,C]
    char* fwd;                           // finish: the workspace of grappa_gb_obc_fwd_f32
    size_t fwd_bytes;
    size_t total;
};

// (the words of the solvent lie behind all others: `off` = the total of rs_layout)
RsGbWs rs_gb_layout(char* base, size_t off, int N, int C, int B, int n_blocks) {
    RsGbWs g;
    WsCarve k{base};
    k.off = off;
    g.p = gb_pass_ws(k, N, C);
    g.ggb = k.take<float>((size_t)N * C * 3);
    g.e_gb = k.take<float>((size_t)B * C), g.terms_gb = k.take<float>(2 * (size_t)B * C);
    g.fwd_bytes = grappa_gb_obc_workspace_bytes(N, C, n_blocks > 0 ? n_blocks : 1);
    g.fwd = k.take<char>(g.fwd_bytes);
    g.total = k.off;
    return g;
}

__global__ __launch_bounds__(NB_NT) void rs_gb_born_kernel(GbArgs a) {
    __shared__ GbShared sh;
    gb_born_body<true>(a, sh);
}

__global__ __launch_bounds__(NB_NT) void rs_gb_pair_kernel(GbArgs a) {
    __shared__ GbShared sh;
    gb_pair_body<true, false, true>(a, sh);
}

struct RsGbChainArgs {
    GbArgs gb;
    const float* v;
    float* g;
    double* part;
};

// (the partials: the text of rs_force_body's epilogue from `const V3 vi` on, word for word -- tests/test_host_relax_gb.py compares the two)
__global__ __launch_bounds__(NB_NT) void rs_gb_chain_kernel(RsGbChainArgs a) {
    __shared__ GbShared sh;
    gb_chain_body<true>(a.gb, sh, [&](const GbLane& w, float cx, float cy, float cz) {
        const RsItem& r = w.r;
        const int C = a.gb.q.C, ni = r.ni;
        float pP = 0.f, pF = 0.f, pv = 0.f, pg = 0.f;
        if (w.owner) {
            const size_t off = ((size_t)w.i * C + w.c) * 3;
            const float* d = a.gb.gdir;
            const V3 gi = {(a.g[off] + d[off]) + cx, (a.g[off + 1] + d[off + 1]) + cy, (a.g[off + 2] + d[off + 2]) + cz};
            a.g[off] = gi.x, a.g[off + 1] = gi.y, a.g[off + 2] = gi.z;
            const V3 vi = {a.v[off], a.v[off + 1], a.v[off + 2]};
            const float g2 = dot(gi, gi), gn = sqrtf(g2);
            pP = -dot(gi, vi);          // F = -g
            pF = g2;
            pv = dot(vi, vi);
            pg = gn <= FLT_MAX ? gn : INFINITY;      // (written so that a NaN counts as non-finite)
        }
        __syncthreads();
        if (w.owner) sh.red[0][w.l] = pP, sh.red[1][w.l] = pF, sh.red[2][w.l] = pv, sh.red[3][w.l] = pg;
        __syncthreads();
        if (w.owner && w.il == 0) {      // the block's partials of one conformation: over its atoms in ascending order, in double
            double sP = 0.0, sF = 0.0, sv = 0.0;
            float mg = 0.f;
            for (int k = 0; k < ni; ++k) {
                const int o = w.cl * ni + k;
                sP += (double)sh.red[0][o], sF += (double)sh.red[1][o], sv += (double)sh.red[2][o];
                mg = fmaxf(mg, sh.red[3][o]);
            }
            double* o = a.part + ((size_t)r.blk * C + w.c) * 4;
            o[0] = sP, o[1] = sF, o[2] = sv, o[3] = (double)mg;
        }
    });
}

// energy with the solvent's two terms, term_energy's rows 6 and 7 and esolv: the conditions of rs_out_kernel, which ran before it and
// left energy without them; the sum in ms_out_gb_kernel's order (csrc/dynamics_steps.hip)
__global__ __launch_bounds__(256) void rs_out_gb_kernel(RsOutArgs a, const float* terms_gb, float* esolv) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, bc = (size_t)a.B * a.C;
    if (gid >= bc) return;
    const int b = (int)(gid / (unsigned)a.C);
    if (nb_clamp(a.atom_molptr[b + 1], a.N) <= nb_clamp(a.atom_molptr[b], a.N)) return;
    const double es = (double)terms_gb[gid] + (double)terms_gb[bc + gid];
    double tot = 0.0;
    for (int q = 0; q < 6; ++q) tot += (double)((q < 4 || a.has_nb) ? a.terms[q * bc + gid] : 0.f);
    a.energy[gid] = (float)(tot + es);
    if (a.term_energy) a.term_energy[6 * bc + gid] = terms_gb[gid], a.term_energy[7 * bc + gid] = terms_gb[bc + gid];
    if (esolv) esolv[gid] = (float)es;
}

// the three solvent launches behind a force launch
void rs_launch_gb(hipStream_t st, const grappa_nb_desc* nb, const RsGb& gb, const RsGeom& q, const RsWs& w, const RsGbWs& gw, int n_items) {
    RsGbChainArgs c = {};
    c.gb.q = q, c.gb.x = w.x, c.gb.charge = nb->charge, c.gb.radius = gb.opts->radius, c.gb.scale = gb.opts->scale, c.gb.k = gb.k;
    c.gb.B = gw.p.B, c.gb.dBdI = gw.p.dBdI, c.gb.w = gw.p.w, c.gb.gdir = gw.ggb, c.gb.part = nullptr, c.gb.born = nullptr, c.gb.status = w.s.status;
    c.v = w.v, c.g = w.g, c.part = w.part;
    const dim3 grid((unsigned)n_items), block(NB_NT);
    GRAPPA_LAUNCH(rs_gb_born_kernel, grid, block, 0, st, c.gb);
    GRAPPA_LAUNCH(rs_gb_pair_kernel, grid, block, 0, st, c.gb);
    GRAPPA_LAUNCH(rs_gb_chain_kernel, grid, block, 0, st, c);
}

// ------------------------------------------------------------------------------------------------ host
// (the argument checks the three calls share: steps_seam_check of csrc/desc_check.h; GRAPPA_SEAM_EMPTY: nothing to do)

// (a cutoff as the three calls carry it: RsCut / rs_cut_make of csrc/rs_force.h; c == NULL: none)

void rs_launch_force(hipStream_t st, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const RsCut* c, const RsGeom& q, const RsWs& w,
                     int n_items) {
    RsForceArgs f;
    f.f = rs_force_in(mm, nb, q, w.x, w.s.status);
    f.v = w.v, f.g = w.g, f.part = w.part;
    if (c) {
        NbCutDev d = c->dev;
        d.box = w.box, d.er = w.er;
        GRAPPA_LAUNCH(rs_force_cut_kernel, dim3((unsigned)n_items), dim3(NB_NT), 0, st, f, d);
    } else {
        GRAPPA_LAUNCH(rs_force_kernel, dim3((unsigned)n_items), dim3(NB_NT), 0, st, f);
    }
}

// the three calls, with and without a cutoff (c == NULL: none) and an implicit solvent (gb == NULL: none, the launches as they were)
int rs_init(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const RsCut* c, const grappa_relax_opts* o, const int* table_dev,
            int n_items, int n_blocks, void* ws, size_t ws_bytes, int* n_running_dev, const RsGb* gb = nullptr) {
    const int rc = steps_seam_check(mm, nb, o && relax_opts_ok(o), table_dev, n_items, n_blocks, ws);
    if (rc != GRAPPA_OK) return rc < 0 ? rc : GRAPPA_OK;
    if (!n_running_dev) return GRAPPA_ERR_ARG;
    const RsWs w = rs_layout((char*)ws, mm->N, mm->C, mm->B, n_blocks, c != nullptr);
    RsGbWs gw = {};
    if (gb) gw = rs_gb_layout((char*)ws, w.total, mm->N, mm->C, mm->B, n_blocks);
    if (ws_bytes < (gb ? gw.total : w.total)) return GRAPPA_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    RsInitArgs a;
    a.N = mm->N, a.C = mm->C, a.B = mm->B;
    a.atom_molptr = mm->atom_molptr, a.start = mm->xyz;
    a.x = w.x, a.v = w.v, a.s = w.s;
    a.dt_start = o->dt_start, a.alpha_start = o->alpha_start;
    a.n_running = n_running_dev;
    const size_t n3 = (size_t)mm->N * mm->C * 3, bc = (size_t)mm->B * mm->C, n = n3 > bc ? n3 : bc;
    GRAPPA_LAUNCH(rs_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    const RsGeom q = rs_geom(mm, table_dev, n_blocks);
    if (c && n_items > 0) {
        const RsBoxArgs b = {q, w.x, nb->exc_ptr, nb->exc_atom, w.box, w.er};
        GRAPPA_LAUNCH(rs_box_kernel, dim3((unsigned)n_items), dim3(NB_NT), 0, st, b);
    }
    if (n_items > 0) rs_launch_force(st, mm, nb, c, q, w, n_items);
    if (gb && n_items > 0) rs_launch_gb(st, nb, *gb, q, w, gw, n_items);
    return grappa_launch_status();
}

int rs_run(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const RsCut* c, const grappa_relax_opts* o, const int* table_dev,
           int n_items, int n_blocks, void* ws, size_t ws_bytes, int n_steps, int* n_running_dev, const RsGb* gb = nullptr) {
    const int rc = steps_seam_check(mm, nb, o && relax_opts_ok(o), table_dev, n_items, n_blocks, ws);
    if (rc < 0) return rc;
    if (n_steps < 1) return GRAPPA_ERR_ARG;
    if (rc != GRAPPA_OK) return GRAPPA_OK;
    if (!n_running_dev) return GRAPPA_ERR_ARG;
    const RsWs w = rs_layout((char*)ws, mm->N, mm->C, mm->B, n_blocks, c != nullptr);
    RsGbWs gw = {};
    if (gb) gw = rs_gb_layout((char*)ws, w.total, mm->N, mm->C, mm->B, n_blocks);
    if (ws_bytes < (gb ? gw.total : w.total)) return GRAPPA_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const RsGeom q = rs_geom(mm, table_dev, n_blocks);
    RsDecideArgs dc;
    dc.o = *o;
    dc.C = mm->C, dc.n_blocks = n_blocks, dc.blk_ptr = q.blk_ptr, dc.part = w.part, dc.s = w.s;
    dc.n_running = n_running_dev, dc.final = 0;
    RsUpdArgs u;
    u.q = q, u.x = w.x, u.v = w.v, u.g = w.g, u.s = w.s, u.dpart = w.dpart, u.max_disp = o->max_disp;
    const unsigned items = (unsigned)n_items, bc = (unsigned)(mm->B * mm->C);
    for (int k = 0; k < n_steps; ++k) {
        GRAPPA_LAUNCH(rs_decide_kernel, dim3(bc), dim3(RS_DNT), 0, st, dc);
        if (n_items > 0) {
            GRAPPA_LAUNCH(rs_vel_kernel, dim3(items), dim3(NB_NT), 0, st, u);
            if (c) GRAPPA_LAUNCH(rs_move_cut_kernel, dim3(items), dim3(NB_NT), 0, st, u, w.box);
            else GRAPPA_LAUNCH(rs_move_kernel, dim3(items), dim3(NB_NT), 0, st, u);
            rs_launch_force(st, mm, nb, c, q, w, n_items);
            if (gb) rs_launch_gb(st, nb, *gb, q, w, gw, n_items);
        }
    }
    return grappa_launch_status();
}

int rs_finish(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const RsCut* c, const grappa_relax_opts* o,
              const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes, float* xyz_out, float* energy, float* term_energy,
              float* grad, float* gmax, int* steps, int* status, const RsGb* gb = nullptr, float* esolv = nullptr) {
    const int rc = steps_seam_check(mm, nb, o && relax_opts_ok(o), table_dev, n_items, n_blocks, ws);
    if (rc != GRAPPA_OK) return rc < 0 ? rc : GRAPPA_OK;
    if (!xyz_out || !energy || !gmax || !steps || !status) return GRAPPA_ERR_ARG;
    const RsWs w = rs_layout((char*)ws, mm->N, mm->C, mm->B, n_blocks, c != nullptr);
    RsGbWs gw = {};
    if (gb) gw = rs_gb_layout((char*)ws, w.total, mm->N, mm->C, mm->B, n_blocks);
    if (ws_bytes < (gb ? gw.total : w.total)) return GRAPPA_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const RsGeom q = rs_geom(mm, table_dev, n_blocks);
    const size_t bc = (size_t)mm->B * mm->C;
    RsDecideArgs dc;
    dc.o = *o;
    dc.C = mm->C, dc.n_blocks = n_blocks, dc.blk_ptr = q.blk_ptr, dc.part = w.part, dc.s = w.s;
    dc.n_running = nullptr, dc.final = 1;
    GRAPPA_LAUNCH(rs_decide_kernel, dim3((unsigned)bc), dim3(RS_DNT), 0, st, dc);
    // (steps_terms_at of csrc/rs_force.h at w.x, in the part of this workspace that the cut or the planned nonbonded call takes)
    const int erc = c ? steps_terms_at(stream, mm, nb, c->opts, table_dev, n_items, n_blocks, w.x, w.e_mm, w.e_nb, w.terms, w.nbcut, w.nbcut_bytes)
                      : steps_terms_at(stream, mm, nb, nullptr, table_dev, n_items, n_blocks, w.x, w.e_mm, w.e_nb, w.terms, w.nbpart,
                                       sizeof(double) * 2 * (size_t)n_blocks * (size_t)mm->C);
    if (erc != GRAPPA_OK) return erc;
    if (gb) {
        const int grc = steps_gb_terms_at(stream, mm, nb, gb->opts, table_dev, n_items, n_blocks, w.x, gw.e_gb, gw.terms_gb, gw.fwd, gw.fwd_bytes);
        if (grc != GRAPPA_OK) return grc;
    }
    RsOutArgs a;
    a.N = mm->N, a.C = mm->C, a.B = mm->B, a.has_nb = nb != nullptr;
    a.atom_molptr = mm->atom_molptr;
    a.x = w.x, a.g = w.g, a.terms = w.terms, a.s = w.s;
    a.xyz_out = xyz_out, a.energy = energy, a.term_energy = term_energy, a.grad = grad, a.gmax = gmax, a.steps = steps, a.status = status;
    const size_t n3 = (size_t)mm->N * mm->C * 3, n = n3 > bc ? n3 : bc;
    GRAPPA_LAUNCH(rs_out_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    if (gb) GRAPPA_LAUNCH(rs_out_gb_kernel, dim3((unsigned)((bc + 255) / 256)), dim3(256), 0, st, a, gw.terms_gb, esolv);
    return grappa_launch_status();
}

}  // namespace

extern "C" size_t grappa_relax_steps_workspace_bytes(int N, int C, int B, int n_blocks) {
    if (N <= 0 || C <= 0 || B <= 0 || n_blocks < 0) return 0;
    return rs_layout(nullptr, N, C, B, n_blocks).total;
}

extern "C" int grappa_relax_steps_init_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_relax_opts* o,
                                           const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes, int* n_running_dev) {
    return rs_init(stream, mm, nb, nullptr, o, table_dev, n_items, n_blocks, ws, ws_bytes, n_running_dev);
}

extern "C" int grappa_relax_steps_run_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_relax_opts* o,
                                          const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes, int n_steps,
                                          int* n_running_dev) {
    return rs_run(stream, mm, nb, nullptr, o, table_dev, n_items, n_blocks, ws, ws_bytes, n_steps, n_running_dev);
}

extern "C" int grappa_relax_steps_finish_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_relax_opts* o,
                                             const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes, float* xyz_out,
                                             float* energy, float* term_energy, float* grad, float* gmax, int* steps, int* status) {
    return rs_finish(stream, mm, nb, nullptr, o, table_dev, n_items, n_blocks, ws, ws_bytes, xyz_out, energy, term_energy, grad, gmax, steps,
                     status);
}

// with a cutoff: cut == NULL is the call above; bad options in cut, or a cut without nb, are refused before anything else is looked at
extern "C" size_t grappa_relax_steps_cut_workspace_bytes(int N, int C, int B, int n_blocks) {
    if (N <= 0 || C <= 0 || B <= 0 || n_blocks < 0) return 0;
    return rs_layout(nullptr, N, C, B, n_blocks, true).total;
}

extern "C" int grappa_relax_steps_init_cut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                               const grappa_relax_opts* o, const int* table_dev, int n_items, int n_blocks, void* ws,
                                               size_t ws_bytes, int* n_running_dev) {
    RsCut c;
    if (cut && !rs_cut_make(cut, nb, c)) return GRAPPA_ERR_ARG;
    return rs_init(stream, mm, nb, cut ? &c : nullptr, o, table_dev, n_items, n_blocks, ws, ws_bytes, n_running_dev);
}

extern "C" int grappa_relax_steps_run_cut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                              const grappa_relax_opts* o, const int* table_dev, int n_items, int n_blocks, void* ws,
                                              size_t ws_bytes, int n_steps, int* n_running_dev) {
    RsCut c;
    if (cut && !rs_cut_make(cut, nb, c)) return GRAPPA_ERR_ARG;
    return rs_run(stream, mm, nb, cut ? &c : nullptr, o, table_dev, n_items, n_blocks, ws, ws_bytes, n_steps, n_running_dev);
}

extern "C" int grappa_relax_steps_finish_cut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                                 const grappa_relax_opts* o, const int* table_dev, int n_items, int n_blocks, void* ws,
                                                 size_t ws_bytes, float* xyz_out, float* energy, float* term_energy, float* grad, float* gmax,
                                                 int* steps, int* status) {
    RsCut c;
    if (cut && !rs_cut_make(cut, nb, c)) return GRAPPA_ERR_ARG;
    return rs_finish(stream, mm, nb, cut ? &c : nullptr, o, table_dev, n_items, n_blocks, ws, ws_bytes, xyz_out, energy, term_energy, grad,
                     gmax, steps, status);
}

// with the GB/SA implicit solvent: gb == NULL is the call above (the _cut_ one with a cut, else the plain one), with its launches and
// its bits.  A cutoff together with the solvent, a solvent without nb or charges, refused options or NULL tables: GRAPPA_ERR_ARG before
// anything else is looked at.
namespace {
// GRAPPA_OK: a solvent to run with (g filled); 1: none, forward; < 0: refused
int rs_gb_check(const grappa_gb_desc* gb, const grappa_nb_desc* nb, const grappa_nb_cut* cut, RsGb& g) {
    if (!gb) return 1;
    if (cut || !nb || !nb->charge || !gb->radius || !gb->scale || !gb_consts(gb, g.k)) return GRAPPA_ERR_ARG;
    g.opts = gb;
    return GRAPPA_OK;
}
}  // namespace

extern "C" size_t grappa_relax_steps_gb_workspace_bytes(int N, int C, int B, int n_blocks) {
    if (N <= 0 || C <= 0 || B <= 0 || n_blocks < 0) return 0;
    return rs_gb_layout(nullptr, rs_layout(nullptr, N, C, B, n_blocks).total, N, C, B, n_blocks).total;
}

extern "C" int grappa_relax_steps_init_gb_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                              const grappa_gb_desc* gb, const grappa_relax_opts* o, const int* table_dev, int n_items,
                                              int n_blocks, void* ws, size_t ws_bytes, int* n_running_dev) {
    RsGb g;
    const int gc = rs_gb_check(gb, nb, cut, g);
    if (gc < 0) return gc;
    if (gc == 1) {
        if (cut) return grappa_relax_steps_init_cut_f32(stream, mm, nb, cut, o, table_dev, n_items, n_blocks, ws, ws_bytes, n_running_dev);
        return grappa_relax_steps_init_f32(stream, mm, nb, o, table_dev, n_items, n_blocks, ws, ws_bytes, n_running_dev);
    }
    return rs_init(stream, mm, nb, nullptr, o, table_dev, n_items, n_blocks, ws, ws_bytes, n_running_dev, &g);
}

extern "C" int grappa_relax_steps_run_gb_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                             const grappa_gb_desc* gb, const grappa_relax_opts* o, const int* table_dev, int n_items,
                                             int n_blocks, void* ws, size_t ws_bytes, int n_steps, int* n_running_dev) {
    RsGb g;
    const int gc = rs_gb_check(gb, nb, cut, g);
    if (gc < 0) return gc;
    if (gc == 1) {
        if (cut) return grappa_relax_steps_run_cut_f32(stream, mm, nb, cut, o, table_dev, n_items, n_blocks, ws, ws_bytes, n_steps, n_running_dev);
        return grappa_relax_steps_run_f32(stream, mm, nb, o, table_dev, n_items, n_blocks, ws, ws_bytes, n_steps, n_running_dev);
    }
    return rs_run(stream, mm, nb, nullptr, o, table_dev, n_items, n_blocks, ws, ws_bytes, n_steps, n_running_dev, &g);
}

extern "C" int grappa_relax_steps_finish_gb_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                                const grappa_gb_desc* gb, const grappa_relax_opts* o, const int* table_dev, int n_items,
                                                int n_blocks, void* ws, size_t ws_bytes, float* xyz_out, float* energy, float* term_energy,
                                                float* grad, float* gmax, int* steps, int* status, float* esolv) {
    RsGb g;
    const int gc = rs_gb_check(gb, nb, cut, g);
    if (gc < 0) return gc;
    if (gc == 1) {
        if (cut)
            return grappa_relax_steps_finish_cut_f32(stream, mm, nb, cut, o, table_dev, n_items, n_blocks, ws, ws_bytes, xyz_out, energy,
                                                     term_energy, grad, gmax, steps, status);
        return grappa_relax_steps_finish_f32(stream, mm, nb, o, table_dev, n_items, n_blocks, ws, ws_bytes, xyz_out, energy, term_energy, grad,
                                             gmax, steps, status);
    }
    return rs_finish(stream, mm, nb, nullptr, o, table_dev, n_items, n_blocks, ws, ws_bytes, xyz_out, energy, term_energy, grad, gmax, steps,
                     status, &g, esolv);
}
