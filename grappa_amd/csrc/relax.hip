// Fused FIRE minimiser under the full MM force field (bonded terms of csrc/mm_energy.hip + Lennard-Jones / Coulomb of
// csrc/nonbonded.hip), fp32, xyz[N,C,3] (include/grappa_hip.h grappa_relax_fire_f32).
//   item   : one workgroup of 256 threads per (molecule, conformation); it loads the molecule once, runs the whole minimisation and
//            writes its results.  Workgroups never talk to each other: an item's bits depend on its own input only.
//   LDS    : x, y, z, q per atom (float4), sigma / 2 and sqrt(eps) per atom (float2), the partial gradients of one step, and a few
//            words for the reductions: 18.1 KB at any molecule size up to RX_MAX atoms.  Velocities and gradients stay in the registers of
//            the atom's owner (thread a % 256).
//   step   : a thread owns one (atom, slice).  Slice s of JS takes the atom's incidences s, s + JS, .. (the gather of
//            mm_gradient_kernel: coefficient times d(internal coordinate)/dx in closed form) and the j atoms s, s + JS, .. ascending
//            (the scheme of nb_pairs_kernel: the atom's sorted exception list is walked in step with j, an exception replaces the pair,
//            an exclusion or j == i is skipped); the owner then adds the slices in slice order.  No Newton's third law, no atomics.
//            P = F.v, |F|^2, |v|^2, max |g_i| and max |d_i| are reduced in a fixed order (butterfly inside a wavefront, the four
//            wavefronts in order); every thread holds the same values, so the branches of FIRE are uniform.  Four barriers per step.
//   tables : the molecule's tuple tables (idx, k, eq, inc_code) and exception lists are read from global memory (L2) in every step.
//   end    : the six energy terms at the final coordinates, thread partials added in double in thread order.
//   shared : the item's prologue, the gradient of a step and the closing energy are csrc/rx_force.h (with csrc/dynamics.hip); FIRE's
//            decision is csrc/fire.h (with csrc/relax_steps.hip); the checks of the descriptors and options are csrc/desc_check.h.
// The loop runs max_steps iterations at the most (<= GRAPPA_STEP_CAP): the kernel always terminates.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"
#include "desc_check.h"
#include "fire.h"
#include "rx_force.h"

namespace {

struct RxArgs {
    grappa_mm_desc mm;
    grappa_nb_desc nb;
    int has_nb;
    grappa_relax_opts o;
    float *xyz_out, *energy, *term_energy, *grad, *gmax;
    int *steps, *status;
};

__global__ __launch_bounds__(RX_NT) void relax_fire_kernel(RxArgs a) {
    __shared__ RxShared sh;
    const grappa_mm_desc& d = a.mm;
    const grappa_relax_opts& o = a.o;
    const int C = d.C, t = threadIdx.x;
    RxItem w;
    if (!rx_begin(d, a.nb, a.has_nb, a.status, sh, w)) return;
    const int b = w.b, c = w.c, m0 = w.m0, n = w.n;
    __syncthreads();

    V3 v[RX_APT], g[RX_APT];
#pragma unroll
    for (int k = 0; k < RX_APT; ++k) v[k] = {0.f, 0.f, 0.f}, g[k] = {0.f, 0.f, 0.f};
    float h = o.dt_start, al = o.alpha_start, gm = 0.f;
    int npos = 0, steps = 0, status = 0;
    for (;;) {
        // ---- the gradient of the current coordinates; max |g_i|, a flag for a non-finite gradient, P = F.v, |F|^2, |v|^2
        // (the sums stay in a loop of their own: formed inside rx_gradient's pass they come out with other bits)
        rx_gradient(d, a.nb, a.has_nb, sh, w, g, [](int, V3) {});
        float bad = 0.f, P = 0.f, F2 = 0.f, v2 = 0.f;
        gm = 0.f;
#pragma unroll
        for (int k = 0; k < RX_APT; ++k) {
            if (t + k * RX_NT < n) {
                const float g2 = dot(g[k], g[k]), gn = sqrtf(g2);
                gm = fmaxf(gm, gn);
                if (!(gn <= FLT_MAX)) bad = 1.f;
                P -= dot(g[k], v[k]);
                F2 += g2;
                v2 += dot(v[k], v[k]);
            }
        }
        rx_reduce(gm, bad, P, F2, v2, sh.wred);
        if (bad != 0.f) {
            gm = INFINITY;
            status = 2;
            break;
        }
        if (gm <= o.tolerance) {
            status = 1;
            break;
        }
        if (steps >= o.max_steps) break;
        // ---- FIRE: mix the velocity towards the force (or stop it), semi-implicit Euler, displacement cap
        float mix, keep;
        const bool downhill = fire_decide(o, P, F2, v2, h, al, npos, mix, keep);
        float dm = 0.f;
#pragma unroll
        for (int k = 0; k < RX_APT; ++k) {
            if (t + k * RX_NT < n) {
                V3 vk = {0.f, 0.f, 0.f};                   // P <= 0: the velocity is dropped, whatever it held
                if (downhill) vk = keep * v[k] - mix * g[k];      // F = -g
                vk = vk - h * g[k];
                v[k] = vk;
                dm = fmaxf(dm, h * sqrtf(dot(vk, vk)));
            }
        }
        dm = rx_reduce_max(dm, sh.wmax);
        const float sc = dm > 0.f ? fminf(1.0f, o.max_disp / dm) : 1.0f;
#pragma unroll
        for (int k = 0; k < RX_APT; ++k) {
            const int il = t + k * RX_NT;
            if (il < n) {
                const float hs = sc * h;
                float4 x = sh.xs[il];
                x.x += hs * v[k].x, x.y += hs * v[k].y, x.z += hs * v[k].z;
                sh.xs[il] = x;
                v[k] = sc * v[k];
            }
        }
        ++steps;
        __syncthreads();
    }

    // ---- results: the coordinates held, the gradient there, and the energy terms (thread partials, added in double in thread order)
#pragma unroll
    for (int k = 0; k < RX_APT; ++k) {
        const int il = t + k * RX_NT;
        if (il < n) {
            const size_t off = ((size_t)(m0 + il) * C + c) * 3;
            const float4 x = sh.xs[il];
            a.xyz_out[off] = x.x, a.xyz_out[off + 1] = x.y, a.xyz_out[off + 2] = x.z;
            if (a.grad) a.grad[off] = g[k].x, a.grad[off + 1] = g[k].y, a.grad[off + 2] = g[k].z;
        }
    }
    // (sh.part is free: its last readers passed the barrier of the reduction that ended the loop)
    const double tot = rx_energies(d, a.nb, a.has_nb, sh, w);
    if (t < 6 && a.term_energy) a.term_energy[((size_t)t * d.B + b) * C + c] = (float)sh.esum[t];
    if (t == 0) {
        a.energy[w.item] = (float)tot;
        a.gmax[w.item] = gm;
        a.steps[w.item] = steps;
        a.status[w.item] = status;
    }
}

}  // namespace

extern "C" int grappa_relax_max_atoms(void) { return RX_MAX; }

extern "C" int grappa_relax_fire_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_relax_opts* o, float* xyz_out,
                                     float* energy, float* term_energy, float* grad, float* gmax, int* steps, int* status) {
    if (!mm || !o || mm->N < 0 || mm->C < 0 || mm->B < 0) return GRAPPA_ERR_ARG;
    if (nb && (nb->N != mm->N || nb->C != mm->C || nb->B != mm->B)) return GRAPPA_ERR_ARG;
    if (!relax_opts_ok(o)) return GRAPPA_ERR_ARG;
    if (mm->N == 0 || mm->C == 0 || mm->B == 0) return GRAPPA_OK;
    if (!mm->xyz || !mm->atom_molptr || !mm->inc_ptr || !xyz_out || !energy || !gmax || !steps || !status) return GRAPPA_ERR_ARG;
    if (!mm_desc_tables_ok(mm, true) || (nb && !nb_desc_tables_ok(nb))) return GRAPPA_ERR_ARG;
    if ((long long)mm->B * mm->C > INT_MAX) return GRAPPA_ERR_ARG;
    RxArgs a;
    a.mm = *mm;
    a.has_nb = nb != nullptr;
    if (nb) a.nb = *nb; else a.nb = grappa_nb_desc{};
    a.o = *o;
    a.xyz_out = xyz_out, a.energy = energy, a.term_energy = term_energy, a.grad = grad, a.gmax = gmax;
    a.steps = steps, a.status = status;
    GRAPPA_LAUNCH(relax_fire_kernel, dim3((unsigned)(mm->B * mm->C)), dim3(RX_NT), 0, reinterpret_cast<hipStream_t>(stream), a);
    return grappa_launch_status();
}
