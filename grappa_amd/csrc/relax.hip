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
// The loop runs max_steps iterations at the most (<= RX_STEP_CAP): the kernel always terminates.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"
#include "mm_geom.h"
#include "nb_pair.h"
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
    const int b = (int)(blockIdx.x / (unsigned)C), c = (int)(blockIdx.x - (unsigned)b * (unsigned)C);
    const size_t item = (size_t)b * C + c;
    const int m0 = rx_clamp(d.atom_molptr[b], d.N), m1 = rx_clamp(d.atom_molptr[b + 1], d.N);
    const int n = m1 - m0;
    if (n <= 0) return;
    if (n > RX_MAX) {          // above the size limit: status 3 and nothing else
        if (t == 0) a.status[item] = 3;
        return;
    }
    for (int il = t; il < n; il += RX_NT) {
        const float* p = d.xyz + ((size_t)(m0 + il) * C + c) * 3;
        sh.xs[il] = make_float4(p[0], p[1], p[2], a.has_nb ? a.nb.charge[m0 + il] : 0.f);
        sh.ps[il] = a.has_nb ? make_float2(0.5f * a.nb.sigma[m0 + il], sqrtf(a.nb.epsilon[m0 + il])) : make_float2(0.f, 0.f);
    }
    // the thread's (atom, slice): up to 256 atoms one unit per thread in JS slices, above that one slice and RX_APT atoms per thread
    const int JS = n > RX_NT ? 1 : (RX_NT / n < RX_JS ? RX_NT / n : RX_JS);
    const int s = n > RX_NT ? 0 : t / n;
    const int il0 = t - s * n;
    const bool active = s < JS;
    __syncthreads();

    V3 v[RX_APT], g[RX_APT];
#pragma unroll
    for (int k = 0; k < RX_APT; ++k) v[k] = {0.f, 0.f, 0.f}, g[k] = {0.f, 0.f, 0.f};
    float h = o.dt_start, al = o.alpha_start, gm = 0.f;
    int npos = 0, steps = 0, status = 0;
    for (;;) {
        // ---- partial gradients of the current coordinates
        if (active)
            for (int il = il0; il < n; il += RX_NT) {
                V3 p = rx_bonded(d, sh, m0 + il, s, JS, m0, n);
                if (a.has_nb) {
                    float elj = 0.f, ec = 0.f;
                    rx_pairs(a.nb, sh, il, s, JS, m0, n, elj, ec, p.x, p.y, p.z);
                }
                const int u = s * n + il;
                sh.part[u] = p.x, sh.part[RX_MAX + u] = p.y, sh.part[2 * RX_MAX + u] = p.z;
            }
        __syncthreads();
        // ---- the owner adds the slices in slice order; max |g_i|, a flag for a non-finite gradient, P = F.v, |F|^2, |v|^2
        float bad = 0.f, P = 0.f, F2 = 0.f, v2 = 0.f;
        gm = 0.f;
#pragma unroll
        for (int k = 0; k < RX_APT; ++k) {
            const int il = t + k * RX_NT;
            if (il < n) {
                V3 gi = {sh.part[il], sh.part[RX_MAX + il], sh.part[2 * RX_MAX + il]};
                for (int q = 1; q < JS; ++q) {
                    const int u = q * n + il;
                    gi.x += sh.part[u], gi.y += sh.part[RX_MAX + u], gi.z += sh.part[2 * RX_MAX + u];
                }
                g[k] = gi;
                const float g2 = dot(gi, gi), gn = sqrtf(g2);
                gm = fmaxf(gm, gn);
                if (!(gn <= FLT_MAX)) bad = 1.f;
                P -= dot(gi, v[k]);
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
        const bool downhill = P > 0.f;
        float mix = 0.f, keep = 0.f;
        if (downhill) {
            mix = al * (sqrtf(v2) / sqrtf(F2));
            keep = 1.0f - al;
            if (npos >= o.n_min) {
                h = fminf(h * o.f_inc, o.dt_max);
                al = al * o.f_alpha;
            }
            ++npos;
        } else {
            h = h * o.f_dec;
            al = o.alpha_start;
            npos = 0;
        }
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
    float e[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int tt = d.mol_ptr[0][b] + t; tt < d.mol_ptr[0][b + 1]; tt += RX_NT) {
        V3 u;
        const float dx = bond_geom(rx_ld(sh, d.idx[0][2 * tt], m0, n), rx_ld(sh, d.idx[0][2 * tt + 1], m0, n), u) - d.eq[0][tt];
        e[0] += 0.5f * d.k[0][tt] * dx * dx;
    }
    for (int tt = d.mol_ptr[1][b] + t; tt < d.mol_ptr[1][b + 1]; tt += RX_NT) {
        V3 e0, e2;
        const float dx = angle_geom(rx_ld(sh, d.idx[1][3 * tt], m0, n), rx_ld(sh, d.idx[1][3 * tt + 1], m0, n),
                                    rx_ld(sh, d.idx[1][3 * tt + 2], m0, n), e0, e2) - d.eq[1][tt];
        e[1] += 0.5f * d.k[1][tt] * dx * dx;
    }
    for (int l = 2; l < 4; ++l)
        for (int tt = d.mol_ptr[l][b] + t; tt < d.mol_ptr[l][b + 1]; tt += RX_NT) {
            V3 d0, d1, d2, d3;
            const int* id = d.idx[l] + 4 * (size_t)tt;
            const float phi = dihedral_geom(rx_ld(sh, id[0], m0, n), rx_ld(sh, id[1], m0, n), rx_ld(sh, id[2], m0, n), rx_ld(sh, id[3], m0, n),
                                            d0, d1, d2, d3);
            e[l] += torsion_energy(d.k[l] + (size_t)tt * d.n_per[l], d.n_per[l], phi, d.offset_torsion);
        }
    if (a.has_nb && active)
        for (int il = il0; il < n; il += RX_NT) {
            float gx = 0.f, gy = 0.f, gz = 0.f;
            rx_pairs(a.nb, sh, il, s, JS, m0, n, e[4], e[5], gx, gy, gz);
        }
    // (sh.part is free: its last readers passed the barrier of the reduction that ended the loop)
#pragma unroll
    for (int q = 0; q < 6; ++q) sh.part[q * RX_NT + t] = e[q];
    __syncthreads();
    if (t < 6) {
        double sum = 0.0;
        for (int k = 0; k < RX_NT; ++k) sum += (double)sh.part[t * RX_NT + k];
        sh.esum[t] = t < 4 ? sum : 0.5 * sum;          // every pair was counted from both of its atoms
    }
    __syncthreads();
    if (t < 6 && a.term_energy) a.term_energy[((size_t)t * d.B + b) * C + c] = (float)sh.esum[t];
    if (t == 0) {
        double tot = 0.0;
        for (int q = 0; q < 6; ++q) tot += sh.esum[q];
        a.energy[item] = (float)tot;
        a.gmax[item] = gm;
        a.steps[item] = steps;
        a.status[item] = status;
    }
}

}  // namespace

extern "C" int grappa_relax_max_atoms(void) { return RX_MAX; }

extern "C" int grappa_relax_fire_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_relax_opts* o, float* xyz_out,
                                     float* energy, float* term_energy, float* grad, float* gmax, int* steps, int* status) {
    if (!mm || !o || mm->N < 0 || mm->C < 0 || mm->B < 0) return GRAPPA_ERR_ARG;
    if (nb && (nb->N != mm->N || nb->C != mm->C || nb->B != mm->B)) return GRAPPA_ERR_ARG;
    // (comparisons written so that a NaN is refused)
    if (!(o->tolerance >= 0.f) || o->max_steps < 0 || o->max_steps > RX_STEP_CAP || !(o->dt_start > 0.f) || !(o->dt_max > 0.f) ||
        !(o->max_disp > 0.f) || o->n_min < 0 || !(o->f_inc > 0.f) || !(o->f_dec > 0.f) || !(o->f_alpha > 0.f) ||
        !(o->alpha_start >= 0.f && o->alpha_start <= 1.f))
        return GRAPPA_ERR_ARG;
    if (!(o->dt_start <= FLT_MAX && o->dt_max <= FLT_MAX && o->max_disp <= FLT_MAX && o->f_inc <= FLT_MAX && o->f_dec <= FLT_MAX &&
          o->f_alpha <= FLT_MAX && o->tolerance <= FLT_MAX))
        return GRAPPA_ERR_ARG;
    if (mm->N == 0 || mm->C == 0 || mm->B == 0) return GRAPPA_OK;
    if (!mm->xyz || !mm->atom_molptr || !mm->inc_ptr || !xyz_out || !energy || !gmax || !steps || !status) return GRAPPA_ERR_ARG;
    long long tuples = 0;
    for (int l = 0; l < 4; ++l) {
        if (mm->T[l] < 0 || mm->T[l] >= (1 << 27) || !mm->mol_ptr[l]) return GRAPPA_ERR_ARG;
        if (mm->T[l] > 0 && (!mm->idx[l] || !mm->k[l])) return GRAPPA_ERR_ARG;
        if (l < 2 && mm->T[l] > 0 && !mm->eq[l]) return GRAPPA_ERR_ARG;
        if (l >= 2 && (mm->n_per[l] < 1 || mm->n_per[l] > 8)) return GRAPPA_ERR_ARG;
        tuples += mm->T[l];
    }
    if (tuples > 0 && !mm->inc_code) return GRAPPA_ERR_ARG;
    if (nb && (!nb->charge || !nb->sigma || !nb->epsilon || !nb->exc_ptr || !nb->exc_atom || !nb->exc_qq || !nb->exc_sigma || !nb->exc_eps))
        return GRAPPA_ERR_ARG;
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
