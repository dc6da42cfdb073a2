// Fused FIRE minimiser under the full MM force field (bonded terms of csrc/mm_energy.hip + Lennard-Jones / Coulomb of
// csrc/nonbonded.hip), fp32, xyz[N,C,3], free (include/grappa_hip.h grappa_relax_fire_f32) or with restraints
// (grappa_relax_fire_restr_f32).  ONE kernel text, fire_kernel<RESTR, ..>, with two instantiations: RESTR = false compiles to the loop
// alone, RESTR = true adds what is said under `Restraints` below, under `if constexpr (RESTR)`, and nothing else.
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
// Restraints (the places marked `restraints` in the kernel): the objective is E_ff + E_r,
//   E_r = sum_r k_r (1 - cos(phi_r - target_r,c)) + sum_i 0.5 pos_k_i |x_i - start_i|^2,
// with frozen atoms.  What a relaxed torsion scan needs: the grid points are the conformations of one molecule, one workgroup each.
//   tables : the item's restraint rows (at most 16 x {4 atoms, k, target}) are loaded into a small LDS block in the prologue (19.5 KB
//            with it); an owner keeps its atoms' frozen flag, tether constant and start coordinates in registers.
//   step   : rx_gradient hands the owner g = grad E_ff.  The owner then walks the item's rows in ascending r and, for a row that names
//            its atom, forms the dihedral from sh.xs (dihedral_geom) and adds k sin(phi - target) dphi/dx; then the tether
//            pos_k (x - start); a frozen atom's gradient is replaced by 0 before anything reads it, and its coordinates are never
//            written.  One fixed order per atom, nothing shared: same input, same bits.  sh.xs is read between the barrier that ends a
//            step and the barrier of the reduction, where nobody writes it: still four barriers per step.
//   end    : the six energy terms are the force field's only; E_r at the same coordinates goes through rx_energies' `extra` sum
//            (thread r: row r; an owner: its atoms' tethers), added in double in thread order.
//   vetting: the tables are device memory, so the kernel vets them before it writes anything (status 5): atoms in range and distinct,
//            k finite and >= 0, the conformation's targets finite, pos_k finite and >= 0, at most 16 rows.
// The loop runs max_steps iterations at the most (<= GRAPPA_STEP_CAP): the kernel always terminates.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"
#include "desc_check.h"
#include "fire.h"
#include "rx_force.h"

namespace {

constexpr int RR_MAX = GRAPPA_RELAX_MAX_DIHEDRALS;

struct RxArgs {
    grappa_mm_desc mm;
    grappa_nb_desc nb;
    int has_nb;
    grappa_relax_opts o;
    float *xyz_out, *energy, *term_energy, *grad, *gmax;
    int *steps, *status;
};

struct RrArgs {
    grappa_mm_desc mm;
    grappa_nb_desc nb;
    int has_nb;
    grappa_relax_opts o;
    const int *frozen, *dih_molptr, *dih_atoms;
    const float *pos_k, *dih_k, *dih_target;
    int R;
    float *xyz_out, *energy, *term_energy, *grad, *gmax;
    int *steps, *status;
    float *restraint_energy, *dih_phi;
};

__device__ __forceinline__ V3 rr_xyz(const RxShared& sh, int il) {
    const float4 p = sh.xs[il];
    return {p.x, p.y, p.z};
}

// ---- restraints: the LDS block of the item's rows (NoRestr: the empty one of fire_kernel<false, ..>).  In the kernel they act in the
// five places marked `restraints`, each under `if constexpr (RESTR)`; the owner's frozen flags, tether constants and start
// coordinates (frz, pk, x0) are registers of the kernel.  (Written out in the kernel's text and not as functions or a policy type that
// take those arrays: both forms were compiled, and either moves the restrained instantiation's loop or costs it scratch)
struct RrShared {
    int at[RR_MAX][4];           // atoms within the molecule
    float k[RR_MAX], tg[RR_MAX];
    float epart[RX_NT];          // thread partials of E_r
    double esum;
};
struct NoRestr {};

// row r of the item at the coordinates held: phi and its four derivatives
__device__ __forceinline__ float rr_dihedral(const RxShared& sh, const RrShared& rs, int r, V3& d0, V3& d1, V3& d2, V3& d3) {
    return dihedral_geom(rr_xyz(sh, rs.at[r][0]), rr_xyz(sh, rs.at[r][1]), rr_xyz(sh, rs.at[r][2]), rr_xyz(sh, rs.at[r][3]), d0, d1, d2, d3);
}

// RESTR = false: Args = RxArgs, RS = NoRestr; RESTR = true: Args = RrArgs, RS = RrShared
template <bool RESTR, class Args, class RS>
__global__ __launch_bounds__(RX_NT) void fire_kernel(Args a) {
    __shared__ RxShared sh;
    __shared__ RS rs;
    const grappa_mm_desc& d = a.mm;
    const grappa_relax_opts& o = a.o;
    const int C = d.C, t = threadIdx.x;
    RxItem w;
    if (!rx_begin(d, a.nb, a.has_nb, a.status, sh, w)) return;
    const int b = w.b, c = w.c, m0 = w.m0, n = w.n;

    int k0 = 0, nr = 0;
    bool frz[RX_APT];
    float pk[RX_APT];
    // ---- restraints, vetting: the item's rows k0 .. k0 + nr and the owner's flags and tether constants are loaded and vetted before
    // anything is written: status 5 and nothing else
    if constexpr (RESTR) {
        k0 = a.R > 0 ? rx_clamp(a.dih_molptr[b], a.R) : 0;
        const int k1 = a.R > 0 ? rx_clamp(a.dih_molptr[b + 1], a.R) : 0;
        nr = k1 - k0;
        float invalid = (nr < 0 || nr > RR_MAX) ? 1.f : 0.f;
        if (invalid == 0.f && t < nr) {
            const int* p = a.dih_atoms + 4 * (size_t)(k0 + t);
            const int i0 = p[0], i1 = p[1], i2 = p[2], i3 = p[3];
            const float kr = a.dih_k[k0 + t], tg = a.dih_target[(size_t)(k0 + t) * C + c];
            if ((unsigned)i0 >= (unsigned)n || (unsigned)i1 >= (unsigned)n || (unsigned)i2 >= (unsigned)n || (unsigned)i3 >= (unsigned)n) invalid = 1.f;
            if (i0 == i1 || i0 == i2 || i0 == i3 || i1 == i2 || i1 == i3 || i2 == i3) invalid = 1.f;
            if (!(kr >= 0.f && kr <= FLT_MAX) || !(fabsf(tg) <= FLT_MAX)) invalid = 1.f;          // (a NaN is refused)
            rs.at[t][0] = i0, rs.at[t][1] = i1, rs.at[t][2] = i2, rs.at[t][3] = i3;
            rs.k[t] = kr, rs.tg[t] = tg;
        }
#pragma unroll
        for (int k = 0; k < RX_APT; ++k) {
            const int il = t + k * RX_NT;
            frz[k] = false, pk[k] = 0.f;
            if (il < n) {
                if (a.frozen) frz[k] = a.frozen[m0 + il] != 0;
                if (a.pos_k) pk[k] = a.pos_k[m0 + il];
                if (!(pk[k] >= 0.f && pk[k] <= FLT_MAX)) invalid = 1.f;
            }
        }
        if (rx_reduce_max(invalid, sh.wmax) != 0.f) {          // (its barrier also publishes sh.xs and the rows)
            if (t == 0) a.status[w.item] = 5;
            return;
        }
    } else {
        __syncthreads();
    }

    V3 v[RX_APT], g[RX_APT], x0[RX_APT];
#pragma unroll
    for (int k = 0; k < RX_APT; ++k) {
        const int il = t + k * RX_NT;
        v[k] = {0.f, 0.f, 0.f}, g[k] = {0.f, 0.f, 0.f};
        if constexpr (RESTR) x0[k] = il < n ? rr_xyz(sh, il) : V3{0.f, 0.f, 0.f};          // restraints: the tethers' start coordinates
    }
    float h = o.dt_start, al = o.alpha_start, gm = 0.f;
    int npos = 0, steps = 0, status = 0;
    for (;;) {
        // ---- the objective's gradient at the current coordinates; max |g_i|, a flag for a non-finite gradient, P = F.v, |F|^2, |v|^2
        // (the sums stay in a loop of their own: formed inside rx_gradient's pass they come out with other bits)
        rx_gradient(d, a.nb, a.has_nb, sh, w, g, [](int, V3) {});
        // restraints, gradient: g = grad E_ff so far; the atom's rows in ascending r, then its tether, then 0 for a frozen atom
        if constexpr (RESTR)
#pragma unroll
        for (int k = 0; k < RX_APT; ++k) {
            const int il = t + k * RX_NT;
            if (il < n) {
                V3 gi = g[k];
                for (int r = 0; r < nr; ++r) {
                    const int p = rs.at[r][0] == il ? 0 : (rs.at[r][1] == il ? 1 : (rs.at[r][2] == il ? 2 : (rs.at[r][3] == il ? 3 : -1)));
                    if (p >= 0) {
                        V3 d0, d1, d2, d3;
                        const float phi = rr_dihedral(sh, rs, r, d0, d1, d2, d3);
                        const float coef = rs.k[r] * sinf(phi - rs.tg[r]);
                        gi = gi + coef * (p == 0 ? d0 : (p == 1 ? d1 : (p == 2 ? d2 : d3)));
                    }
                }
                if (pk[k] != 0.f) gi = gi + pk[k] * (rr_xyz(sh, il) - x0[k]);
                if (frz[k]) gi = {0.f, 0.f, 0.f};
                g[k] = gi;
            }
        }
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
            bool moves = il < n;
            if constexpr (RESTR) moves = moves && !frz[k];          // restraints: a frozen atom's coordinates are never written, they keep their bits
            if (moves) {
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

    // ---- results: the coordinates held, the objective's gradient there, and the force field's energy terms (thread partials, added in
    // double in thread order); restraints, E_r: an owner's tethers and thread r's row r go through rx_energies' `extra` sum
    float er = 0.f;
#pragma unroll
    for (int k = 0; k < RX_APT; ++k) {
        const int il = t + k * RX_NT;
        if (il < n) {
            const size_t off = ((size_t)(m0 + il) * C + c) * 3;
            const float4 x = sh.xs[il];
            a.xyz_out[off] = x.x, a.xyz_out[off + 1] = x.y, a.xyz_out[off + 2] = x.z;
            if (a.grad) a.grad[off] = g[k].x, a.grad[off + 1] = g[k].y, a.grad[off + 2] = g[k].z;
            if constexpr (RESTR)
                if (pk[k] != 0.f) {
                    const V3 dx = rr_xyz(sh, il) - x0[k];
                    er += 0.5f * pk[k] * dot(dx, dx);
                }
        }
    }
    if constexpr (RESTR)
        if (t < nr) {
            V3 d0, d1, d2, d3;
            const float phi = rr_dihedral(sh, rs, t, d0, d1, d2, d3);
            er += rs.k[t] * (1.0f - cosf(phi - rs.tg[t]));
            if (a.dih_phi) a.dih_phi[(size_t)(k0 + t) * C + c] = phi;
        }
    // (sh.part is free: its last readers passed the barrier of the reduction that ended the loop)
    double tot;
    if constexpr (RESTR) tot = rx_energies(d, a.nb, a.has_nb, sh, w, er, rs.epart, &rs.esum);
    else tot = rx_energies(d, a.nb, a.has_nb, sh, w);
    if (t < 6 && a.term_energy) a.term_energy[((size_t)t * d.B + b) * C + c] = (float)sh.esum[t];
    if (t == 0) {
        a.energy[w.item] = (float)tot;
        if constexpr (RESTR) a.restraint_energy[w.item] = (float)rs.esum;
        a.gmax[w.item] = gm;
        a.steps[w.item] = steps;
        a.status[w.item] = status;
    }
}

// no restraints at all: E_r = 0 for every molecule grappa_relax_fire_f32 ran (one with atoms, within the size limit)
__global__ void relax_restr_zero_kernel(const int* __restrict__ atom_molptr, int N, int B, int C, float* __restrict__ restraint_energy) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * C) return;
    const int b = (int)(i / C);
    const int n = rx_clamp(atom_molptr[b + 1], N) - rx_clamp(atom_molptr[b], N);
    if (n > 0 && n <= RX_MAX) restraint_energy[i] = 0.f;
}

// the checks, the arguments and the launch both entries share; `a` arrives with what the objective alone takes
template <bool RESTR, class Args, class RS>
int relax_fire(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_relax_opts* o, Args a, float* xyz_out,
               float* energy, float* term_energy, float* grad, float* gmax, int* steps, int* status) {
    const int rc = mm_seam_check(mm, nb, o && relax_opts_ok(o));
    if (rc != GRAPPA_OK) return rc < 0 ? rc : GRAPPA_OK;
    if (!xyz_out || !energy || !gmax || !steps || !status) return GRAPPA_ERR_ARG;
    a.mm = *mm;
    a.has_nb = nb != nullptr;
    if (nb) a.nb = *nb; else a.nb = grappa_nb_desc{};
    a.o = *o;
    a.xyz_out = xyz_out, a.energy = energy, a.term_energy = term_energy, a.grad = grad, a.gmax = gmax;
    a.steps = steps, a.status = status;
    GRAPPA_LAUNCH((fire_kernel<RESTR, Args, RS>), dim3((unsigned)(mm->B * mm->C)), dim3(RX_NT), 0, reinterpret_cast<hipStream_t>(stream), a);
    return grappa_launch_status();
}

}  // namespace

extern "C" int grappa_relax_max_atoms(void) { return RX_MAX; }
extern "C" int grappa_relax_max_dihedrals(void) { return GRAPPA_RELAX_MAX_DIHEDRALS; }

extern "C" int grappa_relax_fire_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_relax_opts* o, float* xyz_out,
                                     float* energy, float* term_energy, float* grad, float* gmax, int* steps, int* status) {
    return relax_fire<false, RxArgs, NoRestr>(stream, mm, nb, o, RxArgs{}, xyz_out, energy, term_energy, grad, gmax, steps, status);
}

extern "C" int grappa_relax_fire_restr_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_relax_opts* o,
                                           const grappa_relax_restr* r, float* xyz_out, float* energy, float* term_energy, float* grad, float* gmax,
                                           int* steps, int* status, float* restraint_energy, float* dih_phi) {
    if (!restraint_energy) return GRAPPA_ERR_ARG;
    if (r) {
        if (r->R < 0) return GRAPPA_ERR_ARG;
        if (r->R > 0 && (!r->dih_molptr || !r->dih_atoms || !r->dih_k || !r->dih_target)) return GRAPPA_ERR_ARG;
        if (mm && mm->C > 0 && (long long)r->R * mm->C > INT_MAX) return GRAPPA_ERR_ARG;
    }
    if (!r || (r->R == 0 && !r->frozen && !r->pos_k)) {          // no restraints: the unrestrained launch itself, hence its bits
        const int rc = grappa_relax_fire_f32(stream, mm, nb, o, xyz_out, energy, term_energy, grad, gmax, steps, status);
        if (rc != GRAPPA_OK || mm->N == 0 || mm->C == 0 || mm->B == 0) return rc;
        const long long items = (long long)mm->B * mm->C;
        GRAPPA_LAUNCH(relax_restr_zero_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                      mm->atom_molptr, mm->N, mm->B, mm->C, restraint_energy);
        return grappa_launch_status();
    }
    RrArgs a = {};
    a.frozen = r->frozen, a.pos_k = r->pos_k, a.R = r->R;
    a.dih_molptr = r->dih_molptr, a.dih_atoms = r->dih_atoms, a.dih_k = r->dih_k, a.dih_target = r->dih_target;
    a.restraint_energy = restraint_energy, a.dih_phi = dih_phi;
    return relax_fire<true, RrArgs, RrShared>(stream, mm, nb, o, a, xyz_out, energy, term_energy, grad, gmax, steps, status);
}
