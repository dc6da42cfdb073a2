// Fused Langevin dynamics with X-H bond constraints (include/grappa_hip.h grappa_md_langevin_cons_f32): g-BAOAB (Leimkuhler and Matthews
// 2016) with one geodesic sub-step, the force field, the item, the noise and the frames of csrc/dynamics.hip (rx_force.h, md_noise.h).
//   constraints : star clusters, one centre and up to four leaves with one length each; every atom in at most one cluster, so a molecule
//            of n <= 512 atoms has at most 256 of them: thread q integrates ALL atoms of the molecule's q-th cluster through B, A, S, P
//            and O.  An atom in no cluster is integrated by its ordinary owner (thread a % 256) exactly as in csrc/dynamics.hip.  The
//            integration phase therefore needs no communication: three barriers per step, as in the unconstrained kernel.
//   LDS    : the image of csrc/rx_force.h and the kinetic-energy words of csrc/dynamics.hip (19.6 KB) plus, for every atom, the velocity
//            and the inverse mass (float4, 8 KB), the gradient (6 KB) and the atom's cluster (2 KB): 35.6 KB.  A velocity is read and
//            written by the atom's integrating thread alone; the gradient is handed over from rx_gradient's per-atom callback, which
//            runs before the barrier inside the flag reduction.
//   S      : cluster-wise Newton on the multipliers (M-SHAKE), on vectors relative to the centre, at most GRAPPA_MD_CONS_MAX_ITER updates;
//            a cluster that does not converge sets the thread's flag, which is reduced with the non-finite-gradient flag at the next force
//            evaluation (status 4).  P: one direct L x L solve.  Both solves are straight-line Gaussian elimination on a 4 x 4 system
//            padded with identity rows.
//   tables : the constraint tables are device memory, so the kernel vets them before it writes anything (status 5): indices in range and
//            distinct, at least one leaf, lengths finite and positive, at most 256 clusters, and -- through a claim array in LDS -- no atom in two clusters.
// Every loop is bounded by n_steps (<= GRAPPA_STEP_CAP) or by GRAPPA_MD_CONS_MAX_ITER: the kernel always terminates.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"
#include "desc_check.h"
#include "md_cons.h"
#include "md_noise.h"
#include "rx_force.h"

namespace {

struct MdConsArgs {
    grappa_mm_desc mm;
    grappa_nb_desc nb;
    int has_nb;
    float h2, hk, ih2;           // dt / 2, dt / 2 ACC, 2 / dt
    float c1, c2;                // exp(-friction dt), sqrt(1 - c1^2)
    float kt, kt0;               // ACC kB temperature, ACC kB init_temperature
    int thermostat;              // friction > 0
    int n_steps, save_every;
    unsigned first_step;
    const int *cluster_molptr, *cluster_atoms;
    const float* cluster_d;
    int K, constrain_start;
    float tol2;                  // 2 tolerance
    const float* mass;
    const unsigned long long* mol_key;
    const float* vel_in;
    float *xyz_out, *vel_out, *epot, *ekin;
    int *steps, *status;
    float *frames_xyz, *frames_epot, *frames_ekin;
};

struct MdConsShared {
    float4 vw[RX_MAX];           // velocity, inverse mass (0: frozen)
    float g[3][RX_MAX];          // the gradient of the coordinates held
    int cl[RX_MAX];              // the atom's cluster within the molecule, -1: none
};

__device__ __forceinline__ V3 xyz_of(float4 p) { return {p.x, p.y, p.z}; }

// a cluster's atoms in LDS as the slots of csrc/md_cons.h, which holds P, S and the drift
struct LdsCluster {
    const Cluster& c;
    RxShared& sh;
    MdConsShared& cs;
    __device__ __forceinline__ int at(int s) const { return s == 0 ? c.a0 : c.al[s - 1]; }
    __device__ __forceinline__ V3 x(int s) const { return xyz_of(sh.xs[at(s)]); }
    __device__ __forceinline__ V3 v(int s) const { return xyz_of(cs.vw[at(s)]); }
    __device__ __forceinline__ void set_x(int s, V3 p) {
        float4 q = sh.xs[at(s)];
        q.x = p.x, q.y = p.y, q.z = p.z;
        sh.xs[at(s)] = q;
    }
    __device__ __forceinline__ void set_v(int s, V3 p) {
        float4 q = cs.vw[at(s)];
        q.x = p.x, q.y = p.y, q.z = p.z;
        cs.vw[at(s)] = q;
    }
};

// v -= (dt / 2) ACC w g on one atom (a frozen atom is not touched)
__device__ __forceinline__ void cons_kick(MdConsShared& cs, int il, float hk) {
    float4 v = cs.vw[il];
    if (v.w > 0.f) {
        const float kw = hk * v.w;
        v.x -= kw * cs.g[0][il], v.y -= kw * cs.g[1][il], v.z -= kw * cs.g[2][il];
        cs.vw[il] = v;
    }
}

// v = c1 v + c2 s z on one atom
__device__ __forceinline__ void cons_noise(const MdConsArgs& a, MdConsShared& cs, int il, unsigned long long key, unsigned c, unsigned step) {
    float4 v = cs.vw[il];
    if (v.w > 0.f) {
        const V3 z = md_normal3(key, (unsigned)il, c, step, 0u);
        const float sg = a.c2 * sqrtf(a.kt * v.w);
        v.x = a.c1 * v.x + sg * z.x, v.y = a.c1 * v.y + sg * z.y, v.z = a.c1 * v.z + sg * z.z;
        cs.vw[il] = v;
    }
}

__global__ __launch_bounds__(RX_NT) void md_langevin_cons_kernel(MdConsArgs a) {
    __shared__ RxShared sh;
    __shared__ MdConsShared cs;
    __shared__ float kin[RX_NT];
    __shared__ double ksum;
    const grappa_mm_desc& d = a.mm;
    const int C = d.C, t = threadIdx.x;
    RxItem w;
    if (!rx_begin(d, a.nb, a.has_nb, a.status, sh, w)) return;
    const int n = w.n, m0 = w.m0, c = w.c;
    const size_t item = w.item;
    const unsigned long long key = a.mol_key[w.b];

    // ---- the tables are vetted before anything is written: status 5 and nothing else
    const int k0 = rx_clamp(a.cluster_molptr[w.b], a.K), k1 = rx_clamp(a.cluster_molptr[w.b + 1], a.K);
    const int nc = k1 - k0;
    for (int il = t; il < n; il += RX_NT) cs.cl[il] = -1;
    Cluster cl;
    cl.L = 0, cl.a0 = 0, cl.w0 = 0.f;
    int at[CL + 1];
    float dd[CL];
    float invalid = nc > RX_NT ? 1.f : 0.f;
    const bool mine = nc <= RX_NT && t < nc;
    if (mine) {
        const int* p = a.cluster_atoms + (size_t)(k0 + t) * (CL + 1);
        const float* q = a.cluster_d + (size_t)(k0 + t) * CL;
#pragma unroll
        for (int k = 0; k <= CL; ++k) at[k] = p[k];
#pragma unroll
        for (int k = 0; k < CL; ++k) dd[k] = q[k];
        if ((unsigned)at[0] >= (unsigned)n) invalid = 1.f;
        bool leaf = false;
#pragma unroll
        for (int k = 1; k <= CL; ++k) leaf = leaf || at[k] != -1;
        if (!leaf) invalid = 1.f;          // a cluster has at least one leaf
#pragma unroll
        for (int k = 1; k <= CL; ++k)
            if (at[k] != -1) {
                if ((unsigned)at[k] >= (unsigned)n || !(dd[k - 1] > 0.f && dd[k - 1] <= FLT_MAX)) invalid = 1.f;
#pragma unroll
                for (int l = 0; l < k; ++l)
                    if (at[l] == at[k]) invalid = 1.f;
            }
    }
    __syncthreads();
    if (mine && invalid == 0.f) {
#pragma unroll
        for (int k = 0; k <= CL; ++k)
            if (at[k] != -1) cs.cl[at[k]] = t;
    }
    __syncthreads();
    if (mine && invalid == 0.f) {
#pragma unroll
        for (int k = 0; k <= CL; ++k)
            if (at[k] != -1 && cs.cl[at[k]] != t) invalid = 1.f;          // another cluster claimed the atom too
    }
    if (rx_reduce_max(invalid, sh.wmax) != 0.f) {
        if (t == 0) a.status[item] = 5;
        return;
    }

    // ---- the atoms' masses and start velocities, by their ordinary owners
    for (int il = t; il < n; il += RX_NT) {
        const float m = a.mass[m0 + il];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m > 0.f) {          // (a mass that is zero, negative or NaN: a frozen atom, v = 0)
            v.w = 1.0f / m;
            if (a.vel_in) {
                const float* p = a.vel_in + ((size_t)(m0 + il) * C + c) * 3;
                v.x = p[0], v.y = p[1], v.z = p[2];
            } else if (a.kt0 > 0.f) {
                const V3 z = sqrtf(a.kt0 * v.w) * md_normal3(key, (unsigned)il, (unsigned)c, a.first_step, 1u);
                v.x = z.x, v.y = z.y, v.z = z.z;
            }
        }
        cs.vw[il] = v;
    }
    __syncthreads();

    // ---- the thread's cluster (a leaf whose two ends are frozen is no constraint) and its free atoms
    if (mine) {
        cl.a0 = at[0];
        cl.w0 = cs.vw[at[0]].w;
#pragma unroll
        for (int k = 0; k < CL; ++k) cl.al[k] = 0, cl.wl[k] = 0.f, cl.d2[k] = 1.f;
#pragma unroll
        for (int k = 1; k <= CL; ++k)
            if (at[k] != -1) {
                const float wk = cs.vw[at[k]].w;
                cons_add_leaf(cl, at[k], wk, dd[k - 1]);
            }
    }
    const bool has_cl = cl.L > 0;
    bool free_atom[RX_APT];
#pragma unroll
    for (int k = 0; k < RX_APT; ++k) {
        const int il = t + k * RX_NT;
        free_atom[k] = il < n && cs.cl[il] < 0 && cs.vw[il].w > 0.f;
    }
    V3 rref[CL];
    LdsCluster st = {cl, sh, cs};
    bool fail = false;
    if (has_cl) {
        if (a.constrain_start) {
            cons_bonds(cl, rref, st);
            if (!cons_shake(cl, rref, st, a.tol2, a.ih2, false)) fail = true;
        }
        if (a.constrain_start || !a.vel_in) cons_project(cl, st);
    }
    __syncthreads();

    // one force evaluation per pass: the pass closes step `steps` (none on the first pass), tests the flags and opens the next step
    V3 g[RX_APT];
#pragma unroll
    for (int k = 0; k < RX_APT; ++k) g[k] = {0.f, 0.f, 0.f};
    float code;
    int steps = 0, since = 0, frame = 0;
    for (;;) {
        float bad = fail ? 2.f : 0.f;
        rx_gradient(a.mm, a.nb, a.has_nb, sh, w, g, [&](int k, V3 gi) {
            if (!(sqrtf(dot(gi, gi)) <= FLT_MAX)) bad = fmaxf(bad, 1.f);
            const int il = t + k * RX_NT;
            cs.g[0][il] = gi.x, cs.g[1][il] = gi.y, cs.g[2][il] = gi.z;
        });
        code = rx_reduce_max(bad, sh.wmax);
        bool due = false;
        if (steps > 0) {
            // ---- the closing B of the step and its projection, and the frame's coordinates
#pragma unroll
            for (int kk = 0; kk < RX_APT; ++kk)
                if (free_atom[kk]) cons_kick(cs, t + kk * RX_NT, a.hk);
            if (has_cl) {
                cons_kick(cs, cl.a0, a.hk);
#pragma unroll
                for (int k = 0; k < CL; ++k)
                    if (k < cl.L) cons_kick(cs, cl.al[k], a.hk);
                cons_project(cl, st);
            }
            if (a.save_every > 0 && ++since == a.save_every) {
                since = 0;
                due = true;
                if (a.frames_xyz) {
                    float* fx = a.frames_xyz + (size_t)frame * d.N * C * 3;
#pragma unroll
                    for (int kk = 0; kk < RX_APT; ++kk) {
                        const int il = t + kk * RX_NT;
                        if (il < n) {
                            const size_t off = ((size_t)(m0 + il) * C + c) * 3;
                            const float4 x = sh.xs[il];
                            fx[off] = x.x, fx[off + 1] = x.y, fx[off + 2] = x.z;
                        }
                    }
                    __syncthreads();          // an owner reads coordinates that the cluster's thread moves next: a barrier per frame
                }
            }
        }
        // ---- the energies: of a frame that asks for them, and of the state the run ends with
        const bool last = code != 0.f || steps >= a.n_steps;
        if (last || (due && (a.frames_epot || a.frames_ekin))) {
            float mv2 = 0.f;          // of the atoms this thread integrates
#pragma unroll
            for (int kk = 0; kk < RX_APT; ++kk)
                if (free_atom[kk]) {
                    const float4 v = cs.vw[t + kk * RX_NT];
                    mv2 += dot(xyz_of(v), xyz_of(v)) / v.w;
                }
            if (has_cl) {
                const float4 v0 = cs.vw[cl.a0];
                if (v0.w > 0.f) mv2 += dot(xyz_of(v0), xyz_of(v0)) / v0.w;
#pragma unroll
                for (int k = 0; k < CL; ++k)
                    if (k < cl.L && cl.wl[k] > 0.f) {
                        const float4 v = cs.vw[cl.al[k]];
                        mv2 += dot(xyz_of(v), xyz_of(v)) / v.w;
                    }
            }
            const double tot = rx_energies(a.mm, a.nb, a.has_nb, sh, w, mv2, kin, &ksum);
            if (t == 0) {
                const float ep = (float)tot, ek = (float)((0.5 / MD_ACC) * ksum);
                const size_t fo = (size_t)frame * d.B * C + item;
                if (due && a.frames_epot) a.frames_epot[fo] = ep;
                if (due && a.frames_ekin) a.frames_ekin[fo] = ek;
                if (last) a.epot[item] = ep, a.ekin[item] = ek;
            }
        }
        if (due) ++frame;
        if (last) break;
        const unsigned step = a.first_step + (unsigned)steps;
        // ---- B, A, O, A on a free atom, as in csrc/dynamics.hip
#pragma unroll
        for (int kk = 0; kk < RX_APT; ++kk)
            if (free_atom[kk]) {
                const int il = t + kk * RX_NT;
                const float4 vw = cs.vw[il];
                const float kw = a.hk * vw.w;
                V3 vk = xyz_of(vw) - kw * g[kk];
                float4 x = sh.xs[il];
                x.x += a.h2 * vk.x, x.y += a.h2 * vk.y, x.z += a.h2 * vk.z;
                if (a.thermostat) vk = a.c1 * vk + (a.c2 * sqrtf(a.kt * vw.w)) * md_normal3(key, (unsigned)il, (unsigned)c, step, 0u);
                x.x += a.h2 * vk.x, x.y += a.h2 * vk.y, x.z += a.h2 * vk.z;
                sh.xs[il] = x;
                cs.vw[il] = make_float4(vk.x, vk.y, vk.z, vw.w);
            }
        // ---- B P, A S P, O P, A S P on the thread's cluster
        if (has_cl) {
            cons_kick(cs, cl.a0, a.hk);
#pragma unroll
            for (int k = 0; k < CL; ++k)
                if (k < cl.L) cons_kick(cs, cl.al[k], a.hk);
            cons_project(cl, st);
            cons_drift(cl, rref, st, a.h2);
            if (!cons_shake(cl, rref, st, a.tol2, a.ih2, true)) fail = true;
            cons_project(cl, st);
            if (a.thermostat) {
                cons_noise(a, cs, cl.a0, key, (unsigned)c, step);
#pragma unroll
                for (int k = 0; k < CL; ++k)
                    if (k < cl.L) cons_noise(a, cs, cl.al[k], key, (unsigned)c, step);
                cons_project(cl, st);
            }
            cons_drift(cl, rref, st, a.h2);
            if (!cons_shake(cl, rref, st, a.tol2, a.ih2, true)) fail = true;
            cons_project(cl, st);
        }
        ++steps;
        __syncthreads();
    }

    // ---- results: the state held (the velocities by the atoms' ordinary owners: a barrier first)
    __syncthreads();
    for (int il = t; il < n; il += RX_NT) {
        const size_t off = ((size_t)(m0 + il) * C + c) * 3;
        const float4 x = sh.xs[il], v = cs.vw[il];
        a.xyz_out[off] = x.x, a.xyz_out[off + 1] = x.y, a.xyz_out[off + 2] = x.z;
        a.vel_out[off] = v.x, a.vel_out[off + 1] = v.y, a.vel_out[off + 2] = v.z;
    }
    if (t == 0) {
        // a step whose constraint did not converge is completed but not counted
        a.steps[item] = code == 2.f && steps > 0 ? steps - 1 : steps;
        a.status[item] = code == 2.f ? 4 : (code != 0.f ? 2 : 0);
    }
}

}  // namespace

extern "C" int grappa_md_cons_max_leaves(void) { return GRAPPA_MD_CONS_MAX_LEAVES; }
extern "C" int grappa_md_cons_max_iter(void) { return GRAPPA_MD_CONS_MAX_ITER; }

extern "C" int grappa_md_langevin_cons_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_md_opts* o,
                                           const grappa_md_cons* cons, const float* mass, const unsigned long long* mol_key, const float* vel_in,
                                           float* xyz_out, float* vel_out, float* epot, float* ekin, int* steps, int* status, float* frames_xyz,
                                           float* frames_epot, float* frames_ekin) {
    if (cons && cons->K < 0) return GRAPPA_ERR_ARG;
    if (!cons || cons->K == 0)          // no constraints: the unconstrained launch itself, hence its bits
        return grappa_md_langevin_f32(stream, mm, nb, o, mass, mol_key, vel_in, xyz_out, vel_out, epot, ekin, steps, status, frames_xyz, frames_epot,
                                      frames_ekin);
    if (!cons->cluster_molptr || !cons->cluster_atoms || !cons->cluster_d) return GRAPPA_ERR_ARG;
    if (!(cons->tolerance >= 0x1p-20f && cons->tolerance <= 0x1p-7f)) return GRAPPA_ERR_ARG;          // (a NaN is refused)
    const int rc = mm_seam_check(mm, nb, o && md_opts_ok(o));
    if (rc != GRAPPA_OK) return rc < 0 ? rc : GRAPPA_OK;
    if (!mass || !mol_key || !xyz_out || !vel_out || !epot || !ekin || !steps || !status) return GRAPPA_ERR_ARG;
    MdConsArgs a;
    a.mm = *mm;
    a.has_nb = nb != nullptr;
    if (nb) a.nb = *nb; else a.nb = grappa_nb_desc{};
    const MdConsts k = md_consts(o);
    a.h2 = k.h2, a.hk = k.hk, a.ih2 = 1.0f / k.h2, a.c1 = k.c1, a.c2 = k.c2, a.kt = k.kt, a.kt0 = k.kt0, a.thermostat = k.thermostat;
    a.n_steps = o->n_steps, a.save_every = o->save_every, a.first_step = o->first_step;
    a.cluster_molptr = cons->cluster_molptr, a.cluster_atoms = cons->cluster_atoms, a.cluster_d = cons->cluster_d;
    a.K = cons->K, a.constrain_start = cons->constrain_start != 0, a.tol2 = 2.0f * cons->tolerance;
    a.mass = mass, a.mol_key = mol_key, a.vel_in = vel_in;
    a.xyz_out = xyz_out, a.vel_out = vel_out, a.epot = epot, a.ekin = ekin, a.steps = steps, a.status = status;
    a.frames_xyz = frames_xyz, a.frames_epot = frames_epot, a.frames_ekin = frames_ekin;
    GRAPPA_LAUNCH(md_langevin_cons_kernel, dim3((unsigned)(mm->B * mm->C)), dim3(RX_NT), 0, reinterpret_cast<hipStream_t>(stream), a);
    return grappa_launch_status();
}
