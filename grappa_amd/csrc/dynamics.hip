// Fused Langevin molecular dynamics (BAOAB, Leimkuhler and Matthews 2013) under the full MM force field (bonded terms of
// csrc/mm_energy.hip + Lennard-Jones / Coulomb of csrc/nonbonded.hip), fp32, xyz[N,C,3] (include/grappa_hip.h grappa_md_langevin_f32).
//   item   : one workgroup of 256 threads per (molecule, conformation), as in csrc/relax.hip: it loads the molecule once, runs n_steps
//            steps and writes its results.  Workgroups never talk to each other: an item's bits depend on its own input only.
//   LDS    : the image of csrc/rx_force.h (x, y, z, q, sigma / 2, sqrt(eps), the partial gradients of one step, the reduction words)
//            plus 256 floats and a double for the kinetic energy: 19.6 KB at any molecule size up to RX_MAX atoms.  Velocities,
//            gradients, the mass and the two per-atom factors (dt / 2 ACC / m, c2 sqrt(ACC kB T / m)) stay in the registers of the
//            atom's owner (thread a % 256).
//   step   : the owner kicks, drifts, draws the thermostat's noise and drifts again (its own atoms only: no barrier in between),
//            barrier; rx_gradient of csrc/rx_force.h (the partial gradients per (atom, slice), barrier, the owner adds the slices in
//            slice order) and the flag of a non-finite gradient is reduced (one barrier); the closing kick.  Three barriers per step.
//   frame  : every save_every steps the coordinates and, if asked for, the energies (rx_energies): the six potential terms as thread
//            partials in sh.part (its readers of this step passed the reduction's barrier), barrier, seven threads add them and the kinetic partials
//            in double in thread order, barrier.  The next step's partial gradients are written after that barrier and the one that
//            follows its drift, so they cannot overwrite what the seven threads read.  Two barriers per frame with energies.
//   noise  : Philox4x32-10 (csrc/md_philox.h, csrc/md_noise.h), key = mol_key[b], counter = (atom in molecule, conformation, global step, purpose);
//            nothing is kept between steps or launches, so a run can be cut anywhere and continued with first_step advanced.
// The loop runs n_steps (<= GRAPPA_STEP_CAP) iterations: the kernel always terminates.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"
#include "desc_check.h"
#include "md_noise.h"
#include "rx_force.h"

namespace {

struct MdArgs {
    grappa_mm_desc mm;
    grappa_nb_desc nb;
    int has_nb;
    float h2, hk;                // dt / 2, dt / 2 ACC
    float c1, c2;                // exp(-friction dt), sqrt(1 - c1^2)
    float kt, kt0;               // ACC kB temperature, ACC kB init_temperature
    int thermostat;              // friction > 0
    int n_steps, save_every;
    unsigned first_step;
    const float* mass;
    const unsigned long long* mol_key;
    const float* vel_in;
    float *xyz_out, *vel_out, *epot, *ekin;
    int *steps, *status;
    float *frames_xyz, *frames_epot, *frames_ekin;
};

// g = grad E at the coordinates in LDS, into the owners' registers; true (in every thread) if a gradient is not finite.  Two barriers.
__device__ __forceinline__ bool md_force(const MdArgs& a, RxShared& sh, const RxItem& w, V3 (&g)[RX_APT]) {
    float bad = 0.f;
    rx_gradient(a.mm, a.nb, a.has_nb, sh, w, g, [&](int, V3 gi) {
        if (!(sqrtf(dot(gi, gi)) <= FLT_MAX)) bad = 1.f;
    });
    return rx_reduce_max(bad, sh.wmax) != 0.f;
}

// the potential energy (rx_energies) and the kinetic energy 0.5 / ACC sum m v^2 (the owners' partials, added the same way between the same
// barriers) of the state held -> (epot, ekin) in thread 0.  sh.part must be free.  Two barriers.
__device__ __forceinline__ float2 md_energies(const MdArgs& a, RxShared& sh, float* kin, double* ksum, const RxItem& w, const V3 (&v)[RX_APT],
                                              const float (&ms)[RX_APT]) {
    float mv2 = 0.f;
#pragma unroll
    for (int k = 0; k < RX_APT; ++k)
        if ((int)threadIdx.x + k * RX_NT < w.n) mv2 += ms[k] * dot(v[k], v[k]);
    const double tot = rx_energies(a.mm, a.nb, a.has_nb, sh, w, mv2, kin, ksum);
    return threadIdx.x == 0 ? make_float2((float)tot, (float)((0.5 / MD_ACC) * *ksum)) : make_float2(0.f, 0.f);
}

__global__ __launch_bounds__(RX_NT) void md_langevin_kernel(MdArgs a) {
    __shared__ RxShared sh;
    __shared__ float kin[RX_NT];
    __shared__ double ksum;
    const grappa_mm_desc& d = a.mm;
    const int C = d.C, t = threadIdx.x;
    // The item's prologue is rx_begin's (csrc/rx_force.h), written out: through rx_begin this kernel came out 0.7 % slower (2000 steps of
    // 8192 items: 396.7 ms against 393.7 ms, the same arithmetic in another layout), so the two copies must be changed together.
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
    const int JS = n > RX_NT ? 1 : (RX_NT / n < RX_JS ? RX_NT / n : RX_JS);
    const int s = n > RX_NT ? 0 : t / n;
    const int il0 = t - s * n;
    const bool active = s < JS;
    const RxItem w = {b, c, item, m0, n, JS, s, il0, active};
    const unsigned long long key = a.mol_key[b];

    // the owner's atoms: mass (0: frozen), the kick and noise factors, the start velocity
    V3 v[RX_APT], g[RX_APT];
    float ms[RX_APT], kw[RX_APT], sg[RX_APT];
#pragma unroll
    for (int k = 0; k < RX_APT; ++k) {
        const int il = t + k * RX_NT;
        v[k] = {0.f, 0.f, 0.f}, g[k] = {0.f, 0.f, 0.f};
        ms[k] = 0.f, kw[k] = 0.f, sg[k] = 0.f;
        if (il < n) {
            const float m = a.mass[m0 + il];
            if (m > 0.f) {          // (a mass that is zero, negative or NaN: a frozen atom, v = 0)
                const float im = 1.0f / m;
                ms[k] = m, kw[k] = a.hk * im, sg[k] = a.c2 * sqrtf(a.kt * im);
                if (a.vel_in) {
                    const float* p = a.vel_in + ((size_t)(m0 + il) * C + c) * 3;
                    v[k] = {p[0], p[1], p[2]};
                } else if (a.kt0 > 0.f) {
                    v[k] = sqrtf(a.kt0 * im) * md_normal3(key, (unsigned)il, (unsigned)c, a.first_step, 1u);
                }
            }
        }
    }
    __syncthreads();

    // one force evaluation per pass: the pass closes step `steps` (none on the first pass), tests the gradient and opens the next step
    bool bad;
    int steps = 0, since = 0, frame = 0;
    for (;;) {
        bad = md_force(a, sh, w, g);
        bool due = false;
        if (steps > 0) {
            // ---- the closing B of the step, and its frame's coordinates
#pragma unroll
            for (int kk = 0; kk < RX_APT; ++kk)
                if (t + kk * RX_NT < n && kw[kk] > 0.f) v[kk] = v[kk] - kw[kk] * g[kk];
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
                }
            }
        }
        // ---- the energies: of a frame that asks for them, and of the state the run ends with
        const bool last = bad || steps >= a.n_steps;
        if (last || (due && (a.frames_epot || a.frames_ekin))) {
            const float2 e = md_energies(a, sh, kin, &ksum, w, v, ms);
            if (t == 0) {
                const size_t fo = (size_t)frame * d.B * C + item;
                if (due && a.frames_epot) a.frames_epot[fo] = e.x;
                if (due && a.frames_ekin) a.frames_ekin[fo] = e.y;
                if (last) a.epot[item] = e.x, a.ekin[item] = e.y;
            }
        }
        if (due) ++frame;
        if (last) break;
        // ---- B, A, O, A on the owner's atoms (a frozen atom is not touched)
#pragma unroll
        for (int kk = 0; kk < RX_APT; ++kk) {
            const int il = t + kk * RX_NT;
            if (il < n && kw[kk] > 0.f) {
                V3 vk = v[kk] - kw[kk] * g[kk];
                float4 x = sh.xs[il];
                x.x += a.h2 * vk.x, x.y += a.h2 * vk.y, x.z += a.h2 * vk.z;
                if (a.thermostat) vk = a.c1 * vk + sg[kk] * md_normal3(key, (unsigned)il, (unsigned)c, a.first_step + (unsigned)steps, 0u);
                x.x += a.h2 * vk.x, x.y += a.h2 * vk.y, x.z += a.h2 * vk.z;
                sh.xs[il] = x;
                v[kk] = vk;
            }
        }
        ++steps;
        __syncthreads();
    }

    // ---- results: the state held and its energies
#pragma unroll
    for (int k = 0; k < RX_APT; ++k) {
        const int il = t + k * RX_NT;
        if (il < n) {
            const size_t off = ((size_t)(m0 + il) * C + c) * 3;
            const float4 x = sh.xs[il];
            a.xyz_out[off] = x.x, a.xyz_out[off + 1] = x.y, a.xyz_out[off + 2] = x.z;
            a.vel_out[off] = v[k].x, a.vel_out[off + 1] = v[k].y, a.vel_out[off + 2] = v[k].z;
        }
    }
    if (t == 0) {
        a.steps[item] = steps;
        a.status[item] = bad ? 2 : 0;
    }
}

// z of (atom, conformation) for one step and purpose, as md_langevin_kernel draws it: a thread per (atom, conformation)
__global__ __launch_bounds__(256) void md_noise_kernel(const unsigned long long* __restrict__ mol_key, const int* __restrict__ atom_molptr, int N,
                                                       int C, int B, unsigned step, unsigned purpose, float* __restrict__ out) {
    const size_t u = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= (size_t)N * C) return;
    const int atom = (int)(u / (unsigned)C), c = (int)(u - (size_t)atom * C);
    int lo = 0, hi = B - 1;          // the last molecule that starts at or before the atom
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rx_clamp(atom_molptr[mid], N) <= atom) lo = mid; else hi = mid - 1;
    }
    const int m0 = rx_clamp(atom_molptr[lo], N), m1 = rx_clamp(atom_molptr[lo + 1], N);
    V3 z = {0.f, 0.f, 0.f};          // (an atom that no molecule holds)
    if (atom >= m0 && atom < m1) z = md_normal3(mol_key[lo], (unsigned)(atom - m0), (unsigned)c, step, purpose);
    out[3 * u] = z.x, out[3 * u + 1] = z.y, out[3 * u + 2] = z.z;
}

}  // namespace

extern "C" void grappa_md_philox(unsigned long long key, unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned out[4]) {
    uint32_t w[4];
    grappa_philox4x32_10((uint32_t)key, (uint32_t)(key >> 32), c0, c1, c2, c3, w);
    for (int k = 0; k < 4; ++k) out[k] = w[k];
}

extern "C" int grappa_md_noise_f32(void* stream, const unsigned long long* mol_key, const int* atom_molptr, int N, int C, int B, unsigned step,
                                   unsigned purpose, float* out) {
    if (N < 0 || C < 0 || B < 0) return GRAPPA_ERR_ARG;
    if (N == 0 || C == 0 || B == 0) return GRAPPA_OK;
    if (!mol_key || !atom_molptr || !out || (long long)N * C > INT_MAX) return GRAPPA_ERR_ARG;
    const unsigned blocks = (unsigned)(((long long)N * C + 255) / 256);
    GRAPPA_LAUNCH(md_noise_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), mol_key, atom_molptr, N, C, B, step, purpose, out);
    return grappa_launch_status();
}

extern "C" int grappa_md_langevin_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_md_opts* o, const float* mass,
                                      const unsigned long long* mol_key, const float* vel_in, float* xyz_out, float* vel_out, float* epot,
                                      float* ekin, int* steps, int* status, float* frames_xyz, float* frames_epot, float* frames_ekin) {
    const int rc = mm_seam_check(mm, nb, o && md_opts_ok(o));
    if (rc != GRAPPA_OK) return rc < 0 ? rc : GRAPPA_OK;
    if (!mass || !mol_key || !xyz_out || !vel_out || !epot || !ekin || !steps || !status) return GRAPPA_ERR_ARG;
    MdArgs a;
    a.mm = *mm;
    a.has_nb = nb != nullptr;
    if (nb) a.nb = *nb; else a.nb = grappa_nb_desc{};
    const MdConsts k = md_consts(o);
    a.h2 = k.h2, a.hk = k.hk, a.c1 = k.c1, a.c2 = k.c2, a.kt = k.kt, a.kt0 = k.kt0, a.thermostat = k.thermostat;
    a.n_steps = o->n_steps, a.save_every = o->save_every, a.first_step = o->first_step;
    a.mass = mass, a.mol_key = mol_key, a.vel_in = vel_in;
    a.xyz_out = xyz_out, a.vel_out = vel_out, a.epot = epot, a.ekin = ekin, a.steps = steps, a.status = status;
    a.frames_xyz = frames_xyz, a.frames_epot = frames_epot, a.frames_ekin = frames_ekin;
    GRAPPA_LAUNCH(md_langevin_kernel, dim3((unsigned)(mm->B * mm->C)), dim3(RX_NT), 0, reinterpret_cast<hipStream_t>(stream), a);
    return grappa_launch_status();
}
