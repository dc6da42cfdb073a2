// What the two dynamics kernels (csrc/dynamics.hip: a molecule in a workgroup; csrc/dynamics_steps.hip: a molecule over many) share, ONE
// copy each: the units, the option checks, the step's constants and the map from a Philox call (csrc/md_philox.h) to three normal
// deviates.  The random stream is a function of (key, atom in molecule, conformation, step, purpose) alone, so both kernels draw the same
// numbers for the same atom.
#pragma once
#include <float.h>
#include <math.h>

#include "common.h"
#include "desc_check.h"
#include "md_philox.h"
#include "mm_geom.h"

namespace {

constexpr double MD_ACC = 418.4;               // 1 kcal/mol = 418.4 amu A^2 / ps^2
constexpr double MD_KB = 0.0019872041;         // kcal/mol/K

// the option checks of grappa_md_langevin_f32 (comparisons written so that a NaN is refused)
inline bool md_opts_ok(const grappa_md_opts* o) {
    if (!(o->dt > 0.f && o->dt <= FLT_MAX) || !(o->temperature >= 0.f && o->temperature <= FLT_MAX) ||
        !(o->friction >= 0.f && o->friction <= FLT_MAX) || !(o->init_temperature >= 0.f && o->init_temperature <= FLT_MAX))
        return false;
    if (o->n_steps < 0 || o->n_steps > GRAPPA_STEP_CAP || o->save_every < 0) return false;
    return (unsigned long long)o->first_step + (unsigned long long)o->n_steps < (1ull << 32);
}

struct MdConsts {
    float h2, hk;                // dt / 2, dt / 2 ACC
    float c1, c2;                // exp(-friction dt), sqrt(1 - c1^2)
    float kt, kt0;               // ACC kB temperature, ACC kB init_temperature
    int thermostat;              // friction > 0
};

// the step's constants, formed in double and rounded once
inline MdConsts md_consts(const grappa_md_opts* o) {
    MdConsts k;
    const double dt = (double)o->dt, c1 = exp(-(double)o->friction * dt);
    k.h2 = (float)(0.5 * dt), k.hk = (float)(0.5 * dt * MD_ACC);
    k.c1 = (float)c1, k.c2 = (float)sqrt(1.0 - c1 * c1);
    k.kt = (float)(MD_ACC * MD_KB * (double)o->temperature), k.kt0 = (float)(MD_ACC * MD_KB * (double)o->init_temperature);
    k.thermostat = o->friction > 0.f;
    return k;
}

// sqrt(-2 ln u) for u = ((w >> 8) + 0.5) 2^-24.  Both logarithms get an argument that fp32 holds exactly: n + 0.5 has at most 24
// bits below 2^23, and above it 1 - u = ((2^24 - 1 - n) + 0.5) 2^-24 has.  u > 0 always.
__device__ inline float md_radius(uint32_t w) {
    const uint32_t n = w >> 8;
    const float l = n < (1u << 23) ? logf(((float)n + 0.5f) * 0x1p-24f) : log1pf(-(((float)(0xFFFFFFu - n) + 0.5f) * 0x1p-24f));
    return sqrtf(-2.0f * l);
}

// the three normal deviates of (key, atom in molecule, conformation, step, purpose): Box-Muller on 24-bit uniforms of one Philox call
__device__ inline V3 md_normal3(unsigned long long key, unsigned atom, unsigned conf, unsigned step, unsigned purpose) {
    uint32_t w[4];
    grappa_philox4x32_10((uint32_t)key, (uint32_t)(key >> 32), atom, conf, step, purpose, w);
    float sn, cs;
    sincospif((float)(w[1] >> 8) * 0x1p-23f, &sn, &cs);          // the angle 2 pi (w >> 8) 2^-24 in half turns: exact in fp32
    const float cz = cospif((float)(w[3] >> 8) * 0x1p-23f);
    const float r0 = md_radius(w[0]), r2 = md_radius(w[2]);
    return {r0 * cs, r0 * sn, r2 * cz};
}

}  // namespace
