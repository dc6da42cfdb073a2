// Host-side checks of the descriptors of include/grappa_hip.h that several entry points take (csrc/mm_energy.hip, csrc/relax.hip,
// csrc/relax_steps.hip, csrc/dynamics.hip, csrc/dynamics_steps.hip): ONE definition of what a usable table is.  The heads of the entries differ (which sizes may be
// zero, which outputs are required) and stay with them.
#pragma once
#include <float.h>

#include "common.h"

namespace {

constexpr int GRAPPA_STEP_CAP = 1000000;      // steps per call at most (minimiser and dynamics): every loop on the device terminates

// the four tuple levels of a grappa_mm_desc and, with need_inc, the incidence codes that name their tuples
inline bool mm_desc_tables_ok(const grappa_mm_desc* mm, bool need_inc) {
    long long tuples = 0;
    for (int l = 0; l < 4; ++l) {
        if (mm->T[l] < 0 || mm->T[l] >= (1 << 27) || !mm->mol_ptr[l]) return false;
        if (mm->T[l] > 0 && (!mm->idx[l] || !mm->k[l])) return false;
        if (l < 2 && mm->T[l] > 0 && !mm->eq[l]) return false;
        if (l >= 2 && (mm->n_per[l] < 1 || mm->n_per[l] > 8)) return false;
        tuples += mm->T[l];
    }
    return !(need_inc && tuples > 0 && !mm->inc_code);
}

// the per-atom parameters and the exception table of a grappa_nb_desc
inline bool nb_desc_tables_ok(const grappa_nb_desc* nb) {
    return nb->charge && nb->sigma && nb->epsilon && nb->exc_ptr && nb->exc_atom && nb->exc_qq && nb->exc_sigma && nb->exc_eps;
}

// the options of the minimisers (comparisons written so that a NaN is refused)
inline bool relax_opts_ok(const grappa_relax_opts* o) {
    if (!(o->tolerance >= 0.f) || o->max_steps < 0 || o->max_steps > GRAPPA_STEP_CAP || !(o->dt_start > 0.f) || !(o->dt_max > 0.f) ||
        !(o->max_disp > 0.f) || o->n_min < 0 || !(o->f_inc > 0.f) || !(o->f_dec > 0.f) || !(o->f_alpha > 0.f) ||
        !(o->alpha_start >= 0.f && o->alpha_start <= 1.f))
        return false;
    return o->dt_start <= FLT_MAX && o->dt_max <= FLT_MAX && o->max_disp <= FLT_MAX && o->f_inc <= FLT_MAX && o->f_dec <= FLT_MAX &&
           o->f_alpha <= FLT_MAX && o->tolerance <= FLT_MAX;
}

}  // namespace
