// Host-side checks of the descriptors of include/grappa_hip.h that several entry points take (csrc/mm_energy.hip, csrc/relax.hip,
// csrc/relax_steps.hip, csrc/dynamics.hip, csrc/dynamics_cons.hip, csrc/dynamics_steps.hip): ONE definition of what a usable table is, and
// ONE of the argument head the minimisers and the dynamics share (mm_seam_check, steps_seam_check).  What an entry alone takes (its
// output pointers, its restraint or constraint struct, its step counts) stays with it.
#pragma once
#include <float.h>
#include <limits.h>
#include <stdint.h>

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

constexpr int GRAPPA_SEAM_EMPTY = 1;          // mm_seam_check / steps_seam_check: an empty batch, nothing to do (the entry returns GRAPPA_OK)

// The head of every entry that takes (mm, nb, options): GRAPPA_ERR_ARG, GRAPPA_SEAM_EMPTY or GRAPPA_OK.  opts_ok is the entry's verdict on
// its options (relax_opts_ok, md_opts_ok; false for a NULL struct).  The order is observable and fixed: a NULL descriptor, a negative size,
// nb disagreeing with mm and bad options are refused BEFORE an empty batch returns; the MM pointers, the tables and B * C are looked at
// only after it, so an empty batch never has its pointers read.
inline int mm_seam_check(const grappa_mm_desc* mm, const grappa_nb_desc* nb, bool opts_ok) {
    if (!mm || !opts_ok || mm->N < 0 || mm->C < 0 || mm->B < 0) return GRAPPA_ERR_ARG;
    if (nb && (nb->N != mm->N || nb->C != mm->C || nb->B != mm->B)) return GRAPPA_ERR_ARG;
    if (mm->N == 0 || mm->C == 0 || mm->B == 0) return GRAPPA_SEAM_EMPTY;
    if (!mm->xyz || !mm->atom_molptr || !mm->inc_ptr) return GRAPPA_ERR_ARG;
    if (!mm_desc_tables_ok(mm, true) || (nb && !nb_desc_tables_ok(nb))) return GRAPPA_ERR_ARG;
    if ((long long)mm->B * mm->C > INT_MAX) return GRAPPA_ERR_ARG;
    return GRAPPA_OK;
}

// the same for the three calls of a stepwise path (csrc/relax_steps.hip, csrc/dynamics_steps.hip), which also take the work-item table
// and the workspace: negative counts are refused before an empty batch returns, the rest after it
inline int steps_seam_check(const grappa_mm_desc* mm, const grappa_nb_desc* nb, bool opts_ok, const int* table_dev, int n_items, int n_blocks,
                            const void* ws) {
    if (n_items < 0 || n_blocks < 0) return GRAPPA_ERR_ARG;
    const int rc = mm_seam_check(mm, nb, opts_ok);
    if (rc != GRAPPA_OK) return rc;
    if (!table_dev || !ws) return GRAPPA_ERR_ARG;
    if (((uintptr_t)ws & 15) != 0 || ((uintptr_t)table_dev & 15) != 0) return GRAPPA_ERR_ARG;      // (doubles in the workspace, int4 items in the table)
    if ((long long)mm->N * mm->C * 3 > INT_MAX || (long long)n_blocks * mm->C > INT_MAX) return GRAPPA_ERR_ARG;
    if (n_blocks > (long long)mm->N / GRAPPA_NB_IBLOCK + mm->B) return GRAPPA_ERR_ARG;
    return GRAPPA_OK;
}

}  // namespace
