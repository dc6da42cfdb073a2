// The decision FIRE takes once per step, shared by the fused minimiser (csrc/relax.hip) and the stepwise one (csrc/relax_steps.hip).
#pragma once
#include "common.h"

namespace {

// From P = F.v, |F|^2 and |v|^2 of the step: mix the velocity towards the force (downhill: v = keep v + mix F) or drop it, and the new
// time step h, mixing factor al and count npos of downhill steps in a row.  -> downhill.  The options come by value: a reference into
// a kernel's argument struct makes the compiler read the per-item state of rs_decide_kernel with vector loads instead of scalar ones.
__device__ inline bool fire_decide(grappa_relax_opts o, float P, float F2, float v2, float& h, float& al, int& npos, float& mix, float& keep) {
    const bool downhill = P > 0.f;
    mix = 0.f, keep = 0.f;
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
    return downhill;
}

}  // namespace
