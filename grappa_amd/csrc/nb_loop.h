// The tiled pair loop of a work item (csrc/nb_plan.h): ONE text for the energy kernel (nb_pairs_kernel of csrc/nonbonded.hip, which
// describes it under "pairs" and "cutoff") and for the force of the stepwise minimiser and dynamics (rs_force of csrc/rs_force.h), with
// and without a cutoff -- what one of them evaluates, skips or rounds, the others do.
#pragma once
#include <limits.h>

#include <type_traits>

#include "common.h"
#include "nb_cut.h"
#include "nb_pair.h"
#include "nb_plan.h"

namespace {

// what a thread's slice of the pairs adds up to: both energies, the gradient of its (atom, conformation), and the tiles evaluated
struct NbSums {
    float elj, ec, gx, gy, gz;
    int tiles;      // (counted under a cutoff only)
};

// Every thread of the item's workgroup calls it (barriers inside); the thread is slice s of JS of (atom i, conformation c = r.c0 + cl),
// and takes part in the pairs iff `active`.  x: the coordinates [N,C,3]; run: which of the item's conformations still run (an int
// array in LDS; a conformation that has stopped is neither loaded nor asked for a verdict) or the literal nullptr: all run, and the
// test is compiled out (a run-time null test of an LDS address is not folded away: one more scalar branch per tile load).  xs, ps:
// NB_TJ * NB_CW and NB_TJ float4 of LDS.  The pairs of the thread's slice are added to `acc` in ascending j.  Cut: the policy of
// csrc/nb_cut.h (its block numbers checked by nb_cut_blocks_ok before the call).  The sums go in and out BY VALUE: handed down by
// reference through this function to nb_pair, the compiler merged the two pair forms' closing gradient fmas under one more
// predicate, and the cut kernels ran 3 % slower on a 513-atom molecule (profiles/nb_one_loop_isa.txt).
// x is a REFERENCE to the caller's pointer (a kernel argument): taken by value, the stepwise cut force read it once ahead of the loop
// where the two copies read it at each use, the tile loop came to lie 12 bytes earlier in the kernel, and 20 steps of a 50,046-atom
// chain took 1 to 2 % longer; by reference the loop's instructions stand at the addresses they had (same file).
template <class Cut, class Run>
__device__ __forceinline__ NbSums nb_pair_loop(const grappa_nb_desc& d, const float* const& x, const RsItem& r, int C, int s, int JS, int i, int c,
                                               int cl, bool active, Run run, const Cut& cut, float4* xs, float4* ps, NbSums acc) {
    constexpr bool masked = !std::is_null_pointer<Run>::value;
    float elj = acc.elj, ec = acc.ec, gx = acc.gx, gy = acc.gy, gz = acc.gz;
    const int t = threadIdx.x, m0 = r.m0, m1 = r.m1, c0 = r.c0, nc = r.nc;
    float xi = 0.f, yi = 0.f, zi = 0.f, kq = 0.f, hs = 0.f, se = 0.f;
    int ep = 0, ee = 0, nx = INT_MAX;
    if (active) {      // the coordinates are asked for AFTER the parameters: loads return in order, and what the first tile waits for is sigma
        kq = NB_K * d.charge[i];
        hs = 0.5f * d.sigma[i];
        se = 4.0f * sqrtf(d.epsilon[i]);
        ep = d.exc_ptr[i];
        ee = d.exc_ptr[i + 1];
        const float* p = x + ((size_t)i * C + c) * 3;
        xi = p[0], yi = p[1], zi = p[2];
        nx = ep < ee ? d.exc_atom[ep] : INT_MAX;
    }
    int count = 0;
    [[maybe_unused]] const int ntiles = nb_tiles(r), kb0 = nb_first_block(r);      // (read by the cut policy only)
    for (int j0 = m0; j0 < m1; j0 += NB_TJ) {
        if constexpr (Cut::on) {      // NB_NT verdicts at a time; a far tile loads nothing and passes no barrier of the tile
            const int jt = (j0 - m0) / NB_TJ, k = jt & (NB_NT - 1);
            if (k == 0) nb_cut_decide(cut.c, C, r.blk, kb0, ntiles, jt, c0, nc, run, cut.near);
            if (!cut.near[k]) continue;
            ++count;
        }
        const int nj = m1 - j0 < NB_TJ ? m1 - j0 : NB_TJ;
        __syncthreads();
        for (int idx = t; idx < nj * nc; idx += NB_NT) {
            const int jj = idx / nc, cc = idx - jj * nc;
            if constexpr (masked)
                if (!run[cc]) continue;
            const float* p = x + ((size_t)(j0 + jj) * C + c0 + cc) * 3;
            xs[jj * NB_CW + cc] = make_float4(p[0], p[1], p[2], 0.f);
        }
        if (t < nj) ps[t] = make_float4(d.charge[j0 + t], 0.5f * d.sigma[j0 + t], sqrtf(d.epsilon[j0 + t]), 0.f);
        __syncthreads();
        const bool lookup = active && ((i >= j0 && i < j0 + nj) || nx < j0 + nj);
        if (__builtin_amdgcn_ballot_w64(lookup) != 0) {
            if (active) {
                for (int jj = s; jj < nj; jj += JS) {
                    const int j = j0 + jj;
                    const float4 p = ps[jj];
                    float sij = hs + p.y, e4 = se * p.z, kqq = kq * p.x;
                    bool skip = j == i;
                    while (nx < j) {
                        ++ep;
                        nx = ep < ee ? d.exc_atom[ep] : INT_MAX;
                    }
                    bool exc = false;      // (read by the cut policy only)
                    if (nx == j) {
                        const float q = d.exc_qq[ep], e = d.exc_eps[ep];
                        exc = true;
                        sij = d.exc_sigma[ep];
                        e4 = 4.0f * e;
                        kqq = NB_K * q;
                        skip = skip || (q == 0.f && e == 0.f);
                        ++ep;
                        nx = ep < ee ? d.exc_atom[ep] : INT_MAX;
                    }
                    if (!skip) {
                        const float4 xj = xs[jj * NB_CW + cl];
                        if constexpr (Cut::on) {      // an exception is not cut
                            if (exc) nb_pair(xi - xj.x, yi - xj.y, zi - xj.z, sij, e4, kqq, elj, ec, gx, gy, gz);
                            else nb_pair_cut(xi - xj.x, yi - xj.y, zi - xj.z, sij, e4, kqq, cut.c.k, elj, ec, gx, gy, gz);
                        } else {
                            nb_pair(xi - xj.x, yi - xj.y, zi - xj.z, sij, e4, kqq, elj, ec, gx, gy, gz);
                        }
                    }
                }
                while (nx < j0 + nj) {      // partners that belong to other slices
                    ++ep;
                    nx = ep < ee ? d.exc_atom[ep] : INT_MAX;
                }
            }
        } else if (active) {
#pragma unroll 4
            for (int jj = s; jj < nj; jj += JS) {
                const float4 p = ps[jj];
                const float4 xj = xs[jj * NB_CW + cl];
                if constexpr (Cut::on) nb_pair_cut(xi - xj.x, yi - xj.y, zi - xj.z, hs + p.y, se * p.z, kq * p.x, cut.c.k, elj, ec, gx, gy, gz);
                else nb_pair(xi - xj.x, yi - xj.y, zi - xj.z, hs + p.y, se * p.z, kq * p.x, elj, ec, gx, gy, gz);
            }
        }
    }
    return NbSums{elj, ec, gx, gy, gz, count};
}

}  // namespace
