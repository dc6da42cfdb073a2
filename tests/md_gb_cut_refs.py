"""The restatements of the stepwise dynamics in GB/SA implicit solvent under the solvent's cutoff (tests/test_host_gb_cut.py on the CPU,
tests/test_gpu_md_gb_cut.py): md_refs.baoab_ref with the force replaced by bonded + nonbonded + gb_cut_refs.gb_cut_ref (whose gradient
is autograd of the restated, truncated energy), on md_gb_refs' cases with its GB parameters.  The solvent's cutoff is 9 A nominal,
placed per case by gb_cut_refs.place_cutoff on the start coordinates: the molecules are extended chains of about 0.84 A per atom, so
from 65 atoms on most pairs lie beyond it.  With `both`, the nonbonded term runs under a cutoff too (nb_cut_refs.nb_cut_ref):
`Cutoff(rc, 0.8 rc, 1.0)` at the solvent's placed rc -- eps = 1 is OpenMM's companion of GB.

A pair that crosses the solvent's cutoff during a run, which float64 and fp32 may see a step apart, moves the force by the pair's part
of it: the truncation is not smoothed.  tests/test_host_gb_cut.py caps the share of (item, step count) pairs that this makes unsteady."""
import contextlib
import functools

import torch

import gb_cut_refs as gc
import md_gb_refs as mg
import md_refs as md
import md_steps_refs as ms
import nb_cut_refs as nc
import nonbonded_refs as nr
from grappa_amd.solvent import ImplicitSolvent

NOMINAL = 9.0
CASES = mg.CASES
TRAJ_STEPS = ms.TRAJ_STEPS
BOTH_CASE = "s129_C3"          # the run with both cutoffs
CONS_CASE = mg.CONS_CASE


def _batch(name):
    if name == CONS_CASE:
        import md_steps_cons_refs as msc
        return msc.case(CONS_CASE)[0]
    return ms.case(name)


@functools.lru_cache(maxsize=None)
def placed(name):
    """-> (rc, half gap) of the solvent's cutoff at the case's start coordinates"""
    b = _batch(name)
    return gc.place_cutoff(list(b.counts), b.xyz.numpy(), NOMINAL)


def solvent(name, prune=True) -> ImplicitSolvent:
    return ImplicitSolvent(mg.MODEL, cutoff=placed(name)[0], prune=prune)


def nb_cutoff(name, prune=True) -> nc.Cutoff:
    """the nonbonded cutoff of the run with both: at the solvent's rc, switched from 0.8 rc, reaction-field dielectric 1"""
    rc = placed(name)[0]
    return nc.Cutoff(rc, 0.8 * rc, 1.0, prune)


@contextlib.contextmanager
def gb_cut_force(gbs, sv, nb_cut=None):
    """inside: relax_refs.forces (what md_refs.baoab_ref evaluates) adds the truncated GB/SA energy and gradient of `gbs` to its nonbonded
    part, which is all pairs or, with nb_cut, nb_cut_refs.nb_cut_ref's"""
    plain = nr.nb_ref

    def with_gb(params, x, dtype=torch.float64):
        nb = plain(params, x, dtype) if nb_cut is None else nc.nb_cut_ref(params, x, nb_cut, dtype)
        gb = gc.gb_cut_ref(params, gbs, x, sv, dtype, scales=False)
        return dict(nb, energy=nb["energy"] + gb["energy"], grad=nb["grad"] + gb["grad"])

    nr.nb_ref = with_gb
    try:
        yield
    finally:
        nr.nb_ref = plain


def realisations(name, snapshots, both=False, **kw):
    """md_refs.fp32_realisations of the case in the truncated solvent"""
    with gb_cut_force(mg.gb_params(name), solvent(name), nb_cutoff(name) if both else None):
        return md.fp32_realisations(ms.case(name), ms.masses(name), snapshots, **kw)


@functools.lru_cache(maxsize=None)
def verlet32(name, both=False, steps=max(TRAJ_STEPS)):
    """friction 0, 1 fs, from the case coordinates with thermal velocities, after TRAJ_STEPS.  Read-only."""
    return realisations(name, TRAJ_STEPS, both=both, velocities=ms.thermal_velocities(name), n_steps=steps)


def verlet(name, both=False):
    return {k: pair[1] for k, pair in verlet32(name, both)[0].items()}


def steady_counts():
    """md_steps_refs.steady_counts over CASES (and BOTH_CASE with both cutoffs) in the truncated solvent -> {"x": [non-steady, pairs], "v": ...}"""
    out = {"x": [0, 0], "v": [0, 0]}
    for name, both in [(n, False) for n in CASES] + [(BOTH_CASE, True)]:
        b = ms.case(name)
        for k in TRAJ_STEPS:
            r32s = [r[k] for r in verlet32(name, both)]
            for label, idx in (("x", 0), ("v", 1)):
                s = ms.steady(b, r32s, idx)
                out[label][0] += int((~s).sum())
                out[label][1] += s.numel()
    return out


@functools.lru_cache(maxsize=None)
def cons_verlet():
    """-> (float64 restatement with snapshots, fp32 realisations) of CONS_CASE in the truncated solvent: friction 0, 2 fs, thermal velocities"""
    import md_cons_refs as mc
    import md_steps_cons_refs as msc
    batch, cons, m, _ = msc.case(CONS_CASE)
    kw = dict(velocities=msc.thermal_velocities(CONS_CASE), n_steps=max(msc.TRAJ_STEPS), dt=msc.TRAJ_DT)
    with gb_cut_force(list(mg.cons_gb()), solvent(CONS_CASE)):
        return (mc.gbaoab_ref(batch, m, cons, torch.float64, snapshots=msc.TRAJ_STEPS, **kw), mc.fp32_realisations(batch, m, cons, msc.TRAJ_STEPS, **kw))
