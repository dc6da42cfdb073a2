"""The restatements of the stepwise dynamics under a nonbonded cutoff (tests/test_host_md_cut.py on the CPU, tests/test_gpu_md_cut.py):
md_refs.baoab_ref with the force replaced by bonded + nb_cut_refs.nb_cut_ref, on cases of tests/md_steps_refs.py with its masses, keys
and 300 K velocities.  The cutoff is 9 A nominal, placed by nb_cut_refs.place_cutoff on the start coordinates, with a switch from 0.8 rc
and eps = 78.3: the switched Lennard-Jones force vanishes at rc and the reaction-field force there is 0.019 of the bare one, so a pair
that crosses rc during a run, which float64 and fp32 may see a step apart, moves the force by a negligible amount."""
import contextlib
import functools

import torch

import md_refs as md
import md_steps_refs as ms
import nb_cut_refs as nc
import nonbonded_refs as nr

NOMINAL = 9.0
CASES = ["s65_C3", "s129_C3", "s513_C1", ms.MIXED]
TRAJ_STEPS = ms.TRAJ_STEPS


@functools.lru_cache(maxsize=None)
def cutoff(name, prune=True) -> nc.Cutoff:
    b = ms.nve_batch() if name == "nve" else ms.case(name)
    rc, _ = nc.place_cutoff(b.params, b.xyz.numpy(), NOMINAL)
    return nc.Cutoff(rc, 0.8 * rc, 78.3, prune)


@contextlib.contextmanager
def cut_force(cut):
    """inside: relax_refs.forces (what md_refs.baoab_ref evaluates) takes its nonbonded part from nb_cut_refs.nb_cut_ref under `cut`"""
    plain = nr.nb_ref
    nr.nb_ref = lambda params, x, dtype=torch.float64: nc.nb_cut_ref(params, x, cut, dtype)
    try:
        yield
    finally:
        nr.nb_ref = plain


def realisations(name, snapshots, **kw):
    """md_refs.fp32_realisations of the case under its cutoff"""
    with cut_force(cutoff(name)):
        return md.fp32_realisations(ms.case(name), ms.masses(name), snapshots, **kw)


@functools.lru_cache(maxsize=None)
def verlet32(name, steps=max(TRAJ_STEPS)):
    """friction 0, 1 fs, from the case coordinates with thermal velocities, after TRAJ_STEPS.  Read-only."""
    return realisations(name, TRAJ_STEPS, velocities=ms.thermal_velocities(name), n_steps=steps)


def verlet(name):
    return {k: pair[1] for k, pair in verlet32(name)[0].items()}


def steady_counts():
    """md_steps_refs.steady_counts over CASES under the cutoff"""
    out = {"x": [0, 0], "v": [0, 0]}
    for name in CASES:
        b = ms.case(name)
        for k in TRAJ_STEPS:
            r32s = [r[k] for r in verlet32(name)]
            for label, idx in (("x", 0), ("v", 1)):
                s = ms.steady(b, r32s, idx)
                out[label][0] += int((~s).sum())
                out[label][1] += s.numel()
    return out


@functools.lru_cache(maxsize=None)
def nve_drift(dtype):
    """D = max over frames and items of |E_tot - E_tot at step 0| of the restatement in `dtype` under the cutoff (md_steps_refs.NVE)"""
    b, m, v = ms.nve_batch(), ms.masses(ms.NVE_CASE), ms.thermal_velocities(ms.NVE_CASE)
    with cut_force(cutoff("nve")):
        start = md.baoab_ref(b, m, dtype, velocities=v, n_steps=0)
        r = md.baoab_ref(b, m, dtype, velocities=v, **ms.NVE)
    assert not r["status"].any()
    return md.drift(start["epot"] + start["ekin"], r["frame_epot"] + r["frame_ekin"])
