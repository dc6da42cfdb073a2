"""The restatements of the stepwise dynamics in GB/SA implicit solvent (tests/test_host_gb.py on the CPU, tests/test_gpu_md_gb.py):
md_refs.baoab_ref with the force replaced by bonded + nonbonded_refs.nb_ref + gb_refs.gb_ref (whose gradient is autograd of the restated
energy), on cases of tests/md_steps_refs.py with its masses, keys and 300 K velocities, and GB parameters from
`GBParameters.from_elements` on random elements of {H, C, N, O, S} along the molecule's bonds."""
import contextlib
import functools

import numpy as np
import torch

import gb_refs as gr
import md_refs as md
import md_steps_refs as ms
import nonbonded_refs as nr

CASES = ["s65_C3", "s129_C3", "s513_C1", ms.MIXED]
TRAJ_STEPS = ms.TRAJ_STEPS
MODEL = "obc2"


def gb_for(batch, tag):
    """GBParameters of the batch's molecules, in order: random elements of gb_refs.ELEMENTS (keyed by `tag`) along the molecule's bonds"""
    rng = np.random.default_rng(sum(map(ord, tag)) * 6151 + 29)
    return [gr.GBParameters.from_elements(rng.choice(gr.ELEMENTS, size=mol["n"]), np.asarray(mol["idx"][0]).reshape(-1, 2)) for mol in batch.mols]


@functools.lru_cache(maxsize=None)
def _gb_of_case(name):
    return tuple(gb_for(ms.nve_batch() if name == "nve" else ms.case(name), name))


def gb_params(name):
    """the list of GBParameters of the case's molecules, in order ("nve": md_steps_refs.nve_batch)"""
    return list(_gb_of_case(name))


@contextlib.contextmanager
def gb_force(gbs, solvent=MODEL):
    """inside: relax_refs.forces (what md_refs.baoab_ref evaluates) adds the GB/SA energy and gradient of `gbs` to its nonbonded part (the
    solvent's energy is added to the total; the six terms stay the force field's)"""
    plain = nr.nb_ref

    def with_gb(params, x, dtype=torch.float64):
        nb, gb = plain(params, x, dtype), gr.gb_ref(params, gbs, x, solvent, dtype, scales=False)
        return dict(nb, energy=nb["energy"] + gb["energy"], grad=nb["grad"] + gb["grad"])

    nr.nb_ref = with_gb
    try:
        yield
    finally:
        nr.nb_ref = plain


def realisations(name, snapshots, **kw):
    """md_refs.fp32_realisations of the case in the solvent"""
    with gb_force(gb_params(name)):
        return md.fp32_realisations(ms.case(name), ms.masses(name), snapshots, **kw)


@functools.lru_cache(maxsize=None)
def verlet32(name, steps=max(TRAJ_STEPS)):
    """friction 0, 1 fs, from the case coordinates with thermal velocities, after TRAJ_STEPS.  Read-only."""
    return realisations(name, TRAJ_STEPS, velocities=ms.thermal_velocities(name), n_steps=steps)


def verlet(name):
    return {k: pair[1] for k, pair in verlet32(name)[0].items()}


def steady_counts():
    """md_steps_refs.steady_counts over CASES in the solvent"""
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
    """D = max over frames and items of |E_tot - E_tot at step 0| of the restatement in `dtype` in the solvent (md_steps_refs.NVE)"""
    b, m, v = ms.nve_batch(), ms.masses(ms.NVE_CASE), ms.thermal_velocities(ms.NVE_CASE)
    with gb_force(gb_params("nve")):
        start = md.baoab_ref(b, m, dtype, velocities=v, n_steps=0)
        r = md.baoab_ref(b, m, dtype, velocities=v, **ms.NVE)
    assert not r["status"].any()
    return md.drift(start["epot"] + start["ekin"], r["frame_epot"] + r["frame_ekin"])


# ---- one constrained case: md_steps_cons_refs' star clusters across the block border, in the solvent
CONS_CASE = "span64"


@functools.lru_cache(maxsize=None)
def cons_gb():
    import md_steps_cons_refs as msc
    return tuple(gb_for(msc.case(CONS_CASE)[0], CONS_CASE))


@functools.lru_cache(maxsize=None)
def cons_verlet():
    """-> (float64 restatement with snapshots, fp32 realisations) of CONS_CASE: friction 0, 2 fs, thermal velocities"""
    import md_cons_refs as mc
    import md_steps_cons_refs as msc
    batch, cons, m, _ = msc.case(CONS_CASE)
    kw = dict(velocities=msc.thermal_velocities(CONS_CASE), n_steps=max(msc.TRAJ_STEPS), dt=msc.TRAJ_DT)
    with gb_force(list(cons_gb())):
        return (mc.gbaoab_ref(batch, m, cons, torch.float64, snapshots=msc.TRAJ_STEPS, **kw), mc.fp32_realisations(batch, m, cons, msc.TRAJ_STEPS, **kw))
