"""The inputs and restatements of the stepwise dynamics' tests (tests/test_host_md_steps.py on the CPU, tests/test_gpu_md_steps.py): the
trajectory cases of tests/relax_steps_refs.py -- molecules around the i-block of 64 atoms and above the fused kernel's 512 -- with
masses, keys and 300 K velocities generated the way tests/md_refs.py generates them for its own cases, and the float64 / fp32
restatements of the loop (md_refs.baoab_ref, which works at any molecule size) with their rotated siblings, computed once and shared.

The yardstick is the float64 restatement, as for the fused kernel; the gate and the sense of "steady" are those of
tests/test_gpu_md.py (_gate_state), restated in `steady` so that the CPU test can decide from the restatement alone whether the gate
is calibrated by the unturned fp32 run on (nearly) all items."""
import functools

import numpy as np
import torch

import md_refs as md
import relax_steps_refs as rs
from grappa_amd import constants

TRAJ_CASES = rs.TRAJ_CASES
TRAJ_STEPS = md.TRAJ_STEPS          # 1, 5, 40
MIXED = rs.MIXED
NVE_CASE = "s2_130_9_C3"
NVE = dict(dt=0.0005, friction=0.0, n_steps=400, save_every=50)
TRAJ_FACTOR, ULP_X = 4, 2.0 ** -20          # the gate of tests/test_gpu_md.py


def case(name) -> "rs.rr.Batch":
    return rs.case(name)


@functools.lru_cache(maxsize=None)
def masses(name) -> np.ndarray:
    """(N,) float32 in amu: atomic numbers drawn from {1, 6, 7, 8}"""
    rng = np.random.default_rng(sum(map(ord, name)) * 104729 + 17)
    z = rng.choice([1, 6, 7, 8], size=case(name).N)
    return np.array([constants.ATOMIC_MASSES[int(a)] for a in z], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def keys(name) -> np.ndarray:
    from grappa_amd.dynamics import mol_keys
    return mol_keys(sum(map(ord, name)), case(name).B)


@functools.lru_cache(maxsize=None)
def thermal_velocities(name, temperature=300.0) -> torch.Tensor:
    """(N, C, 3) float32: sqrt(ACC kB T / m) times normal deviates of the case's own rng"""
    b = case(name)
    rng = np.random.default_rng(sum(map(ord, name)) * 15485863 + 3)
    s = np.sqrt(md.ACC * md.KB * temperature / masses(name).astype(np.float64))
    return torch.from_numpy((s[:, None, None] * rng.standard_normal((b.N, b.xyz.shape[1], 3))).astype(np.float32))


@functools.lru_cache(maxsize=None)
def verlet32(name, steps=max(TRAJ_STEPS)):
    """friction 0, 1 fs, from the case coordinates with thermal_velocities: md_refs.fp32_realisations after TRAJ_STEPS (the input as it is,
    then its rotations; each entry {k: (fp32 (xyz, vel), float64 (xyz, vel))}).  Read-only."""
    return md.fp32_realisations(case(name), masses(name), TRAJ_STEPS, velocities=thermal_velocities(name), n_steps=steps)


def verlet(name):
    """the float64 restatement of the unturned input: {k: (xyz, vel)}"""
    return {k: pair[1] for k, pair in verlet32(name)[0].items()}


def item_max(batch, t):
    """(N, C, 3) -> (B, C): the largest row norm of each (molecule, conformation); 0 for a molecule without atoms"""
    C = t.shape[1]
    return torch.stack([t[int(batch.ptr[k]):int(batch.ptr[k + 1])].double().norm(dim=-1).max(0).values if batch.counts[k] else torch.zeros(C, dtype=torch.float64)
                        for k in range(batch.B)])


def steady(batch, r32s, idx):
    """(B, C) bool, in the sense of test_gpu_md._gate_state: all rotated fp32 siblings lie within TRAJ_FACTOR x the unturned fp32 run's
    distance to float64 + the floor.  r32s: the realisations at one step count; idx 0: x, 1: v"""
    each = torch.stack([item_max(batch, r32[idx].double() - own64[idx]) for r32, own64 in r32s])
    floor = ULP_X * (1.0 if idx == 0 else item_max(batch, r32s[0][1][idx]))
    return (each[1:] <= TRAJ_FACTOR * each[0] + floor).all(0)


def steady_counts(names=TRAJ_CASES):
    """-> {"x": (non-steady, pairs), "v": ..., "worst": {label: (case, steps, non-steady, items)}} over all (item, step count) pairs"""
    out = {"x": [0, 0], "v": [0, 0], "worst": {}}
    for name in names:
        b = case(name)
        for k in TRAJ_STEPS:
            r32s = [r[k] for r in verlet32(name)]
            for label, idx in (("x", 0), ("v", 1)):
                s = steady(b, r32s, idx)
                out[label][0] += int((~s).sum())
                out[label][1] += s.numel()
                w = out["worst"].get(label)
                if w is None or int((~s).sum()) * w[3] > w[2] * s.numel():
                    out["worst"][label] = (name, k, int((~s).sum()), s.numel())
    return out


# energy conservation: s2_130_9_C3 from its relaxed coordinates
@functools.lru_cache(maxsize=None)
def nve_batch():
    b = rs.case(NVE_CASE)
    x = rs.converged(NVE_CASE)["xyz"].float().numpy()
    mols, p = [], 0
    for mol in b.mols:
        mols.append(dict(mol, xyz=np.ascontiguousarray(x[p:p + mol["n"]])))
        p += mol["n"]
    return rs.rr.Batch(mols)


@functools.lru_cache(maxsize=None)
def nve_drift(dtype):
    """D = max over frames and items of |E_tot - E_tot at step 0| of the restatement in `dtype`"""
    b, m, v = nve_batch(), masses(NVE_CASE), thermal_velocities(NVE_CASE)
    start = md.baoab_ref(b, m, dtype, velocities=v, n_steps=0)
    r = md.baoab_ref(b, m, dtype, velocities=v, **NVE)
    assert not r["status"].any()
    return md.drift(start["epot"] + start["ekin"], r["frame_epot"] + r["frame_ekin"])
