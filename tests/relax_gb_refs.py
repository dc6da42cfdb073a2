"""The restatements of the stepwise minimiser in GB/SA implicit solvent (tests/test_host_relax_gb.py on the CPU,
tests/test_gpu_relax_gb.py): relax_refs.fire_ref run inside md_gb_refs.gb_force, so that the force of the loop is bonded +
nonbonded_refs.nb_ref + gb_refs.gb_ref (whose gradient is autograd of the restated energy), in float64 (the truth) and float32 (what
calibrates the trajectory bound), on cases of tests/relax_steps_refs.py with GB parameters from md_gb_refs.gb_for.

The cases are named by the sizes at which the kernels can go wrong (the i-block and the j-tile are 64 atoms): one atom short of a
block, a full block, one atom more, three blocks, nine tiles with a short last one, two conformation chunks per block, and the mixed
batch with a single atom in it.  The start coordinates are those of relax_steps_refs with the atoms of any pair that lies within
gb_refs.GAP_OTHER of a branch border of H nudged away (gb_refs.clear_borders): the branch a pair takes at the start must not depend on
the precision that judges it."""
import functools

import numpy as np
import torch

import gb_refs as gr
import md_gb_refs as mg
import relax_refs as rr
import relax_steps_refs as rs

MODEL = mg.MODEL
MIXED = rs.MIXED
TRAJ_CASES = ["s63_C3", "s64_C1", "s65_C3", "s129_C3", "s513_C1", "s9_65_C17", MIXED]
CONV_CASES = ["s65_C1", "s2_130_9_C3", "s513_C1"]
CONV_CPU_CASES = CONV_CASES[:2]          # (s513_C1 in float64 takes minutes on the CPU; on the GPU no float64 trajectory is needed)
CONV_MAX_STEPS = rs.CONV_MAX_STEPS
# The molecules of the convergence cases on which "the solvent minimum lies below the vacuum minimiser's coordinates, on the solvent
# surface" is asserted: FIRE is a local minimiser, so the ordering is a statement about one basin, and it is asserted where the float64
# restatement shows it with a margin (tests/test_host_relax_gb.py: more than 1 kcal/mol for every conformation).  The 2-atom molecule has
# no strain for the solvent to release (both runs end within 3e-5 kcal/mol of each other), and the 9-atom one ends in another basin than
# the vacuum run from the same start (which happens to be the lower one by 1 kcal/mol in two of three conformations): neither is listed.
# s513_C1 is not listed either: in float64 the solvent run meets the tolerance after 295 steps at -1317.9 kcal/mol, the vacuum run after 1120
# steps at coordinates that lie at -1346.9 on the solvent surface -- a deeper basin, reached by the longer walk.
ORDERED = {"s65_C1": (0,), "s2_130_9_C3": (1,)}
ORDER_MARGIN = 1.0
TAG = {}          # case -> the tag its GB elements are drawn by, where the case's own name gives no uphill step or too many thin margins


@functools.lru_cache(maxsize=None)
def gb_params_of(name):
    return tuple(mg.gb_for(rs.case(name), TAG.get(name, name)))


def gb_params(name):
    """the list of GBParameters of the case's molecules, in order"""
    return list(gb_params_of(name))


@functools.lru_cache(maxsize=None)
def case(name) -> rr.Batch:
    """relax_steps_refs.case(name) with its start coordinates cleared of branch borders.  Computed once and shared: treat as read-only"""
    b = rs.case(name)
    rng = np.random.default_rng(sum(map(ord, name)) * 4099 + 5)
    x = gr.clear_borders(gb_params(name), b.xyz, rng)
    mols, p = [], b.ptr
    for k, m in enumerate(b.mols):
        mols.append({**m, "xyz": x[int(p[k]):int(p[k + 1])].numpy().copy()})
    return rr.Batch(mols)


def forces(name, batch, x, dtype=torch.float64, scales=False):
    """relax_refs.forces of `batch` at x in the solvent of case `name`: E and G hold the solvent term, the six terms stay the force
    field's, and "solv" is the solvent restatement itself (energy (B,C), terms (2,B,C), grad).  scales: the gate's scales abs_e and
    abs_f have the solvent's own (gb_refs) added, as relax_refs.forces adds the nonbonded ones to the bonded ones"""
    gbs = gb_params(name) if isinstance(name, str) else list(name)
    with mg.gb_force(gbs, MODEL):
        r = rr.forces(batch, x, dtype, True)
    solv = gr.gb_ref(batch.params, gbs, x, MODEL, dtype, scales=scales)
    r = dict(r, solv=solv)
    if scales:
        r["abs_e"], r["abs_f"] = r["abs_e"] + solv["abs_e"].double(), r["abs_f"] + solv["abs_g"].double()
    return r


@functools.lru_cache(maxsize=None)
def forces_of(name, dtype=torch.float64):
    b = case(name)
    return forces(name, b, b.xyz, dtype, scales=dtype == torch.float64)


@functools.lru_cache(maxsize=None)
def trajectory(name, dtype=torch.float64):
    """tolerance 0, 40 steps, snapshots after relax_refs.TRAJ_STEPS, in the solvent"""
    with mg.gb_force(gb_params(name), MODEL):
        return rr.fire_ref(case(name), dtype, True, snapshots=rr.TRAJ_STEPS, tolerance=0.0, max_steps=max(rr.TRAJ_STEPS))


@functools.lru_cache(maxsize=None)
def converged(name):
    """the float64 restatement in the solvent with the default options and CONV_MAX_STEPS"""
    with mg.gb_force(gb_params(name), MODEL):
        return rr.fire_ref(case(name), torch.float64, True, max_steps=CONV_MAX_STEPS)


@functools.lru_cache(maxsize=None)
def converged_in_vacuum(name):
    """the same start relaxed on the vacuum surface (what `relax` without a solvent hands to `simulate` in one)"""
    return rr.fire_ref(case(name), torch.float64, True, max_steps=CONV_MAX_STEPS)


def margin_ok(name, max_steps):
    """(B, C) bool: |P| / (Fn vn) >= BRANCH_MARGIN in every compared loop iteration 1 .. max_steps - 1 of the float64 restatement"""
    b = case(name)
    ok = torch.ones(b.B, b.xyz.shape[1], dtype=torch.bool)
    for t in trajectory(name)["margin"][1:max_steps]:
        ok &= ~(t.abs() < rr.BRANCH_MARGIN)          # (nan: the item has stopped, a single atom)
    return ok


def has_uphill_step(name, max_steps=max(rr.TRAJ_STEPS)):
    return any(bool((p <= 0).any()) for p in trajectory(name)["P"][1:max_steps])
