"""The restatements of the stepwise minimiser under a nonbonded cutoff (tests/test_host_relax_cut.py on the CPU,
tests/test_gpu_relax_cut.py): relax_refs.fire_ref with the force replaced by bonded + nb_cut_refs.nb_cut_ref
(md_cut_refs.cut_force), on cases of tests/relax_steps_refs.py.  The cutoff is md_cut_refs.cutoff's: 9 A nominal, placed by
nb_cut_refs.place_cutoff on the start coordinates, with a switch from 0.8 rc and eps = 78.3, so that a pair which crosses rc during a
run -- float64 and fp32 may see it a step apart -- moves the force by a negligible amount.

float64 is the truth, float32 the yardstick that calibrates the trajectory gate; both are computed once and shared: read-only."""
import functools

import torch

import md_cut_refs as mc
import relax_refs as rr
import relax_steps_refs as rs

# the block edge; three blocks; above the fused limit (25 of 81 tiles at the start); five conformation chunks per block (the box index
# c0 + cl); mixed
TRAJ_CASES = ["s63_C3", "s64_C1", "s65_C3", "s129_C3", "s513_C1", "s9_65_C17", rs.MIXED]
CONV_CASES = ["s65_C1", "s2_130_9_C3", "s513_C1"]
CONV_CPU_CASES = CONV_CASES[:2]          # (on the GPU no float64 trajectory is needed)
CONV_MAX_STEPS = rs.CONV_MAX_STEPS
TRAJ_STEPS = rr.TRAJ_STEPS
MIXED = rs.MIXED


def cutoff(name, prune=True):
    return mc.cutoff(name, prune)


def forces_at(name, x, dtype=torch.float64):
    """relax_refs.forces of the case at x (N, C, 3) under the case's cutoff"""
    with mc.cut_force(cutoff(name)):
        return rr.forces(rs.case(name), x, dtype, True)


@functools.lru_cache(maxsize=None)
def forces_of(name, dtype=torch.float64):
    return forces_at(name, rs.case(name).xyz, dtype)


@functools.lru_cache(maxsize=None)
def trajectory(name, dtype=torch.float64):
    """tolerance 0, 40 steps, snapshots after TRAJ_STEPS"""
    with mc.cut_force(cutoff(name)):
        return rr.fire_ref(rs.case(name), dtype, True, snapshots=TRAJ_STEPS, tolerance=0.0, max_steps=max(TRAJ_STEPS))


@functools.lru_cache(maxsize=None)
def converged(name):
    """the float64 restatement with the default options and CONV_MAX_STEPS"""
    with mc.cut_force(cutoff(name)):
        return rr.fire_ref(rs.case(name), torch.float64, True, max_steps=CONV_MAX_STEPS)


def margin_ok(name, max_steps):
    """relax_steps_refs.margin_ok on the trajectory under the cutoff: (B, C) bool, |P| / (Fn vn) >= BRANCH_MARGIN in every compared loop
    iteration 1 .. max_steps - 1 of the float64 restatement"""
    b = rs.case(name)
    ok = torch.ones(b.B, b.xyz.shape[1], dtype=torch.bool)
    for t in trajectory(name)["margin"][1:max_steps]:
        ok &= ~(t.abs() < rr.BRANCH_MARGIN)          # (nan: the item has stopped, a single atom)
    return ok


def has_uphill_step(name, max_steps=max(TRAJ_STEPS)):
    return any(bool((p <= 0).any()) for p in trajectory(name)["P"][1:max_steps])
