"""The case table of the stepwise minimiser's tests (tests/test_host_relax_steps.py on the CPU, tests/test_gpu_relax_steps.py): molecules
around the i-block of 64 atoms and above the fused kernel's 512, built by relax_refs.gen_molecule and run through relax_refs.fire_ref,
the float64 (the truth) and float32 (what calibrates the trajectory bound) restatement of the loop of include/grappa_hip.h.

A case is named "s" + its molecule sizes joined by "_" + "_C" + its conformations, and seeded from the name alone."""
import functools

import numpy as np
import torch

import relax_refs as rr

# the i-block edge; three blocks (the cross-block reduction); the first sizes the fused kernel refuses; more than 16 conformations
# (two conformation chunks per block); mixed
TRAJ_CASES = ["s63_C3", "s64_C1", "s65_C3", "s129_C3", "s513_C1", "s513_C3", "s9_65_C17", "s1_2_17_130_5_64_C3"]
CONV_CASES = ["s65_C1", "s2_130_9_C3", "s513_C1"]
CONV_CPU_CASES = CONV_CASES[:2]          # (s513_C1 takes 14 s in float64; on the GPU no float64 trajectory is needed)
CONV_MAX_STEPS = 3000
MIXED = "s1_2_17_130_5_64_C3"


def name_of(sizes, C) -> str:
    return "s" + "_".join(str(n) for n in sizes) + f"_C{C}"


def parse(name):
    """-> (sizes, C)"""
    body, c = name[1:].rsplit("_C", 1)
    return tuple(int(n) for n in body.split("_")), int(c)


@functools.lru_cache(maxsize=None)
def case(name) -> rr.Batch:
    """computed once and shared: treat as read-only"""
    sizes, C = parse(name)
    assert name_of(sizes, C) == name
    rng = np.random.default_rng(sum(map(ord, name)) * 7919 + C)
    return rr.Batch([rr.gen_molecule(n, C, rng) for n in sizes])


@functools.lru_cache(maxsize=None)
def unbonded(name) -> rr.Batch:
    """case(name) without its bonded tuples (T = 0 at every level): the coordinates and the nonbonded parameters, exceptions included,
    stay, so the force of the stepwise paths is the nonbonded term alone.  Computed once and shared: treat as read-only"""
    b = case(name)
    idx = [torch.zeros(0, a, dtype=torch.int64) for a in rr.ARITY]
    mol_ptr = [torch.zeros(b.B + 1, dtype=torch.int32) for _ in rr.ARITY]
    return rr.Batch.from_tables(b.counts, idx, mol_ptr, [k[:0] for k in b.ks], [None if q is None else q[:0] for q in b.eqs], b.n_per,
                                b.params, b.xyz)


@functools.lru_cache(maxsize=None)
def forces_of(name, dtype=torch.float64):
    b = case(name)
    return rr.forces(b, b.xyz, dtype, True)


@functools.lru_cache(maxsize=None)
def trajectory(name, dtype=torch.float64):
    """tolerance 0, 40 steps, snapshots after relax_refs.TRAJ_STEPS"""
    return rr.fire_ref(case(name), dtype, True, snapshots=rr.TRAJ_STEPS, tolerance=0.0, max_steps=max(rr.TRAJ_STEPS))


@functools.lru_cache(maxsize=None)
def converged(name):
    """the float64 restatement with the default options and CONV_MAX_STEPS"""
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


def n_blocks(batch) -> int:
    """i-blocks of the nonbonded plan for the batch's molecules"""
    from grappa_amd import _lib
    t = _lib.load().grappa_nonbonded_iblock()
    return sum((n + t - 1) // t for n in batch.counts)
