"""CPU: X-H constraints on the stepwise dynamics -- the new symbols, how grappa_amd/dynamics.py routes a constrained batch when the
backend has `md_steps_cons` and when it has not (recording fakes defined here), that P, S and the 4 x 4 elimination exist once, and the
condition that tests/test_gpu_md_steps_cons.py puts on its own inputs, decided from the restatement alone: every restated state finite
with status 0, no S of more than 2 updates, and at most one in ten (item, step count) pairs not steady (md_steps_refs.steady)."""
import os
import re

import numpy as np
import pytest
import torch

import md_cons_refs as mc
import md_steps_cons_refs as msc
import relax_refs as rr
from grappa_amd import _lib, backend
from grappa_amd.constraints import ConstraintBatch, Constraints
from grappa_amd.dynamics import simulate
from grappa_amd.nonbonded import Cutoff
from grappa_amd.parameters import Parameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"grappa_md_steps_cons_workspace_bytes", "grappa_md_steps_init_cons_f32", "grappa_md_steps_run_cons_f32",
         "grappa_md_steps_finish_cons_f32"}


class Fused:
    """a backend WITHOUT md_steps_cons: records which seam was called and with which keywords; the outputs stay as they were given"""
    limit = 40

    def __init__(self):
        self.calls = []

    def relax_max_atoms(self):
        return self.limit

    def _record(self, which, args, kw):
        self.calls.append(dict(which=which, opts=dict(args[7]), vel_in=args[10], **kw))

    def md_langevin(self, *a, **kw):
        self._record("fused", a, kw)

    def md_steps(self, *a, **kw):
        self._record("steps", a, kw)


class Both(Fused):
    """... and one WITH it"""

    def md_steps_cons(self, *a, **kw):
        self._record("steps_cons", a, kw)


@pytest.fixture(params=[Both, Fused], ids=["with_md_steps_cons", "without"])
def fake(request):
    old = backend._BACKEND
    be = request.param()
    backend.set_backend(be)
    yield be
    backend.set_backend(old)


def _parameters(mol):
    ids = np.arange(mol["n"])
    k3, k4 = mol["ks"][2].astype(np.float64), mol["ks"][3].astype(np.float64)
    return Parameters(atoms=ids, bonds=mol["idx"][0], bond_k=mol["ks"][0], bond_eq=mol["eqs"][0], angles=mol["idx"][1], angle_k=mol["ks"][1],
                      angle_eq=mol["eqs"][1], propers=mol["idx"][2], proper_ks=np.abs(k3), proper_phases=np.where(k3 >= 0, 0.0, np.pi),
                      impropers=mol["idx"][3], improper_ks=np.abs(k4), improper_phases=np.where(k4 >= 0, 0.0, np.pi))


def _mol(name):
    """the first molecule of a case -> (molecule, Parameters, xyz (C, n, 3), masses, Constraints)"""
    batch, cons, m, _ = msc.case(name)
    mol = batch.mols[0]
    return mol, _parameters(mol), mol["xyz"].transpose(1, 0, 2), m[:mol["n"]], cons[0]


REFUSAL = r"fused path only"


# ------------------------------------------------------------------------------------------------ the symbols
def test_symbols_header_and_signatures():
    assert NAMES <= set(_lib.SIGNATURES)
    lib = _lib.load()          # binds every name of SIGNATURES: AttributeError for one that is not exported
    text = open(os.path.join(ROOT, "include", "grappa_hip.h")).read()
    for n in NAMES:
        assert getattr(lib, n) is not None
        assert re.search(r"\b" + n + r"\(", text), f"{n} is not declared in the header"
    assert lib.grappa_abi_version() == 11 == _lib.ABI_VERSION
    sig = _lib.SIGNATURES
    # the _cut_ calls with the constraints added
    for call in ("init", "run", "finish"):
        assert len(sig[f"grappa_md_steps_{call}_cons_f32"][1]) == len(sig[f"grappa_md_steps_{call}_cut_f32"][1]) + 1
    assert len(sig["grappa_md_steps_cons_workspace_bytes"][1]) == 6
    # the header states the launches of a step, which tests/test_gpu_md_steps_cons.py counts
    assert re.search(r"a step is THREE launches, FOUR under a cutoff", text)
    # workspace: nothing for an empty batch or K < 0; K == 0: the workspace of the call forwarded to; K > 0: the claim and failure words more
    w, plain, cut = lib.grappa_md_steps_cons_workspace_bytes, lib.grappa_md_steps_workspace_bytes, lib.grappa_md_steps_cut_workspace_bytes
    assert w(0, 3, 1, 0, 1, 0) == 0 and w(10, 0, 1, 1, 1, 0) == 0 and w(10, 3, 0, 1, 1, 0) == 0 and w(65, 3, 1, 2, -1, 0) == 0
    assert w(65, 3, 1, 2, 0, 0) == plain(65, 3, 1, 2) and w(65, 3, 1, 2, 0, 1) == cut(65, 3, 1, 2)
    for with_cut, base in ((0, plain), (1, cut)):
        assert base(650, 3, 1, 12) + 4 * 650 + 4 * 12 * 3 <= w(650, 3, 1, 12, 5, with_cut) <= base(650, 3, 1, 12) + 4 * 650 + 4 * 12 * 3 + 512
    assert w(650, 3, 1, 12, 5, 0) == w(650, 3, 1, 12, 500, 0)          # any number of clusters
    # the host refuses before it touches the device (no GPU is needed for these): NULL descriptors, with and without constraints
    cons = _lib.MdCons(cluster_molptr=None, cluster_atoms=None, cluster_d=None, K=-1, tolerance=2.0 ** -19, constrain_start=1)
    import ctypes as C
    for c in (None, C.byref(cons)):
        assert lib.grappa_md_steps_init_cons_f32(None, None, None, None, None, c, None, None, None, None, 0, 0, None, 0) == -1
        assert lib.grappa_md_steps_run_cons_f32(None, None, None, None, None, c, None, None, None, 0, 0, None, 0, 0, 1, None, None, None) == -1
        assert lib.grappa_md_steps_finish_cons_f32(None, None, None, None, None, c, None, 0, 0, None, 0, None, None, None, None, None, None) == -1


def test_one_copy_of_the_projection_the_shake_and_the_elimination():
    """csrc/dynamics_cons.hip and csrc/dynamics_steps.hip include ONE P, ONE S and ONE 4 x 4 elimination: csrc/md_cons.h's"""
    src = lambda f: open(os.path.join(ROOT, "grappa_amd", "csrc", f)).read()      # noqa: E731
    files = [f for f in sorted(os.listdir(os.path.join(ROOT, "grappa_amd", "csrc"))) if f.endswith((".h", ".hip"))]
    defs = lambda name: [f for f in files if re.search(r"\b(float|V3|bool|int|void) " + name + r"\(", src(f))]      # noqa: E731
    for name in ("cons_project", "cons_shake", "cons_drift", "solve4"):
        assert defs(name) == ["md_cons.h"], (name, defs(name))
    assert [f for f in files if re.search(r"\bstruct Cluster\b", src(f))] == ["md_cons.h"]
    for f in ("dynamics_cons.hip", "dynamics_steps.hip"):
        assert '#include "md_cons.h"' in src(f) and "cons_project(" in src(f) and "cons_shake(" in src(f), f
    assert "md_cons.h" in src("Makefile")
    # the stepwise kernels are written without inline assembly
    assert "asm" not in re.sub(r"//.*", "", src("dynamics_steps.hip")) and "asm" not in re.sub(r"//.*", "", src("md_cons.h"))


# ------------------------------------------------------------------------------------------------ the front end
def test_stepwise_true_sends_the_constraints_down_the_stepwise_path(fake):
    _, p, xyz, m, cons = _mol("mix")
    kw = dict(device="cpu", stepwise=True, constraints=cons, n_steps=12, save_every=4, steps_per_launch=5, constrain_start=False,
              velocities=np.zeros_like(xyz))
    if isinstance(fake, Both):
        simulate(p, xyz, m, None, **kw)
        assert [c["which"] for c in fake.calls] == ["steps_cons"]
        call = fake.calls[0]
        assert isinstance(call["constraints"], ConstraintBatch) and call["constraints"].B == 1 and call["constrain_start"] is False
        assert int(call["constraints"].cluster_atoms.shape[0]) == cons.n_clusters
        assert call["steps_per_call"] == 4 and call["opts"]["n_steps"] == 12 and "cutoff" not in call
        fake.calls.clear()
        simulate(p, xyz, m, None, **{**kw, "constrain_start": True})
        assert fake.calls[0]["constrain_start"] is True
    else:
        with pytest.raises(ValueError, match=REFUSAL):
            simulate(p, xyz, m, None, **kw)
        assert not fake.calls, "a refused call reached the backend"


def test_auto_above_the_limit_goes_stepwise_with_the_constraints(fake):
    mol, p, xyz, m, cons = _mol("span64")
    assert mol["n"] > fake.limit
    if isinstance(fake, Both):
        simulate(p, xyz, m, mol["nb"], device="cpu", stepwise="auto", constraints=cons, n_steps=3)
        assert [c["which"] for c in fake.calls] == ["steps_cons"]
        assert fake.calls[0]["constraints"].B == 1 and fake.calls[0]["constrain_start"] is True and "cutoff" not in fake.calls[0]
    else:
        with pytest.raises(ValueError, match=REFUSAL):
            simulate(p, xyz, m, mol["nb"], device="cpu", stepwise="auto", constraints=cons, n_steps=3)
        assert not fake.calls
    fake.calls.clear()
    with pytest.raises(ValueError, match=r"above the limit of 40 atoms"):          # stepwise=False still refuses the size
        simulate(p, xyz, m, mol["nb"], device="cpu", constraints=cons, n_steps=3)
    assert not fake.calls


def test_auto_with_a_cutoff_goes_stepwise_with_the_constraints_and_the_cutoff(fake):
    mol, p, xyz, m, cons = _mol("mix")
    assert mol["n"] <= fake.limit
    for cutoff in (9.0, Cutoff(9.0, 7.2, 78.3)):
        fake.calls.clear()
        kw = dict(device="cpu", stepwise="auto", constraints=cons, cutoff=cutoff, n_steps=3)
        if isinstance(fake, Both):
            simulate(p, xyz, m, mol["nb"], **kw)
            assert [c["which"] for c in fake.calls] == ["steps_cons"]
            call = fake.calls[0]
            assert isinstance(call["cutoff"], Cutoff) and call["cutoff"].distance == 9.0 and call["constraints"].B == 1
            assert call["constrain_start"] is True
        else:
            with pytest.raises(ValueError, match=r"constraints run on the fused path only, a cutoff on the stepwise path only"):
                simulate(p, xyz, m, mol["nb"], **kw)
            assert not fake.calls
    fake.calls.clear()
    with pytest.raises(ValueError, match=r"a cutoff runs on the stepwise path only"):
        simulate(p, xyz, m, mol["nb"], device="cpu", constraints=cons, cutoff=9.0, n_steps=3)
    assert not fake.calls


def test_auto_within_the_limit_and_without_a_cutoff_stays_fused(fake):
    mol, p, xyz, m, cons = _mol("mix")
    simulate(p, xyz, m, mol["nb"], device="cpu", stepwise="auto", constraints=cons, n_steps=3)
    simulate(p, xyz, m, mol["nb"], device="cpu", constraints=cons, n_steps=3)
    assert [c["which"] for c in fake.calls] == ["fused", "fused"]
    assert all(isinstance(c["constraints"], ConstraintBatch) and c["constrain_start"] is True for c in fake.calls)


def test_without_constraints_the_calls_are_the_ones_made_without_the_keyword(fake):
    mol, p, xyz, m, _ = _mol("mix")
    for kw in (dict(stepwise=True), dict(stepwise="auto", cutoff=9.0), dict(stepwise="auto"), {}):
        fake.calls.clear()
        simulate(p, xyz, m, mol["nb"], device="cpu", n_steps=3, **kw)
        without = fake.calls[:]
        fake.calls.clear()
        simulate(p, xyz, m, mol["nb"], device="cpu", n_steps=3, constraints=None, **kw)
        assert len(fake.calls) == len(without) == 1
        a, b = fake.calls[0], without[0]
        assert a["which"] == b["which"] == ("fused" if kw in ({}, dict(stepwise="auto")) else "steps")
        assert sorted(a) == sorted(b) and "constraints" not in a and "constrain_start" not in a
        assert a["opts"] == b["opts"] and a.get("cutoff") == b.get("cutoff")


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
INPUTS = [(n, False) for n in msc.OWN] + [(n, True) for n in msc.CUT_CASES]


def test_the_inputs_of_the_gpu_tests_are_finite_quick_to_constrain_and_steady():
    """A condition on the inputs, not a measurement: every restated state is finite with status 0, no S needs more than 2 updates, and
    over all (item, step count) pairs of the cases at most one in ten is not steady (tests/test_gpu_md.py _gate_state), for x and for v
    -- the project's cap, as tests/test_host_md_steps.py applies it.  With these seeds, where this was written: 0 of 3 + 3 + 1 + 15
    items at 1 / 5 / 40 steps, and 0 of 3 + 1 under the cutoffs; the float32 restatement's rounding differs a little between CPUs."""
    total = {"x": [0, 0], "v": [0, 0]}
    for name, cut in INPUTS:
        batch = msc.case(name)[0]
        r = msc.verlet(name, cut)
        live = torch.tensor([n > 0 for n in batch.counts])
        assert not r["status"].any() and bool((r["steps"][live] == max(msc.TRAJ_STEPS)).all()), (name, cut)
        assert r["updates"] <= 2, f"{name}: an S took {r['updates']} updates"
        for real in msc.verlet32(name, cut):
            for k in msc.TRAJ_STEPS:
                for state in real[k]:
                    assert bool(torch.isfinite(state[0]).all()) and bool(torch.isfinite(state[1]).all()), (name, cut, k)
        n = msc.steady_counts(name, cut)
        print(f"{name}{' under its cutoff' if cut else ''}: not steady: x {n['x'][0]} of {n['x'][1]}, v {n['v'][0]} of {n['v'][1]} (item, step count) pairs")
        assert n["x"][1] == n["v"][1] == 3 * batch.B * batch.xyz.shape[1]
        for label in ("x", "v"):
            total[label][0] += n[label][0]
            total[label][1] += n[label][1]
    for label in ("x", "v"):
        assert total[label][1] == 3 * (3 + 3 + 1 + 15 + 3 + 1) and 10 * total[label][0] <= total[label][1], (label, total[label])


def test_the_cases_have_the_geometry_they_are_there_for():
    span = msc.blocks_of("span64")
    assert all(c == 0 for c, _ in span) and any(1 in lv for _, lv in span) and any(0 in lv for _, lv in span)
    assert msc.case("span64")[0].counts == [113] and len(span) == 21
    scat = msc.blocks_of("scattered130")
    assert msc.case("scattered130")[0].counts == [136] and len(scat) == 31
    assert any(c > min(lv) for c, lv in scat) and any(c < max(lv) for c, lv in scat)          # centres above and below their leaves
    batch, cons, _, _ = msc.case("k300")
    assert batch.counts == [600] and cons[0].n_clusters == 300 and 600 > 512 and 300 > 256
    # the heavy atoms fill blocks 0 .. 4 along the chain, the leaves blocks 5 .. 9: the molecule is longer than the cutoff by more than a
    # block of the chain spans, and whole blocks lie farther apart than the cutoff, so tiles are really skipped
    x = batch.xyz[:, 0].double()
    extent = float((x.max(0).values - x.min(0).values).max())
    span_of_a_block = max(float((x[k:k + 64].max(0).values - x[k:k + 64].min(0).values).norm()) for k in range(0, 256, 64))
    rc = msc.cutoff("k300").distance
    assert extent > rc + span_of_a_block, (extent, span_of_a_block)
    assert float(torch.cdist(x[0:64], x[192:256]).min()) > rc and float(torch.cdist(x[320:384], x[512:576]).min()) > rc
    batch, cons, _, _ = msc.case("mixed")
    assert batch.counts == [2, 7, 0, 67, 5] and [None if c is None else c.n_clusters for c in cons][1:3] == [None, None]
    assert batch.xyz.shape[1] == 3
    # every atom in at most one cluster, any order of the table: what the device vets
    for name in msc.OWN:
        for c in msc.case(name)[1]:
            if c is not None:
                used = c.clusters[c.clusters >= 0]
                assert used.size == np.unique(used).size
