"""CPU: the nonbonded cutoff on the minimiser's front ends (`relax_graph`, `relax`, `Grappa.relax`, `torsion_scan` and the signature of
`HipBackend.relax_steps`) through the recording fake of tests/test_host_relax_steps.py, the new symbols, and the conditions
tests/test_gpu_relax_cut.py puts on its own inputs, decided from the restatement of tests/relax_cut_refs.py alone."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import relax_cut_refs as rc
import relax_refs as rr
import relax_steps_refs as rs
from grappa_amd import _lib, backend
from grappa_amd.nonbonded import Cutoff, NonbondedBatch
from grappa_amd.relax import RELAX_DEFAULTS, graph_from_parameters, relax, relax_graph, torsion_scan
from test_host_relax_steps import FakeBackend, _big, _small

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"grappa_relax_steps_cut_workspace_bytes", "grappa_relax_steps_init_cut_f32", "grappa_relax_steps_run_cut_f32",
         "grappa_relax_steps_finish_cut_f32"}


# ------------------------------------------------------------------------------------------------ front ends
class CutFake(FakeBackend):
    """the recording fake of tests/test_host_relax_steps.py whose relax_steps also takes (and records) a cutoff"""

    def relax_steps(self, *args, cutoff=None, **kw):
        super().relax_steps(*args, **kw)
        self.calls[-1]["cutoff"] = cutoff


@pytest.fixture
def fake():
    old = backend._BACKEND
    be = CutFake()
    backend.set_backend(be)
    yield be
    backend.set_backend(old)


@pytest.fixture
def strict():          # the fake of the existing host tests as it stands: its relax_steps does not know the keyword
    old = backend._BACKEND
    be = FakeBackend()
    backend.set_backend(be)
    yield be
    backend.set_backend(old)


def _wrapper(p):
    """a Grappa that predicts `p` on the CPU without a model"""
    from grappa_amd.grappa import Grappa
    w = object.__new__(Grappa)
    w.device = "cpu"
    w.predict = lambda molecule: p
    return w


OPTS = dict(max_steps=2, tolerance=0.0)


def test_auto_with_a_cutoff_goes_stepwise_whatever_the_size(fake):
    mol, p, xyz = _small()
    relax(p, xyz, mol["nb"], device="cpu", stepwise="auto", cutoff=9.0, **OPTS)
    assert [c["which"] for c in fake.calls] == ["steps"] and fake.calls[-1]["cutoff"] == Cutoff(9.0)
    assert fake.calls[-1]["opts"] == {**RELAX_DEFAULTS, **OPTS}          # the cutoff is no relaxation option
    relax(p, xyz, mol["nb"], device="cpu", stepwise=True, cutoff=Cutoff(9.0, 7.2, 1.0), **OPTS)
    assert fake.calls[-1]["which"] == "steps" and fake.calls[-1]["cutoff"] == Cutoff(9.0, 7.2, 1.0)
    g = graph_from_parameters(p, xyz)
    relax_graph(g, NonbondedBatch([mol["nb"]]), stepwise="auto", cutoff=6.0, check_every=5, **OPTS)
    assert fake.calls[-1]["which"] == "steps" and fake.calls[-1]["cutoff"] == Cutoff(6.0) and fake.calls[-1]["check_every"] == 5
    r = _wrapper(p).relax(None, xyz, mol["nb"], stepwise="auto", cutoff=Cutoff(8.0, prune=False), **OPTS)
    assert fake.calls[-1]["which"] == "steps" and fake.calls[-1]["cutoff"] == Cutoff(8.0, prune=False) and len(fake.calls) == 4
    assert r.xyz.shape == xyz.shape and r.steps.tolist() == [2, 2, 2]


def test_without_a_cutoff_the_calls_are_todays(strict):
    mol, p, xyz = _small()
    relax(p, xyz, mol["nb"], device="cpu", stepwise="auto", **OPTS)
    relax(p, xyz, mol["nb"], device="cpu", stepwise=True, cutoff=None, **OPTS)
    _, pb, xb = _big()
    relax(pb, xb, None, device="cpu", stepwise="auto", cutoff=None, **OPTS)
    relax_graph(graph_from_parameters(p, xyz), NonbondedBatch([mol["nb"]]), stepwise=True, cutoff=None, **OPTS)
    w = _wrapper(p)
    w.relax(None, xyz, mol["nb"], stepwise=True, **OPTS)
    w.relax(None, xyz, mol["nb"], stepwise=True, cutoff=None, **OPTS)
    w.relax(None, xyz, mol["nb"], **OPTS)
    assert [c["which"] for c in strict.calls] == ["fire", "steps", "steps", "steps", "steps", "steps", "fire"]
    assert all("cutoff" not in c for c in strict.calls)
    assert inspect.signature(type(strict).relax_steps).parameters.get("cutoff") is None


def test_front_end_refusals(fake):
    mol, p, xyz = _small()
    g = graph_from_parameters(p, xyz)
    nbb = NonbondedBatch([mol["nb"]])
    w = _wrapper(p)
    for kw in ({}, {"stepwise": False}):
        with pytest.raises(ValueError, match=r'stepwise="auto"'):
            relax(p, xyz, mol["nb"], device="cpu", cutoff=9.0, **kw)
        with pytest.raises(ValueError, match=r'stepwise="auto"'):
            relax_graph(g, nbb, cutoff=9.0, **kw)
        with pytest.raises(ValueError, match=r'stepwise="auto"'):
            w.relax(None, xyz, mol["nb"], cutoff=9.0, **kw)
    with pytest.raises(ValueError, match="needs the nonbonded parameters"):
        relax(p, xyz, None, device="cpu", stepwise="auto", cutoff=9.0)
    with pytest.raises(ValueError, match="needs the nonbonded parameters"):
        relax_graph(g, None, stepwise="auto", cutoff=9.0)
    with pytest.raises(ValueError, match="needs the nonbonded parameters"):
        w.relax(None, xyz, None, stepwise="auto", cutoff=9.0)
    with pytest.raises(ValueError, match="distance"):
        relax(p, xyz, mol["nb"], device="cpu", stepwise="auto", cutoff=-3.0)
    with pytest.raises(ValueError, match="distance"):
        relax_graph(g, nbb, stepwise="auto", cutoff=float("nan"))
    from grappa_amd.restraints import RestraintBatch, Restraints
    restr = Restraints(position_k=np.ones(9))
    with pytest.raises(ValueError, match="restraints are taken by the fused minimiser only"):
        relax(p, xyz, mol["nb"], device="cpu", stepwise="auto", cutoff=9.0, restraints=restr)
    with pytest.raises(ValueError, match="restraints are taken by the fused minimiser only"):
        relax_graph(g, nbb, stepwise="auto", cutoff=9.0, restraints=RestraintBatch([restr], 3, atom_counts=[9]))
    with pytest.raises(ValueError, match="takes no cutoff"):
        torsion_scan(p, xyz[0], [0, 1, 2, 4], angles=[0.0, 1.0], nonbonded=mol["nb"], device="cpu", cutoff=9.0)
    with pytest.raises(ValueError, match="takes no cutoff"):
        w.torsion_scan(None, xyz[0], [0, 1, 2, 4], angles=[0.0, 1.0], nonbonded=mol["nb"], cutoff=Cutoff(9.0))
    assert not fake.calls, "a refused call reached the backend"
    assert "cutoff" not in RELAX_DEFAULTS


def test_the_backend_seam_takes_a_cutoff_after_the_workspace():
    from grappa_amd.backend import HipBackend
    par = inspect.signature(HipBackend.relax_steps).parameters
    assert par["cutoff"].default is None and list(par)[-2:] == ["workspace", "cutoff"]
    doc = HipBackend.relax_steps.__doc__
    assert "grappa_relax_steps_cut_workspace_bytes" in doc and "four launches" in doc


def test_symbols_header_and_abi():
    assert NAMES <= set(_lib.SIGNATURES)
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "grappa_hip.h")).read()
    for n in NAMES:
        assert getattr(lib, n) is not None and re.search(r"\b" + n + r"\(", text), n
    assert lib.grappa_abi_version() == 11 == _lib.ABI_VERSION
    sig = _lib.SIGNATURES
    for n in ("init", "run", "finish"):          # the existing argument lists with `cut` after nb
        old, new = sig[f"grappa_relax_steps_{n}_f32"][1], sig[f"grappa_relax_steps_{n}_cut_f32"][1]
        assert len(new) == len(old) + 1 and new[:3] == old[:3] and new[4:] == old[3:] and new[3] == C.POINTER(_lib.NbCut)
    # the plain size plus the boxes, the ranges and the workspace of the cut energy entry, each piece on a 256-byte boundary
    w, wc, wn = lib.grappa_relax_steps_workspace_bytes, lib.grappa_relax_steps_cut_workspace_bytes, lib.grappa_nonbonded_cut_workspace_bytes
    up = lambda n: (n + 255) // 256 * 256      # noqa: E731
    for N, Cc, B, nblk in ((65, 3, 1, 2), (6500, 1, 1, 102), (74, 17, 2, 3)):
        assert wc(N, Cc, B, nblk) == w(N, Cc, B, nblk) + up(32 * nblk * Cc) + up(8 * nblk) + up(wn(Cc, nblk)), (N, Cc, B, nblk)
    assert wc(0, 3, 1, 0) == 0 and wc(10, 0, 1, 1) == 0 and wc(10, 3, 0, 1) == 0
    # the host refuses before it touches the device
    cut = _lib.NbCut(cutoff=9.0, switch_distance=0.0, rf_dielectric=78.3, prune=1)
    assert lib.grappa_relax_steps_init_cut_f32(None, None, None, C.byref(cut), None, None, 0, 0, None, 0, None) == -1          # a cut without nb
    assert lib.grappa_relax_steps_init_cut_f32(None, None, None, None, None, None, 0, 0, None, 0, None) == -1                  # forwards: NULL mm
    assert lib.grappa_relax_steps_run_cut_f32(None, None, None, C.byref(cut), None, None, 0, 0, None, 0, 1, None) == -1
    assert lib.grappa_relax_steps_finish_cut_f32(None, None, None, C.byref(cut), None, None, 0, 0, None, 0, None, None, None, None, None, None,
                                                 None) == -1


def test_one_definition_of_the_cut_carrier_and_of_the_box_launch():
    src = lambda f: open(os.path.join(ROOT, "grappa_amd", "csrc", f)).read()      # noqa: E731
    files = [f for f in sorted(os.listdir(os.path.join(ROOT, "grappa_amd", "csrc"))) if f.endswith((".h", ".hip"))]
    assert [f for f in files if re.search(r"\bstruct RsCut\b", src(f))] == ["rs_force.h"]
    assert [f for f in files if re.search(r"\bbool rs_cut_make\(", src(f))] == ["rs_force.h"]
    # the body nb_cut_box_range stands behind two kernels: the energy entry's and the one the two stepwise paths share
    assert [f for f in files if re.search(r"__global__[^;{]*_box_kernel\(", src(f))] == ["nonbonded.hip", "rs_force.h"]
    for f in ("relax_steps.hip", "dynamics_steps.hip"):
        assert "rs_box_kernel" in src(f) and "rs_cut_make" in src(f)


# ------------------------------------------------------------------------------------------------ conditions on the GPU inputs
def test_case_tables():
    assert set(rc.TRAJ_CASES) <= set(rs.TRAJ_CASES) | {"s9_65_C17"} and rc.CONV_CASES == rs.CONV_CASES and rc.MIXED in rc.TRAJ_CASES
    for name in rc.TRAJ_CASES + rc.CONV_CASES:
        cut = rc.cutoff(name)
        assert abs(cut.distance - 9.0) <= 0.051 and cut.switch_distance == 0.8 * cut.distance and cut.rf_dielectric == 78.3 and cut.prune
        assert not rc.cutoff(name, False).prune and rc.cutoff(name, False).distance == cut.distance


@pytest.mark.parametrize("name", rc.TRAJ_CASES)
def test_the_restated_trajectories_are_finite_and_go_uphill_once(name):
    """every restated state is finite, every item with more than one atom runs all 40 steps, and a step with P <= 0 occurs within them"""
    b = rs.case(name)
    real = torch.tensor([n > 1 for n in b.counts])[:, None].expand(b.B, b.xyz.shape[1])
    worst = 0.0
    for dtype in (torch.float64, torch.float32):
        tr = rc.trajectory(name, dtype)
        assert sorted(tr["snap"]) == list(rc.TRAJ_STEPS)
        assert all(bool(torch.isfinite(x).all()) for x in tr["snap"].values()) and bool(torch.isfinite(tr["xyz"]).all())
        assert bool((tr["steps"][real] == max(rc.TRAJ_STEPS)).all()) and bool((tr["status"][real] == 0).all())
    for k in rc.TRAJ_STEPS:
        worst = max(worst, float((rc.trajectory(name, torch.float32)["snap"][k].double() - rc.trajectory(name)["snap"][k]).abs().max()))
    print(f"{name}: largest |x_fp32 - x_f64| over the snapshots {worst:.3e} A")
    assert rc.has_uphill_step(name), f"{name}: no step with P <= 0 within 40 steps"
    # the cutoff is part of the force: the trajectory is not the all-pairs one (where every pair lies within rc it would be, bar the
    # reaction field, which eps = 78.3 keeps)
    assert not torch.equal(rc.trajectory(name)["snap"][5], rs.trajectory(name)["snap"][5])


def test_branch_margin_of_the_trajectory_cases():
    """at most one in ten (item, step count) pairs loses the branch margin, and no case loses all of its items"""
    total = below = 0
    per_step = {}
    for name in rc.TRAJ_CASES:
        real = torch.tensor([n > 1 for n in rs.case(name).counts])[:, None]
        for k in rc.TRAJ_STEPS:
            ok = rc.margin_ok(name, k)
            r = real.expand_as(ok)
            total += int(r.sum())
            below += int((~ok & r).sum())
            n = per_step.setdefault(k, [0, 0])
            n[0] += int((~ok & r).sum())
            n[1] += int(r.sum())
            assert bool((ok & r).any()), f"{name}, {k} steps: every conformation is below the branch margin"
    print(f"below the branch margin: {below} of {total} (item, step count) pairs; per step count {per_step}")
    assert total == 180 and 10 * below <= total, (below, total)


@pytest.mark.parametrize("name", rc.CONV_CPU_CASES)
def test_convergence_cases_converge_in_float64(name):
    r = rc.converged(name)
    print(f"{name}: steps {r['steps'].flatten().tolist()}")
    assert bool((r["status"] == 1).all()), (r["status"].tolist(), r["steps"].tolist())
    assert bool((r["steps"] <= rc.CONV_MAX_STEPS).all()) and bool((r["gmax"] <= RELAX_DEFAULTS["tolerance"]).all())
    e0, e1 = rc.forces_of(name)["E"], rc.forces_at(name, r["xyz"])["E"]
    assert bool((e1 <= e0).all())
