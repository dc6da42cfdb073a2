"""CPU: the stepwise minimiser's front ends (grappa_amd/relax.py: `stepwise`, `check_every`) through a fake backend whose relax_steps
and relax_fire are the float64 restatement of tests/relax_refs.py, the new symbols, and the properties of the case table that
tests/test_gpu_relax_steps.py relies on: the branch margin, a step with P <= 0 in every trajectory case, and convergence in float64."""
import os
import re

import numpy as np
import pytest
import torch

import relax_refs as rr
import relax_steps_refs as rs
from grappa_amd import _lib, backend
from grappa_amd.nonbonded import NonbondedParameters
from grappa_amd.parameters import Parameters
from grappa_amd.relax import CHECK_EVERY_DEFAULT, RELAX_DEFAULTS, RelaxResult, graph_from_parameters, relax, relax_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeBackend:
    """relax_fire and relax_steps = the float64 restatement; records which one was called and with what"""
    limit = 40

    def __init__(self):
        self.calls = []

    def relax_max_atoms(self):
        return self.limit

    def _restate(self, which, plan, xyz, ks, eqs, n_per, nb, opts, xyz_out, energy, gmax, steps, status, counts, **extra):
        self.calls.append(dict(which=which, opts=dict(opts), nb=nb, counts=list(counts), **extra))
        params = None
        if nb is not None:
            ptr = np.concatenate([[0], np.cumsum(counts)])
            params = [NonbondedParameters(nb.charge[ptr[b]:ptr[b + 1]].numpy(), nb.sigma[ptr[b]:ptr[b + 1]].numpy(),
                                          nb.epsilon[ptr[b]:ptr[b + 1]].numpy(), *nb.exceptions_of(b)) for b in range(len(counts))]
        b = rr.Batch.from_tables(counts, [plan.idx32[lv].long() for lv in rr.LEVELS], [plan.mol_ptr[lv] for lv in rr.LEVELS], ks, eqs, n_per,
                                 params, xyz)
        r = rr.fire_ref(b, torch.float64, nb is not None, **opts)
        xyz_out.copy_(r["xyz"])
        f = rr.forces(b, r["xyz"], torch.float64, nb is not None)
        energy.copy_(f["E"]), gmax.copy_(r["gmax"]), steps.copy_(r["steps"]), status.copy_(r["status"])

    def relax_fire(self, plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, xyz_out, energy, gmax, steps, status, term_energy=None, grad=None,
                   atom_counts_host=None):
        self._restate("fire", plan, xyz, ks, eqs, n_per, nb, opts, xyz_out, energy, gmax, steps, status, list(atom_counts_host))

    def relax_steps(self, plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, xyz_out, energy, gmax, steps, status, term_energy=None, grad=None,
                    atom_counts_host=None, check_every=None, workspace=None):
        self._restate("steps", plan, xyz, ks, eqs, n_per, nb, opts, xyz_out, energy, gmax, steps, status, list(atom_counts_host),
                      check_every=check_every)


@pytest.fixture
def fake():
    old = backend._BACKEND
    be = FakeBackend()
    backend.set_backend(be)
    yield be
    backend.set_backend(old)


def _parameters(mol):
    ids = np.arange(mol["n"])
    mag = lambda k: np.abs(k).astype(np.float64)                                    # noqa: E731
    phase = lambda k: np.where(k >= 0, 0.0, np.pi)                                  # noqa: E731
    return Parameters(atoms=ids, bonds=mol["idx"][0], bond_k=mol["ks"][0].astype(np.float64), bond_eq=mol["eqs"][0].astype(np.float64),
                      angles=mol["idx"][1], angle_k=mol["ks"][1].astype(np.float64), angle_eq=mol["eqs"][1].astype(np.float64),
                      propers=mol["idx"][2], proper_ks=mag(mol["ks"][2]), proper_phases=phase(mol["ks"][2]), impropers=mol["idx"][3],
                      improper_ks=mag(mol["ks"][3]), improper_phases=phase(mol["ks"][3]))


def _small():
    mol = rr.case("n9_C3").mols[0]
    return mol, _parameters(mol), mol["xyz"].transpose(1, 0, 2)


def _big(n=41):          # one atom above the fake backend's limit
    mol = rr.gen_molecule(n, 1, np.random.default_rng(1))
    return mol, _parameters(mol), mol["xyz"].transpose(1, 0, 2)


def test_auto_takes_the_fused_kernel_within_the_limit_and_the_stepwise_path_above_it(fake):
    _, p, xyz = _small()
    relax(p, xyz, None, device="cpu", stepwise="auto", max_steps=3, tolerance=0.0)
    assert [c["which"] for c in fake.calls] == ["fire"]
    _, pb, xb = _big()
    r = relax(pb, xb, None, device="cpu", stepwise="auto", max_steps=3, tolerance=0.0)
    assert [c["which"] for c in fake.calls] == ["fire", "steps"] and fake.calls[-1]["counts"] == [41]
    assert fake.calls[-1]["check_every"] == CHECK_EVERY_DEFAULT == 32
    assert r.steps.tolist() == [3] and r.xyz.shape == xb.shape
    # a batch with one molecule above the limit goes stepwise as a whole: it is not split
    from grappa_amd.batch import batch
    g = batch([graph_from_parameters(p, xyz[:1]), graph_from_parameters(pb, xb)])
    relax_graph(g, None, stepwise="auto", max_steps=2, tolerance=0.0)
    assert fake.calls[-1]["which"] == "steps" and fake.calls[-1]["counts"] == [9, 41] and len(fake.calls) == 3


def test_stepwise_true_takes_the_stepwise_path_for_a_small_molecule(fake):
    mol, p, xyz = _small()
    r = relax(p, xyz, mol["nb"], device="cpu", stepwise=True, check_every=5, max_steps=7, tolerance=0.0)
    call = fake.calls[-1]
    assert [c["which"] for c in fake.calls] == ["steps"] and call["check_every"] == 5 and call["counts"] == [9]
    assert call["opts"] == {**RELAX_DEFAULTS, "max_steps": 7, "tolerance": 0.0}          # neither new parameter is a relaxation option
    # result shapes as today
    assert isinstance(r, RelaxResult) and r.xyz.shape == xyz.shape and r.xyz.dtype == np.float64
    assert r.energy.shape == r.gradient_max.shape == r.steps.shape == r.status.shape == (3,)
    assert r.steps.tolist() == [7, 7, 7] and r.status.tolist() == [0, 0, 0]
    from grappa_amd.batch import batch
    g = batch([graph_from_parameters(p, xyz), graph_from_parameters(p, xyz[::-1].copy())])
    x0 = g.nodes["n1"].data["xyz"].clone()
    rg = relax_graph(g, None, stepwise=True)
    assert rg.xyz.shape == (18, 3, 3) and rg.energy.shape == rg.gradient_max.shape == rg.steps.shape == rg.status.shape == (2, 3)
    assert torch.equal(g.nodes["n1"].data["xyz"], x0) and bool(rg.converged.all()) and fake.calls[-1]["which"] == "steps"


def test_stepwise_false_still_refuses_a_molecule_above_the_limit(fake):
    _, pb, xb = _big()
    for kw in ({}, {"stepwise": False}, {"stepwise": False, "check_every": 4}):
        with pytest.raises(ValueError, match="above the limit"):
            relax(pb, xb, None, device="cpu", **kw)
        with pytest.raises(ValueError, match="above the limit"):
            relax_graph(graph_from_parameters(pb, xb), None, **kw)
    assert not fake.calls, "a refused call reached the backend"


def test_bad_stepwise_parameters_are_refused(fake):
    _, p, xyz = _small()
    g = graph_from_parameters(p, xyz)
    for bad in (0, 2.5, -1):
        for sw in (False, True, "auto"):
            with pytest.raises(ValueError, match="check_every"):
                relax(p, xyz, None, device="cpu", stepwise=sw, check_every=bad)
            with pytest.raises(ValueError, match="check_every"):
                relax_graph(g, None, stepwise=sw, check_every=bad)
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="stepwise"):
            relax_graph(g, None, stepwise=bad)
    with pytest.raises(TypeError, match="unknown relaxation option"):
        relax_graph(g, None, stepwise=True, timestep=0.1)
    with pytest.raises(TypeError, match="unknown relaxation option"):
        relax(p, xyz, None, device="cpu", stepwise="auto", chunk=3)
    assert not fake.calls, "a refused call reached the backend"
    assert "stepwise" not in RELAX_DEFAULTS and "check_every" not in RELAX_DEFAULTS


def test_symbols_header_and_abi():
    names = {"grappa_relax_steps_workspace_bytes", "grappa_relax_steps_init_f32", "grappa_relax_steps_run_f32", "grappa_relax_steps_finish_f32"}
    assert names <= set(_lib.SIGNATURES)
    lib = _lib.load()          # binds every name of SIGNATURES: AttributeError for one that is not exported
    for n in names:
        assert getattr(lib, n) is not None
    text = open(os.path.join(ROOT, "include", "grappa_hip.h")).read()
    for n in names:
        assert re.search(r"\b" + n + r"\(", text), f"{n} is not declared in the header"
    assert lib.grappa_abi_version() == 11 == _lib.ABI_VERSION
    assert len(_lib.SIGNATURES["grappa_relax_steps_workspace_bytes"][1]) == 4
    assert len(_lib.SIGNATURES["grappa_relax_steps_run_f32"][1]) == len(_lib.SIGNATURES["grappa_relax_steps_init_f32"][1]) + 1
    # the option struct is the fused kernel's, unchanged
    assert [n for n, _ in _lib.RelaxOpts._fields_] == ["tolerance", "max_steps", "dt_start", "dt_max", "max_disp", "n_min", "f_inc", "f_dec",
                                                       "alpha_start", "f_alpha"]
    assert sorted(RELAX_DEFAULTS) == sorted(n for n, _ in _lib.RelaxOpts._fields_)
    assert len(_lib.SIGNATURES["grappa_relax_fire_f32"][1]) == 11 and _lib.relax_max_atoms() == 512
    # workspace bytes: nothing for an empty batch, growing with every argument
    w = lib.grappa_relax_steps_workspace_bytes
    assert w(0, 3, 1, 0) == 0 and w(10, 0, 1, 1) == 0 and w(10, 3, 0, 1) == 0
    assert 0 < w(65, 3, 1, 2) < w(6500, 3, 1, 102) and w(65, 3, 1, 2) < w(65, 17, 1, 2) and w(65, 3, 1, 2) <= w(65, 3, 9, 2)
    assert w(65, 3, 1, 2) >= 3 * 65 * 3 * 3 * 4          # x, v and g at the least


def test_branch_margin_of_the_trajectory_cases():
    """what the trajectory test of tests/test_gpu_relax_steps.py needs from its cases: at most a quarter of all conformations fall below
    |P| / (Fn vn) = 0.01 in a compared step, never all of one case, and every case has a step with P <= 0"""
    total = below = 0
    for name in rs.TRAJ_CASES:
        ok = rs.margin_ok(name, max(rr.TRAJ_STEPS))
        real = torch.tensor([n > 1 for n in rs.case(name).counts])[:, None].expand_as(ok)          # (a single atom has no trajectory)
        total += int(real.sum())
        below += int((~ok & real).sum())
        assert bool((ok & real).any()), f"{name}: every conformation is below the branch margin"
        assert rs.has_uphill_step(name), f"{name}: no step with P <= 0 among the compared steps"
        tr = rs.trajectory(name)
        assert bool((tr["steps"][real] == max(rr.TRAJ_STEPS)).all()) and bool((tr["status"][real] == 0).all())
    print(f"below the branch margin: {below} of {total} conformations")
    assert total == 63 and 4 * below <= total, (below, total)


def test_case_names_and_sizes():
    assert rs.parse("s9_65_C17") == ((9, 65), 17) and rs.name_of((1, 2, 17, 130, 5, 64), 3) == rs.MIXED
    assert rs.case(rs.MIXED).counts == [1, 2, 17, 130, 5, 64] and rs.case("s513_C1").counts == [_lib.relax_max_atoms() + 1]
    assert rs.n_blocks(rs.case(rs.MIXED)) == 1 + 1 + 1 + 3 + 1 + 1 and rs.n_blocks(rs.case("s64_C1")) == 1 and rs.n_blocks(rs.case("s65_C3")) == 2


@pytest.mark.parametrize("name", rs.CONV_CPU_CASES)
def test_convergence_cases_converge_in_float64(name):
    r = rs.converged(name)
    print(f"{name}: steps {r['steps'].flatten().tolist()}")
    assert bool((r["status"] == 1).all()), (r["status"].tolist(), r["steps"].tolist())
    assert bool((r["steps"] <= rs.CONV_MAX_STEPS).all()) and bool((r["gmax"] <= RELAX_DEFAULTS["tolerance"]).all())
    b = rs.case(name)
    e0, e1 = rr.forces(b, b.xyz)["E"], rr.forces(b, r["xyz"])["E"]
    assert bool((e1 <= e0).all())
