"""CPU: how grappa_amd/dynamics.py hands constraints to the backend seam, against a recording fake of `HipBackend.md_langevin` defined
here (tests/conftest.py's backend is not involved): what is refused, which launch gets constrain_start, the temperature's divisor, and
that constraints=None makes exactly the call made without the keyword."""
import numpy as np
import pytest
import torch

import md_cons_refs as mc
from grappa_amd import backend
from grappa_amd.constraints import ConstraintBatch, Constraints
from grappa_amd.dynamics import KB, simulate, simulate_graph
from grappa_amd.parameters import Parameters
from grappa_amd.relax import graph_from_parameters

EKIN = 7.5


class Recorder:
    """md_langevin records its arguments and returns the start with a fixed kinetic energy; md_steps must not be reached"""
    limit = 40

    def __init__(self):
        self.calls = []

    def relax_max_atoms(self):
        return self.limit

    def md_langevin(self, plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, mass, mol_key, vel_in, xyz_out, vel_out, epot, ekin, steps, status,
                    **kw):
        self.calls.append(dict(opts=dict(opts), xyz=xyz.clone(), vel_in=None if vel_in is None else vel_in.clone(), mass=mass.clone(),
                               key=mol_key.clone(), kw={k: v for k, v in kw.items() if k not in ("frames_xyz", "frames_epot", "frames_ekin")}))
        xyz_out.copy_(xyz)
        vel_out.zero_()
        epot.zero_()
        ekin.fill_(EKIN)
        steps.fill_(opts["n_steps"])
        status.zero_()

    def md_steps(self, *a, **kw):
        raise AssertionError("the stepwise path was taken")


@pytest.fixture
def fake():
    old = backend._BACKEND
    be = Recorder()
    backend.set_backend(be)
    yield be
    backend.set_backend(old)


def _parameters(mol):
    ids = np.arange(mol["n"])
    k3, k4 = mol["ks"][2].astype(np.float64), mol["ks"][3].astype(np.float64)
    return Parameters(atoms=ids, bonds=mol["idx"][0], bond_k=mol["ks"][0], bond_eq=mol["eqs"][0], angles=mol["idx"][1], angle_k=mol["ks"][1],
                      angle_eq=mol["eqs"][1], propers=mol["idx"][2], proper_ks=np.abs(k3), proper_phases=np.where(k3 >= 0, 0.0, np.pi),
                      impropers=mol["idx"][3], improper_ks=np.abs(k4), improper_phases=np.where(k4 >= 0, 0.0, np.pi))


def _mix():
    batch, cons, m, _ = mc.case("mix")
    mol = batch.mols[0]
    return mol, _parameters(mol), mol["xyz"].transpose(1, 0, 2), m[:18], cons[0]


def test_constraints_are_refused_on_the_stepwise_path(fake):
    mol, p, xyz, m, cons = _mix()
    with pytest.raises(ValueError, match="fused path only"):
        simulate(p, xyz, m, None, device="cpu", stepwise=True, constraints=cons, n_steps=2)
    g = graph_from_parameters(p, xyz)
    with pytest.raises(ValueError, match="fused path only"):
        simulate_graph(g, m, None, stepwise=True, constraints=ConstraintBatch([cons]), n_steps=2)
    fake.limit = 17          # "auto" for a batch above the limit would go stepwise
    with pytest.raises(ValueError, match="fused path only"):
        simulate_graph(g, m, None, stepwise="auto", constraints=ConstraintBatch([cons]), n_steps=2)
    fake.limit = 40
    assert not fake.calls, "a refused call reached the backend"
    simulate_graph(g, m, None, stepwise="auto", constraints=ConstraintBatch([cons]), n_steps=2)          # within the limit: fused
    assert len(fake.calls) == 1
    with pytest.raises(TypeError):
        simulate_graph(g, m, None, constraints=[cons], n_steps=2)
    with pytest.raises(TypeError):
        simulate(p, xyz, m, None, device="cpu", constraints=ConstraintBatch([cons]), n_steps=2)
    with pytest.raises(ValueError, match="describe 2 molecules"):
        simulate_graph(g, m, None, constraints=ConstraintBatch([cons, None]), n_steps=2)


def test_only_the_first_launch_constrains_the_start(fake):
    mol, p, xyz, m, cons = _mix()
    g = graph_from_parameters(p, xyz)
    cb = ConstraintBatch([cons], tolerance=2.0 ** -18)
    simulate_graph(g, m, None, constraints=cb, n_steps=25, steps_per_launch=10)
    assert [c["kw"]["constrain_start"] for c in fake.calls] == [True, False, False]
    assert [c["opts"]["n_steps"] for c in fake.calls] == [10, 10, 5] and [c["opts"]["first_step"] for c in fake.calls] == [0, 10, 20]
    for c in fake.calls:
        got = c["kw"]["constraints"]
        assert isinstance(got, ConstraintBatch) and got.tolerance == 2.0 ** -18 and torch.equal(got.cluster_atoms, cb.cluster_atoms)
    fake.calls.clear()
    simulate_graph(g, m, None, constraints=cb, constrain_start=False, first_step=25, n_steps=12, steps_per_launch=10,
                   velocities=torch.zeros(18, 3, 3))
    assert [c["kw"]["constrain_start"] for c in fake.calls] == [False, False]


def test_the_temperature_divides_by_the_reduced_degrees_of_freedom(fake):
    mol, p, xyz, m, cons = _mix()
    r = simulate(p, xyz, m, None, device="cpu", constraints=cons, n_steps=1)
    assert cons.n_constraints == 6
    assert np.allclose(r.temperature, 2.0 * EKIN / ((3 * 18 - 6) * KB), rtol=1e-6)
    free = simulate(p, xyz, m, None, device="cpu", n_steps=1)
    assert np.allclose(free.temperature, 2.0 * EKIN / (3 * 18 * KB), rtol=1e-6)
    # frozen atoms: a bond frozen at both ends removes no degree of freedom, one frozen at one end does
    mf = m.copy()
    mf[[int(cons.clusters[0, 0]), int(cons.clusters[0, 1])]] = 0.0
    k = int(np.nonzero((cons.clusters[:, 1:] >= 0).sum(1) >= 2)[0][0])
    mf[int(cons.clusters[k, 1])] = 0.0
    moving = int((mf > 0).sum())
    r = simulate(p, xyz, mf, None, device="cpu", constraints=cons, n_steps=1)
    assert np.allclose(r.temperature, 2.0 * EKIN / ((3 * moving - cons.n_constraints_moving(mf)) * KB), rtol=1e-6)
    # the divisor is floored at 1: ethane with everything frozen but one carbon, which three fixed lengths hold: 3 - 3 by the count
    batch, ce, me, _ = mc.case("ethane64")
    mol = dict(batch.mols[0], xyz=batch.mols[0]["xyz"][:, :1])
    centre = int(ce[0].clusters[0, 0])
    m1 = np.where(np.arange(8) == centre, me, 0.0).astype(np.float32)
    assert ce[0].n_constraints_moving(m1) == 3
    r = simulate(_parameters(mol), mol["xyz"].transpose(1, 0, 2), m1, None, device="cpu", constraints=ce[0], n_steps=1)
    assert np.allclose(r.temperature, 2.0 * EKIN / KB, rtol=1e-6)


def test_a_moving_centre_held_by_four_frozen_leaves_is_refused(fake):
    """four fixed lengths over-determine a point (the projection's system is singular): refused on the host, nothing launched"""
    batch, c4, m, _ = mc.case("xh4")
    mol = batch.mols[0]
    m4 = np.array([12.011, 0.0, 0.0, 0.0, 0.0], dtype=np.float32)
    with pytest.raises(ValueError, match="over-determine"):
        simulate(_parameters(mol), mol["xyz"].transpose(1, 0, 2), m4, None, device="cpu", constraints=c4[0], n_steps=1)
    assert not fake.calls
    for ok in (np.array([12.011, 0.0, 0.0, 0.0, 1.008]), np.array([0.0, 0.0, 0.0, 0.0, 0.0]), m):          # three frozen, all frozen, none
        simulate(_parameters(mol), mol["xyz"].transpose(1, 0, 2), ok.astype(np.float32), None, device="cpu", constraints=c4[0], n_steps=1)
    assert len(fake.calls) == 3


class FailsOnce(Recorder):
    """conformation `who` ends launch `when` with status 4 after 3 steps; every other launch runs it as if nothing had happened"""

    def __init__(self, who, when):
        super().__init__()
        self.who, self.when = who, when

    def md_langevin(self, plan, xyz, *a, **kw):
        xyz_out, vel_out, epot, steps, status = a[9], a[10], a[11], a[13], a[14]
        super().md_langevin(plan, xyz, *a, **kw)
        launch = len(self.calls) - 1
        xyz_out.add_(1.0)
        vel_out.fill_(float(launch + 1))
        epot.fill_(float(launch + 1))
        for k in ("frames_xyz", "frames_epot", "frames_ekin"):
            if kw.get(k) is not None:
                kw[k].fill_(float(launch + 1))
        if launch == self.when:
            status[0, self.who], steps[0, self.who] = 4, 3


@pytest.mark.parametrize("when", [0, 1])
def test_a_constraint_failure_outlasts_the_launches_of_a_run(when):
    """a later launch would run the failed item on from its broken state (the kernel keeps no memory of the failure): the front end
    keeps what the failing launch returned for it and discards what later launches write -- steps, frames, state"""
    mol, p, xyz, m, cons = _mix()
    old = backend._BACKEND
    be = FailsOnce(who=1, when=when)
    backend.set_backend(be)
    try:
        r = simulate_graph(graph_from_parameters(p, xyz), m, None, constraints=ConstraintBatch([cons]), n_steps=30, save_every=5, steps_per_launch=10)
    finally:
        backend.set_backend(old)
    assert len(be.calls) == 3
    assert r.status.tolist() == [[0, 4, 0]] and r.steps.tolist() == [[30, 10 * when + 3, 30]]
    x0 = torch.from_numpy(np.ascontiguousarray(xyz.transpose(1, 0, 2)))
    near = lambda a, b: bool(((a - b).abs() <= 1e-5).all())      # noqa: E731  (the fake adds 1.0 per launch, rounding each time)
    assert near(r.xyz[:, 0], x0[:, 0] + 3.0) and near(r.xyz[:, 1], x0[:, 1] + 1.0 + when) and near(r.xyz[:, 2], x0[:, 2] + 3.0)
    assert r.velocities[:, 1].unique().tolist() == [1.0 + when] and r.velocities[:, 0].unique().tolist() == [3.0]
    assert r.potential_energy.tolist() == [[3.0, 1.0 + when, 3.0]]
    # frames: two per launch; the failing launch's own frames stand (the kernel decides which of them it reached), later ones are NaN
    live = 2 * (when + 1)
    assert bool((r.frames[:live, :, 1] == torch.arange(1, when + 2).repeat_interleave(2)[:, None, None]).all())
    assert bool(torch.isnan(r.frames[live:, :, 1]).all()) and bool(torch.isnan(r.frame_potential_energy[live:, 0, 1]).all())
    assert bool(torch.isnan(r.frame_kinetic_energy[live:, 0, 1]).all())
    assert bool(torch.isfinite(r.frames[:, :, [0, 2]]).all()) and r.frame_potential_energy[:, 0, 0].tolist() == [1.0, 1.0, 2.0, 2.0, 3.0, 3.0]


def test_without_constraints_the_call_is_the_one_made_without_the_keyword(fake):
    mol, p, xyz, m, _ = _mix()
    g = graph_from_parameters(p, xyz)
    opts = dict(seed=4, n_steps=25, save_every=5, steps_per_launch=10, friction=3.0)
    a = simulate_graph(g, m, None, **opts)
    plain, fake.calls = fake.calls, []
    b = simulate_graph(g, m, None, constraints=None, constrain_start=True, **opts)
    assert len(plain) == len(fake.calls) == 3
    for x, y in zip(plain, fake.calls):
        assert x["opts"] == y["opts"] and sorted(x["kw"]) == sorted(y["kw"]) == ["atom_counts_host"] and x["kw"] == y["kw"]
        assert torch.equal(x["xyz"], y["xyz"]) and torch.equal(x["mass"], y["mass"]) and torch.equal(x["key"], y["key"])
        assert (x["vel_in"] is None) == (y["vel_in"] is None) and (x["vel_in"] is None or torch.equal(x["vel_in"], y["vel_in"]))
    assert torch.equal(a.temperature, b.temperature) and torch.equal(a.xyz, b.xyz)
    # and through the numpy front end
    fake.calls.clear()
    simulate(p, xyz, m, None, device="cpu", n_steps=3)
    simulate(p, xyz, m, None, device="cpu", constraints=None, n_steps=3)
    assert fake.calls[0]["kw"] == fake.calls[1]["kw"] and sorted(fake.calls[0]["kw"]) == ["atom_counts_host"]
