"""CPU: restraints on the stepwise dynamics -- the new symbols and signatures, every refusal of grappa_amd/dynamics.py by message, the
calls it makes (recorded through a fake backend: none differs without restraints, frozen atoms are folded into the masses before
n_moving reads them, every segment of a long run gets the ORIGINAL reference), the restated gradient of E_r against central
differences, and what tests/test_gpu_md_restr.py rests on, decided from the restatement alone: every restated state finite, at most one
in ten (item, step count) pairs not steady in test_gpu_md._gate_state's sense (md_steps_refs.steady), and the NVE drift of the
restatement with E_tot = epot + E_r + ekin in fp32 and float64."""
import os
import re

import numpy as np
import pytest
import torch

import md_refs as md
import md_restr_refs as mr
import md_steps_refs as ms
import relax_refs as rr
import relax_restr_refs as rs
from grappa_amd import _lib, backend, dynamics
from grappa_amd.dynamics import MDResult, simulate, simulate_graph
from grappa_amd.nonbonded import NonbondedBatch
from grappa_amd.relax import graph_from_parameters
from grappa_amd.restraints import RestraintBatch, Restraints
from test_host_md_steps_cons import _parameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"grappa_md_steps_restr_workspace_bytes", "grappa_md_steps_init_restr_f32", "grappa_md_steps_run_restr_f32",
         "grappa_md_steps_finish_restr_f32"}


class Recorder:
    """a backend that records which seam was called, with which masses, start coordinates and keywords; the outputs stay as given"""
    limit = 40

    def __init__(self):
        self.calls = []

    def relax_max_atoms(self):
        return self.limit

    def _record(self, which, args, kw):
        self.calls.append(dict(which=which, opts=dict(args[7]), x_in=args[1], mass=args[8], **kw))

    def md_langevin(self, *a, **kw):
        self._record("fused", a, kw)

    def md_steps(self, *a, **kw):
        self._record("steps", a, kw)

    def md_steps_cons(self, *a, **kw):
        self._record("steps_cons", a, kw)

    def md_steps_gb(self, *a, **kw):
        self._record("steps_gb", a, kw)

    def md_steps_restr(self, *a, **kw):
        self._record("steps_restr", a, kw)


class NoRestraints(Recorder):
    md_steps_restr = None


@pytest.fixture
def fake():
    old = backend._BACKEND
    be = Recorder()
    backend.set_backend(be)
    yield be
    backend.set_backend(old)


def _mol():
    """the 17-atom molecule of the mixed case -> (mol, Parameters, xyz (C, n, 3), masses, Restraints with one dihedral, tethers, frozen)"""
    c = mr.case(mr.MIXED)
    b = c["batch"]
    mol = b.mols[2]
    p0 = int(b.ptr[2])
    m = c["masses_in"][p0:p0 + 17]
    frozen = np.zeros(17, dtype=bool)
    frozen[[3, 11]] = True
    res = Restraints(frozen=frozen, position_k=np.where(np.arange(17) % 4 == 0, 20.0, 0.0), dihedrals=[mol["idx"][2][0]], dihedral_k=150.0,
                     dihedral_targets=[[0.1, 0.2, 0.3]])
    return mol, _parameters(mol), mol["xyz"].transpose(1, 0, 2), m, res


# ------------------------------------------------------------------------------------------------------------------------- the C ABI
def test_symbols_and_signatures():
    header = open(os.path.join(ROOT, "include", "grappa_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert NAMES <= set(re.findall(r"\b(grappa_[a-z0-9_]+)\s*\(", code)) and NAMES <= set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 11 and "#define GRAPPA_ABI_VERSION 11" in header
    fields = [f for f, _ in _lib.MdRestr._fields_]
    assert fields == ["pos_k", "pos_ref", "dih_molptr", "dih_atoms", "dih_k", "dih_target", "R"]
    struct = re.search(r"typedef struct grappa_md_restr \{(.*?)\} grappa_md_restr;", code, flags=re.S).group(1)
    assert re.findall(r"(\w+);", struct) == fields
    # the _restr_ calls are the _gbcut_ calls with `r` directly after gbcut, plus the restraint outputs at the end
    P = _lib.C.POINTER(_lib.MdRestr)
    for which, extra in (("init", 0), ("run", 2), ("finish", 2)):
        res_g, args_g = _lib.SIGNATURES[f"grappa_md_steps_{which}_gbcut_f32"]
        res_r, args_r = _lib.SIGNATURES[f"grappa_md_steps_{which}_restr_f32"]
        assert res_r is res_g and args_r[:8] == args_g[:8] and args_r[8] is P, which
        assert args_r[9:len(args_r) - extra] == args_g[8:] and all(a is _lib.C.c_void_p for a in args_r[len(args_r) - extra:]), which
    lib = _lib.load()
    assert lib.grappa_md_steps_restr_workspace_bytes(0, 1, 1, 1, 0, 0, 0, 0) == 0
    for K, cut, gb, gbcut, plain in ((0, 0, 0, 0, lib.grappa_md_steps_workspace_bytes(100, 3, 2, 3)),
                                     (0, 1, 0, 0, lib.grappa_md_steps_cut_workspace_bytes(100, 3, 2, 3)),
                                     (5, 1, 0, 0, lib.grappa_md_steps_cons_workspace_bytes(100, 3, 2, 3, 5, 1)),
                                     (5, 0, 1, 0, lib.grappa_md_steps_gb_workspace_bytes(100, 3, 2, 3, 5)),
                                     (0, 1, 1, 1, lib.grappa_md_steps_gbcut_workspace_bytes(100, 3, 2, 3, 0))):
        need = lib.grappa_md_steps_restr_workspace_bytes(100, 3, 2, 3, K, cut, gb, gbcut)
        assert plain + 100 * 3 * 3 * 4 <= need <= plain + 100 * 3 * 3 * 4 + 256, "the reference lies behind the words of the call without restraints"
    text = open(os.path.join(ROOT, "grappa_amd", "dynamics.py")).read()
    assert "constraint or restraint tables refused" in text


# ------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_by_message(fake):
    mol, p, xyz, m, res = _mol()
    kw = dict(device="cpu", n_steps=3)
    with pytest.raises(ValueError, match='restraints run on the stepwise path only: pass stepwise="auto"'):
        simulate(p, xyz, m, mol["nb"], restraints=res, stepwise=False, **kw)
    with pytest.raises(ValueError, match='restraints run on the stepwise path only'):
        simulate(p, xyz, m, mol["nb"], restraints=res, **kw)          # the default is the fused path
    with pytest.raises(TypeError, match="restraints must be Restraints or None"):
        simulate(p, xyz, m, mol["nb"], restraints=RestraintBatch([res], 3), stepwise="auto", **kw)
    with pytest.raises(ValueError, match="restraint_reference needs restraints"):
        simulate(p, xyz, m, mol["nb"], restraint_reference=xyz, stepwise="auto", **kw)
    with pytest.raises(ValueError, match="restraint_reference must have the shape of xyz"):
        simulate(p, xyz, m, mol["nb"], restraints=res, restraint_reference=xyz[:2], stepwise="auto", **kw)
    g = graph_from_parameters(p, xyz)
    nb = NonbondedBatch([mol["nb"]])
    with pytest.raises(TypeError, match="restraints must be a RestraintBatch or None"):
        simulate_graph(g, m, nb, restraints=res, stepwise=True, n_steps=3)
    with pytest.raises(ValueError, match="restraint_reference needs restraints"):
        simulate_graph(g, m, nb, restraint_reference=torch.zeros(17, 3, 3), stepwise=True, n_steps=3)
    with pytest.raises(ValueError, match="restraints run on the stepwise path only"):
        simulate_graph(g, m, nb, restraints=RestraintBatch([res], 3), stepwise=False, n_steps=3)
    with pytest.raises(ValueError, match=r"restraint_reference must be a \(17, 3, 3\) tensor"):
        simulate_graph(g, m, nb, restraints=RestraintBatch([res], 3), restraint_reference=torch.zeros(17, 3, 2), stepwise=True, n_steps=3)
    # the checks relax_graph applies to its RestraintBatch, with its messages
    with pytest.raises(ValueError, match="the restraint batch describes 1 molecules in 2 conformations, the graph 1 in 3"):
        simulate_graph(g, m, nb, restraints=RestraintBatch([Restraints(position_k=np.ones(17))], 2), stepwise=True, n_steps=3)
    with pytest.raises(ValueError, match="atoms per molecule differ"):
        simulate_graph(g, m, nb, restraints=RestraintBatch([Restraints(position_k=np.ones(16))], 3), stepwise=True, n_steps=3)
    far = Restraints(dihedrals=[[0, 1, 2, 17]], dihedral_k=1.0, dihedral_targets=0.0)
    with pytest.raises(ValueError, match="molecule 0: a restrained dihedral names atom 17, the molecule has 17 atoms"):
        simulate_graph(g, m, nb, restraints=RestraintBatch([far], 3), stepwise=True, n_steps=3)
    assert not fake.calls, "a refused call reached the backend"
    old = backend._BACKEND
    backend.set_backend(NoRestraints())
    try:
        with pytest.raises(ValueError, match="the backend has no restraints on the stepwise dynamics"):
            simulate(p, xyz, m, mol["nb"], restraints=res, stepwise="auto", **kw)
    finally:
        backend.set_backend(old)


def test_relax_graph_applies_the_shared_checks():
    import importlib
    relax = importlib.import_module("grappa_amd.relax")
    src = open(os.path.join(ROOT, "grappa_amd", "relax.py")).read()
    assert src.count("the restraint batch does not describe the graph's molecules") == 1
    assert "check_restraint_batch(restraints, B, C, counts, dev)" in src
    assert "check_restraint_batch(restraints, B, C, counts, dev)" in open(os.path.join(ROOT, "grappa_amd", "dynamics.py")).read()
    assert callable(relax.check_restraint_batch)


def test_the_backend_seam_refuses_frozen_and_needs_its_outputs():
    """HipBackend.md_steps_restr decides these before it touches the device"""
    from grappa_amd.backend_mm import MMBackend
    _, _, _, _, res = _mol()
    args = (None,) * 17
    with pytest.raises(TypeError, match="restraints must be a RestraintBatch"):
        MMBackend.md_steps_restr(None, *args, restraints=res, restraint_energy=torch.zeros(1, 3))
    with pytest.raises(ValueError, match="fold them into the masses"):
        MMBackend.md_steps_restr(None, *args, restraints=RestraintBatch([res], 3), restraint_energy=torch.zeros(1, 3))
    free = RestraintBatch([Restraints(position_k=np.ones(17))], 3)
    with pytest.raises(ValueError, match="restraint_energy"):
        MMBackend.md_steps_restr(None, *args, restraints=free)
    with pytest.raises(TypeError, match="go together"):
        MMBackend.md_steps_restr(None, *args, restraints=free, restraint_energy=torch.zeros(1, 3), solvent="obc2")


# ------------------------------------------------------------------------------------------------------------------------- the calls made
def test_none_makes_exactly_the_calls_of_today(fake):
    mol, p, xyz, m, res = _mol()
    fake.limit = 200
    simulate(p, xyz, m, mol["nb"], device="cpu", n_steps=3)
    simulate(p, xyz, m, mol["nb"], device="cpu", n_steps=3, restraints=None, restraint_reference=None)
    simulate(p, xyz, m, mol["nb"], device="cpu", n_steps=3, stepwise=True, restraints=None)
    simulate(p, xyz, m, mol["nb"], device="cpu", n_steps=3, stepwise="auto", cutoff=9.0, restraints=None)
    assert [c["which"] for c in fake.calls] == ["fused", "fused", "steps", "steps"]
    assert fake.calls[0].keys() == fake.calls[1].keys()
    for c in fake.calls:
        assert not {"restraints", "restraint_reference", "restraint_energy", "dihedral_out", "frames_restraint_energy", "frames_dihedrals"} & set(c), sorted(c)
    r = simulate(p, xyz, m, mol["nb"], device="cpu", n_steps=3)
    assert r.restraint_energy is None and r.dihedrals is None and r.frames_restraint_energy is None and r.frames_dihedrals is None
    assert [f for f in MDResult.__dataclass_fields__][-4:] == ["restraint_energy", "dihedrals", "frames_restraint_energy", "frames_dihedrals"]


def test_restraints_go_stepwise_with_frozen_atoms_folded_into_the_masses(fake):
    from grappa_amd.constraints import Constraints
    mol, p, xyz, m, res = _mol()
    fake.limit = 200          # within the fused limit: "auto" goes stepwise all the same
    r = simulate(p, xyz, m, mol["nb"], device="cpu", n_steps=4, save_every=2, stepwise="auto", restraints=res)
    (c,) = fake.calls
    assert c["which"] == "steps_restr" and c["constraints"] is None and c["gb"] is None and c["solvent"] is None and "cutoff" not in c
    rb = c["restraints"]
    assert isinstance(rb, RestraintBatch) and rb.frozen is None and rb.pos_k is not None and rb.R == 1, "the frozen array is not sent down"
    mass = c["mass"].numpy()
    assert not mass[[3, 11]].any() and bool((mass[[i for i in range(17) if i not in (3, 11)]] > 0).all())
    assert c["restraint_reference"] is c["x_in"], "None resolves to the call's xyz"
    assert tuple(c["restraint_energy"].shape) == (1, 3) and tuple(c["dihedral_out"].shape) == (1, 3)
    assert tuple(c["frames_restraint_energy"].shape) == (2, 1, 3) and tuple(c["frames_dihedrals"].shape) == (2, 1, 3)
    assert r.restraint_energy.shape == (3,) and r.dihedrals.shape == (1, 3)
    assert r.frames_restraint_energy.shape == (3, 2) and r.frames_dihedrals.shape == (1, 3, 2)
    # the temperature divides by the moving atoms: 15 of 17.  The fake leaves ekin 0, so read n_moving off a run with ekin set
    g = graph_from_parameters(p, xyz)
    nb = NonbondedBatch([mol["nb"]])

    class Ekin(Recorder):
        def md_steps_restr(self, *a, **kw):
            a[14].fill_(1.0)

    old = backend._BACKEND
    backend.set_backend(Ekin())
    try:
        t = simulate_graph(g, m, nb, restraints=RestraintBatch([res], 3, atom_counts=[17]), stepwise=True, n_steps=1).temperature
    finally:
        backend.set_backend(old)
    assert torch.allclose(t, torch.full((1, 3), 2.0 / (3.0 * dynamics.KB * 15)))
    # with constraints, check_masses and the degrees of freedom read the folded masses: freezing both ends of a bond removes the constraint
    fake.calls.clear()
    bond = mol["idx"][0][0]
    cons = Constraints([[int(bond[0]), int(bond[1]), -1, -1, -1]], [[1.0, 0.0, 0.0, 0.0]])
    fz = np.zeros(17, dtype=bool)
    fz[[int(bond[0]), int(bond[1])]] = True

    class Both(Ekin):
        pass

    backend.set_backend(Both())
    try:
        t2 = simulate(p, xyz, m, mol["nb"], device="cpu", n_steps=1, stepwise=True, constraints=cons, restraints=Restraints(frozen=fz)).temperature
    finally:
        backend.set_backend(old)
    assert np.allclose(t2, 2.0 / (3.0 * 15 * dynamics.KB)), "no constraint is counted between two frozen atoms"


def test_every_segment_gets_the_original_reference(fake, monkeypatch):
    mol, p, xyz, m, res = _mol()
    monkeypatch.setattr(dynamics, "MAX_STEPS_PER_LAUNCH", 4)
    g = graph_from_parameters(p, xyz)
    nb = NonbondedBatch([mol["nb"]])
    rb = RestraintBatch([res], 3, atom_counts=[17])
    simulate_graph(g, m, nb, restraints=rb, stepwise=True, n_steps=6)
    a, b = fake.calls
    assert a["opts"]["n_steps"] == 4 and b["opts"]["n_steps"] == 2 and b["opts"]["first_step"] == 4
    assert b["x_in"] is not a["x_in"], "the second segment starts where the first ended"
    assert a["restraint_reference"] is a["x_in"] and b["restraint_reference"] is a["x_in"], "the reference must never be the segment's x_in"
    fake.calls.clear()
    ref = torch.randn(17, 3, 3)
    simulate_graph(g, m, nb, restraints=rb, restraint_reference=ref, stepwise=True, n_steps=6)
    assert all(torch.equal(c["restraint_reference"], ref) for c in fake.calls) and len(fake.calls) == 2


# ------------------------------------------------------------------------------------------------------------------------- the restatement
def test_empty_tables_return_the_unpatched_tensors():
    b = ms.case("s65_C3")
    plain = rr.forces(b, b.xyz, torch.float64, True)
    for rb in (None, RestraintBatch([None], 3, atom_counts=b.counts)):
        with mr.restr_force(rb):
            f = rr.forces(b, b.xyz, torch.float64, True)
        assert set(f) == set(plain) and all(torch.equal(f[k], plain[k]) for k in plain)
    assert rr.forces.__name__ == "forces", "the context restores relax_refs.forces"


def test_restated_gradient_against_central_differences():
    c = mr.case(mr.MIXED)
    b, rb = c["batch"], c["rb"]
    x = b.xyz.double()
    ref = mr.reference_of(b, offset=c["offset"]).double()
    with mr.restr_force(rb, offset=c["offset"]):
        f = rr.forces(b, x, torch.float64, True)
    plain = rr.forces(b, x, torch.float64, True)
    g = f["G"] - plain["G"]
    assert torch.equal(f["E"], plain["E"]), "E stays the force field's"
    tb = rs.Tables(b, rb)
    rng = np.random.default_rng(3)
    rows = np.unique(np.concatenate([tb.ix.reshape(-1).numpy()[rng.integers(0, tb.ix.numel(), 12)], np.flatnonzero(tb.pos_k.numpy() > 0)[:6]]))
    h = 1e-5
    for i in rows:
        for d in range(3):
            e = []
            for s in (h, -h):
                xx = x.clone()
                xx[i, :, d] += s
                e.append(rs.restraint_terms(b, tb, xx, ref)["E"].sum(0))
            fd = (e[0] - e[1]) / (2 * h)
            assert torch.allclose(fd, g[i, :, d], rtol=1e-6, atol=1e-5), (i, d, fd, g[i, :, d])
    assert float(g[0].norm()) > 1.0, "the single atom is pulled towards its displaced reference"
    assert not plain["G"][0].any(), "... and feels no force-field force"


def test_the_cases_are_what_the_issue_asks_for():
    c = mr.case("s65_C3")
    row = c["rb"].dih_atoms[0].tolist()
    assert 64 in row and min(row) < 64 and list(c["frozen"]) == [5, 63, 64] and int((c["rb"].pos_k > 0).sum()) >= 20
    assert not c["masses"][c["frozen"]].any() and bool((c["masses_in"][c["frozen"]] > 0).all()) and c["rb"].frozen is None
    c = mr.case("s129_C3")
    assert c["rb"].R == 4 and {a // 64 for a in c["rb"].dih_atoms.reshape(-1).tolist()} == {0, 1, 2}
    c = mr.case(mr.MIXED)
    assert np.diff(c["rb"].dih_molptr.numpy()).tolist() == [0, 0, 16, 2, 0, 0] and [r is None for r in c["rb"].items] == [False, True, False, False, True, False]
    assert float(c["rb"].pos_k[0]) >= 5 and bool((c["offset"][0].abs() >= 0.2).all()) and not c["offset"][1:].any()
    assert mr.case("s9_65_C17")["batch"].xyz.shape[1] == 17 and mr.SHORT == {"s513_C1": (1, 5)}
    for name in mr.CASES:
        rb, b = mr.case(name)["rb"], mr.case(name)["batch"]
        assert bool((rb.dih_k >= 100).all()) and bool((rb.dih_k <= 239).all()) and bool(((rb.pos_k == 0) | ((rb.pos_k >= 5) & (rb.pos_k <= 50))).all())
        if rb.R:
            phi0 = mr.energy_at(b, rb, b.xyz, offset=mr.case(name)["offset"])[1]
            d = torch.remainder(rb.dih_target.double() - phi0 + np.pi, 2 * np.pi) - np.pi
            assert bool((d.abs() >= 0.3 - 1e-6).all()) and bool((d.abs() <= 1.5 + 1e-6).all()), name
            assert bool((rb.dih_target[:, 1:] != rb.dih_target[:, :1]).all()) or rb.C == 1, "targets differ per conformation"


def test_every_restated_state_is_finite_and_the_gate_is_calibrated():
    for name in mr.CASES:
        for k in mr.SHORT.get(name, mr.TRAJ_STEPS):
            for r32, r64 in (r[k] for r in mr.verlet32(name)):
                assert all(bool(torch.isfinite(t).all()) for t in (*r32, *r64)), (name, k)
    n = mr.steady_counts()
    print(f"restrained trajectories: not steady {n['x'][0]} of {n['x'][1]} (x), {n['v'][0]} of {n['v'][1]} (v)")
    for label in ("x", "v"):
        assert 10 * n[label][0] <= n[label][1], (label, n[label])


def test_the_restatement_conserves_energy_with_the_restraint_energy_counted():
    d32, d64 = mr.nve_drift(torch.float32), mr.nve_drift(torch.float64)
    b, rb = mr.nve_case()
    m, v = ms.masses(ms.NVE_CASE), ms.thermal_velocities(ms.NVE_CASE)
    with mr.restr_force(rb):
        start = md.baoab_ref(b, m, torch.float64, velocities=v, n_steps=0)
        r = md.baoab_ref(b, m, torch.float64, velocities=v, **ms.NVE)
    without = md.drift(start["epot"] + start["ekin"], r["frame_epot"] + r["frame_ekin"])
    er = torch.stack([mr.energy_at(b, rb, x)[0] for x in r["frame_xyz"]])
    print(f"NVE with restraints, restated: D_f32 {d32:.4f}, D_f64 {d64:.4f} kcal/mol; without E_r in the sum {without:.4f}; E_r up to {float(er.max()):.2f}")
    # D is the integrator's O(dt^2) band, not rounding: fp32 and float64 agree on it, and half the step gives a quarter of it (a third
    # is asked for: the band is a maximum over 8 frames of an oscillating error, not the error's amplitude itself)
    assert d32 <= 1.25 * d64 and d64 <= 1.25 * d32, (d32, d64)
    half = dict(ms.NVE, dt=ms.NVE["dt"] / 2, n_steps=2 * ms.NVE["n_steps"], save_every=2 * ms.NVE["save_every"])
    with mr.restr_force(rb):
        rh = md.baoab_ref(b, m, torch.float64, velocities=v, **half)
    erh = torch.stack([mr.energy_at(b, rb, x)[0] for x in rh["frame_xyz"]])
    er0 = mr.energy_at(b, rb, start["xyz"])[0]
    dh = md.drift(start["epot"] + er0 + start["ekin"], rh["frame_epot"] + erh + rh["frame_ekin"])
    print(f"half the step: D_f64 {dh:.4f}, ratio {d64 / dh:.2f}")
    assert 3 * dh <= d64, "the restated integrator conserves epot + E_r + ekin to second order in dt"
    assert without > 4 * d64, "E_r is a real part of the conserved sum: leaving it out must show"
