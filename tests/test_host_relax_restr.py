"""CPU: restraints for the fused minimiser (grappa_amd/restraints.py, the restraint keywords of grappa_amd/relax.py) without a GPU --
the layout and every refusal of Restraints / RestraintBatch, the front ends through recording fakes, set_dihedral, the symbol table,
the restatement of tests/relax_restr_refs.py (no restraints = relax_refs.fire_ref exactly; the E_r gradient against central
differences), and the conditions tests/test_gpu_relax_restr.py rests on, decided from the float64 restatement alone: finite states, the
branch margin, convergence with the defaults and with the default scan stiffness, and the known answer of the 4-atom chain."""
import numpy as np
import pytest
import torch

import relax_refs as rr
import relax_restr_refs as rs
from grappa_amd import _lib, backend
from grappa_amd.parameters import Parameters
from grappa_amd.relax import RELAX_DEFAULTS, SCAN_K_DEFAULT, RelaxResult, ScanResult, graph_from_parameters, relax, relax_graph, scan_starts, torsion_scan
from grappa_amd.restraints import MAX_DIHEDRALS, RestraintBatch, Restraints, dihedral_angle, set_dihedral


# ------------------------------------------------------------------------------------------------ Restraints / RestraintBatch
def test_layout_and_dtypes():
    a = Restraints(frozen=[0, 1, 0, 0, 0], position_k=[0, 0, 2.5, 0, 0], dihedrals=[[0, 1, 2, 3], [1, 2, 3, 4]], dihedral_k=[10.0, 20.0],
                   dihedral_targets=[[0.1, 0.2, 0.3], [1.0, 1.1, 1.2]])
    b = Restraints(dihedrals=[[3, 2, 1, 0]], dihedral_k=5.0, dihedral_targets=[0.5])          # (R,): every conformation
    rb = RestraintBatch([a, None, b], 3, atom_counts=[5, 2, 4])
    assert rb.B == 3 and rb.R == 3 and rb.C == 3 and not rb.empty
    assert rb.dih_molptr.dtype == torch.int32 and rb.dih_molptr.tolist() == [0, 2, 2, 3]
    assert rb.dih_atoms.dtype == torch.int32 and rb.dih_atoms.tolist() == [[0, 1, 2, 3], [1, 2, 3, 4], [3, 2, 1, 0]]
    assert rb.dih_k.dtype == torch.float32 and rb.dih_k.tolist() == [10.0, 20.0, 5.0]
    assert rb.dih_target.dtype == torch.float32 and rb.dih_target.shape == (3, 3) and rb.dih_target.is_contiguous()
    assert rb.dih_target[2].tolist() == [0.5, 0.5, 0.5] and np.allclose(rb.dih_target[1].numpy(), [1.0, 1.1, 1.2])
    assert rb.frozen.dtype == torch.int32 and rb.frozen.tolist() == [0, 1, 0, 0, 0] + [0] * 6
    assert rb.pos_k.dtype == torch.float32 and rb.pos_k.tolist() == [0, 0, 2.5, 0, 0] + [0] * 6
    moved = rb.to("cpu")
    assert moved.R == 3 and torch.equal(moved.dih_atoms, rb.dih_atoms) and torch.equal(moved.frozen, rb.frozen) and moved.atom_counts == [5, 2, 4]
    none = RestraintBatch([None, Restraints()], 2)
    assert none.empty and none.R == 0 and none.frozen is None and none.pos_k is None and none.dih_molptr.tolist() == [0, 0, 0]
    assert none.dih_target.shape == (0, 2) and Restraints().empty and a.n_atoms == 5 and b.n_atoms is None


@pytest.mark.parametrize("kw,match", [
    (dict(dihedrals=[[0, 1, 2, 2]], dihedral_k=1.0, dihedral_targets=[0.0]), "distinct"),
    (dict(dihedrals=[[0, 1, 2, -1]], dihedral_k=1.0, dihedral_targets=[0.0]), "negative"),
    (dict(dihedrals=[[0, 1, 2, 3]], dihedral_k=-1.0, dihedral_targets=[0.0]), "non-negative"),
    (dict(dihedrals=[[0, 1, 2, 3]], dihedral_k=float("inf"), dihedral_targets=[0.0]), "finite"),
    (dict(dihedrals=[[0, 1, 2, 3]], dihedral_k=float("nan"), dihedral_targets=[0.0]), "finite"),
    (dict(dihedrals=[[0, 1, 2, 3]], dihedral_k=1.0, dihedral_targets=[float("nan")]), "finite"),
    (dict(dihedrals=[[0, 1, 2, 3]], dihedral_k=1.0, dihedral_targets=[[0.0, float("inf")]]), "finite"),
    (dict(dihedrals=[[0, 1, 2, 3]], dihedral_k=[1.0, 2.0], dihedral_targets=[0.0]), "one dihedral_k per dihedral"),
    (dict(dihedrals=[[0, 1, 2, 3]], dihedral_k=1.0, dihedral_targets=[0.0, 1.0]), "dihedral_targets must be"),
    (dict(dihedrals=[[0, 1, 2, 3]]), "need dihedral_k"),
    (dict(dihedral_k=1.0), "need dihedrals"),
    (dict(dihedrals=[[0.0, 1.0, 2.0, 3.0]], dihedral_k=1.0, dihedral_targets=[0.0]), "integer"),
    (dict(dihedrals=[[k, k + 1, k + 2, k + 3] for k in range(MAX_DIHEDRALS + 1)], dihedral_k=1.0, dihedral_targets=[0.0] * (MAX_DIHEDRALS + 1)), "at most"),
    (dict(position_k=[0.0, -1.0]), "position_k"),
    (dict(position_k=[0.0, float("nan")]), "position_k"),
    (dict(frozen=[0, 1], position_k=[0.0, 1.0, 2.0]), "same atoms"),
])
def test_restraints_refuse_what_the_kernel_would(kw, match):
    with pytest.raises(ValueError, match=match):
        Restraints(**kw)


def test_batch_refusals():
    d = Restraints(dihedrals=[[0, 1, 2, 5]], dihedral_k=1.0, dihedral_targets=[[0.0, 1.0]])
    with pytest.raises(ValueError, match="names atom 5"):          # an index equal to n
        RestraintBatch([d], 2, atom_counts=[5])
    RestraintBatch([d], 2, atom_counts=[6])
    with pytest.raises(ValueError, match="holds 2 conformations"):
        RestraintBatch([d], 3)
    with pytest.raises(ValueError, match="name 3 atoms"):
        RestraintBatch([Restraints(frozen=[1, 0, 0])], 1, atom_counts=[4])
    with pytest.raises(ValueError, match="atom_counts is required"):
        RestraintBatch([Restraints(frozen=[1, 0, 0]), None], 1)
    with pytest.raises(ValueError, match="names 1 molecules"):
        RestraintBatch([None, None], 1, atom_counts=[4])
    with pytest.raises(TypeError):
        RestraintBatch([object()], 1)
    with pytest.raises(ValueError, match="C must be"):
        RestraintBatch([None], -1)
    assert MAX_DIHEDRALS == 16


# ------------------------------------------------------------------------------------------------ front ends
class Recorder:
    """a backend that records how relax_fire / relax_steps were called and writes zeros"""
    limit = 40

    def __init__(self):
        self.calls = []

    def relax_max_atoms(self):
        return self.limit

    def relax_fire(self, *args, **kw):
        self.calls.append(("fire", sorted(kw)))
        args[8].zero_()          # xyz_out
        if "dihedral_out" in kw:
            kw["dihedral_out"].fill_(0.25), kw["restraint_energy"].fill_(1.5)

    def relax_steps(self, *args, **kw):
        self.calls.append(("steps", sorted(kw)))


@pytest.fixture
def rec():
    old = backend._BACKEND
    be = Recorder()
    backend.set_backend(be)
    yield be
    backend.set_backend(old)


def _parameters(mol, ids=None):
    ids = np.arange(mol["n"]) if ids is None else ids
    k3, k4 = mol["ks"][2].astype(np.float64), mol["ks"][3].astype(np.float64)
    return Parameters(atoms=ids, bonds=ids[mol["idx"][0]], bond_k=mol["ks"][0], bond_eq=mol["eqs"][0], angles=ids[mol["idx"][1]], angle_k=mol["ks"][1],
                      angle_eq=mol["eqs"][1], propers=ids[mol["idx"][2]], proper_ks=np.abs(k3), proper_phases=np.where(k3 >= 0, 0.0, np.pi),
                      impropers=ids[mol["idx"][3]], improper_ks=np.abs(k4), improper_phases=np.where(k4 >= 0, 0.0, np.pi))


def test_no_restraints_reach_the_backend_with_no_new_keyword(rec):
    mol = rr.case("n9_C3").mols[0]
    p, xyz = _parameters(mol), mol["xyz"].transpose(1, 0, 2)
    r = relax(p, xyz, device="cpu")
    assert rec.calls[-1] == ("fire", ["atom_counts_host"]) and r.restraint_energy is None and r.dihedrals is None
    relax_graph(graph_from_parameters(p, xyz), restraints=None)
    assert rec.calls[-1] == ("fire", ["atom_counts_host"])
    relax(p, xyz, device="cpu", stepwise=True)
    assert rec.calls[-1] == ("steps", ["atom_counts_host", "check_every"])
    assert RelaxResult(1, 2, 3, 4, 5).restraint_energy is None and RelaxResult(1, 2, 3, 4, 5).dihedrals is None


def test_restraints_reach_the_backend_and_the_result(rec):
    mol = rr.case("n9_C3").mols[0]
    p, xyz = _parameters(mol), mol["xyz"].transpose(1, 0, 2)
    res = Restraints(dihedrals=[mol["idx"][2][0]], dihedral_k=100.0, dihedral_targets=[[0.1, 0.2, 0.3]])
    r = relax(p, xyz, device="cpu", restraints=res)
    assert rec.calls[-1] == ("fire", ["atom_counts_host", "dihedral_out", "restraint_energy", "restraints"])
    assert r.restraint_energy.shape == (3,) and r.dihedrals.shape == (1, 3) and r.restraint_energy.tolist() == [1.5] * 3 and r.dihedrals[0, 0] == 0.25
    r = relax(p, xyz, device="cpu", restraints=res, stepwise="auto")          # within the limit: the fused path
    assert rec.calls[-1][0] == "fire"
    with pytest.raises(ValueError, match="fused minimiser only"):
        relax(p, xyz, device="cpu", restraints=res, stepwise=True)
    g = graph_from_parameters(p, xyz)
    with pytest.raises(ValueError, match="fused minimiser only"):
        relax_graph(g, restraints=RestraintBatch([res], 3), stepwise=True)
    with pytest.raises(TypeError):
        relax_graph(g, restraints=res)
    with pytest.raises(TypeError):
        relax(p, xyz, device="cpu", restraints=RestraintBatch([res], 3))
    with pytest.raises(ValueError, match="conformations"):
        relax_graph(g, restraints=RestraintBatch([res, None], 3))
    with pytest.raises(ValueError, match="names atom"):
        relax(p, xyz, device="cpu", restraints=Restraints(dihedrals=[[0, 1, 2, 9]], dihedral_k=1.0, dihedral_targets=[0.0]))
    n = len(rec.calls)
    rec.limit = 8          # the molecule is now above the limit: "auto" would go stepwise, which takes no restraints
    for sw in (False, "auto"):
        with pytest.raises(ValueError, match="above the limit"):
            relax(p, xyz, device="cpu", restraints=res, stepwise=sw)
    assert len(rec.calls) == n


def test_torsion_scan_front_end(rec):
    mol = rr.case("n9_C3").mols[0]
    ids = 100 + 7 * np.random.default_rng(0).permutation(9)
    p = _parameters(mol, ids)
    x = mol["xyz"][:, 0].astype(np.float64)
    dih = mol["idx"][2][0]
    s = torsion_scan(p, x, ids[dih], device="cpu")
    assert isinstance(s, ScanResult) and s.angles.shape == (24,) and np.allclose(np.diff(s.angles), np.deg2rad(15.0)) and s.angles[0] == -np.pi
    assert s.xyz.shape == (24, 9, 3) and s.dihedrals.shape == s.energy.shape == s.restraint_energy.shape == s.steps.shape == s.status.shape == (24,)
    assert rec.calls[-1][0] == "fire" and "restraints" in rec.calls[-1][1] and len(rec.calls) == 1          # one call for the whole grid
    starts, idx = scan_starts(p, x, ids[dih], s.angles)
    assert idx == dih.tolist()
    for a, y in zip(s.angles, starts):
        assert abs(np.angle(np.exp(1j * (dihedral_angle(y, *dih) - a)))) < 1e-12
    assert SCAN_K_DEFAULT == 239.0
    with pytest.raises(ValueError, match="four distinct atom ids"):
        torsion_scan(p, x, [ids[0], ids[1], ids[2], 5], device="cpu")
    with pytest.raises(ValueError, match="one conformation"):
        torsion_scan(p, mol["xyz"].transpose(1, 0, 2), ids[dih], device="cpu")
    with pytest.raises(ValueError, match="k must be"):
        torsion_scan(p, x, ids[dih], k=-1.0, device="cpu")
    from grappa_amd import Grappa
    assert callable(Grappa.torsion_scan)


# ------------------------------------------------------------------------------------------------ set_dihedral
def _internal(x, idx):
    x = torch.from_numpy(np.asarray(x))[:, None, :]
    from oracle.cpu_ref import bond_angle, bond_length
    b = bond_length(*[x[torch.from_numpy(idx[0][:, j])] for j in range(2)]).numpy()[:, 0]
    a = bond_angle(*[x[torch.from_numpy(idx[1][:, j])] for j in range(3)]).numpy()[:, 0]
    return b, a


def test_set_dihedral():
    mol = rr.case("n33_C3").mols[0]
    x = mol["xyz"][:, 0].astype(np.float64)
    bonds = mol["idx"][0]
    b0, a0 = _internal(x, mol["idx"])
    for row in mol["idx"][2][[0, 7, 20]]:
        i, j, k, l = row.tolist()
        for target in (-3.0, -0.4, 0.0, 1.3, np.pi):
            y = set_dihedral(x, bonds, row, target)
            assert abs(np.angle(np.exp(1j * (dihedral_angle(y, i, j, k, l) - target)))) <= 1e-12
            b1, a1 = _internal(y, mol["idx"])
            assert np.abs(b1 - b0).max() <= 1e-12, "a bond length changed"
            # an angle spans the rotation only if it is a proper's -- it never is: angles are i-j-k with j the centre, one side each
            assert np.abs(a1 - a0).max() <= 1e-12, "an angle changed"
            moved = np.abs(y - x).max(1) > 0
            from grappa_amd.restraints import rotating_side
            side = rotating_side(33, bonds, j, k)
            assert not moved[~side].any() and not moved[i] and not moved[j] and not moved[k], "the i-side moved"
    assert set_dihedral(x, bonds, mol["idx"][2][0], 0.5).dtype == np.float64
    # a ring bond: nothing rotates
    ring_bonds = np.array([[0, 1], [1, 2], [2, 3], [3, 4], [4, 5], [5, 0], [0, 6]])
    xr = np.random.default_rng(1).normal(size=(7, 3))
    assert np.array_equal(set_dihedral(xr, ring_bonds, [0, 1, 2, 3], 1.0), xr)
    assert np.array_equal(set_dihedral(xr, ring_bonds, [6, 0, 1, 2], 1.0), xr)          # (0-1 is in the ring too)
    with pytest.raises(ValueError, match="distinct"):
        set_dihedral(xr, ring_bonds, [0, 1, 1, 2], 1.0)


# ------------------------------------------------------------------------------------------------ symbols
def test_symbols_are_exported_and_bound():
    import grappa_amd
    for name in ("Restraints", "RestraintBatch", "set_dihedral", "ScanResult", "torsion_scan"):
        assert name in grappa_amd.__all__ and hasattr(grappa_amd, name)
    assert {"grappa_relax_fire_restr_f32", "grappa_relax_max_dihedrals"} <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["grappa_relax_fire_restr_f32"][1]) == 14
    assert [f[0] for f in _lib.RelaxRestr._fields_] == ["frozen", "pos_k", "dih_molptr", "dih_atoms", "dih_k", "dih_target", "R"]
    lib = _lib.load()
    assert _lib.relax_max_dihedrals() == lib.grappa_relax_max_dihedrals() == MAX_DIHEDRALS
    assert lib.grappa_abi_version() == 11
    import inspect
    from grappa_amd.backend_mm import MMBackend
    p = inspect.signature(MMBackend.relax_fire).parameters
    assert all(p[k].default is None for k in ("restraints", "restraint_energy", "dihedral_out"))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", ["n9_C3", "mixed"])
def test_without_restraints_the_restatement_is_fire_ref(name):
    b = rr.case(name)
    want = rr.fire_ref(b, torch.float64, True, snapshots=(1, 5), max_steps=12, tolerance=0.0)
    for rb in (None, RestraintBatch([None] * b.B, b.xyz.shape[1]), RestraintBatch([Restraints()] * b.B, b.xyz.shape[1], atom_counts=b.counts)):
        got = rs.fire_restr_ref(b, rb, torch.float64, True, snapshots=(1, 5), max_steps=12, tolerance=0.0)
        for k in ("xyz", "steps", "status", "gmax"):
            assert torch.equal(got[k], want[k]), k
        assert all(torch.equal(got["snap"][s], want["snap"][s]) for s in (1, 5))
        assert all(torch.equal(a.nan_to_num(7.0), w.nan_to_num(7.0)) for a, w in zip(got["margin"] + got["P"], want["margin"] + want["P"]))


@pytest.mark.parametrize("name", ["n4_C3", "n65_C1"])
def test_restraint_gradient_against_central_differences(name):
    b, rb, _ = rs.case(name)
    tb = rs.Tables(b, rb)
    x = b.xyz.double() + 0.05 * torch.from_numpy(np.random.default_rng(3).normal(size=tuple(b.xyz.shape)))          # (away from the start: tethers pull)
    got = rs.restraint_terms(b, tb, x, b.xyz)
    h = 1e-5
    rng = np.random.default_rng(4)
    atoms = sorted(set(tb.ix.reshape(-1).tolist()) | set(rng.choice(b.N, 4, replace=False).tolist()))
    for a in atoms:
        for c in range(x.shape[1]):
            for d in range(3):
                xp, xm = x.clone(), x.clone()
                xp[a, c, d] += h
                xm[a, c, d] -= h
                fd = (rs.restraint_terms(b, tb, xp, b.xyz)["E"].sum() - rs.restraint_terms(b, tb, xm, b.xyz)["E"].sum()) / (2 * h)
                assert abs(float(fd) - float(got["G"][a, c, d])) <= 1e-6 * max(1.0, abs(float(fd))), (a, c, d, float(fd), float(got["G"][a, c, d]))
    assert bool((got["abs_g"] + 1e-12 >= got["G"].norm(dim=-1)).all())


def test_case_table():
    for name, (sizes, C, spec, nb) in rs.CASES.items():
        b, rb, _ = rs.case(name)
        tb = rs.Tables(b, rb)
        assert rb.B == b.B and rb.C == C
        phi0 = rs.dihedral_t(b.xyz.double(), tb.ix)
        off = torch.remainder(rb.dih_target.double() - phi0 + np.pi, 2 * np.pi) - np.pi
        assert bool(((off.abs() >= 0.3 - 1e-6) & (off.abs() <= 1.5 + 1e-6)).all()), name          # 0.3 .. 1.5 rad from the start
        if C > 1 and rb.R:
            assert bool((rb.dih_target[:, 0] != rb.dih_target[:, 1]).all())
    b, rb, _ = rs.case("mixed")
    assert rb.dih_molptr.tolist() == [0, 0, 0, 16, 16, 16] and bool(rb.frozen[20:85].any()) and bool((rb.pos_k[20:85] > 0).any())
    assert not rb.frozen[:20].any() and rs.case("n257_C1")[0].counts == [257] and rs.case("max")[0].counts == [rr.max_atoms()]
    b4 = rs.case("n4_C3")[0]
    assert [int(i.shape[0]) for i in b4.idx] == [3, 2, 1, 0]


# ------------------------------------------------------------------------------------------------ what the GPU tests rest on
def test_restated_states_are_finite_and_the_branch_margin_mostly_holds():
    fails = total = 0
    for name, steps in rs.TRAJ:
        t = rs.trajectory(name, torch.float64, rs.total_steps(name))
        assert bool(torch.isfinite(t["snap"][steps]).all()) and bool(torch.isfinite(t["gmax"]).all()), name
        assert bool(torch.isfinite(rs.trajectory(name, torch.float32, rs.total_steps(name))["snap"][steps]).all()), name
        ok = rs.margin_ok(name, steps)
        fails, total = fails + int((~ok).sum()), total + ok.numel()
    print(f"{fails} of {total} (item, step count) pairs fail the branch margin")
    assert 10 * fails <= total


@pytest.mark.parametrize("name", rs.CONV_CASES)
def test_convergence_cases_converge_in_float64_with_the_defaults(name):
    r = rs.converged(name)
    print(name, "steps", r["steps"].flatten().tolist(), "status", r["status"].flatten().tolist())
    assert bool((r["status"] == 1).all()) and bool((r["steps"] < RELAX_DEFAULTS["max_steps"]).all())
    assert rs.CONV_OPTS == {}


def test_fire_defaults_with_the_default_scan_stiffness():
    """k = 239 kcal/mol on one proper of a 33-atom molecule, targets all round the circle from rotated starts: the float64 restatement
    with RELAX_DEFAULTS stays finite, never raises the objective by more than rounding between start and end, and converges"""
    mol = rr.case("n33_C3").mols[0]
    row = mol["idx"][2][7]
    angles = -np.pi + np.deg2rad(30.0) * np.arange(12)
    x0 = mol["xyz"][:, 0].astype(np.float64)
    starts = np.stack([set_dihedral(x0, mol["idx"][0], row, a) for a in angles])
    m = dict(mol, xyz=starts.transpose(1, 0, 2).astype(np.float32))
    b = rr.Batch([m])
    rb = RestraintBatch([Restraints(dihedrals=[row], dihedral_k=SCAN_K_DEFAULT, dihedral_targets=angles[None, :])], 12, atom_counts=[33])
    r = rs.fire_restr_ref(b, rb, torch.float64, True)
    tb = rs.Tables(b, rb)
    end = rs.objective(b, tb, r["xyz"], b.xyz)
    dev = (torch.remainder(end["phi"][0] - torch.from_numpy(angles) + np.pi, 2 * np.pi) - np.pi).abs()
    print("steps", r["steps"].flatten().tolist(), "status", r["status"].flatten().tolist(), "max |phi - target|", float(dev.max()))
    assert bool(torch.isfinite(r["xyz"]).all()) and bool((r["status"] == 1).all())
    begin = rs.objective(b, tb, b.xyz, b.xyz)
    assert bool((end["E"] + end["Er"] <= begin["E"] + begin["Er"]).all())


def test_known_answer_of_the_four_atom_chain_in_float64():
    """at a restrained minimum of a 4-atom chain bonds and angles sit at equilibrium: the energy is the torsion series at the dihedral
    reached (1e-4 kcal/mol) and k sin(phi - target) balances the series' derivative (tolerance x 2 A)"""
    b, rb, nb = rs.case("n4_C3")
    assert nb is False
    tol = 0.01
    r = rs.fire_restr_ref(b, rb, torch.float64, False, tolerance=tol)
    assert bool((r["status"] == 1).all()), r["status"].tolist()
    end = rs.objective(b, rs.Tables(b, rb), r["xyz"], b.xyz, torch.float64, False)
    e, de = rs.series(b.ks[2][0].numpy(), end["phi"][0].numpy())
    print("E - series", (end["E"][0].numpy() - e).tolist(), "torque balance", (float(rb.dih_k[0]) * np.sin(end["phi"][0].numpy() - rb.dih_target[0].numpy()) + de).tolist())
    assert np.abs(end["E"][0].numpy() - e).max() <= 1e-4
    assert np.abs(float(rb.dih_k[0]) * np.sin(end["phi"][0].numpy() - rb.dih_target[0].double().numpy()) + de).max() <= tol * 2.0
