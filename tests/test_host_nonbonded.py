"""CPU: the host side of the nonbonded term (grappa_amd/nonbonded.py, MolData.from_arrays, the Lennard-Jones columns of
ForceFieldTemplates) and the float64 restatement the GPU tests measure against (tests/nonbonded_refs.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kernel_refs as kr
import nonbonded_refs as nr
from grappa_amd.constants import COULOMB_CONSTANT
from grappa_amd.nonbonded import NonbondedBatch, NonbondedParameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _from_bonds(bonds, n, **kw):
    q = np.linspace(-0.4, 0.6, n)
    s = np.linspace(2.0, 3.0, n)
    e = np.linspace(0.05, 0.15, n)
    return NonbondedParameters.from_bonds(bonds, q, s, e, **kw), q, s, e


def _split(p):
    pairs = [tuple(r) for r in p.exception_idx.tolist()]
    excl = [pr for pr, qq, e in zip(pairs, p.exception_chargeprod, p.exception_epsilon) if qq == 0 and e == 0]
    return sorted(excl), sorted(set(pairs) - set(excl))


# ----------------------------------------------------------------------------------------------------------------- from_bonds
def test_from_bonds_butane_chain():
    # C0-C1-C2-C3: bonded 01 12 23; two bonds apart 02 13; three bonds apart 03
    p, q, s, e = _from_bonds([(0, 1), (1, 2), (2, 3)], 4)
    excl, one4 = _split(p)
    assert excl == [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)] and one4 == [(0, 3)]
    k = [tuple(r) for r in p.exception_idx.tolist()].index((0, 3))
    assert p.exception_chargeprod[k] == pytest.approx(q[0] * q[3] / 1.2, rel=1e-15)
    assert p.exception_sigma[k] == pytest.approx((s[0] + s[3]) / 2, rel=1e-15)
    assert p.exception_epsilon[k] == pytest.approx(0.5 * np.sqrt(e[0] * e[3]), rel=1e-15)
    p2, *_ = _from_bonds([(3, 2), (1, 0), (2, 1)], 4, coulomb14scale=0.5, lj14scale=1.0)      # bond order and direction do not matter
    assert np.array_equal(p2.exception_idx, p.exception_idx)
    assert p2.exception_chargeprod[k] == pytest.approx(0.5 * q[0] * q[3]) and p2.exception_epsilon[k] == pytest.approx(np.sqrt(e[0] * e[3]))


@pytest.mark.parametrize("n", [3, 4, 5])
def test_from_bonds_small_rings_have_no_14_pair(n):
    # 3-ring: all pairs bonded.  4-ring: 02 and 13 are two bonds apart (the torsion 0-1-2-3 ends on the bond 3-0).  5-ring: every
    # non-bonded pair is two bonds apart the short way round, whatever the long way says
    p, *_ = _from_bonds([(i, (i + 1) % n) for i in range(n)], n)
    excl, one4 = _split(p)
    assert one4 == [] and excl == [(i, j) for i in range(n) for j in range(i + 1, n)]


def test_from_bonds_cyclohexane():
    # opposite atoms are three bonds apart both ways round: 03, 14, 25, each once; the other 12 pairs are one or two bonds apart
    p, *_ = _from_bonds([(i, (i + 1) % 6) for i in range(6)], 6)
    excl, one4 = _split(p)
    assert one4 == [(0, 3), (1, 4), (2, 5)] and len(excl) == 12 and p.exception_idx.shape == (15, 2)


def test_from_bonds_without_bonds():
    for n in (1, 2):
        p, *_ = _from_bonds([], n)
        assert p.exception_idx.shape == (0, 2) and p.exception_epsilon.shape == (0,) and p.n_atoms == n


# ------------------------------------------------------------------------------------------------------------------- validate
@pytest.mark.parametrize("idx, eps, what", [([[0, 1], [1, 0]], 0.1, "twice"), ([[1, 1], [0, 2]], 0.1, "itself"), ([[0, 3], [0, 1]], 0.1, "outside"),
                                            ([[0, 1], [0, 2]], -0.1, "negative")])
def test_validate_rejects(idx, eps, what):
    p = NonbondedParameters(np.zeros(3), np.ones(3), np.ones(3), np.array(idx), np.zeros(2), np.ones(2), np.full(2, eps))
    with pytest.raises(ValueError, match=what):
        p.validate()


def test_validate_rejects_shapes_and_round_trips():
    with pytest.raises(ValueError):
        NonbondedParameters(np.zeros(3), np.ones(2), np.ones(3)).validate()
    with pytest.raises(ValueError):
        NonbondedParameters(np.zeros(3), np.ones(3), np.ones(3), np.array([[0, 1]]), np.zeros(2), np.ones(1), np.ones(1)).validate()
    p, *_ = _from_bonds([(0, 1), (1, 2), (2, 3)], 4)
    d = p.to_dict()
    assert all(k.startswith("nbparam_") for k in d) and len(d) == 7
    p2 = NonbondedParameters.from_dict(d).validate()
    for k in d:
        assert np.array_equal(getattr(p2, k[len("nbparam_"):]), getattr(p, k[len("nbparam_"):]))


# -------------------------------------------------------------------------------------------------------------- NonbondedBatch
def test_batch_tables():
    a, *_ = _from_bonds([(0, 1), (1, 2), (2, 3), (3, 4)], 5)
    b, *_ = _from_bonds([], 1)
    c, *_ = _from_bonds([(i, (i + 1) % 6) for i in range(6)], 6)
    nb = NonbondedBatch([a, b, c])
    assert nb.B == 3 and nb.N == 12 and nb.atom_molptr.tolist() == [0, 5, 6, 12] and nb.atom_molptr.dtype == torch.int32
    ptr, atom = nb.exc_ptr.tolist(), nb.exc_atom.tolist()
    assert len(ptr) == 13 and ptr[0] == 0 and ptr[-1] == len(atom) == 2 * (len(a.exception_idx) + len(c.exception_idx))
    assert ptr[5] == ptr[6]                                                   # the single atom has no exception
    seen = {}
    for i in range(12):
        part = atom[ptr[i]:ptr[i + 1]]
        assert part == sorted(part) and len(set(part)) == len(part), "partners ascend per atom"
        mol = 0 if i < 5 else 2
        lo, hi = nb.atom_molptr.tolist()[mol], nb.atom_molptr.tolist()[mol + 1]
        assert all(lo <= j < hi and j != i for j in part), "batch-global indices inside the atom's molecule"
        for k, j in zip(range(ptr[i], ptr[i + 1]), part):
            seen[(i, j)] = (float(nb.exc_qq[k]), float(nb.exc_sigma[k]), float(nb.exc_eps[k]))
    assert all((j, i) in seen and seen[(j, i)] == v for (i, j), v in seen.items()), "both directions, same parameters"
    for m, p in enumerate((a, b, c)):
        idx, qq, sg, ep = nb.exceptions_of(m)
        assert np.array_equal(idx, p.exception_idx)
        for got, want in ((qq, p.exception_chargeprod), (sg, p.exception_sigma), (ep, p.exception_epsilon)):
            assert np.array_equal(got, want.astype(np.float32))
    empty = NonbondedBatch([b, b])
    assert empty.exc_ptr.tolist() == [0, 0, 0] and empty.exc_atom.numel() == 1      # non-NULL tables for the C ABI


def test_work_item_plan_is_built_on_the_host():
    """grappa_nonbonded_plan (host code of libgrappa_hip.so): [n_items, n_blocks, 0, 0 | blk_ptr | (molecule, first atom, block, first
    conformation) per item]; every (atom block, conformation) is covered exactly once, whatever C"""
    import ctypes as C
    from grappa_amd import _lib
    lib, T = _lib.load(), _lib.nonbonded_iblock()
    sizes = [1, 0, T, 2 * T + 3, 5]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    N, B = int(ptr[-1]), len(sizes)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    for Cc in (1, 3, 33):
        need = lib.grappa_nonbonded_plan(N, Cc, B, vp(ptr), None, 0)
        tab = np.full(need, -7, dtype=np.int32)
        assert lib.grappa_nonbonded_plan(N, Cc, B, vp(ptr), vp(tab), need) == need
        n_items, n_blk = int(tab[0]), int(tab[1])
        assert n_blk == 1 + 0 + 1 + 3 + 1 and tab[4:4 + B + 1].tolist() == [0, 1, 1, 2, 5, 6]
        off = 4 + (B + 1 + 3) // 4 * 4
        items = tab[off:off + 4 * n_items].reshape(n_items, 4)
        assert need == off + 4 * n_items and not (tab == -7).any()
        cover = np.zeros((n_blk, Cc), dtype=int)
        for k, (mol, i0, blk, c0) in enumerate(items.tolist()):
            assert ptr[mol] <= i0 < ptr[mol + 1] and (i0 - ptr[mol]) % T == 0 and blk == tab[4 + mol] + (i0 - ptr[mol]) // T
            nxt = [r[3] for r in items[k + 1:].tolist() if r[2] == blk]
            c1 = min(nxt) if nxt else Cc
            ni = min(T, ptr[mol + 1] - i0)
            assert 0 <= c0 < c1 <= Cc and ni * (c1 - c0) <= 256 and c1 - c0 <= 16
            cover[blk, c0:c1] += 1
        assert (cover == 1).all()
        assert lib.grappa_nonbonded_plan(N, Cc, B, vp(ptr), vp(tab), need - 1) == -3
    bad = ptr.copy()
    bad[2] = 0                                                  # descending range
    assert lib.grappa_nonbonded_plan(N, 3, B, vp(bad), None, 0) == -1
    assert lib.grappa_nonbonded_plan(N - 1, 3, B, vp(ptr), None, 0) == -1 and lib.grappa_nonbonded_plan(N, 0, B, vp(ptr), None, 0) == -1
    assert lib.grappa_nonbonded_plan(N, 3, B, None, None, 0) == -1


# ------------------------------------------------------------------------------------------------------- the float64 restatement
def _pair(q0, q1, sigma, eps, r):
    x = torch.tensor([[[0.0, 0.0, 0.0]], [[0.0, r, 0.0]]], dtype=torch.float64)
    return nr.nb_ref([NonbondedParameters([q0, q1], [sigma, sigma], [eps, eps])], x, torch.float64)


def test_restatement_known_answers():
    out = _pair(0.0, 0.0, 3.0, 0.25, 2 ** (1 / 6) * 3.0)          # (parameters the batch's float32 tables hold exactly)
    assert float(out["energy"]) == pytest.approx(-0.25, rel=1e-13) and float(out["grad"].abs().max()) < 1e-13
    out = _pair(1.0, 1.0, 3.0, 0.0, 1.0)
    assert float(out["energy"]) == pytest.approx(COULOMB_CONSTANT, rel=1e-14) == pytest.approx(332.0637, rel=1e-6)
    assert float(out["terms"][1]) == pytest.approx(COULOMB_CONSTANT, rel=1e-14) and float(out["terms"][0]) == 0.0
    assert out["grad"][1, 0].tolist() == pytest.approx([0.0, -COULOMB_CONSTANT, 0.0], rel=1e-14)      # repulsion: E falls as atom 1 moves away


def test_restatement_gradient_is_the_derivative_of_its_energy():
    rng = np.random.default_rng(5)
    p, xyz = nr.gen_molecule(20, 2, rng)
    nb = [p]
    x = torch.from_numpy(xyz).double()
    out = nr.nb_ref(nb, x)
    h = 1e-5
    fd = torch.zeros_like(x)
    for a in range(20):
        for k in range(3):
            xp, xm = x.clone(), x.clone()
            xp[a, :, k] += h
            xm[a, :, k] -= h
            fd[a, :, k] = (nr.nb_ref(nb, xp)["energy"][0] - nr.nb_ref(nb, xm)["energy"][0]) / (2 * h)
    # central differences: error h^2 E''' / 6 ~ 1e-10 x the third derivative; against sum_j |f_ij| that is below 1e-6
    assert bool(((fd - out["grad"]).abs().amax(-1) <= 1e-6 * out["abs_f"]).all()) and float(out["abs_f"].max()) > 1.0
    assert torch.allclose(out["terms"].sum(0), out["energy"], rtol=1e-13, atol=0)


@pytest.mark.parametrize("name", sorted(nr.case_table()))
def test_fp32_restatement_is_finite_and_inside_the_floor(name):
    """the inputs of every GPU case keep the fp32 restatement finite and its own error below the gate's floor (64 u32 x scale), so
    the gate of the GPU test stays within three floors"""
    params, nb, x, r64, r32 = nr.case(name)
    for k in ("energy", "terms", "grad"):
        assert bool(torch.isfinite(r32[k]).all()) and bool(torch.isfinite(r64[k]).all()), k
    for k, sc in (("energy", "abs_e"), ("terms", "abs_terms")):
        assert bool(((r32[k].double() - r64[k]).abs() <= nr.C_GATE * kr.U32 * r64[sc]).all()), k
    assert bool(((r32["grad"].double() - r64["grad"]).abs().amax(-1) <= nr.C_GATE * kr.U32 * r64["abs_f"]).all())
    nr.gate_all(r32["energy"], r32["terms"], r32["grad"], r64, r32, name)
    if name == "coincident_excluded":
        assert bool((x[0] == x[1]).all()) and float(r64["abs_e"].min()) > 0


# --------------------------------------------------------------------------------------------------------------------- MolData
def _molecule(n=5):
    from grappa_amd.molecule import Molecule
    return Molecule.from_graph([6] * n, [(i, i + 1) for i in range(n - 1)], [0.0] * n)


def test_moldata_from_arrays(tmp_path):
    from grappa_amd.moldata import MolData
    rng = np.random.default_rng(0)
    mol, C, n = _molecule(), 4, 5
    xyz, e, enb = rng.normal(size=(C, n, 3)), rng.normal(size=C), rng.normal(size=C)
    g, gnb = rng.normal(size=(C, n, 3)), rng.normal(size=(C, n, 3))
    md = MolData.from_arrays(mol, xyz, e, enb, g, gnb, smiles="CCCCC")
    want = (e - enb) - (e - enb).mean()
    assert np.allclose(md.energy_ref, want, rtol=0, atol=1e-15) and abs(md.energy_ref.mean()) < 1e-15
    assert np.array_equal(md.gradient_ref, g - gnb) and np.array_equal(md.energy, e) and md.mol_id == "CCCCC"
    assert np.array_equal(md.extras["nonbonded_energy_reference_ff"], enb) and np.array_equal(md.extras["nonbonded_gradient_reference_ff"], gnb)
    assert MolData.from_arrays(mol, xyz, e, enb, sequence="AG").mol_id == "AG"
    assert MolData.from_arrays(mol, xyz, e, enb, smiles="C", sequence="AG", mol_id="x7").mol_id == "x7"
    md0 = MolData.from_arrays(mol, xyz, e, enb, ff_energy=e + 1)
    assert md0.mol_id == "" and not md0.gradient.any() and not md0.gradient_ref.any() and md0.gradient.shape == xyz.shape
    assert not md0.extras["nonbonded_gradient_reference_ff"].any() and np.array_equal(md0.ff_energy["reference_ff"], e + 1)
    with pytest.raises(AssertionError, match="nonbonded_gradient"):
        MolData.from_arrays(mol, xyz, e, enb, gradient=g)
    back = MolData.from_dict(md.to_dict())
    for k in ("nonbonded_energy_reference_ff", "nonbonded_gradient_reference_ff"):
        assert np.array_equal(back.extras[k], md.extras[k])
    assert np.array_equal(back.energy_ref, md.energy_ref) and np.array_equal(back.gradient_ref, md.gradient_ref)
    md.save(str(tmp_path / "r.npz"))
    assert np.array_equal(MolData.load(str(tmp_path / "r.npz")).extras["nonbonded_energy_reference_ff"], enb)
    assert md.to_dgl().nodes["n1"].data["gradient_ref"].shape == (n, C, 3)


# ---------------------------------------------------------------------------------------------------------- ForceFieldTemplates
XML = """<ForceField>
 <AtomTypes><Type name="t0" class="C" element="C" mass="12.0"/><Type name="t1" class="H" element="H" mass="1.0"/></AtomTypes>
 <Residues><Residue name="XXX"><Atom name="CA" type="t0"/><Atom name="HA" type="t1"/><Atom name="HB" type="t1"/><Bond from="0" to="1"/><Bond from="0" to="2"/></Residue></Residues>
 <NonbondedForce coulomb14scale="0.8333" lj14scale="0.25"><Atom type="t0" charge="-0.2" sigma="0.34" epsilon="0.4184"/><Atom type="t1" charge="0.1" sigma="0.1" epsilon="0.0"/></NonbondedForce>
</ForceField>
"""


def _atom(i, name, res, resi, x):
    return f"ATOM  {i:5d} {name:<4s} {res:3s} A{resi:4d}    {x:8.3f}{0.0:8.3f}{0.0:8.3f}  1.00  0.00\n"


def test_force_field_templates_keep_lennard_jones(tmp_path):
    from grappa_amd import nonbonded
    from grappa_amd.pdb import ForceFieldTemplates, graph_from_pdb
    (tmp_path / "ff.xml").write_text(XML)
    (tmp_path / "m.pdb").write_text(_atom(1, "HA", "XXX", 1, 1.0) + _atom(2, "CA", "XXX", 1, 0.0) + _atom(3, "HB", "XXX", 1, -1.0))
    ff = ForceFieldTemplates(str(tmp_path / "ff.xml"))
    assert ff.sigma["t0"] == pytest.approx(3.4, rel=1e-14) and ff.epsilon["t0"] == pytest.approx(0.1, rel=1e-14)
    assert ff.sigma["t1"] == pytest.approx(1.0, rel=1e-14) and ff.epsilon["t1"] == 0.0 and ff.charge["t0"] == -0.2
    assert ff.coulomb14scale == 0.8333 and ff.lj14scale == 0.25
    g = graph_from_pdb(str(tmp_path / "m.pdb"), str(tmp_path / "ff.xml"))
    assert sorted(g) == ["bonds", "charges", "residue_ptr", "residue_templates", "xyz", "z"]
    g2, p = nonbonded.from_pdb(str(tmp_path / "m.pdb"), str(tmp_path / "ff.xml"))
    assert sorted(g2) == sorted(g) and np.array_equal(g2["bonds"], g["bonds"])
    assert p.sigma.tolist() == pytest.approx([1.0, 3.4, 1.0]) and p.epsilon.tolist() == pytest.approx([0.0, 0.1, 0.0])      # file order: HA, CA, HB
    assert p.charge.tolist() == pytest.approx([0.1, -0.2, 0.1]) and _split(p) == ([(0, 1), (0, 2), (1, 2)], [])


# ------------------------------------------------------------------------------------------------------------------- hygiene
def test_module_does_not_import_the_oracle():
    code = "import sys, grappa_amd.nonbonded; assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules)"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
    src = open(os.path.join(ROOT, "grappa_amd", "nonbonded.py")).read()
    assert "oracle" not in src
