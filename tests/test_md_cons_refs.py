"""CPU: the constraint tables (grappa_amd/constraints.py), the new entry points of the library, and the restatement of the constrained
loop (tests/md_cons_refs.py) on its own -- what the GPU tests of tests/test_gpu_md_cons.py lean on."""
import ctypes

import numpy as np
import pytest
import torch

import md_cons_refs as mc
import md_refs as md
from grappa_amd import _lib
from grappa_amd.constraints import ConstraintBatch, Constraints, hydrogen_constraints


# ------------------------------------------------------------------------------------------------ the library
def test_the_library_exports_and_binds_the_constraint_entry_points():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("grappa_md_cons_max_leaves", "grappa_md_cons_max_iter", "grappa_md_langevin_cons_f32"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.md_cons_limits() == (4, mc.MAX_ITER) and mc.MAX_ITER == 8
    assert [f[0] for f in _lib.MdCons._fields_] == ["cluster_molptr", "cluster_atoms", "cluster_d", "K", "tolerance", "constrain_start"]
    assert len(_lib.SIGNATURES["grappa_md_langevin_cons_f32"][1]) == len(_lib.SIGNATURES["grappa_md_langevin_f32"][1]) + 1
    assert _lib.load().grappa_abi_version() == 11


# ------------------------------------------------------------------------------------------------ from_bonds
METHANOL = dict(bonds=[[0, 1], [0, 2], [0, 3], [0, 4], [4, 5]], is_h=[False, True, True, True, False, True],
                lengths=[1.09, 1.10, 1.11, 1.43, 0.96])          # C H H H O H


def test_from_bonds_on_a_methanol_like_graph():
    c = Constraints.from_bonds(METHANOL["bonds"], METHANOL["is_h"], METHANOL["lengths"])
    assert c.clusters.tolist() == [[0, 1, 2, 3, -1], [4, 5, -1, -1, -1]] and c.clusters.dtype == np.int32
    assert np.array_equal(c.lengths, np.array([[1.09, 1.10, 1.11, 0.0], [0.96, 0.0, 0.0, 0.0]], dtype=np.float32))
    assert c.n_clusters == 2 and c.n_constraints == 4
    assert c.n_constraints_moving([12.0, 1.0, 1.0, 1.0, 16.0, 1.0]) == 4
    assert c.n_constraints_moving([0.0, 0.0, 1.0, 1.0, 16.0, 1.0]) == 3          # C-H1 with both ends frozen constrains nothing
    # the bond may name its hydrogen first
    flipped = Constraints.from_bonds([[1, 0], [2, 0], [0, 3], [4, 0], [5, 4]], METHANOL["is_h"], METHANOL["lengths"])
    assert flipped.clusters.tolist() == c.clusters.tolist()


def test_from_bonds_refusals_and_free_hydrogen_pairs():
    with pytest.raises(ValueError, match="bonded to 2 atoms"):          # a bridging hydrogen
        Constraints.from_bonds([[0, 1], [1, 2]], [False, True, False], [1.0, 1.0])
    with pytest.raises(ValueError, match="5 hydrogens"):
        Constraints.from_bonds([[0, k] for k in range(1, 6)], [False] + [True] * 5, [1.0] * 5)
    h2 = Constraints.from_bonds([[0, 1]], [True, True], [0.74])          # H-H is left free
    assert h2.n_clusters == 0 and h2.clusters.shape == (0, 5) and h2.lengths.shape == (0, 4)
    with pytest.raises(ValueError, match="one cluster only"):
        Constraints([[0, 1, -1, -1, -1], [2, 1, -1, -1, -1]], [[1.0, 0, 0, 0], [1.0, 0, 0, 0]])
    with pytest.raises(ValueError, match="finite and positive"):
        Constraints([[0, 1, -1, -1, -1]], [[0.0, 0, 0, 0]])


def test_hydrogen_constraints_take_the_predicted_equilibrium_lengths():
    from grappa_amd.parameters import Parameters
    z = np.zeros((0, 4), np.int64)
    p = Parameters(atoms=np.array([10, 11, 12, 13, 14, 15]), bonds=np.array(METHANOL["bonds"]) + 10, bond_k=np.ones(5), bond_eq=np.array(METHANOL["lengths"]),
                   angles=np.zeros((0, 3), np.int64), angle_k=np.zeros(0), angle_eq=np.zeros(0), propers=z, proper_ks=np.zeros((0, 3)),
                   proper_phases=np.zeros((0, 3)), impropers=z, improper_ks=np.zeros((0, 2)), improper_phases=np.zeros((0, 2)))
    c = hydrogen_constraints(p, [6, 1, 1, 1, 8, 1])
    assert c.clusters.tolist() == [[0, 1, 2, 3, -1], [4, 5, -1, -1, -1]]
    assert np.allclose(c.lengths[0, :3], [1.09, 1.10, 1.11]) and np.isclose(c.lengths[1, 0], 0.96)


def test_the_batch_layout():
    a = Constraints.from_bonds(METHANOL["bonds"], METHANOL["is_h"], METHANOL["lengths"])
    b = Constraints.from_bonds([[0, 1]], [False, True], [1.0])
    cb = ConstraintBatch([a, None, b, Constraints.from_bonds([[0, 1]], [True, True], [0.74])])
    assert cb.cluster_molptr.tolist() == [0, 2, 2, 3, 3] and cb.cluster_molptr.dtype == torch.int32 and cb.K == 3 and cb.B == 4
    assert cb.cluster_atoms.tolist() == [[0, 1, 2, 3, -1], [4, 5, -1, -1, -1], [0, 1, -1, -1, -1]]          # indices WITHIN each molecule
    assert cb.cluster_atoms.dtype == torch.int32 and cb.cluster_d.dtype == torch.float32 and cb.cluster_d.shape == (3, 4)
    assert cb.tolerance == 2.0 ** -19
    m = np.array([12.0, 1, 1, 1, 16, 1] + [12.0] * 3 + [0.0, 0.0] + [1.0, 1.0])
    assert cb.n_constraints_host(m, [6, 3, 2, 2]).tolist() == [4, 0, 0, 0]
    moved = cb.to("cpu")
    assert moved.K == 3 and torch.equal(moved.cluster_atoms, cb.cluster_atoms)
    empty = ConstraintBatch([None, None])
    assert empty.K == 0 and empty.cluster_molptr.tolist() == [0, 0, 0] and empty.cluster_atoms.shape == (0, 5)
    for bad in (0.0, 2.0 ** -21, 2.0 ** -6, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tolerance"):
            ConstraintBatch([a], tolerance=bad)
    with pytest.raises(TypeError):
        ConstraintBatch([[0, 1]])


# ------------------------------------------------------------------------------------------------ the restatement alone
def test_the_cases_are_what_the_gpu_tests_need():
    sizes = {n: mc.case(n)[0].counts for n in mc.CASES}
    assert sizes["xh_C1"] == [2] and sizes["xh4"] == [5] and sizes["mix"] == [18, 7, 0] and sizes["edge256"] == [255, 256, 257]
    assert sizes["k256"] == [512] and sizes["ethane64"] == [8] and mc.case("ethane64")[0].xyz.shape[1] == 64
    assert mc.tables("xh_C1").K == 1 and mc.tables("xh4").leaf.tolist() == [[1, 2, 3, 4]]
    mix = mc.case("mix")[1]
    assert sorted((mix[0].clusters[:, 1:] >= 0).sum(1).tolist()) == [1, 2, 3] and mix[1] is None and mix[2] is None
    assert mix[0].n_constraints < 18 - mix[0].n_clusters          # free atoms next to the clusters
    # scattered: the same molecule in another order, and no leaf's ordinary owner (its own index) is its cluster's thread
    sc = mc.case("scattered")[1][0]
    assert sorted((sc.clusters[:, 1:] >= 0).sum(1).tolist()) == [1, 2, 3]
    for q, row in enumerate(sc.clusters.tolist()):
        assert all(a != q for a in row[1:] if a >= 0)
    assert not np.array_equal(mc.case("scattered")[2][:18], mc.case("mix")[2][:18])
    # edge256: in the molecule of 257 atoms a cluster has atoms on both sides of index 256
    last = mc.case("edge256")[1][2].clusters
    assert any(row[0] < 256 <= max(row[1:]) for row in last.tolist())
    k = mc.case("k256")[1][0]
    assert k.n_clusters == 256 and k.n_constraints == 256
    assert (mc.case("ethane64")[1][0].clusters[:, 1:] >= 0).sum(1).tolist() == [3, 3]
    assert mc.degrees_of_freedom("ethane64").tolist() == [18] and mc.degrees_of_freedom("mix").tolist() == [48, 21, 0]


@pytest.mark.parametrize("name", ["xh_C3", "xh4", "mix", "scattered"])
def test_newton_converges_well_inside_the_cap_and_holds_the_lengths(name):
    """40 steps of 2 fs in float32 and float64: every S converges in at most MAX_ITER / 2 updates (the issue's survey: 3), the bonds
    are at their lengths within the tolerance and P leaves r . (v_k - v_0) at rounding"""
    batch, cons, m, _ = mc.case(name)
    tab = mc.tables(name)
    for dtype, veps in ((torch.float32, 2.0 ** -18), (torch.float64, 2.0 ** -40)):
        r = mc.gbaoab_ref(batch, m, cons, dtype, velocities=mc.thermal_velocities(name), n_steps=40, dt=mc.TRAJ_DT)
        assert r["updates"] <= mc.MAX_ITER // 2, r["updates"]
        assert not r["status"].any()
        err, _ = mc.bond_errors(tab, r["xyz"])
        ulp = 4 * 2.0 ** -23 * float(r["xyz"].abs().max()) if dtype == torch.float32 else 0.0
        assert float((err * tab.d[tab.leaf >= 0][:, None]).max()) <= mc.TOL * mc.D_XH * 1.0001 + ulp
        ve = mc.velocity_errors(tab, r["xyz"], r["vel"])
        print(f"{name} {dtype}: updates {r['updates']}, bond error {float(err.max()):.3e} of d, |r.(vk - v0)| / (|r| max|v|) = "
              f"{float(ve.max() / r['vel'].abs().max()):.3e}")
        assert float(ve.max()) <= veps * float(r["vel"].abs().max())


@pytest.mark.parametrize("name", ["xh_C1", "edge256", "k256", "ethane64"])
def test_newton_converges_well_inside_the_cap_on_the_other_cases(name):
    """the remaining cases, 40 steps of 2 fs in float32 (the arithmetic of the kernel)"""
    batch, cons, m, keys = mc.case(name)
    start = dict(keys=keys, init_temperature=600.0) if name == "ethane64" else dict(velocities=mc.thermal_velocities(name))
    r = mc.gbaoab_ref(batch, m, cons, torch.float32, n_steps=40, dt=mc.TRAJ_DT, **start)
    assert r["updates"] <= mc.MAX_ITER // 2 and not r["status"].any() and bool((r["steps"] == 40).all())
    err, _ = mc.bond_errors(mc.tables(name), r["xyz"])
    assert float(err.max()) <= mc.TOL + 4 * 2.0 ** -23 * float(r["xyz"].abs().max()) / mc.D_XH


def test_projection_is_idempotent_to_rounding():
    for name in ("xh4", "mix"):
        batch, cons, m, _ = mc.case(name)
        for dtype, eps in ((torch.float32, 2.0 ** -20), (torch.float64, 2.0 ** -48)):
            mm = torch.from_numpy(m).to(dtype)
            w = torch.where(mm > 0, 1.0 / mm, torch.zeros_like(mm))
            cl = mc.Clusters(mc.tables(name), w, dtype)
            x, v = batch.xyz.to(dtype), mc.thermal_velocities(name).to(dtype)
            once = cl.project(x, v)
            twice = cl.project(x, once)
            assert float((once - v).abs().max()) > 0.1          # it does something
            assert float((twice - once).abs().max()) <= eps * float(v.abs().max())
            free = torch.ones(batch.N, dtype=torch.bool)
            tab = mc.tables(name)
            free[tab.centre] = False
            free[tab.leaf[tab.leaf >= 0]] = False
            assert torch.equal(once[free], v[free])          # free atoms are not touched


def test_an_unsatisfiable_cluster_sets_the_flag_in_both_dtypes():
    batch, cons, m, _, v = mc.unsatisfiable()
    for dtype in (torch.float32, torch.float64):
        r = mc.gbaoab_ref(batch, m, cons, dtype, velocities=v, n_steps=3, dt=0.001)
        assert r["status"].tolist() == [[4]] and r["steps"].tolist() == [[0]]
        ok = mc.gbaoab_ref(batch, m, cons, dtype, velocities=v * 0.001, n_steps=3, dt=0.001)
        assert ok["status"].tolist() == [[0]] and ok["steps"].tolist() == [[3]]


def test_frozen_ends():
    """a frozen centre and a frozen leaf keep their bits while the bond holds; a cluster frozen at both ends is ignored"""
    batch, cons, m, _ = mc.case("mix")
    tab = mc.tables("mix")
    sizes = (tab.leaf >= 0).sum(1)
    one, three = int(torch.nonzero(sizes == 1)[0]), int(torch.nonzero(sizes == 3)[0])
    mf = m.copy()
    mf[int(tab.centre[three])] = 0.0                                   # a frozen centre
    mf[int(tab.leaf[three, 0])] = 0.0                                  # ... one of whose leaves is frozen too: that bond is absent
    two = int(torch.nonzero(sizes == 2)[0])
    mf[int(tab.leaf[two, 1])] = 0.0                                    # a frozen leaf on a moving centre
    mf[[int(tab.centre[one]), int(tab.leaf[one, 0])]] = 0.0            # a cluster with both ends frozen
    r = mc.gbaoab_ref(batch, mf, cons, torch.float32, velocities=mc.thermal_velocities("mix"), n_steps=10, dt=mc.TRAJ_DT)
    assert not r["status"].any()
    for a in np.nonzero(mf[:18] == 0)[0]:
        assert torch.equal(r["xyz"][a], batch.xyz[a]) and not r["vel"][a].any()
    err, _ = mc.bond_errors(tab, r["xyz"])
    k, j = torch.nonzero(tab.leaf >= 0, as_tuple=True)
    held = torch.tensor([not (mf[int(tab.centre[a])] == 0 and mf[int(tab.leaf[a, b])] == 0) for a, b in zip(k.tolist(), j.tolist())])
    assert float(err[held].max()) <= 2 * mc.TOL


def test_the_trajectory_yardstick_is_steady_for_the_chosen_seeds():
    """the share of items that the farthest sibling calibrates, from the restatement alone, stays within tests/test_gpu_md.py's own
    share on its cases (22 of 309 for v): see the gate in tests/test_gpu_md_cons.py"""
    shaky = total = 0
    for name in mc.TRAJ_CASES:
        batch = mc.case(name)[0]
        for n_steps in mc.TRAJ_STEPS:
            each = torch.stack([mc.item_max(batch, r[n_steps][0][1].double() - r[n_steps][1][1]) for r in mc.verlet32(name)])
            floor = 2.0 ** -20 * mc.item_max(batch, mc.verlet(name)["snap"][n_steps][1])
            steady = (each[1:] <= 4 * each[0] + floor).all(0)
            shaky, total = shaky + int((~steady).sum()), total + steady.numel()
    print(f"{shaky} of {total} items calibrated by the farthest sibling")
    assert shaky * 309 <= 22 * total
