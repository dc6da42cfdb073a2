"""CPU: the nonbonded cutoff's front ends (`Cutoff`, `simulate(..., cutoff=)`) through recording fakes, the new symbols, properties of
the restatement of tests/nb_cut_refs.py alone, and the conditions tests/test_gpu_nb_cut.py puts on its own inputs."""
import os
import re

import numpy as np
import pytest
import torch

import nb_cut_refs as nc
import nonbonded_refs as nr
from grappa_amd import _lib, backend
from grappa_amd.dynamics import simulate, simulate_graph
from grappa_amd.nonbonded import Cutoff, NonbondedBatch, as_cutoff
from grappa_amd.relax import graph_from_parameters
from test_host_md_steps import FakeBackend, _big, _small

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"grappa_nonbonded_cut_workspace_bytes", "grappa_nonbonded_fwd_cut_f32", "grappa_md_steps_cut_workspace_bytes",
         "grappa_md_steps_init_cut_f32", "grappa_md_steps_run_cut_f32", "grappa_md_steps_finish_cut_f32"}


# ------------------------------------------------------------------------------------------------ Cutoff
def test_cutoff_validates_as_the_abi_does():
    c = Cutoff(9.0)
    assert c.as_opts() == {"cutoff": 9.0, "switch_distance": 0.0, "rf_dielectric": 78.3, "prune": 1}
    assert Cutoff(9.0, 7.2, 1.0, False).as_opts() == {"cutoff": 9.0, "switch_distance": 7.2, "rf_dielectric": 1.0, "prune": 0}
    assert Cutoff(9.0, 0).as_opts()["switch_distance"] == 0.0
    assert as_cutoff(None) is None and as_cutoff(c) is c and as_cutoff(6.5) == Cutoff(6.5) and as_cutoff(np.float32(6.5)) == Cutoff(6.5)
    for bad in (0.0, -1.0, float("inf"), float("nan"), "9", None, True):
        with pytest.raises(ValueError, match="distance"):
            Cutoff(bad)
    for bad in (9.0, 10.0, -1.0, float("nan"), "7"):
        with pytest.raises(ValueError, match="switch_distance"):
            Cutoff(9.0, bad)
    for bad in (0.5, float("inf"), float("nan"), None):
        with pytest.raises(ValueError, match="rf_dielectric"):
            Cutoff(9.0, None, bad)
    with pytest.raises(ValueError, match="prune"):
        Cutoff(9.0, prune=2)
    assert [n for n, _ in _lib.NbCut._fields_] == ["cutoff", "switch_distance", "rf_dielectric", "prune"]


# ------------------------------------------------------------------------------------------------ front ends
class CutFake(FakeBackend):
    """the recording fake of tests/test_host_md_steps.py whose md_steps also takes (and records) a cutoff"""

    def md_steps(self, *args, cutoff=None, **kw):
        super().md_steps(*args, **kw)
        self.calls[-1]["cutoff"] = cutoff


@pytest.fixture
def fake():
    old = backend._BACKEND
    be = CutFake()
    backend.set_backend(be)
    yield be
    backend.set_backend(old)


@pytest.fixture
def strict():          # the fake of the existing host tests as it stands: its md_steps does not know the keyword
    old = backend._BACKEND
    be = FakeBackend()
    backend.set_backend(be)
    yield be
    backend.set_backend(old)


def test_auto_with_a_cutoff_goes_stepwise_whatever_the_size(fake):
    mol, p, xyz, m = _small()
    simulate(p, xyz, m, mol["nb"], device="cpu", stepwise="auto", n_steps=2, cutoff=9.0)
    assert [c["which"] for c in fake.calls] == ["steps"] and fake.calls[-1]["cutoff"] == Cutoff(9.0)
    simulate(p, xyz, m, mol["nb"], device="cpu", stepwise=True, n_steps=2, cutoff=Cutoff(9.0, 7.2, 1.0))
    assert fake.calls[-1]["which"] == "steps" and fake.calls[-1]["cutoff"] == Cutoff(9.0, 7.2, 1.0)
    g = graph_from_parameters(p, xyz)
    simulate_graph(g, m, NonbondedBatch([mol["nb"]]), stepwise="auto", n_steps=2, cutoff=6.0)
    assert fake.calls[-1]["which"] == "steps" and fake.calls[-1]["cutoff"] == Cutoff(6.0) and len(fake.calls) == 3


def test_without_a_cutoff_the_calls_are_todays(strict):
    mol, p, xyz, m = _small()
    simulate(p, xyz, m, mol["nb"], device="cpu", stepwise="auto", n_steps=2)
    simulate(p, xyz, m, mol["nb"], device="cpu", stepwise=True, n_steps=2, cutoff=None)
    _, pb, xb, mb = _big()
    simulate(pb, xb, mb, None, device="cpu", stepwise="auto", n_steps=2, cutoff=None)
    assert [c["which"] for c in strict.calls] == ["fused", "steps", "steps"]
    assert all("cutoff" not in c for c in strict.calls)


def test_front_end_refusals(fake):
    mol, p, xyz, m = _small()
    g = graph_from_parameters(p, xyz)
    nbb = NonbondedBatch([mol["nb"]])
    for kw in ({}, {"stepwise": False}):
        with pytest.raises(ValueError, match=r'stepwise="auto"'):
            simulate(p, xyz, m, mol["nb"], device="cpu", n_steps=2, cutoff=9.0, **kw)
        with pytest.raises(ValueError, match=r'stepwise="auto"'):
            simulate_graph(g, m, nbb, n_steps=2, cutoff=9.0, **kw)
    with pytest.raises(ValueError, match="needs the nonbonded parameters"):
        simulate(p, xyz, m, None, device="cpu", stepwise="auto", n_steps=2, cutoff=9.0)
    with pytest.raises(ValueError, match="needs the nonbonded parameters"):
        simulate_graph(g, m, None, stepwise="auto", n_steps=2, cutoff=9.0)
    with pytest.raises(ValueError, match="distance"):
        simulate(p, xyz, m, mol["nb"], device="cpu", stepwise="auto", n_steps=2, cutoff=-3.0)
    from grappa_amd.constraints import Constraints
    cons = Constraints(np.array([[0, 1, -1, -1, -1]]), np.array([[1.09, 0.0, 0.0, 0.0]]))
    with pytest.raises(ValueError, match="constraints run on the fused path only"):
        simulate(p, xyz, m, mol["nb"], device="cpu", stepwise="auto", n_steps=2, cutoff=9.0, constraints=cons)
    assert not fake.calls, "a refused call reached the backend"


def test_symbols_header_and_abi():
    assert NAMES <= set(_lib.SIGNATURES)
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "grappa_hip.h")).read()
    for n in NAMES:
        assert getattr(lib, n) is not None and re.search(r"\b" + n + r"\(", text), n
    assert "typedef struct grappa_nb_cut" in text and lib.grappa_abi_version() == 11 == _lib.ABI_VERSION
    sig = _lib.SIGNATURES
    # the existing argument lists with `cut` after nb
    for n in ("init", "run", "finish"):
        old, new = sig[f"grappa_md_steps_{n}_f32"][1], sig[f"grappa_md_steps_{n}_cut_f32"][1]
        assert len(new) == len(old) + 1 and new[:3] == old[:3] and new[4:] == old[3:]
    assert len(sig["grappa_nonbonded_fwd_cut_f32"][1]) == 12
    w, wc = lib.grappa_md_steps_workspace_bytes, lib.grappa_md_steps_cut_workspace_bytes
    assert wc(0, 3, 1, 0) == 0 and wc(65, 3, 1, 2) > w(65, 3, 1, 2) and wc(65, 3, 1, 2) - w(65, 3, 1, 2) >= 88 * 2 * 3
    assert lib.grappa_nonbonded_cut_workspace_bytes(3, 0) == 0 and lib.grappa_nonbonded_cut_workspace_bytes(3, 2) >= 56 * 6
    # the host refuses before it touches the device
    assert lib.grappa_nonbonded_fwd_cut_f32(None, None, None, None, 0, 0, None, None, None, None, None, 0) == -1
    cut = _lib.NbCut(cutoff=9.0, switch_distance=0.0, rf_dielectric=78.3, prune=1)
    import ctypes as C
    assert lib.grappa_md_steps_init_cut_f32(None, None, None, C.byref(cut), None, None, None, None, None, 0, 0, None, 0) == -1      # a cut without nb
    assert lib.grappa_md_steps_init_cut_f32(None, None, None, None, None, None, None, None, None, 0, 0, None, 0) == -1             # forwards: NULL mm
    assert lib.grappa_md_steps_run_cut_f32(None, None, None, C.byref(cut), None, None, None, None, 0, 0, None, 0, 0, 1, None, None, None) == -1
    assert lib.grappa_md_steps_finish_cut_f32(None, None, None, C.byref(cut), None, None, 0, 0, None, 0, None, None, None, None, None, None) == -1


def test_one_definition_of_the_rule_and_of_the_pair():
    src = lambda f: open(os.path.join(ROOT, "grappa_amd", "csrc", f)).read()      # noqa: E731
    files = [f for f in sorted(os.listdir(os.path.join(ROOT, "grappa_amd", "csrc"))) if f.endswith((".h", ".hip"))]
    defs = lambda name: [f for f in files if re.search(r"\b(void|float|bool) " + name + r"\(", src(f))]      # noqa: E731
    assert defs("nb_pair_cut") == ["nb_pair.h"] and defs("nb_cut_decide") == ["nb_cut.h"] and defs("nb_cut_gap2") == ["nb_cut.h"]
    assert defs("nb_cut_box_write") == ["nb_cut.h"] and defs("rs_force") == ["rs_force.h"]
    assert "nb_cut.h" in src("Makefile")


# ------------------------------------------------------------------------------------------------ the restatement alone
def test_a_cutoff_above_the_diameter_without_reaction_field_is_the_plain_lennard_jones():
    params, _, x, r64, _ = nr.case("mixed")
    got = nc.nb_cut_ref(params, x, Cutoff(1000.0, None, 1.0), torch.float64)
    assert torch.allclose(got["terms"][0], r64["terms"][0], rtol=1e-13, atol=0)
    # eps = 1: k_rf = 0, the Coulomb energy is the plain one shifted by K q q / rc per pair, so its gradient is the plain one
    assert torch.allclose(got["grad"], r64["grad"], rtol=1e-12, atol=1e-12)


def test_the_energy_is_continuous_at_the_cutoff_and_the_gradient_is_its_derivative():
    from grappa_amd.nonbonded import NonbondedParameters
    p = [NonbondedParameters([0.4, -0.3], [3.0, 3.4], [0.1, 0.2])]
    for cut in (Cutoff(6.0, 4.8, 78.3), Cutoff(6.0, 4.8, 1.0), Cutoff(6.0, None, 78.3)):
        rc = nc.constants(cut)["rc"]
        pos = lambda r: torch.tensor([[[0.0, 0.0, 0.0]], [[r, 0.0, 0.0]]], dtype=torch.float64)      # noqa: E731
        inside, outside = nc.nb_cut_ref(p, pos(rc * (1 - 1e-9)), cut), nc.nb_cut_ref(p, pos(rc * (1 + 1e-9)), cut)
        assert float(outside["energy"].abs().max()) == 0.0 and float(outside["grad"].abs().max()) == 0.0
        # (k_rf and c_rf are rounded to float32, as the library holds them: each leaves u32 of its term)
        k = nc.constants(cut)
        bound = 4 * 2.0 ** -24 * 332.0637 * 0.12 * (1 / rc + k["krf"] * rc * rc + k["crf"])
        assert abs(float(inside["terms"][1])) < bound, "the reaction-field Coulomb energy vanishes at rc"
        if cut.switch_distance:
            assert abs(float(inside["terms"][0])) < 1e-12, "the switched Lennard-Jones energy vanishes at rc"
        for r in (3.3, 4.7, 4.9, 5.5, 5.95):
            h = 1e-6
            fd = (float(nc.nb_cut_ref(p, pos(r + h), cut)["energy"]) - float(nc.nb_cut_ref(p, pos(r - h), cut)["energy"])) / (2 * h)
            g = float(nc.nb_cut_ref(p, pos(r), cut)["grad"][1, 0, 0])
            assert abs(fd - g) <= 1e-7 * max(1.0, abs(g)), (cut, r, fd, g)


def test_the_gradient_of_a_molecule_is_the_finite_difference_of_its_energy():
    params, _, x = nc.inputs("c129_C3")
    cut = nc.cutoff_of("c129_C3", 6.0, True, 78.3)
    x64 = x[:, :1].double()
    g = nc.nb_cut_ref(params, x64, cut)["grad"]
    rng = np.random.default_rng(5)
    for atom, ax in zip(rng.integers(0, 129, 6), rng.integers(0, 3, 6)):
        h = 1e-5
        xp, xm = x64.clone(), x64.clone()
        xp[atom, 0, ax] += h
        xm[atom, 0, ax] -= h
        fd = (float(nc.nb_cut_ref(params, xp, cut)["energy"]) - float(nc.nb_cut_ref(params, xm, cut)["energy"])) / (2 * h)
        assert abs(fd - float(g[atom, 0, ax])) <= 1e-6 * max(1.0, abs(fd)), (atom, ax, fd, float(g[atom, 0, ax]))


# ------------------------------------------------------------------------------------------------ conditions on the GPU inputs
def test_the_inputs_of_the_gpu_tests_keep_their_distance_from_every_edge():
    """for every case the half gap around the placed cutoff is at least 1e-4 A (the fp32 error of r is about 1e-6 A), no tile has d2
    within a relative 1e-5 of the threshold, and on the 513-atom chain the expected tiles are fewer than all tiles"""
    for name, nominal in nc.CASES:
        rc, half = nc.placed(name, nominal)
        assert abs(rc - nominal) <= nc.WINDOW + 1e-6 and half >= 1e-4, (name, nominal, rc, half)
        params, _, x = nc.inputs(name)
        got, full, closest = nc.expected_tiles(params, x.numpy(), nc.cutoff_of(name, nominal, False, 78.3))
        assert closest >= 1e-5, (name, nominal, closest)
        assert (got <= full).all() and (got >= 1).all()
        if name == "c513_C3":
            assert got.sum() < full.sum() and got.sum() == 25 and full.sum() == 81, (got.sum(), full.sum())
        if name == "c513_far_exception":          # the exception between the ends keeps the whole row of both end blocks
            assert got[0] == 9 and got[-1] == 9 and got.sum() < full.sum()
    got, full, _ = nc.expected_tiles(*[nc.inputs("c129_C3")[k] for k in (0,)], nc.inputs("c129_C3")[2].numpy(), nc.cutoff_of("c129_C3", 6.0, False, 78.3))
    assert got.sum() == 7 and full.sum() == 9
    got, full, _ = nc.expected_tiles(nc.inputs("c513_C3")[0], nc.inputs("c513_C3")[2].numpy(), nc.cutoff_of("c513_C3", 6.0, False, 78.3), prune=False)
    assert (got == full).all()


def test_the_big_chain_takes_its_verdicts_in_two_batches_and_keeps_its_distance_from_the_threshold():
    """257 tiles per work item, one more than a batch of verdicts holds; no tile has d2 within a relative 1e-5 (above nb_cut_refs.MARGIN)
    of the threshold; far fewer tiles than all are expected (every item its own tile at least, so the last item tile 256)"""
    params, _, x = nc.inputs(nc.BIG)
    assert (nc.BIG, nc.BIG_CUTOFF) not in nc.CASES and x.shape == (16448, 1, 3)
    got, full, closest = nc.expected_tiles(params, x.numpy(), Cutoff(nc.BIG_CUTOFF, 0.8 * nc.BIG_CUTOFF))      # (the GPU test's cutoff)
    assert len(got) == 257 and (full == 257).all() and 257 > nc.NT
    assert closest >= 1e-5 > nc.MARGIN, closest
    assert (got >= 2).all() and got.sum() < full.sum() // 16, (got.min(), got.sum())
