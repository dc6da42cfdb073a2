"""CPU: the GB/SA implicit solvent on the minimiser's front ends (`relax_graph`, `relax`, `Grappa.relax`, `torsion_scan` and the
signature of `HipBackend.relax_steps_gb`) through the recording fake of tests/test_host_relax_steps.py, the new symbols, the workspace
arithmetic, the one arithmetic of the FIRE partials, and the conditions tests/test_gpu_relax_gb.py puts on its own inputs, decided from
the restatement of tests/relax_gb_refs.py alone."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import gb_refs as gr
import relax_gb_refs as rg
import relax_refs as rr
import relax_steps_refs as rs
from grappa_amd import _lib, backend
from grappa_amd.nonbonded import NonbondedBatch
from grappa_amd.relax import RELAX_DEFAULTS, RelaxResult, graph_from_parameters, relax, relax_graph, torsion_scan
from grappa_amd.solvent import GBBatch, GBParameters, ImplicitSolvent
from test_host_relax_steps import FakeBackend, _big, _small

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"grappa_relax_steps_gb_workspace_bytes", "grappa_relax_steps_init_gb_f32", "grappa_relax_steps_run_gb_f32",
         "grappa_relax_steps_finish_gb_f32"}


# ------------------------------------------------------------------------------------------------ front ends
class GbFake(FakeBackend):
    """the recording fake of tests/test_host_relax_steps.py with a relax_steps_gb that records the solvent's arguments and runs the
    vacuum restatement (what it computes is not looked at here: the solvent restatement is tests/relax_gb_refs.py's)"""

    def relax_steps_gb(self, plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, xyz_out, energy, gmax, steps, status, term_energy=None, grad=None,
                       atom_counts_host=None, check_every=None, workspace=None, gb=None, solvent=None, esolv=None):
        self._restate("steps_gb", plan, xyz, ks, eqs, n_per, nb, opts, xyz_out, energy, gmax, steps, status, list(atom_counts_host),
                      check_every=check_every, gb=gb, solvent=solvent, esolv=esolv)
        esolv.fill_(-1.5)


@pytest.fixture
def fake():
    old = backend._BACKEND
    be = GbFake()
    backend.set_backend(be)
    yield be
    backend.set_backend(old)


@pytest.fixture
def strict():          # the fake of the existing host tests as it stands: it has no relax_steps_gb and its seams know no new keyword
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


def _gbp(n=9):
    return GBParameters.from_elements(np.full(n, 6), [(a, a + 1) for a in range(n - 1)])


OPTS = dict(max_steps=2, tolerance=0.0)


def test_without_a_solvent_the_calls_are_todays(strict):
    mol, p, xyz = _small()
    relax(p, xyz, mol["nb"], device="cpu", stepwise="auto", **OPTS)
    relax(p, xyz, mol["nb"], device="cpu", stepwise=True, implicit_solvent=None, gb=None, **OPTS)
    _, pb, xb = _big()
    relax(pb, xb, None, device="cpu", stepwise="auto", implicit_solvent=None, **OPTS)
    relax_graph(graph_from_parameters(p, xyz), NonbondedBatch([mol["nb"]]), stepwise=True, implicit_solvent=None, gb=None, **OPTS)
    w = _wrapper(p)
    w.relax(None, xyz, mol["nb"], stepwise=True, **OPTS)
    w.relax(None, xyz, mol["nb"], stepwise=True, implicit_solvent=None, **OPTS)
    r = w.relax(None, xyz, mol["nb"], **OPTS)
    assert [c["which"] for c in strict.calls] == ["fire", "steps", "steps", "steps", "steps", "steps", "fire"]
    assert all(not {"gb", "solvent", "esolv", "implicit_solvent", "cutoff"} & set(c) for c in strict.calls)
    assert r.esolv is None and RelaxResult(1, 2, 3, 4, 5).esolv is None
    assert [f for f in RelaxResult.__dataclass_fields__][-3:] == ["restraint_energy", "dihedrals", "esolv"]


def test_a_solvent_reaches_relax_steps_gb_with_its_tables(fake):
    mol, p, xyz = _small()          # nine atoms: within the fused limit, "auto" goes stepwise all the same
    gbp = _gbp()
    r = relax(p, xyz, mol["nb"], device="cpu", stepwise="auto", implicit_solvent="obc1", gb=gbp, check_every=5, **OPTS)
    a = fake.calls[-1]
    assert [c["which"] for c in fake.calls] == ["steps_gb"] and a["counts"] == [9] and a["check_every"] == 5
    assert a["solvent"] == ImplicitSolvent("obc1") and isinstance(a["gb"], GBBatch) and a["gb"].counts == [9] and "cutoff" not in a
    assert a["opts"] == {**RELAX_DEFAULTS, **OPTS}          # the solvent is no relaxation option
    assert tuple(a["esolv"].shape) == (1, 3) and r.esolv.shape == r.energy.shape == (3,) and r.esolv.tolist() == [-1.5] * 3
    relax(p, xyz, mol["nb"], device="cpu", stepwise=True, implicit_solvent=ImplicitSolvent(surface_tension=0.0), gb=gbp, **OPTS)
    assert fake.calls[-1]["which"] == "steps_gb" and fake.calls[-1]["solvent"].surface_tension == 0.0
    g = graph_from_parameters(p, xyz)
    rg_ = relax_graph(g, NonbondedBatch([mol["nb"]]), stepwise="auto", implicit_solvent="obc2", gb=GBBatch([gbp]), **OPTS)
    assert fake.calls[-1]["which"] == "steps_gb" and tuple(rg_.esolv.shape) == (1, 3) and rg_.restraint_energy is None


def test_grappa_relax_builds_the_parameters_from_the_elements(fake):
    """Grappa.relax(..., implicit_solvent=) makes GBParameters.from_elements of the molecule's atomic numbers and bonds (atom ids mapped
    to positions), as Grappa.simulate does; without the keyword nothing of the solvent is passed on"""
    from types import SimpleNamespace
    mol, p, xyz = _small()
    n = 9
    z = np.where(np.arange(n) % 3 == 0, 7, 1)
    ids = np.arange(n) + 100          # atom ids that are not positions
    molecule = SimpleNamespace(atomic_numbers=z, bonds=[(100 + a, 101 + a) for a in range(n - 1)], atoms=ids)
    w = _wrapper(p)
    w.relax(molecule, xyz, mol["nb"], implicit_solvent="obc2", stepwise="auto", **OPTS)
    w.relax(molecule, xyz, mol["nb"], **OPTS)
    a, b = fake.calls
    want = GBParameters.from_elements(z, [(k, k + 1) for k in range(n - 1)])
    assert a["which"] == "steps_gb" and np.allclose(a["gb"].radius.numpy(), want.radius) and want.radius.tolist().count(1.3) == 5
    assert b["which"] == "fire" and "gb" not in b


def test_what_a_solvent_refuses(fake):
    mol, p, xyz = _small()
    g, nbb, gbp, w = graph_from_parameters(p, xyz), NonbondedBatch([mol["nb"]]), _gbp(), _wrapper(p)
    kw = dict(implicit_solvent="obc2", gb=gbp)
    gkw = dict(implicit_solvent="obc2", gb=GBBatch([gbp]))
    for more in ({}, {"stepwise": False}):          # the default is the fused path
        with pytest.raises(ValueError, match=r'stepwise="auto"'):
            relax(p, xyz, mol["nb"], device="cpu", **kw, **more)
        with pytest.raises(ValueError, match=r'stepwise="auto"'):
            relax_graph(g, nbb, **gkw, **more)
        with pytest.raises(ValueError, match=r'stepwise="auto"'):
            w.relax(None, xyz, mol["nb"], **kw, **more)
    with pytest.raises(ValueError, match="needs the nonbonded parameters"):
        relax(p, xyz, None, device="cpu", stepwise="auto", **kw)
    with pytest.raises(ValueError, match="needs the nonbonded parameters"):
        relax_graph(g, None, stepwise="auto", **gkw)
    with pytest.raises(ValueError, match="cutoff"):
        relax(p, xyz, mol["nb"], device="cpu", stepwise="auto", cutoff=9.0, **kw)
    with pytest.raises(ValueError, match="cutoff"):
        relax_graph(g, nbb, stepwise="auto", cutoff=9.0, **gkw)
    with pytest.raises(ValueError, match="cutoff"):
        w.relax(None, xyz, mol["nb"], stepwise="auto", cutoff=9.0, **kw)
    from grappa_amd.restraints import RestraintBatch, Restraints
    restr = Restraints(position_k=np.ones(9))
    with pytest.raises(ValueError, match="restraints are taken by the fused minimiser only"):
        relax(p, xyz, mol["nb"], device="cpu", stepwise="auto", restraints=restr, **kw)
    with pytest.raises(ValueError, match="restraints are taken by the fused minimiser only"):
        relax_graph(g, nbb, stepwise="auto", restraints=RestraintBatch([restr], 3, atom_counts=[9]), **gkw)
    with pytest.raises(TypeError, match="GBParameters"):
        relax(p, xyz, mol["nb"], device="cpu", stepwise="auto", implicit_solvent="obc2")
    with pytest.raises(TypeError, match="GBBatch"):
        relax_graph(g, nbb, stepwise="auto", implicit_solvent="obc2", gb=gbp)
    with pytest.raises(ValueError, match="implicit_solvent"):
        relax(p, xyz, mol["nb"], device="cpu", stepwise="auto", gb=gbp)
    with pytest.raises(ValueError, match="model"):
        relax(p, xyz, mol["nb"], device="cpu", stepwise="auto", implicit_solvent="gbn2", gb=gbp)
    # a GBBatch made for another batch, or checked against a smaller offset than the solvent's
    with pytest.raises(ValueError, match="atoms"):
        relax(p, xyz, mol["nb"], device="cpu", stepwise="auto", implicit_solvent="obc2", gb=GBParameters([1.5], [0.8]))
    with pytest.raises(ValueError, match="atoms"):
        relax_graph(g, nbb, stepwise="auto", implicit_solvent="obc2", gb=GBBatch([_gbp(8)]))
    with pytest.raises(ValueError, match="offset"):
        relax_graph(g, nbb, stepwise="auto", implicit_solvent=ImplicitSolvent(offset=1.75), gb=GBBatch([gbp]))
    with pytest.raises(ValueError, match="no implicit solvent"):
        torsion_scan(p, xyz[0], [0, 1, 2, 4], angles=[0.0, 1.0], nonbonded=mol["nb"], device="cpu", **kw)
    with pytest.raises(ValueError, match="no implicit solvent"):
        w.torsion_scan(None, xyz[0], [0, 1, 2, 4], angles=[0.0, 1.0], nonbonded=mol["nb"], implicit_solvent="obc2")
    assert not fake.calls, "a refused call reached the backend"
    assert "implicit_solvent" not in RELAX_DEFAULTS and "gb" not in RELAX_DEFAULTS


def test_a_backend_without_the_seam_is_refused(strict):
    mol, p, xyz = _small()
    with pytest.raises(ValueError, match="relax_steps_gb"):
        relax(p, xyz, mol["nb"], device="cpu", stepwise="auto", implicit_solvent="obc2", gb=_gbp())
    assert not strict.calls


def test_the_backend_seam():
    from grappa_amd.backend import HipBackend
    par = inspect.signature(HipBackend.relax_steps_gb).parameters
    plain = inspect.signature(HipBackend.relax_steps).parameters
    assert list(par) == [k for k in plain if k != "cutoff"] + ["gb", "solvent", "esolv"]
    assert par["gb"].default is None and par["solvent"].default == "obc2" and par["esolv"].default is None
    doc = HipBackend.relax_steps_gb.__doc__
    assert "grappa_relax_steps_gb_workspace_bytes" in doc and "seven launches" in doc
    assert list(plain)[-2:] == ["workspace", "cutoff"]          # the seam without solvent is the one it was


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_header_and_abi():
    assert NAMES <= set(_lib.SIGNATURES)
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "grappa_hip.h")).read()
    for n in NAMES:
        assert getattr(lib, n) is not None and re.search(r"\b" + n + r"\(", text), n
    assert lib.grappa_abi_version() == 11 == _lib.ABI_VERSION
    sig = _lib.SIGNATURES
    for n in ("init", "run", "finish"):          # the _cut_ argument lists with `gb` after cut; finish also takes where esolv goes
        old, new = sig[f"grappa_relax_steps_{n}_cut_f32"][1], sig[f"grappa_relax_steps_{n}_gb_f32"][1]
        tail = 1 if n == "finish" else 0
        assert len(new) == len(old) + 1 + tail and new[:4] == old[:4] and new[4] == C.POINTER(_lib.GbDesc)
        assert new[5:len(new) - tail] == old[4:]
    # the header states the launches, which tests/test_gpu_relax_gb.py counts
    assert re.search(r"7 launches per step; init\s+\*?\s*gains the same three: 5", text) and re.search(r"grad is the total gradient\.\s+9 launches", text)
    # the host refuses before it touches the device (no GPU is needed for these)
    gb = _lib.GbDesc(radius=None, scale=None, **ImplicitSolvent().as_opts())
    assert lib.grappa_relax_steps_init_gb_f32(None, None, None, None, C.byref(gb), None, None, 0, 0, None, 0, None) == -1
    assert lib.grappa_relax_steps_run_gb_f32(None, None, None, None, C.byref(gb), None, None, 0, 0, None, 0, 1, None) == -1
    assert lib.grappa_relax_steps_finish_gb_f32(None, None, None, None, C.byref(gb), None, None, 0, 0, None, 0, None, None, None, None, None, None,
                                                None, None) == -1
    assert lib.grappa_relax_steps_init_gb_f32(None, None, None, None, None, None, None, 0, 0, None, 0, None) == -1      # gb == NULL: the plain call's answer


def test_the_workspace_is_the_plain_one_plus_the_solvents_words():
    """behind rs_layout's total: B, dBdI, w [N,C], the fixed-B gradient [N,C,3], e_gb [B,C], terms_gb [2,B,C] and the workspace of
    grappa_gb_obc_fwd_f32, each piece on a 256-byte boundary; the plain size is what it was (14 pieces of the state, 4 of the finish)"""
    lib = _lib.load()
    w, wg, wo = lib.grappa_relax_steps_workspace_bytes, lib.grappa_relax_steps_gb_workspace_bytes, lib.grappa_gb_obc_workspace_bytes
    up = lambda n: (n + 255) // 256 * 256      # noqa: E731
    for N, Cc, B, nblk in ((65, 3, 1, 2), (6500, 1, 1, 102), (74, 17, 2, 3), (513, 1, 1, 9), (1, 1, 1, 1)):
        nc, bc, kc = N * Cc, B * Cc, nblk * Cc
        plain = 3 * up(12 * nc) + 9 * up(4 * bc) + up(32 * kc) + up(4 * kc) + 2 * up(4 * bc) + up(24 * bc) + up(16 * kc)
        assert w(N, Cc, B, nblk) == plain, (N, Cc, B, nblk)
        assert wg(N, Cc, B, nblk) == plain + 3 * up(4 * nc) + up(12 * nc) + up(4 * bc) + up(8 * bc) + up(wo(N, Cc, nblk)), (N, Cc, B, nblk)
    assert wg(0, 3, 1, 0) == 0 and wg(10, 0, 1, 1) == 0 and wg(10, 3, 0, 1) == 0 and wg(65, 3, 1, -1) == 0
    assert wg(9, 1, 1, 0) == w(9, 1, 1, 0) + 3 * up(36) + up(108) + up(4) + up(8) + up(wo(9, 1, 1))          # (no block: the entry's size for one)


def _body(text, start, end):
    i = text.index(start)
    return text[i:text.index(end, i) + len(end)]


def test_one_arithmetic_for_the_partials():
    """the FIRE partials are produced by two epilogues: rs_force_body's (from g = bonded + nonbonded) and rs_gb_chain_kernel's (from the
    total gradient).  A shared function would have had to leave rs_force_kernel and rs_force_cut_kernel their instruction streams; the
    second copy is pinned instead: from the load of v to the store of the fourth partial the two texts are the same, word for word"""
    src = open(os.path.join(ROOT, "grappa_amd", "csrc", "relax_steps.hip")).read()
    force = src[src.index("void rs_force_body("):src.index("void rs_force_kernel(")]
    chain = src[src.index("void rs_gb_chain_kernel("):src.index("void rs_out_gb_kernel(")]
    a, b = (_body(t, "const V3 vi = ", "o[3] = (double)mg;") for t in (force, chain))
    assert a == b and "pg = gn <= FLT_MAX ? gn : INFINITY;" in a and "sP += (double)sh.red[0][o]" in a and a.count("__syncthreads();") == 2
    # the sum's order, that of ms_gb_chain_kernel: (g + ggb) + chain
    dyn = open(os.path.join(ROOT, "grappa_amd", "csrc", "dynamics_steps.hip")).read()
    assert "(a.g[off] + d[off]) + cx, (a.g[off + 1] + d[off + 1]) + cy, (a.g[off + 2] + d[off + 2]) + cz" in chain
    assert "(c.g[off] + c.a.gdir[off]) + cx, (c.g[off + 1] + c.a.gdir[off + 1]) + cy, (c.g[off + 2] + c.a.gdir[off + 2]) + cz" in dyn
    # the passes are csrc/gb_pass.h's, under the same instantiations as the dynamics'
    for t in (src, dyn):
        assert "gb_born_body<true>(a, sh)" in t and "gb_pair_body<true, false, true>(a, sh)" in t and "gb_chain_body<true>(" in t
    files = [f for f in sorted(os.listdir(os.path.join(ROOT, "grappa_amd", "csrc"))) if f.endswith((".h", ".hip"))]
    for body in ("gb_born_body", "gb_pair_body", "gb_chain_body"):
        assert [f for f in files if re.search(r"\bvoid " + body + r"\(", open(os.path.join(ROOT, "grappa_amd", "csrc", f)).read())] == ["gb_pass.h"]


# ------------------------------------------------------------------------------------------------ conditions on the GPU inputs
def test_case_tables():
    assert rg.TRAJ_CASES == ["s63_C3", "s64_C1", "s65_C3", "s129_C3", "s513_C1", "s9_65_C17", "s1_2_17_130_5_64_C3"]
    assert rg.CONV_CASES == ["s65_C1", "s2_130_9_C3", "s513_C1"] and rg.CONV_CPU_CASES == rg.CONV_CASES[:2] and rg.MIXED == rg.TRAJ_CASES[-1]
    for name in rg.TRAJ_CASES + rg.CONV_CASES:
        b, gbs = rg.case(name), rg.gb_params(name)
        assert [g.n_atoms for g in gbs] == b.counts == rs.case(name).counts


@pytest.mark.parametrize("name", rg.TRAJ_CASES + rg.CONV_CASES)
def test_no_pair_starts_on_a_branch_border(name):
    rep = gr.border_report(rg.gb_params(name), rg.case(name).xyz)
    moved = int((rg.case(name).xyz != rs.case(name).xyz).any(-1).sum())
    print(name, rep, f"{moved} (atom, conformation)s nudged")
    assert rep["disagree"] == 0 and rep["gap"] >= gr.GAP_OTHER


@pytest.mark.parametrize("name", rg.TRAJ_CASES)
def test_the_restated_trajectories_are_finite_and_go_uphill_once(name):
    """every restated state is finite, every item with more than one atom runs all 40 steps, and a step with P <= 0 occurs within them"""
    b = rg.case(name)
    real = torch.tensor([n > 1 for n in b.counts])[:, None].expand(b.B, b.xyz.shape[1])
    for dtype in (torch.float64, torch.float32):
        tr = rg.trajectory(name, dtype)
        assert sorted(tr["snap"]) == list(rr.TRAJ_STEPS)
        assert all(bool(torch.isfinite(x).all()) for x in tr["snap"].values()) and bool(torch.isfinite(tr["xyz"]).all())
        assert bool((tr["steps"][real] == max(rr.TRAJ_STEPS)).all()) and bool((tr["status"][real] == 0).all())
    worst = max(float((rg.trajectory(name, torch.float32)["snap"][k].double() - rg.trajectory(name)["snap"][k]).abs().max()) for k in rr.TRAJ_STEPS)
    print(f"{name}: largest |x_fp32 - x_f64| over the snapshots {worst:.3e} A")
    assert rg.has_uphill_step(name), f"{name}: no step with P <= 0 within 40 steps"
    # the solvent is part of the force: the trajectory is not the vacuum one
    if not (rg.case(name).xyz != rs.case(name).xyz).any():
        assert not torch.equal(rg.trajectory(name)["snap"][5], rs.trajectory(name)["snap"][5])


def test_branch_margin_of_the_trajectory_cases():
    """at most one in ten (item, step count) pairs loses the branch margin, and no case loses all of its items"""
    total = below = 0
    for name in rg.TRAJ_CASES:
        real = torch.tensor([n > 1 for n in rg.case(name).counts])[:, None]
        for k in rr.TRAJ_STEPS:
            ok = rg.margin_ok(name, k)
            r = real.expand_as(ok)
            total += int(r.sum())
            below += int((~ok & r).sum())
            assert bool((ok & r).any()), f"{name}, {k} steps: every conformation is below the branch margin"
    print(f"below the branch margin: {below} of {total} (item, step count) pairs")
    assert total == 180 and 10 * below <= total, (below, total)


def test_the_restated_force_is_the_vacuum_force_plus_the_solvent():
    name = "s65_C3"
    b = rg.case(name)
    wet, dry = rg.forces_of(name), rr.forces(b, b.xyz, torch.float64, True)
    want = gr.gb_ref(b.params, rg.gb_params(name), b.xyz, rg.MODEL, torch.float64, scales=False)
    assert torch.allclose(wet["E"] - dry["E"], want["energy"], rtol=0, atol=1e-9) and torch.allclose(wet["G"] - dry["G"], want["grad"], rtol=0, atol=1e-9)
    assert torch.equal(wet["terms"], dry["terms"]) and torch.equal(wet["solv"]["energy"], want["energy"])
    assert bool((wet["abs_e"] > dry["abs_e"]).all()) and bool((wet["abs_f"] > dry["abs_f"]).all())


@pytest.mark.parametrize("name", rg.CONV_CPU_CASES)
def test_convergence_cases_converge_in_float64_below_the_vacuum_minimum(name):
    """observed: s65_C1 634 steps (385 in vacuum), the solvent energy 266.97 -> -120.04 against -113.37 kcal/mol at the vacuum minimiser's
    coordinates; s2_130_9_C3 33 to 873 steps (33 to 1059 in vacuum), its 130-atom molecule 425 .. 565 -> -289.5 .. -289.7 against -273.9 ..
    -278.5.  The ordering is the reason the feature exists: the vacuum minimum is not the solvent's.  It is asserted on the molecules of
    relax_gb_refs.ORDERED, where it holds with a margin of ORDER_MARGIN."""
    r, v = rg.converged(name), rg.converged_in_vacuum(name)
    b = rg.case(name)
    print(f"{name}: steps {r['steps'].flatten().tolist()} (in vacuum {v['steps'].flatten().tolist()})")
    assert bool((r["status"] == 1).all()), (r["status"].tolist(), r["steps"].tolist())
    assert bool((r["steps"] <= rg.CONV_MAX_STEPS).all()) and bool((r["gmax"] <= RELAX_DEFAULTS["tolerance"]).all())
    e0, e1, ev = rg.forces_of(name)["E"], rg.forces(name, b, r["xyz"])["E"], rg.forces(name, b, v["xyz"])["E"]
    print(f"  solvent energy: start {e0.flatten().tolist()}\n  at its minimum {e1.flatten().tolist()}\n  at the vacuum minimum {ev.flatten().tolist()}")
    assert bool((e1 < e0).all()) and bool((v["status"] == 1).all())
    which = list(rg.ORDERED[name])
    assert bool((e1[which] < ev[which] - rg.ORDER_MARGIN).all()), "the solvent minimum is not below the vacuum minimiser's coordinates"
