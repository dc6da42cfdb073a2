"""CPU: the GB/SA implicit solvent's host side (grappa_amd/solvent.py) and the float64 restatement the GPU tests are gated against
(tests/gb_refs.py): the restatement's own properties, the parameter tables, validation, and the conditions the GPU tests' inputs have to
meet -- asserted here, so that the reference alone satisfies them."""
import numpy as np
import pytest
import torch

import gb_refs as gr
from grappa_amd.constants import COULOMB_CONSTANT
from grappa_amd.nonbonded import NonbondedParameters
from grappa_amd.solvent import GBBatch, GBParameters, ImplicitSolvent, as_implicit_solvent


def _nbp(q):
    q = np.asarray(q, dtype=np.float64)
    return NonbondedParameters(q, np.full(q.shape, 2.0), np.full(q.shape, 0.1)).validate()


def _x(rows):
    """(n, 3) -> (n, 1, 3) float32 tensor"""
    return torch.tensor(rows, dtype=torch.float32)[:, None, :]


# ------------------------------------------------------------------------------------------------------------------------- restatement
def test_a_lone_ion_is_the_born_formula():
    """radius 2 A, charge 1: B = R - offset = 1.91 and E_pol = -(K/2)(1 - 1/78.5) q^2 / B = -85.820"""
    r = gr.gb_ref([_nbp([1.0])], [GBParameters([2.0], [0.8])], _x([[0.3, -0.2, 0.1]]), ImplicitSolvent(surface_tension=0.0))
    assert abs(float(r["born"][0, 0]) - 1.91) < 1e-6
    want = -0.5 * COULOMB_CONSTANT * (1 - 1 / 78.5) / float(r["born"][0, 0])
    # (the restatement holds K (1/eps_in - 1/eps_out) rounded to float32, as the kernel does: one float32 rounding of the constant)
    assert abs(float(r["terms"][0, 0, 0]) - want) < 2.0 ** -23 * abs(want) and abs(want + 85.820) < 1e-3
    assert float(r["terms"][1, 0, 0]) == 0.0 and float(r["grad"].abs().max()) == 0.0


def test_equal_dielectrics_without_surface_tension_give_exactly_zero():
    nbp, gbp, x = gr.inputs("n2_C3")
    r = gr.gb_ref(nbp, gbp, x, ImplicitSolvent("obc2", 3.0, 3.0, 0.0))
    assert bool((r["energy"] == 0).all()) and bool((r["grad"] == 0).all())


def test_autograd_matches_finite_differences_away_from_kinks():
    """central differences of the float64 energy, h = 1e-5 A (the `branches` case keeps every pair 1e-3 A from a border)"""
    for name in ("branches", "n2_C3"):
        nbp, gbp, x = gr.inputs(name)
        r = gr.gb_ref(nbp, gbp, x)
        x64 = x.double()
        h = 1e-5
        for i in range(x.shape[0]):
            for k in range(3):
                xp, xm = x64.clone(), x64.clone()
                xp[i, :, k] += h
                xm[i, :, k] -= h
                # (gb_ref rounds nothing of float64 coordinates: it takes them as they are)
                fd = (gr.gb_ref(nbp, gbp, xp)["energy"][0] - gr.gb_ref(nbp, gbp, xm)["energy"][0]) / (2 * h)
                assert float((fd - r["grad"][i, :, k]).abs().max()) < 1e-6 * max(1.0, float(r["grad"].abs().max())), (name, i, k)


def test_obc1_and_obc2_differ():
    nbp, gbp, x = gr.inputs("n2_C3")
    a, b = gr.gb_ref(nbp, gbp, x, "obc1"), gr.gb_ref(nbp, gbp, x, "obc2")
    assert float((a["born"] - b["born"]).abs().min()) > 1e-4 and float((a["energy"] - b["energy"]).abs().min()) > 1e-3


def test_far_apart_fragments_tend_to_the_sum_of_the_parts():
    """a neutral pair of atoms (a dipole) and a charged one: what the whole has beyond its parts is the screened charge-dipole term of
    E_pol, which falls as 1/r^2, and the descreening of the Born radii, which falls as 1/r^4: four times the distance, less than a tenth"""
    gA, gB = GBParameters([1.7, 1.5], [0.72, 0.85]), GBParameters([1.55], [0.79])
    qA, qB = [0.4, -0.4], [1.0]
    xA, xB = [[0.0, 0.0, 0.0], [1.3, 0.0, 0.0]], [[0.0, 0.4, 0.0]]
    parts = float(gr.gb_ref([_nbp(qA)], [gA], _x(xA))["energy"][0, 0] + gr.gb_ref([_nbp(qB)], [gB], _x(xB))["energy"][0, 0])
    gap = []
    for dist in (20.0, 80.0, 320.0):
        xs = xA + [[dist, 0.4, 0.0]]
        e = float(gr.gb_ref([_nbp(qA + qB)], [GBParameters([1.7, 1.5, 1.55], [0.72, 0.85, 0.79])], _x(xs))["energy"][0, 0])
        gap.append(abs(e - parts))
    assert gap[1] < gap[0] / 10 and gap[2] < gap[1] / 10 and gap[2] < 1e-2 and gap[0] < 0.5, gap


def test_fp32_restatement_stays_near_float64():
    """the relative error of B is a few 1e-6 even where the tanh saturates (B up to 34 A on the 1.5 A lattice)"""
    r64, r32 = gr.refs("nTp1_C3")
    assert float(r64["born"].max()) > 30.0
    assert float(((r32["born"] - r64["born"]).abs() / r64["born"]).max()) < 4e-6


# ------------------------------------------------------------------------------------------------------------------------- parameters
def test_from_elements_tables():
    #            C  H(C) N  H(N) O  S   F  Si  P   Cl  Br
    z = np.array([6, 1, 7, 1, 8, 16, 9, 14, 15, 17, 35])
    bonds = [(0, 1), (0, 2), (3, 2), (0, 4), (0, 5)]
    p = GBParameters.from_elements(z, bonds)
    assert p.radius.tolist() == [1.7, 1.2, 1.55, 1.3, 1.5, 1.8, 1.5, 2.1, 1.85, 1.7, 1.5]
    assert p.scale.tolist() == [0.72, 0.85, 0.79, 0.85, 0.85, 0.96, 0.88, 0.8, 0.86, 0.8, 0.8]
    assert GBParameters.from_elements([1, 7], np.zeros((0, 2))).radius.tolist() == [1.2, 1.55]          # no bond: a plain hydrogen
    with pytest.raises(ValueError):
        GBParameters.from_elements([1, 7], [(0, 2)])
    d = p.to_dict()
    q = GBParameters.from_dict(d)
    assert np.array_equal(q.radius, p.radius) and np.array_equal(q.scale, p.scale) and sorted(d) == ["gbparam_radius", "gbparam_scale"]


def test_validation():
    for bad in (dict(model="hct"), dict(solute_dielectric=0.0), dict(solvent_dielectric=-1.0), dict(solvent_dielectric=float("nan")),
                dict(surface_tension=-1e-3), dict(probe=float("inf")), dict(offset=-0.1), dict(probe=True)):
        with pytest.raises(ValueError):
            ImplicitSolvent(**bad)
    assert as_implicit_solvent(None) is None and as_implicit_solvent("obc1").model == "obc1"
    s = ImplicitSolvent()
    assert as_implicit_solvent(s) is s
    with pytest.raises(ValueError):
        as_implicit_solvent(1.0)
    with pytest.raises(Exception):
        s.model = "obc1"          # frozen
    o = s.as_opts()
    assert (o["alpha"], o["beta"], o["gamma"]) == (1.0, 0.8, 4.85) and ImplicitSolvent("obc1").as_opts()["gamma"] == 2.909125
    assert (o["offset"], o["eps_in"], o["eps_out"], o["surface_tension"], o["probe"]) == (0.09, 1.0, 78.5, 0.0054, 1.4)
    for r, sc in (([0.09, 1.5], [0.8, 0.8]), ([0.05, 1.5], [0.8, 0.8]), ([1.5, float("nan")], [0.8, 0.8]), ([1.5, 1.5], [0.0, 0.8]),
                  ([1.5, 1.5], [0.8, -0.1]), ([1.5, 1.5], [0.8]), ([[1.5, 1.5]], [[0.8, 0.8]])):
        with pytest.raises(ValueError):
            GBParameters(r, sc).validate()
    with pytest.raises(ValueError):
        GBBatch([GBParameters([0.5], [0.8])], offset=0.6)
    b = GBBatch([GBParameters([1.5, 1.7], [0.8, 0.72]), GBParameters([], []), GBParameters([1.2], [0.85])])
    assert (b.B, b.N, b.counts) == (3, 3, [2, 0, 1]) and b.radius.dtype == torch.float32 and b.scale.tolist() == pytest.approx([0.8, 0.72, 0.85])


def test_the_numpy_door_checks_its_arguments():
    from grappa_amd.solvent import solvent_energy
    nbp, gbp, x = gr.inputs("n2_C3")
    xs = x.numpy().transpose(1, 0, 2)
    with pytest.raises(ValueError):
        solvent_energy(nbp[0], gbp[0], xs, device="cpu", model=None)
    with pytest.raises(ValueError):
        solvent_energy(nbp[0], GBParameters([1.5], [0.8]), xs, device="cpu")
    with pytest.raises(ValueError):
        solvent_energy(nbp[0], gbp[0], xs[:, :1], device="cpu")
    with pytest.raises(ValueError):
        solvent_energy([nbp[0]], [gbp[0], gbp[0]], [xs], device="cpu")


# ------------------------------------------------------------------------------------------------------------------------- GPU inputs
def test_branches_case_takes_every_branch_well_inside():
    nbp, gbp, x = gr.inputs("branches")
    rep = gr.border_report(gbp, x)
    print("branches:", rep)
    assert rep["disagree"] == 0 and rep["gap"] >= gr.GAP_BRANCHES
    assert all(rep["counts"][k] >= 1 for k in ("swallowed", "inside", "far", "overlap")), rep["counts"]


@pytest.mark.parametrize("name", [n for n in gr.CASES if n != "branches"])
def test_no_pair_sits_on_a_branch_border(name):
    nbp, gbp, x = gr.inputs(name)
    rep = gr.border_report(gbp, x)
    print(name, rep)
    assert rep["disagree"] == 0 and rep["gap"] >= gr.GAP_OTHER


def test_both_regimes_are_covered():
    """chain513: at least half of the atoms have B_i below half of their saturation value 1/(1/o_i - 1/R_i); the lattice cases reach
    saturation"""
    sat = gr.refs("chain513")[0]["sat"]
    low = float((sat < 0.5).double().mean())
    hi = float(gr.refs("nTp1_C3")[0]["sat"].max())
    print(f"chain513: {low:.3f} of the atoms below half saturation; lattice: B up to {hi:.3f} of saturation")
    assert low >= 0.5 and hi > 0.95


@pytest.mark.parametrize("name", gr.CASES)
def test_the_floors_of_the_gate_are_tight(name):
    """64 u32 scale against what it gates, in every case, the saturated lattice included: per atom at most 1 % of the atom's own
    gradient at the median and 0.1 % of the case's largest gradient at the most; at most 0.2 % of |E| (where E is not a cancelling
    sum: |E| >= 1 kcal/mol) and 0.02 % of B; and, against the fp32 restatement's own error, the median floor at most 300 times the
    median error and the smallest floor-to-error ratio at least 1 (the floor is no tighter than fp32 arithmetic itself)"""
    r64, r32 = gr.refs(name)
    u = 64 * 2.0 ** -24
    fl, gn = u * r64["abs_g"], r64["grad"].norm(dim=-1)
    err = (r32["grad"] - r64["grad"]).abs().amax(-1)
    live = fl > 0
    assert bool((u * r64["abs_born"] <= 2e-4 * r64["born"]).all())
    if not bool(live.any()):          # single atoms: no pair, no gradient
        return
    big = r64["energy"].abs() >= 1.0
    print(f"{name}: floor / |g_i| median {float((fl[live] / gn[live].clamp_min(1e-30)).median()):.2e}, largest floor / largest |g| "
          f"{float(fl.max() / gn.max()):.2e}; fp32 error / floor largest {float((err[live] / fl[live]).max()):.3f}, median floor / median error "
          f"{float(fl[live].median() / err[live].median().clamp_min(1e-30)):.0f}; energy floor / |E| largest "
          f"{float((u * r64['abs_e'][big] / r64['energy'][big].abs()).max()) if bool(big.any()) else 0.0:.2e}")
    assert float((fl[live] / gn[live].clamp_min(1e-30)).median()) <= 1e-2 and float(fl.max()) <= 1e-3 * float(gn.max())
    assert bool((u * r64["abs_e"][big] <= 2e-3 * r64["energy"][big].abs()).all())
    assert float((err[live] / fl[live]).max()) <= 1.0
    if err[live].numel() >= 8:
        assert float(fl[live].median()) <= 300 * float(err[live].median())


def test_the_scales_are_positive_and_finite():
    for name in ("branches", "mixed", "chain513"):
        r64 = gr.refs(name)[0]
        n_atoms = [p.n_atoms for p in gr.inputs(name)[0]]
        ptr = np.concatenate([[0], np.cumsum(n_atoms)])
        for k in ("abs_g", "abs_born", "abs_I"):
            assert bool(torch.isfinite(r64[k]).all()) and bool((r64["abs_born"] > 0).all()), (name, k)
        for b, n in enumerate(n_atoms):
            if n > 1:
                assert bool((r64["abs_g"][ptr[b]:ptr[b + 1]] > 0).all()) and bool((r64["abs_e"][b] > 0).all()), (name, b)


# ------------------------------------------------------------------------------------------------------------------------- the dynamics' C ABI
MD_NAMES = {"grappa_md_steps_gb_workspace_bytes", "grappa_md_steps_init_gb_f32", "grappa_md_steps_run_gb_f32", "grappa_md_steps_finish_gb_f32"}


def test_symbols_header_and_host_refusals():
    import ctypes as C
    import os
    import re
    from grappa_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "grappa_hip.h")).read()
    lib = _lib.load()
    for n in MD_NAMES | {"grappa_gb_obc_workspace_bytes", "grappa_gb_obc_fwd_f32"}:
        assert n in _lib.SIGNATURES and getattr(lib, n) is not None and re.search(r"\b" + n + r"\(", text), n
    sig = _lib.SIGNATURES
    # the _cons_ calls with the solvent added; run and finish also take where the solvent's energy goes
    assert len(sig["grappa_md_steps_init_gb_f32"][1]) == len(sig["grappa_md_steps_init_cons_f32"][1]) + 1
    assert len(sig["grappa_md_steps_run_gb_f32"][1]) == len(sig["grappa_md_steps_run_cons_f32"][1]) + 2
    assert len(sig["grappa_md_steps_finish_gb_f32"][1]) == len(sig["grappa_md_steps_finish_cons_f32"][1]) + 2
    # the header states the launches, which tests/test_gpu_md_gb.py and tests/test_gpu_gb.py count
    assert re.search(r"5 launches, 6 with constraints", text) and re.search(r"4 launches, 3 with grad == NULL", text)
    w, cons_w = lib.grappa_md_steps_gb_workspace_bytes, lib.grappa_md_steps_cons_workspace_bytes
    assert w(0, 3, 1, 0, 0) == 0 and w(10, 0, 1, 1, 0) == 0 and w(10, 3, 0, 1, 0) == 0 and w(65, 3, 1, 2, -1) == 0
    for K in (0, 5):          # the words of a run without solvent first, the solvent's behind them: B, dBdI, w, the fixed-B gradient, the entry's own
        extra = w(650, 3, 1, 12, K) - cons_w(650, 3, 1, 12, K, 0)
        assert extra >= 4 * 6 * 650 * 3 + lib.grappa_gb_obc_workspace_bytes(650, 3, 12)
    # the host refuses before it touches the device (no GPU is needed for these)
    gb = _lib.GbDesc(radius=None, scale=None, **ImplicitSolvent().as_opts())
    assert lib.grappa_md_steps_init_gb_f32(None, None, None, None, None, None, C.byref(gb), None, None, None, None, 0, 0, None, 0) == -1
    assert lib.grappa_md_steps_run_gb_f32(None, None, None, None, None, None, C.byref(gb), None, None, None, 0, 0, None, 0, 0, 1, None, None, None, None) == -1
    assert lib.grappa_md_steps_finish_gb_f32(None, None, None, None, None, None, C.byref(gb), None, 0, 0, None, 0, None, None, None, None, None, None, None) == -1
    assert lib.grappa_md_steps_init_gb_f32(None, None, None, None, None, None, None, None, None, None, None, 0, 0, None, 0) == -1      # gb == NULL: the _cons_ call's answer
    assert lib.grappa_gb_obc_fwd_f32(None, None, C.byref(gb), None, 0, 0, None, None, None, None, None, 0) == -1


def test_one_text_for_the_three_passes():
    """csrc/gb_obc.hip and csrc/dynamics_steps.hip run ONE tile loop and ONE text of each pass: csrc/gb_loop.h's and csrc/gb_pass.h's"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = lambda f: open(os.path.join(root, "grappa_amd", "csrc", f)).read()      # noqa: E731
    files = [f for f in sorted(os.listdir(os.path.join(root, "grappa_amd", "csrc"))) if f.endswith((".h", ".hip"))]
    defs = lambda pat: [f for f in files if re.search(pat, src(f))]      # noqa: E731
    assert defs(r"\bvoid gb_tile_loop\(") == ["gb_loop.h"] and defs(r"\bfloat gb_h\(") == ["gb_loop.h"] and defs(r"\bfloat gb_dh\(") == ["gb_loop.h"]
    for body in ("gb_born_body", "gb_pair_body", "gb_chain_body"):
        assert defs(r"\bvoid " + body + r"\(") == ["gb_pass.h"], body
        for f in ("gb_obc.hip", "dynamics_steps.hip"):
            assert re.search(r"\b" + body + r"<", src(f)), (body, f)
    assert defs(r"void nb_reduce_kernel\(") == ["nb_reduce.h"]


# ------------------------------------------------------------------------------------------------------------------------- the front ends
class Recorder:
    """a backend that records which seam was called and with which keywords; the outputs stay as they were given"""
    limit = 40

    def __init__(self):
        self.calls = []

    def relax_max_atoms(self):
        return self.limit

    def _record(self, which, args, kw):
        self.calls.append(dict(which=which, opts=dict(args[7]), **kw))

    def md_langevin(self, *a, **kw):
        self._record("fused", a, kw)

    def md_steps(self, *a, **kw):
        self._record("steps", a, kw)

    def md_steps_cons(self, *a, **kw):
        self._record("steps_cons", a, kw)

    def md_steps_gb(self, *a, **kw):
        self._record("steps_gb", a, kw)


class NoSolvent(Recorder):
    md_steps_gb = None


@pytest.fixture
def fake():
    from grappa_amd import backend
    old = backend._BACKEND
    be = Recorder()
    backend.set_backend(be)
    yield be
    backend.set_backend(old)


def _small():
    """a molecule within the fused limit, one above it -> (Parameters, xyz (C, n, 3), masses, NonbondedParameters, GBParameters, Constraints)"""
    from test_host_md_steps_cons import _mol
    out = []
    for name in ("span64", "k300"):
        mol, p, xyz, m, cons = _mol(name)
        gbp = GBParameters.from_elements(np.full(mol["n"], 6), np.asarray(mol["idx"][0]).reshape(-1, 2))
        out.append((p, xyz, m, mol["nb"], gbp, cons))
    return out


def test_none_makes_exactly_the_calls_of_today(fake):
    from grappa_amd.dynamics import simulate
    (p, xyz, m, nbp, gbp, cons), big = _small()[0], _small()[1]
    fake.limit = 200
    simulate(p, xyz, m, nbp, device="cpu", n_steps=3)
    simulate(p, xyz, m, nbp, device="cpu", n_steps=3, implicit_solvent=None, gb=None)
    simulate(big[0], big[1], big[2], big[3], device="cpu", n_steps=3, stepwise="auto", implicit_solvent=None)
    simulate(big[0], big[1], big[2], big[3], device="cpu", n_steps=3, stepwise="auto", constraints=big[5], implicit_solvent=None)
    assert [c["which"] for c in fake.calls] == ["fused", "fused", "steps", "steps_cons"]
    assert fake.calls[0].keys() == fake.calls[1].keys()
    for c in fake.calls:
        assert not {"gb", "solvent", "esolv", "frames_esolv", "implicit_solvent"} & set(c), sorted(c)
    r = simulate(p, xyz, m, nbp, device="cpu", n_steps=3)
    assert r.esolv is None and r.frames_esolv is None


def test_a_solvent_goes_stepwise_with_its_tables(fake):
    from grappa_amd.dynamics import simulate
    p, xyz, m, nbp, gbp, cons = _small()[0]
    fake.limit = 200          # within the fused limit: "auto" goes stepwise all the same
    r = simulate(p, xyz, m, nbp, device="cpu", n_steps=4, save_every=2, stepwise="auto", implicit_solvent="obc1", gb=gbp)
    simulate(p, xyz, m, nbp, device="cpu", n_steps=4, stepwise=True, implicit_solvent=ImplicitSolvent(), gb=gbp, constraints=cons)
    a, b = fake.calls
    assert a["which"] == b["which"] == "steps_gb"
    assert a["solvent"] == ImplicitSolvent("obc1") and isinstance(a["gb"], GBBatch) and a["gb"].counts == [gbp.n_atoms] and a["constraints"] is None
    assert tuple(a["esolv"].shape) == (1, xyz.shape[0]) and tuple(a["frames_esolv"].shape) == (2, 1, xyz.shape[0]) and "cutoff" not in a
    assert b["constraints"] is not None and b["constrain_start"] is True and b["frames_esolv"] is None
    assert r.esolv.shape == r.potential_energy.shape and r.frames_esolv.shape == r.frame_potential_energy.shape


def test_what_a_solvent_refuses(fake):
    from grappa_amd import backend
    from grappa_amd.dynamics import simulate
    p, xyz, m, nbp, gbp, cons = _small()[0]
    fake.limit = 200
    kw = dict(device="cpu", n_steps=3, implicit_solvent="obc2", gb=gbp)
    with pytest.raises(ValueError, match="nonbonded"):
        simulate(p, xyz, m, None, stepwise="auto", **kw)
    with pytest.raises(ValueError, match='stepwise="auto"'):
        simulate(p, xyz, m, nbp, stepwise=False, **kw)
    with pytest.raises(ValueError, match='stepwise="auto"'):
        simulate(p, xyz, m, nbp, **kw)          # the default is the fused path
    with pytest.raises(ValueError, match="cutoff"):
        simulate(p, xyz, m, nbp, stepwise="auto", cutoff=9.0, **kw)
    with pytest.raises(TypeError, match="GBParameters"):
        simulate(p, xyz, m, nbp, stepwise="auto", device="cpu", n_steps=3, implicit_solvent="obc2")
    with pytest.raises(ValueError, match="implicit_solvent"):
        simulate(p, xyz, m, nbp, stepwise="auto", device="cpu", n_steps=3, gb=gbp)
    with pytest.raises(ValueError, match="model"):
        simulate(p, xyz, m, nbp, stepwise="auto", device="cpu", n_steps=3, implicit_solvent="gbn2", gb=gbp)
    with pytest.raises(ValueError, match="atoms"):
        simulate(p, xyz, m, nbp, stepwise="auto", device="cpu", n_steps=3, implicit_solvent="obc2", gb=GBParameters([1.5], [0.8]))
    # a batch checked against the default offset, a solvent with a larger one than the smallest radius allows
    from grappa_amd.dynamics import simulate_graph
    from grappa_amd.nonbonded import NonbondedBatch
    from grappa_amd.relax import graph_from_parameters
    with pytest.raises(ValueError, match="offset"):
        simulate_graph(graph_from_parameters(p, xyz), m, NonbondedBatch([nbp]), stepwise="auto", n_steps=3, implicit_solvent=ImplicitSolvent(offset=1.75),
                       gb=GBBatch([gbp]))
    assert GBBatch([gbp]).check_offset(0.5).offset == 0.09
    assert fake.calls == []
    backend.set_backend(NoSolvent())
    with pytest.raises(ValueError, match="md_steps_gb"):
        simulate(p, xyz, m, nbp, stepwise="auto", **kw)


def test_grappa_simulate_builds_the_parameters_from_the_elements(fake):
    """Grappa.simulate(..., implicit_solvent=) makes GBParameters.from_elements of the molecule's atomic numbers and bonds (atom ids
    mapped to positions); without the keyword nothing of the solvent is passed on"""
    from types import SimpleNamespace
    from grappa_amd.grappa import Grappa
    p, xyz, m, nbp, gbp, cons = _small()[0]
    n = gbp.n_atoms
    z = np.where(np.arange(n) % 3 == 0, 7, 1)
    ids = np.arange(n) + 100          # atom ids that are not positions
    mol = SimpleNamespace(atomic_numbers=z, bonds=[(100 + a, 101 + a) for a in range(n - 1)], atoms=ids)
    me = SimpleNamespace(predict=lambda molecule: p, device="cpu")
    fake.limit = 200
    Grappa.simulate(me, mol, xyz, nbp, implicit_solvent="obc2", stepwise="auto", n_steps=2)
    Grappa.simulate(me, mol, xyz, nbp, n_steps=2)
    a, b = fake.calls
    want = GBParameters.from_elements(z, [(k, k + 1) for k in range(n - 1)])
    assert a["which"] == "steps_gb" and np.allclose(a["gb"].radius.numpy(), want.radius) and 1.3 in want.radius and 1.2 not in want.radius
    assert b["which"] == "fused" and "gb" not in b


# ------------------------------------------------------------------------------------------------------------------------- the dynamics' inputs
def test_the_inputs_of_the_dynamics_tests_are_finite_and_mostly_steady():
    """over the dynamics cases in the solvent, at most one in ten (item, step count) pairs is not steady in md_steps_refs.steady's
    sense, for x and for v, so that the gate of tests/test_gpu_md_gb.py is calibrated by the unturned fp32 run on nearly all items"""
    import md_gb_refs as mg
    for name in mg.CASES:
        for real in mg.verlet32(name):
            for k in mg.TRAJ_STEPS:
                for state in real[k]:
                    assert bool(torch.isfinite(state[0]).all()) and bool(torch.isfinite(state[1]).all()), (name, k)
    n = mg.steady_counts()
    print(f"not steady in the solvent: x {n['x'][0]} of {n['x'][1]}, v {n['v'][0]} of {n['v'][1]} (item, step count) pairs")
    assert 10 * n["x"][0] <= n["x"][1] and 10 * n["v"][0] <= n["v"][1], n


def test_the_restated_force_holds_the_solvent_only_inside_the_context():
    import md_gb_refs as mg
    import md_steps_refs as ms
    import relax_refs as rr
    b = ms.case("s65_C3")
    plain = rr.forces(b, b.xyz, torch.float64)
    with mg.gb_force(mg.gb_params("s65_C3")):
        wet = rr.forces(b, b.xyz, torch.float64)
    want = gr.gb_ref(b.params, mg.gb_params("s65_C3"), b.xyz, mg.MODEL, torch.float64, scales=False)
    assert torch.allclose(wet["E"] - plain["E"], want["energy"], rtol=0, atol=1e-9) and torch.allclose(wet["G"] - plain["G"], want["grad"], rtol=0, atol=1e-9)
    assert torch.equal(plain["E"], rr.forces(b, b.xyz, torch.float64)["E"])
