"""CPU: temperature ladders and replica exchange on the stepwise dynamics -- the restated exchange (tests/md_remd_refs.py) and its
properties, the restated ladder run on the exchange cases of tests/test_gpu_md_remd.py with the condition those cases must meet (decided
here from the float64 restatement alone), the new symbols and signatures, every refusal by message with nothing reaching the backend,
the calls made (recorded through a fake backend: none differs without replicas), the alignment of the run calls, and the shape of the
four new entries of csrc/dynamics_steps.hip."""
import math
import os
import re

import numpy as np
import pytest
import torch

import md_refs as md
import md_remd_refs as mx
import md_steps_refs as ms
from grappa_amd import _lib, backend
from grappa_amd.dynamics import MDResult, simulate, simulate_graph
from grappa_amd.nonbonded import NonbondedBatch
from grappa_amd.relax import graph_from_parameters
from grappa_amd.replica import ReplicaExchange, acceptance
from test_host_md_restr import Recorder, _mol
from test_host_md_steps import _top_level_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"grappa_md_remd_workspace_bytes", "grappa_md_remd_init_f32", "grappa_md_remd_run_f32", "grappa_md_remd_finish_f32"}


class Ladders(Recorder):
    def md_steps_remd(self, *a, **kw):
        self._record("steps_remd", a, kw)


class NoLadders(Recorder):
    md_steps_remd = None


@pytest.fixture
def fake():
    old = backend._BACKEND
    be = Ladders()
    backend.set_backend(be)
    yield be
    backend.set_backend(old)


# ------------------------------------------------------------------------------------------------------------------------- the exchange
T3 = np.array([300.0, 330.0, 365.0], dtype=np.float32)
KEY = np.uint64(0x0123456789ABCDEF)


def test_the_uniform_and_the_decision_against_hand_computed_values():
    # the generator: word 0 of Philox(key, (s, 0, g, 2)), restated by md_refs.philox and exported by the library
    for s, g in ((0, 1), (1, 8), (6, 4000000000)):
        w = md.philox(KEY, s, 0, g, 2)
        assert [int(v) for v in w] == list(_lib.md_philox(int(KEY), s, 0, g, 2))
        assert mx.uniform(KEY, s, g) == (int(w[0]) + 0.5) / 4294967296.0 and 0.0 < mx.uniform(KEY, s, g) < 1.0
        assert mx.uniform(KEY, s, g, philox=_lib.md_philox) == mx.uniform(KEY, s, g)
    # D by hand: beta = 1 / (kB T); slots 0 and 1 at 300 K and 330 K; U_lo - U_hi = -2 kcal/mol
    d_beta = 1.0 / (0.0019872041 * 300.0) - 1.0 / (0.0019872041 * 330.0)
    assert abs(d_beta - 0.152485) < 1e-5
    slots, who = np.arange(3), np.arange(3)
    for g in range(2, 40, 2):          # even attempts: the pair (0, 1)
        u = mx.uniform(KEY, 0, g)
        for dU, in ((-2.0,), (-12.0,), (3.0,)):
            new, inv, dec = mx.exchange_ref(slots, who, T3, np.array([10.0 + dU, 10.0, 0.0]), KEY, g, 1, np.zeros(3))
            (s, lo, hi, D, uu, ok, acc), = dec
            assert (s, lo, hi, ok) == (0, 0, 1, True) and uu == u and abs(D - d_beta * dU) < 1e-12
            want = dU >= 0 or u < math.exp(d_beta * dU)          # both branches: D >= 0 always accepts, else u against exp(D)
            assert acc == want and (new.tolist() == [1, 0, 2]) == want
    us = [mx.uniform(KEY, 0, g) for g in range(2, 40, 2)]
    assert min(us) < math.exp(-2.0 * d_beta) < max(us), "the hand-computed cases meet both branches at dU = -2"


def test_the_exchange_keeps_a_permutation_and_is_symmetric_in_the_pair():
    rng = np.random.default_rng(5)
    C = 7
    T = mx.ladder(C, 280.0, 15.0)
    slots = rng.permutation(C)
    for g in range(3, 60, 3):
        U = rng.normal(0.0, 8.0, C)
        who = mx.inverse(slots)
        new, inv, dec = mx.exchange_ref(slots, who, T, U, KEY, g, 3, np.zeros(C))
        assert sorted(new.tolist()) == list(range(C)) and all(new[inv[s]] == s for s in range(C))
        assert [d[0] for d in dec] == list(range((g // 3) % 2, C - 1, 2)), "attempt a names the pairs of parity a mod 2"
        for s, lo, hi, D, u, ok, acc in dec:
            assert acc == (D >= 0 or u < math.exp(D))
            if D >= 0:
                assert acc
        # symmetric: the two replicas of every pair relabelled (each takes the other's index and energy): the same decisions
        perm = np.arange(C)
        for s, lo, hi, *_ in dec:
            perm[lo], perm[hi] = hi, lo
        slots2, U2 = np.empty_like(slots), np.empty_like(U)
        slots2[perm], U2[perm] = slots, U
        new2, _, dec2 = mx.exchange_ref(slots2, mx.inverse(slots2), T, U2, KEY, g, 3, np.zeros(C))
        assert [(d[0], d[3], d[4], d[6]) for d in dec2] == [(d[0], d[3], d[4], d[6]) for d in dec] and np.array_equal(new2[perm], new)
        slots = new


def test_nothing_moves_for_a_stopped_member_or_an_energy_that_is_not_finite():
    slots, who = np.array([1, 0, 2]), np.array([1, 0, 2])
    U = np.array([0.0, 50.0, 0.0])          # replica 1 holds slot 0 with the higher energy: D > 0, always accepted
    new, _, dec = mx.exchange_ref(slots, who, T3, U, KEY, 2, 1, np.zeros(3))
    assert dec[0][6] and new.tolist() == [0, 1, 2]
    for status, UU in ((np.array([2, 0, 0]), U), (np.array([0, 4, 0]), U), (np.zeros(3), np.array([np.nan, 50.0, 0.0])),
                       (np.zeros(3), np.array([0.0, np.inf, 0.0]))):
        new, inv, dec = mx.exchange_ref(slots, who, T3, UU, KEY, 2, 1, status)
        assert not dec[0][5] and not dec[0][6] and new.tolist() == slots.tolist() and inv.tolist() == who.tolist()


def test_acceptance_counts_pairs_by_parity():
    xs = np.array([[[0, 1, 2]], [[1, 0, 2]], [[1, 0, 2]], [[1, 0, 2]], [[2, 0, 1]]])          # attempts 1 .. 5
    a = acceptance(xs, np.arange(3))
    assert a.shape == (1, 2) and a[0, 0] == 0.5 and abs(a[0, 1] - 1.0 / 3.0) < 1e-12
    assert np.isnan(acceptance(np.zeros((0, 1, 3), dtype=np.int64), np.arange(3))).all()


# ------------------------------------------------------------------------------------------------------------------------- the ladder run
@pytest.mark.parametrize("K", mx.EXCHANGE_K)
@pytest.mark.parametrize("name", list(mx.EXCHANGE_CASES))
def test_the_exchange_cases_decide_both_ways_by_a_margin(name, K):
    """A condition on the inputs, not a measurement: on the float64 restatement every state is finite, the slots are valid, and the case
    has at least one accepted and one rejected decision with |ln u - D| >= 0.5, so that an fp32 run decides alike"""
    r = mx.exchange_run(name, K)
    assert bool(torch.isfinite(r["xyz"]).all()) and bool(torch.isfinite(r["vel"]).all()) and not r["status"].any()
    C = len(mx.EXCHANGE_CASES[name])
    assert len(r["log"]) == mx.EXCHANGE_STEPS // K
    for row in r["log"]:
        assert all(sorted(s.tolist()) == list(range(C)) for s in row["slots"]) and bool(np.isfinite(row["U"]).all())
    acc, rej = mx.decisive(r)
    print(f"{name}, K = {K}: {acc} accepted and {rej} rejected decisions with |ln u - D| >= 0.5")
    assert acc >= 1 and rej >= 1, (name, K, acc, rej)


def test_a_ladder_without_exchanges_is_the_scalar_restatement_per_conformation():
    name = "s65_C3"
    b, m, k, v = ms.case(name), ms.masses(name), ms.keys(name), ms.thermal_velocities(name)
    T = mx.ladder(3, 250.0, 60.0)
    r = mx.ladder_ref(b, m, k, T, 0, 5, v)
    assert r["slots"].tolist() == [[0, 1, 2]] and not r["log"]
    for c in range(3):
        s = md.baoab_ref(b, m, torch.float64, velocities=v, keys=k, temperature=float(T[c]), friction=mx.FRICTION, dt=0.001, n_steps=5)
        assert torch.equal(r["xyz"][:, c], s["xyz"][:, c]) and torch.equal(r["vel"][:, c], s["vel"][:, c])


def test_restraints_compose_with_the_ladder_restatement():
    import md_restr_refs as mr
    c = mr.case("s65_C3")
    with mr.restr_force(c["rb"]):
        r = mx.ladder_ref(c["batch"], c["masses"], c["keys"], mx.EXCHANGE_CASES["s65_C3"], 4, 8, c["vel"],
                          erestr_at=lambda x: mr.energy_at(c["batch"], c["rb"], x)[0])
    free = mx.ladder_ref(c["batch"], c["masses"], c["keys"], mx.EXCHANGE_CASES["s65_C3"], 4, 8, c["vel"])
    assert len(r["log"]) == 2 and bool(torch.isfinite(r["xyz"]).all()) and not torch.equal(r["xyz"], free["xyz"])
    assert not np.array_equal(r["log"][0]["U"], free["log"][0]["U"])


# ------------------------------------------------------------------------------------------------------------------------- the C ABI
def test_symbols_and_signatures():
    header = open(os.path.join(ROOT, "include", "grappa_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert NAMES <= set(re.findall(r"\b(grappa_[a-z0-9_]+)\s*\(", code)) and NAMES <= set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 11 and "#define GRAPPA_ABI_VERSION 11" in header
    fields = [f for f, _ in _lib.MdRemd._fields_]
    assert fields == ["temperatures", "slots_in", "exchange_every", "init_at_ladder"]
    struct = re.search(r"typedef struct grappa_md_remd \{(.*?)\} grappa_md_remd;", code, flags=re.S).group(1)
    assert re.findall(r"(\w+);", struct) == fields
    # the ladder's calls are the _restr_ calls with `x` directly after r, plus the logs (run) and slots_out (finish) at the end
    P = _lib.C.POINTER(_lib.MdRemd)
    for which, extra in (("init", 0), ("run", 3), ("finish", 1)):
        res_r, args_r = _lib.SIGNATURES[f"grappa_md_steps_{which}_restr_f32"]
        res_x, args_x = _lib.SIGNATURES[f"grappa_md_remd_{which}_f32"]
        assert res_x is res_r and args_x[:9] == args_r[:9] and args_x[9] is P, which
        assert args_x[10:len(args_x) - extra] == args_r[9:] and all(a is _lib.C.c_void_p for a in args_x[len(args_x) - extra:]), which
    lib = _lib.load()
    for n in NAMES:
        assert getattr(lib, n) is not None
    w, wr = lib.grappa_md_remd_workspace_bytes, lib.grappa_md_steps_restr_workspace_bytes
    assert w(0, 1, 1, 1, 0, 0, 0, 0, 0) == 0 and w(10, 0, 1, 1, 0, 0, 0, 0, 0) == 0
    for K, cut, gb, gbcut in ((0, 0, 0, 0), (5, 1, 0, 0), (5, 0, 1, 0), (0, 1, 1, 1)):
        # the ladder's words lie behind everything else: six arrays of B * C words, each rounded up to 256 bytes
        assert w(100, 3, 2, 3, K, cut, gb, gbcut, 1) == wr(100, 3, 2, 3, K, cut, gb, gbcut) + 6 * 256
        assert w(100, 3, 2, 3, K, cut, gb, gbcut, 0) < w(100, 3, 2, 3, K, cut, gb, gbcut, 1)
    assert w(100, 17, 2, 3, 0, 0, 0, 0, 0) > w(100, 3, 2, 3, 0, 0, 0, 0, 0)
    # the host refuses before it touches the device (no GPU is needed for these)
    assert lib.grappa_md_remd_init_f32(*([None] * 14), 0, 0, None, 0) == -1
    assert lib.grappa_md_remd_run_f32(*([None] * 13), 0, 0, None, 0, 0, 1, *([None] * 9)) == -1
    assert lib.grappa_md_remd_finish_f32(*([None] * 11), 0, 0, None, 0, *([None] * 10)) == -1
    x = _lib.MdRemd(temperatures=None, slots_in=None, exchange_every=0, init_at_ladder=0)          # a NULL ladder; a negative K
    assert lib.grappa_md_remd_init_f32(*([None] * 9), _lib.C.byref(x), *([None] * 4), 0, 0, None, 0) == -1
    x = _lib.MdRemd(temperatures=1 << 12, slots_in=None, exchange_every=-1, init_at_ladder=0)
    assert lib.grappa_md_remd_init_f32(*([None] * 9), _lib.C.byref(x), *([None] * 4), 0, 0, None, 0) == -1
    # exchanges without a thermostat: refused by the plan, whatever else the call holds
    o = _lib.MdOpts(dt=0.001, temperature=300.0, friction=0.0, init_temperature=0.0, n_steps=4, save_every=0, first_step=0)
    x = _lib.MdRemd(temperatures=1 << 12, slots_in=None, exchange_every=2, init_at_ladder=0)
    assert lib.grappa_md_remd_init_f32(None, None, None, None, _lib.C.byref(o), None, None, None, None, _lib.C.byref(x), *([None] * 4), 0, 0, None, 0) == -1


def test_the_new_entries_follow_the_shape_of_the_others():
    """csrc/dynamics_steps.hip: each grappa_md_remd_* entry builds the plan from the pointers it takes and makes one call, names no other
    entry, and the ladder's words are carved in ms_carve, last"""
    blocks = _top_level_blocks(open(os.path.join(ROOT, "grappa_amd", "csrc", "dynamics_steps.hip")).read())
    entries = [(h, b) for h, b in blocks if 'extern "C"' in h and "grappa_md_remd_" in h]
    assert {re.search(r"grappa_md_remd_\w+", h).group(0) for h, _ in entries} == NAMES and len(entries) == 4
    for h, b in entries:
        name = re.search(r"grappa_md_remd_\w+", h).group(0)
        assert "grappa_md_" not in b, f"{name} names another entry"
        assert b.count(";") <= 5, f"{name} has grown: {b.count(';')} statements"
        assert "_workspace_bytes" in name or "ms_plan(mm, nb, cut, cons, gb, gbcut, r, p, x, o)" in b, f"{name} does not build the plan"
    callers = [(h, b) for h, b in blocks if re.search(r"\bms_remd_layout\(", b)]
    assert len(callers) == 1 and "ms_carve(" in callers[0][0]
    body = callers[0][1]
    assert body.index("ms_remd_layout(") > body.index("ms_restr_ref(") > body.index("ms_gb_layout(") > body.index("ms_layout("), "the ladder's words come last"
    plan = next(b for h, b in blocks if re.search(r"\bms_plan\(", h))
    assert "exchange_every" in plan and "friction" in plan, "the ladder's refusals are in ms_plan"


# ------------------------------------------------------------------------------------------------------------------------- the front ends
def test_replica_exchange_validates_on_the_host_what_the_device_vets():
    with pytest.raises(ValueError, match="temperatures must be a non-empty 1-D sequence"):
        ReplicaExchange([])
    with pytest.raises(ValueError, match="temperatures must be a non-empty 1-D sequence"):
        ReplicaExchange([[300.0, 310.0]])
    with pytest.raises(ValueError, match="temperatures must be finite"):
        ReplicaExchange([300.0, float("nan")])
    with pytest.raises(ValueError, match="temperatures must be finite"):
        ReplicaExchange([300.0, 1e39])
    with pytest.raises(ValueError, match="temperatures must be >= 0"):
        ReplicaExchange([300.0, -1.0])
    with pytest.raises(ValueError, match="temperatures must be positive when replicas exchange"):
        ReplicaExchange([300.0, 0.0], exchange_every=5)
    assert ReplicaExchange([300.0, 0.0]).exchange_every == 0
    for bad in (-1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="exchange_every must be an integer >= 0"):
            ReplicaExchange([300.0, 310.0], exchange_every=bad)
    for bad in ([0, 0], [0, 2], [-1, 0], [[0, 1], [1, 1]]):
        with pytest.raises(ValueError, match="slots must be a permutation of 0 .. C-1 for every molecule"):
            ReplicaExchange([300.0, 310.0], slots=bad)
    with pytest.raises(ValueError, match=r"slots must be integers of shape \(C,\) or \(B, C\)"):
        ReplicaExchange([300.0, 310.0], slots=[0, 1, 2])
    with pytest.raises(ValueError, match=r"slots must be integers of shape"):
        ReplicaExchange([300.0, 310.0], slots=[0.0, 1.0])
    r = ReplicaExchange([300.0, 310.0, 320.0], 4, slots=[2, 0, 1])
    assert r.C == 3 and r.temperatures.dtype == np.float32 and r.slots_for(2).tolist() == [[2, 0, 1], [2, 0, 1]]
    with pytest.raises(ValueError, match="slots describe 2 molecules, the batch has 3"):
        ReplicaExchange([300.0, 310.0], slots=[[0, 1], [1, 0]]).slots_for(3)


def test_refusals_by_message(fake):
    mol, p, xyz, m, res = _mol()
    rep = ReplicaExchange([300.0, 320.0, 340.0], 4)
    kw = dict(device="cpu", n_steps=8)
    with pytest.raises(ValueError, match='replicas run on the stepwise path only: pass stepwise="auto"'):
        simulate(p, xyz, m, mol["nb"], replicas=rep, stepwise=False, **kw)
    with pytest.raises(ValueError, match="replicas run on the stepwise path only"):
        simulate(p, xyz, m, mol["nb"], replicas=rep, **kw)          # the default is the fused path
    with pytest.raises(TypeError, match="replicas must be a ReplicaExchange or None"):
        simulate(p, xyz, m, mol["nb"], replicas=[300.0, 320.0, 340.0], stepwise="auto", **kw)
    with pytest.raises(ValueError, match="the ladder has 2 temperatures, the molecule has 3 conformations"):
        simulate(p, xyz, m, mol["nb"], replicas=ReplicaExchange([300.0, 320.0]), stepwise="auto", **kw)
    with pytest.raises(ValueError, match=r"replica exchange needs a thermostat \(friction > 0\)"):
        simulate(p, xyz, m, mol["nb"], replicas=rep, stepwise="auto", friction=0.0, **kw)
    with pytest.raises(ValueError, match=r"first_step must be a multiple of exchange_every \(4\)"):
        simulate(p, xyz, m, mol["nb"], replicas=rep, stepwise="auto", first_step=6, **kw)
    g = graph_from_parameters(p, xyz)
    nb = NonbondedBatch([mol["nb"]])
    with pytest.raises(TypeError, match="replicas must be a ReplicaExchange or None"):
        simulate_graph(g, m, nb, replicas=(300.0,), stepwise=True, n_steps=3)
    with pytest.raises(ValueError, match="replicas run on the stepwise path only"):
        simulate_graph(g, m, nb, replicas=rep, stepwise=False, n_steps=3)
    with pytest.raises(ValueError, match="the ladder has 2 temperatures, the batch has 3 conformations"):
        simulate_graph(g, m, nb, replicas=ReplicaExchange([300.0, 320.0]), stepwise=True, n_steps=3)
    with pytest.raises(ValueError, match="slots describe 2 molecules, the batch has 1"):
        simulate_graph(g, m, nb, replicas=ReplicaExchange([300.0, 320.0, 340.0], slots=[[0, 1, 2], [0, 1, 2]]), stepwise=True, n_steps=3)
    with pytest.raises(ValueError, match="common multiple"):
        simulate_graph(g, m, nb, replicas=ReplicaExchange([300.0, 320.0, 340.0], 999983), stepwise=True, n_steps=4, save_every=2)
    assert not fake.calls, "a refused call reached the backend"
    old = backend._BACKEND
    backend.set_backend(NoLadders())
    try:
        with pytest.raises(ValueError, match="the backend has no temperature ladders on the stepwise dynamics"):
            simulate(p, xyz, m, mol["nb"], replicas=rep, stepwise="auto", **kw)
    finally:
        backend.set_backend(old)


def test_the_backend_seam_decides_before_it_touches_the_device():
    from grappa_amd.backend_mm import MMBackend
    args = (None,) * 17
    with pytest.raises(TypeError, match="restraints must be a RestraintBatch or None"):
        MMBackend.md_steps_remd(None, *args, restraints=object())
    with pytest.raises(TypeError, match="go together"):
        MMBackend.md_steps_remd(None, *args, solvent="obc2")
    with pytest.raises(ValueError, match="exchange_every must be an integer >= 0"):
        MMBackend.md_steps_remd(None, *args, exchange_every=-2)
    fams = MMBackend._MD_STEPS_FAMILIES
    assert list(fams)[-1] == "_remd" and fams["_remd"][0][:-1] == fams["_restr"][0] and fams["_remd"][1][:-1] == fams["_restr"][1]

    class Lib:
        def __getattr__(self, name):
            return name
    be = type("B", (), {"lib": Lib()})()
    assert [MMBackend._md_steps_entry(be, "_remd", w)[1] for w in ("workspace_bytes", "init", "run", "finish")] == \
        ["grappa_md_remd_workspace_bytes", "grappa_md_remd_init_f32", "grappa_md_remd_run_f32", "grappa_md_remd_finish_f32"]
    assert MMBackend._md_steps_entry(be, "_gb", "run")[1] == "grappa_md_steps_run_gb_f32"
    assert MMBackend._md_steps_entry(be, "", "workspace_bytes")[1] == "grappa_md_steps_workspace_bytes"
    assert all(MMBackend._md_steps_entry(be, f, w)[1] in _lib.SIGNATURES for f in fams for w in ("workspace_bytes", "init", "run", "finish"))


def test_none_makes_exactly_the_calls_of_today(fake):
    mol, p, xyz, m, res = _mol()
    fake.limit = 200
    simulate(p, xyz, m, mol["nb"], device="cpu", n_steps=3)
    simulate(p, xyz, m, mol["nb"], device="cpu", n_steps=3, replicas=None)
    simulate(p, xyz, m, mol["nb"], device="cpu", n_steps=3, stepwise=True, replicas=None)
    simulate(p, xyz, m, mol["nb"], device="cpu", n_steps=3, stepwise="auto", cutoff=9.0, replicas=None)
    simulate(p, xyz, m, mol["nb"], device="cpu", n_steps=3, stepwise="auto", restraints=res, replicas=None)
    assert [c["which"] for c in fake.calls] == ["fused", "fused", "steps", "steps", "steps_restr"]
    assert fake.calls[0].keys() == fake.calls[1].keys()
    for c in fake.calls:
        assert not {"temperatures", "slots", "exchange_every", "init_at_ladder", "slots_out", "exchange_slots", "exchange_epot", "exchange_erestr"} & set(c)
    r = simulate(p, xyz, m, mol["nb"], device="cpu", n_steps=3)
    assert r.slots is None and r.exchange_slots is None and r.exchange_energy is None
    assert {"slots", "exchange_slots", "exchange_energy"} <= set(MDResult.__dataclass_fields__)


def test_replicas_go_stepwise_with_the_ladder_and_its_outputs(fake):
    mol, p, xyz, m, res = _mol()
    fake.limit = 200          # within the fused limit: "auto" goes stepwise all the same
    rep = ReplicaExchange([300.0, 320.0, 340.0], 4, slots=[1, 0, 2])
    r = simulate(p, xyz, m, mol["nb"], device="cpu", n_steps=12, save_every=6, stepwise="auto", replicas=rep, friction=2.0, steps_per_launch=5)
    (c,) = fake.calls
    assert c["which"] == "steps_remd" and c["constraints"] is None and c["gb"] is None and "restraints" not in c and "cutoff" not in c
    assert c["temperatures"].tolist() == [300.0, 320.0, 340.0] and c["temperatures"].dtype == torch.float32
    assert c["slots"].tolist() == [[1, 0, 2]] and c["slots"].dtype == torch.int32 and c["exchange_every"] == 4
    assert c["init_at_ladder"] is True, "init_temperature was left at None"
    assert tuple(c["slots_out"].shape) == (1, 3) and tuple(c["exchange_slots"].shape) == (3, 1, 3) and tuple(c["exchange_epot"].shape) == (3, 1, 3)
    assert c["exchange_erestr"] is None and c["opts"]["n_steps"] == 12
    assert r.slots.shape == (3,) and r.exchange_slots.shape == (3, 3) and r.exchange_energy.shape == (3, 3) and r.exchange_energy.dtype == np.float64
    simulate(p, xyz, m, mol["nb"], device="cpu", n_steps=12, stepwise=True, replicas=ReplicaExchange([300.0, 320.0, 340.0]), init_temperature=50.0,
             restraints=res, cutoff=None)
    c = fake.calls[-1]
    assert c["which"] == "steps_remd" and c["init_at_ladder"] is False and c["exchange_every"] == 0 and c["slots"] is None
    assert c["exchange_slots"] is None and c["restraints"] is not None and tuple(c["restraint_energy"].shape) == (1, 3)


class _RecordingLib:
    """the loaded library, but the three calls of a ladder run are recorded and answer GRAPPA_OK: nothing reaches a device"""

    def __init__(self):
        self.real, self.calls = _lib.load(), []

    def __getattr__(self, name):
        if name.startswith("grappa_md_remd_") and name.endswith("_f32"):
            return lambda *a: self.calls.append((name, a)) or 0
        return getattr(self.real, name)


def _recorded_run(n_steps, every, K, spc, first_step=0, logs=True):
    """HipBackend._md_steps on host tensors through _RecordingLib -> (the run calls as (step0, n, frame rows, log rows), all calls)"""
    from grappa_amd.backend_mm import MMBackend

    class Be(MMBackend):
        def __init__(self):
            self.lib = _RecordingLib()

        def _stream(self):
            return None

        def _item_table(self, nb, counts, N, Cc, dev):
            return torch.zeros(64, dtype=torch.int32), 3, 2, None

    b, m = ms.case("s65_C3"), ms.masses("s65_C3")
    N, B, C = b.N, b.B, 3
    o = {**md.MD_OPTS, "n_steps": n_steps, "save_every": every, "friction": 1.0, "first_step": first_step}
    F, X = (n_steps // every if every else 0), (n_steps // K if K else 0)
    f32, i32 = (lambda *sh: torch.zeros(*sh)), (lambda *sh: torch.zeros(*sh, dtype=torch.int32))
    fx, fe = (f32(F, N, C, 3), f32(F, B, C)) if F else (None, None)
    xs, xe = (i32(X, B, C), f32(X, B, C)) if X and logs else (None, None)
    be = Be()
    be.md_steps_remd(b.plan("cpu"), b.xyz, b.ks, b.eqs, b.n_per, False, None, o, torch.from_numpy(m), torch.zeros(B, dtype=torch.int64), None,
                     f32(N, C, 3), f32(N, C, 3), f32(B, C), f32(B, C), i32(B, C), i32(B, C), frames_xyz=fx, frames_epot=fe, atom_counts_host=b.counts,
                     steps_per_call=spc, workspace=torch.zeros(1 << 22, dtype=torch.uint8), temperatures=torch.tensor([300.0, 310.0, 320.0]),
                     exchange_every=K, slots_out=i32(B, C), exchange_slots=xs, exchange_epot=xe)
    row = lambda ptr, t: None if ptr is None else (ptr - t.data_ptr()) // (t[0].numel() * t.element_size())      # noqa: E731
    runs = []
    for name, a in be.lib.calls:
        if name == "grappa_md_remd_run_f32":
            assert len(a) == 28 and a[24] is None and a[27] is None          # frames_phi; exch_erestr
            runs.append((a[17], a[18], None if fx is None else (row(a[19], fx), row(a[20], fe)), None if xs is None else (row(a[25], xs), row(a[26], xe))))
    return runs, [name for name, _ in be.lib.calls]


def test_run_calls_are_cut_at_common_multiples_of_save_every_and_exchange_every():
    """HipBackend._md_steps through a library that records: init, the run calls, finish; every run call begins at a multiple of
    lcm(save_every, exchange_every), and its frame and log pointers are the rows of that call's first frame and first attempt"""
    for n_steps, every, K, spc, chunk in ((24, 6, 4, 13, 12), (24, 6, 4, 30, 24), (24, 6, 4, 5, 12), (20, 0, 4, 10, 8), (20, 0, 4, 1, 4),
                                          (20, 5, 0, 12, 10), (20, 0, 0, 7, 7), (30, 10, 4, 1000, 30)):
        runs, names = _recorded_run(n_steps, every, K, spc)
        assert names == ["grappa_md_remd_init_f32"] + ["grappa_md_remd_run_f32"] * len(runs) + ["grappa_md_remd_finish_f32"]
        assert [r[0] for r in runs] == list(range(0, n_steps, chunk)), (every, K, spc, runs)
        assert [r[1] for r in runs] == [min(chunk, n_steps - s0) for s0 in range(0, n_steps, chunk)]
        for s0, n, frames, logs in runs:
            assert (every == 0 or s0 % every == 0) and (K == 0 or s0 % K == 0)
            assert frames == (None if every == 0 else (s0 // every, s0 // every))
            assert logs == (None if K == 0 else (s0 // K, s0 // K)), (every, K, spc, s0, logs)
    # a continued run: the rows are counted from the call's own start, the library's step0 too
    runs, _ = _recorded_run(16, 0, 4, 8, first_step=40)
    assert [(r[0], r[1], r[3]) for r in runs] == [(0, 8, (0, 0)), (8, 8, (2, 2))]
    # without logs the calls are cut alike (one rule) and carry no log pointer
    runs, _ = _recorded_run(20, 0, 4, 10, logs=False)
    assert [(r[0], r[1], r[3]) for r in runs] == [(0, 8, None), (8, 8, None), (16, 4, None)]


def test_replica_exchange_takes_the_slots_a_run_returned():
    """`ReplicaExchange(..., slots=result.slots)`: a tensor (of any device: it is brought to the host first), (C,) or (B, C)"""
    r = ReplicaExchange([300.0, 310.0, 320.0], 4, slots=torch.tensor([[2, 0, 1], [0, 1, 2]], dtype=torch.int32))
    assert isinstance(r.slots, np.ndarray) and r.slots.dtype == np.int32 and r.slots.tolist() == [[2, 0, 1], [0, 1, 2]]
    assert ReplicaExchange([300.0, 310.0, 320.0], slots=torch.tensor([2, 0, 1])).slots_for(2).tolist() == [[2, 0, 1], [2, 0, 1]]
    with pytest.raises(ValueError, match="slots must be a permutation"):
        ReplicaExchange([300.0, 310.0, 320.0], slots=torch.tensor([2, 2, 1]))
    src = open(os.path.join(ROOT, "grappa_amd", "replica.py")).read()
    assert src.index("slots.detach().cpu().numpy()") < src.index("np.asarray(slots)"), "a device tensor must not reach np.asarray"
