"""GPU: temperature ladders and replica exchange on the stepwise dynamics (csrc/md_remd.h and csrc/dynamics_steps.hip through
HipBackend.md_steps_remd and grappa_amd/dynamics.py).  Every output AND the workspace lie between guard regions that must come back
untouched.

A ladder without exchanges is, conformation by conformation, the scalar run at that conformation's temperature bit for bit -- which
carries every float64 gate of the scalar runs over to the ladder.  The decisions are recomputed on the host in float64 from the logged
energies (tests/md_remd_refs.py) with the library's own generator; a run with exchanges is, bit for bit, ladder runs without exchanges
chained by the logged swaps."""
import numpy as np
import pytest
import torch

import md_cons_refs as mc
import md_cut_refs as mcut
import md_gb_cut_refs as mgc
import md_gb_refs as mg
import md_refs as md
import md_remd_refs as mx
import md_restr_refs as mr
import md_steps_cons_refs as msc
import md_steps_refs as ms
import relax_refs as rr
import relax_steps_refs as rst
from grappa_amd import _lib
from grappa_amd._marshal import GrappaHipError
from grappa_amd.solvent import GBBatch
from test_gpu_md_restr import _run as _scalar_run
from test_gpu_md_steps import FILL, FILL_B, FILL_I, GUARD_B, _bits, _dev_keys, _fill_of, _guarded, _with_coincident

pytestmark = pytest.mark.gpu

STATE = ("xyz", "vel", "epot", "ekin", "steps", "status")
FRAMES = ("frames_xyz", "frames_epot", "frames_ekin")


@pytest.fixture(scope="module")
def hip():
    from grappa_amd.backend import HipBackend
    return HipBackend()


def _ladder_run(hip, batch, masses, keys, T, K=0, slots=None, at_ladder=False, rb=None, ref=None, vel=None, xyz=None, cons=None, cutoff=None,
                gbs=None, solvent=None, steps_per_call=1000, logs=True, unwritten=(), **opts):
    """one call of HipBackend.md_steps_remd on a relax_refs.Batch -> dict of CPU tensors (the state, the frames, slots, and the logs xs,
    xe, xr); asserts the guards around every output and around the workspace.  T None: no ladder (x == NULL)"""
    o = {**md.MD_OPTS, **opts}
    plan = batch.plan("cuda")
    x = (batch.xyz if xyz is None else xyz).to("cuda")
    N, B, Cc = batch.N, batch.B, x.shape[1]
    F = o["n_steps"] // o["save_every"] if o["save_every"] > 0 and o["n_steps"] > 0 else 0
    X = o["n_steps"] // K if K > 0 else 0
    f32, i32 = torch.float32, torch.int32
    shapes = {"xyz": ((N, Cc, 3), f32), "vel": ((N, Cc, 3), f32), "epot": ((B, Cc), f32), "ekin": ((B, Cc), f32), "steps": ((B, Cc), i32),
              "status": ((B, Cc), i32), "slots": ((B, Cc), i32)}
    if F:
        shapes.update({"frames_xyz": ((F, N, Cc, 3), f32), "frames_epot": ((F, B, Cc), f32), "frames_ekin": ((F, B, Cc), f32)})
    if X and logs:
        shapes.update(xs=((X, B, Cc), i32), xe=((X, B, Cc), f32))
        if rb is not None:
            shapes["xr"] = ((X, B, Cc), f32)
    if gbs is not None:
        shapes["esolv"] = ((B, Cc), f32)
    if rb is not None:
        shapes.update(er=((B, Cc), f32), phi=((rb.R, Cc), f32))
        if F:
            shapes.update(frames_er=((F, B, Cc), f32), frames_phi=((F, rb.R, Cc), f32))
    bufs = {k: _guarded(*v) for k, v in shapes.items()}
    out = {k: v[1] for k, v in bufs.items()}
    ks = [k.to("cuda") for k in batch.ks]
    eqs = [None if q is None else q.to("cuda") for q in batch.eqs]
    args = (plan, x, ks, eqs, batch.n_per, False, batch.nonbonded().to("cuda"), o, torch.from_numpy(np.asarray(masses, dtype=np.float32)).to("cuda"),
            _dev_keys(keys), None if vel is None else vel.to("cuda"), out["xyz"], out["vel"], out["epot"], out["ekin"], out["steps"], out["status"])
    kw = dict(frames_xyz=out.get("frames_xyz"), frames_epot=out.get("frames_epot"), frames_ekin=out.get("frames_ekin"), atom_counts_host=batch.counts,
              steps_per_call=steps_per_call)
    Kc = 0
    if cons is not None:
        from grappa_amd.constraints import ConstraintBatch
        cb = ConstraintBatch(cons, tolerance=mc.TOL)
        Kc = int(cb.cluster_atoms.shape[0])
        kw.update(constraints=cb.to("cuda"), constrain_start=True)
    if cutoff is not None:
        kw["cutoff"] = cutoff
    gbcut = False
    if gbs is not None:
        from grappa_amd.solvent import as_implicit_solvent
        gbcut = as_implicit_solvent(solvent).cutoff is not None
        kw.update(gb=GBBatch(gbs).to("cuda"), solvent=solvent, esolv=out["esolv"])
    if rb is not None:
        kw.update(restraints=rb.to("cuda"), restraint_reference=None if ref is None else ref.to("cuda"), restraint_energy=out["er"],
                  dihedral_out=out["phi"], frames_restraint_energy=out.get("frames_er"), frames_dihedrals=out.get("frames_phi"))
    need = int(hip.lib.grappa_md_remd_workspace_bytes(N, Cc, B, rst.n_blocks(batch), Kc, int(cutoff is not None), int(gbs is not None), int(gbcut),
                                                      int(rb is not None)))
    wbuf = torch.full((GUARD_B + need + GUARD_B,), FILL_B, dtype=torch.uint8, device="cuda")
    try:
        hip.md_steps_remd(*args, **kw, workspace=wbuf[GUARD_B:GUARD_B + need],
                          temperatures=None if T is None else torch.from_numpy(np.asarray(T, dtype=np.float32)).to("cuda"),
                          slots=None if slots is None else torch.as_tensor(np.asarray(slots), dtype=torch.int32).reshape(B, Cc).to("cuda"),
                          exchange_every=K, init_at_ladder=at_ladder, slots_out=out["slots"], exchange_slots=out.get("xs"),
                          exchange_epot=out.get("xe"), exchange_erestr=out.get("xr"))
    finally:
        torch.cuda.synchronize()
        for k, (buf, _) in bufs.items():
            assert bool((buf[:64] == _fill_of(buf)).all()) and bool((buf[-64:] == _fill_of(buf)).all()), f"written outside {k}"
        assert bool((wbuf[:GUARD_B] == FILL_B).all()) and bool((wbuf[-GUARD_B:] == FILL_B).all()), "written outside the workspace"
        _ladder_run.last = {"out": {k: v.cpu().clone() for k, v in out.items()}, "workspace": wbuf[GUARD_B:GUARD_B + need].cpu()}
    for k in STATE + ("slots",):
        if out[k].numel() and k not in unwritten:
            assert not bool((out[k] == _fill_of(out[k])).all()), f"{k} was not written"
    return {k: v.cpu().clone() for k, v in out.items()}


def _inputs(name):
    return ms.case(name), ms.masses(name), ms.keys(name), ms.thermal_velocities(name)


def _conf_equal(lad, sca, c, what, keys):
    """conformation c of a ladder run against conformation c of a scalar run: the same bits"""
    for k in keys:
        a, b = lad[k], sca[k]
        if k in ("xyz", "vel", "phi"):
            a, b = a[:, c], b[:, c]
        elif k in ("frames_xyz", "frames_phi"):
            a, b = a[:, :, c], b[:, :, c]
        else:
            a, b = a[..., c], b[..., c]
        assert torch.equal(_bits(a), _bits(b)), f"{what}: {k} of conformation {c} differs"


def _ladder_is_the_scalar_runs(hip, what, batch, m, keys, T, vel, rb=None, ref=None, confs=None, extra=(), **kw):
    lad = _ladder_run(hip, batch, m, keys, T, rb=rb, ref=ref, vel=vel, at_ladder=vel is None, **kw)
    assert torch.equal(lad["slots"], torch.arange(len(T), dtype=torch.int32)[None].expand_as(lad["slots"])), f"{what}: slots of a ladder without exchanges"
    names = STATE + (FRAMES if "frames_xyz" in lad else ()) + tuple(extra)
    for c in range(len(T)) if confs is None else confs:
        sca = _scalar_run(hip, batch, m, keys, rb, ref=ref, vel=vel, **{**kw, "temperature": float(T[c]), "init_temperature": float(T[c]) if vel is None else 0.0})
        _conf_equal(lad, sca, c, what, names)
    return lad


# ------------------------------------------------------------------------------------------------ 1. a ladder without exchanges
@pytest.mark.parametrize("name", ["s65_C3", "s9_65_C17", ms.MIXED, "s9_C1", "s17_C2"])
@pytest.mark.parametrize("friction", [1.0, 50.0])
@pytest.mark.parametrize("n_steps", [5, 40])
def test_ladder_without_exchanges_is_the_scalar_run_of_each_conformation(hip, name, n_steps, friction):
    b, m, k, v = _inputs(name)
    T = mx.ladder(b.xyz.shape[1], 250.0, 35.0)
    _ladder_is_the_scalar_runs(hip, name, b, m, k, T, v, n_steps=n_steps, friction=friction, save_every=5, dt=0.001)


@pytest.mark.parametrize("friction", [1.0, 50.0])
@pytest.mark.parametrize("n_steps", [5, 40])
@pytest.mark.parametrize("name", ["s65_C3", "s9_65_C17"])
def test_drawn_velocities_are_drawn_at_the_slot_temperature(hip, name, n_steps, friction):
    b, m, k, _ = _inputs(name)
    T = mx.ladder(b.xyz.shape[1], 250.0, 35.0)
    _ladder_is_the_scalar_runs(hip, name, b, m, k, T, None, n_steps=n_steps, friction=friction, save_every=5, dt=0.001, first_step=3)
    # ... and at the scalar init_temperature when init_at_ladder is 0
    lad = _ladder_run(hip, b, m, k, T, at_ladder=False, n_steps=0, init_temperature=123.0)
    sca = _scalar_run(hip, b, m, k, None, n_steps=0, init_temperature=123.0)
    assert torch.equal(_bits(lad["vel"]), _bits(sca["vel"]))


def test_ladder_under_a_cutoff(hip):
    name = "s129_C3"
    b, m, k, v = _inputs(name)
    _ladder_is_the_scalar_runs(hip, "cutoff", b, m, k, mx.ladder(3, 250.0, 60.0), v, cutoff=mcut.cutoff(name), n_steps=5, friction=5.0, dt=0.001)


def test_ladder_with_constraints(hip):
    name = "span64"
    b, cons, m, k = msc.case(name)
    _ladder_is_the_scalar_runs(hip, "constraints", b, m, k, mx.ladder(b.xyz.shape[1], 250.0, 60.0), msc.thermal_velocities(name), cons=cons,
                               n_steps=5, friction=5.0, dt=msc.TRAJ_DT)


def test_ladder_in_implicit_solvent(hip):
    name = "s65_C3"
    b, m, k, v = _inputs(name)
    _ladder_is_the_scalar_runs(hip, "obc2", b, m, k, mx.ladder(3, 250.0, 60.0), v, gbs=mg.gb_params(name), solvent=mg.MODEL, extra=("esolv",),
                               n_steps=5, friction=5.0, dt=0.001)


def test_ladder_in_cut_off_solvent_under_a_cutoff_with_constraints(hip):
    name = mgc.CONS_CASE
    b, cons, m, k = msc.case(name)
    _ladder_is_the_scalar_runs(hip, "cut-off obc2 + cutoff + constraints", b, m, k, mx.ladder(b.xyz.shape[1], 250.0, 60.0), msc.thermal_velocities(name),
                               cons=cons, cutoff=mgc.nb_cutoff(name), gbs=list(mg.cons_gb()), solvent=mgc.solvent(name), extra=("esolv",), n_steps=5,
                               friction=5.0, dt=msc.TRAJ_DT)


def test_ladder_with_restraints(hip):
    c = mr.case("s65_C3")
    _ladder_is_the_scalar_runs(hip, "restraints", c["batch"], c["masses"], c["keys"], mx.ladder(3, 250.0, 60.0), c["vel"], rb=c["rb"],
                               extra=("er", "phi"), n_steps=5, friction=5.0, dt=0.001)


def test_equal_temperatures_are_the_scalar_run(hip):
    name = "s9_65_C17"
    b, m, k, v = _inputs(name)
    lad = _ladder_run(hip, b, m, k, np.full(17, 310.0, dtype=np.float32), vel=v, n_steps=40, friction=50.0, save_every=5, dt=0.001)
    sca = _scalar_run(hip, b, m, k, None, vel=v, n_steps=40, friction=50.0, save_every=5, dt=0.001, temperature=310.0)
    for key in STATE + FRAMES:
        assert torch.equal(_bits(lad[key]), _bits(sca[key])), key


def test_the_launch_path_of_a_large_molecule(hip):
    b, m, k, v = _inputs("s513_C1")
    lad = _ladder_is_the_scalar_runs(hip, "s513_C1", b, m, k, np.array([320.0], dtype=np.float32), v, n_steps=5, friction=5.0, dt=0.001)
    ex = _ladder_run(hip, b, m, k, np.array([320.0], dtype=np.float32), K=1, vel=v, n_steps=5, friction=5.0, dt=0.001)
    for key in STATE:          # C = 1: never a pair
        assert torch.equal(_bits(ex[key]), _bits(lad[key])), key
    assert not ex["xs"].any() and bool(torch.isfinite(ex["xe"]).all())


# ------------------------------------------------------------------------------------------------ 2. decisions
def _check_decisions(what, got, T, keys, K, first_step=0, status=None):
    """every decision of the log recomputed in float64 from the logged energies, the previous row of slots and the library's generator
    -> (accepted, rejected, left out)"""
    xs, xe = got["xs"].numpy(), got["xe"].double().numpy()
    U = xe + (got["xr"].double().numpy() if "xr" in got else 0.0)
    X, B, C = xs.shape
    prev = np.tile(np.arange(C), (B, 1))
    acc = rej = skipped = total = 0
    for i in range(X):
        g = first_step + (i + 1) * K
        a = g // K
        for b in range(B):
            st = np.zeros(C, dtype=np.int64) if status is None else status[b]
            if xs[i, b, 0] == FILL_I:          # a molecule without atoms, or a refused one: its rows are untouched
                assert bool((xs[i, b] == FILL_I).all())
                continue
            _, _, dec = mx.exchange_ref(prev[b], mx.inverse(prev[b]), T, np.where(st == 0, U[i, b], np.nan), keys[b], g, K, st, philox=_lib.md_philox)
            moved = np.nonzero(xs[i, b] != prev[b])[0]
            for c in moved:          # alternation: a replica that moved belongs to a pair of the attempt's parity
                assert min(prev[b, c], xs[i, b, c]) % 2 == a % 2 and abs(int(prev[b, c]) - int(xs[i, b, c])) == 1, (what, i, b, c)
            for s, lo, hi, D, u, ok, accept in dec:
                swapped = xs[i, b, lo] == s + 1 and xs[i, b, hi] == s
                stayed = xs[i, b, lo] == s and xs[i, b, hi] == s + 1
                assert swapped or stayed, (what, i, b, s)
                if not ok:
                    assert stayed, f"{what}: a pair with a stopped member was swapped"
                    continue
                total += 1
                if D < 0 and abs(u - np.exp(D)) <= 1e-9:
                    skipped += 1
                    continue
                assert swapped == accept, f"{what}: attempt {a}, molecule {b}, slots ({s}, {s + 1}): D = {D}, u = {u}, logged {'swap' if swapped else 'stay'}"
                acc, rej = acc + int(accept), rej + int(not accept)
            prev[b] = xs[i, b]
    assert 100 * skipped <= total, (what, skipped, total)
    return acc, rej, skipped


@pytest.mark.parametrize("K", mx.EXCHANGE_K)
@pytest.mark.parametrize("name", list(mx.EXCHANGE_CASES))
def test_every_decision_is_the_float64_decision(hip, name, K):
    b, m, k, v = _inputs(name)
    T = mx.EXCHANGE_CASES[name]
    got = _ladder_run(hip, b, m, k, T, K=K, vel=v, n_steps=mx.EXCHANGE_STEPS, friction=mx.FRICTION, dt=0.001)
    assert bool((got["steps"][torch.tensor(b.counts) > 0] == mx.EXCHANGE_STEPS).all()) and not got["status"].any()
    acc, rej, skipped = _check_decisions(name, got, T, k, K)
    print(f"{name}, K = {K}: {acc} accepted, {rej} rejected, {skipped} left out")
    assert acc >= 1 and rej >= 1, (name, K, acc, rej)
    assert torch.equal(got["slots"], got["xs"][-1]) or 0 in b.counts
    rows = torch.tensor(b.counts) > 0
    assert bool((got["slots"][rows].sort(dim=1).values == torch.arange(len(T), dtype=torch.int32)).all())


def test_decisions_with_restraints_count_the_restraint_energy(hip):
    c = mr.case("s65_C3")
    T = mx.EXCHANGE_CASES["s65_C3"]
    got = _ladder_run(hip, c["batch"], c["masses"], c["keys"], T, K=4, rb=c["rb"], vel=c["vel"], n_steps=40, friction=mx.FRICTION, save_every=8, dt=0.001)
    assert bool((got["xr"] > 0).any())
    acc, rej, _ = _check_decisions("restrained", got, T, c["keys"], 4)
    assert acc + rej >= 1
    # the step of a frame and of an attempt: the attempt read the frame's own rows
    assert torch.equal(_bits(got["xe"][1::2]), _bits(got["frames_epot"])) and torch.equal(_bits(got["xr"][1::2]), _bits(got["frames_er"]))


def test_pairs_by_the_number_of_slots(hip):
    b, m, k, v = _inputs("s17_C2")          # C = 2: odd attempts have no pair
    got = _ladder_run(hip, b, m, k, mx.EXCHANGE_CASES["s17_C2"], K=1, vel=v, n_steps=20, friction=mx.FRICTION, dt=0.001)
    xs = got["xs"].numpy()
    prev = np.concatenate([np.arange(2)[None, None], xs[:-1]])
    for i in range(20):
        if (i + 1) % 2 == 1:
            assert np.array_equal(xs[i], prev[i]), f"attempt {i + 1} moved a replica"
    b1, m1, k1, v1 = _inputs("s9_C1")          # C = 1: never a pair
    got = _ladder_run(hip, b1, m1, k1, np.array([300.0], dtype=np.float32), K=1, vel=v1, n_steps=8, friction=mx.FRICTION, dt=0.001)
    assert not got["xs"].any() and not got["slots"].any()


# ------------------------------------------------------------------------------------------------ 3. composition
@pytest.mark.parametrize("name", ["s65_C3", "s9_65_C17"])
def test_a_run_with_exchanges_is_ladder_runs_chained_by_the_logged_swaps(hip, name):
    b, m, k, v = _inputs(name)
    T, K = mx.EXCHANGE_CASES[name], 4
    kw = dict(friction=mx.FRICTION, dt=0.001)
    whole = _ladder_run(hip, b, m, k, T, K=K, vel=v, n_steps=3 * K, **kw)
    C = len(T)
    slots, x, vel = np.tile(np.arange(C), (b.B, 1)), b.xyz, v
    for i in range(3):
        seg = _ladder_run(hip, b, m, k, T, K=0, slots=slots, vel=vel, xyz=x, n_steps=K, first_step=i * K, **kw)
        assert np.array_equal(seg["slots"].numpy(), slots)
        new = whole["xs"][i].numpy()
        vel = seg["vel"].clone().numpy()
        for mol in range(b.B):
            for c in range(C):
                if new[mol, c] != slots[mol, c]:
                    vel[int(b.ptr[mol]):int(b.ptr[mol + 1]), c] *= np.float32(np.sqrt(np.float64(T[new[mol, c]]) / np.float64(T[slots[mol, c]])))
        slots, x, vel = new.copy(), seg["xyz"], torch.from_numpy(vel)
    assert torch.equal(_bits(whole["xyz"]), _bits(x)) and torch.equal(_bits(whole["vel"]), _bits(vel)), "x or v"
    assert np.array_equal(whole["slots"].numpy(), slots)
    # ekin behind an accepted swap at the last step: the rescaled partials against 0.5 sum m v^2 / ACC in float64 from vel_out
    last, before = whole["xs"][-1].numpy(), whole["xs"][-2].numpy()
    mm = torch.from_numpy(np.asarray(m, dtype=np.float32))
    checked = 0
    for mol in range(b.B):
        p0, p1 = int(b.ptr[mol]), int(b.ptr[mol + 1])
        for c in range(C):
            if last[mol, c] == before[mol, c]:
                continue
            vv = whole["vel"][p0:p1, c]
            e64 = float((mm[p0:p1].double() * (vv.double() ** 2).sum(-1)).sum() * (0.5 / md.ACC))
            e32 = float((mm[p0:p1] * (vv * vv).sum(-1)).sum() * np.float32(0.5 / md.ACC))
            err, bound = abs(float(whole["ekin"][mol, c]) - e64), 4 * abs(e32 - e64)
            print(f"{name}: ekin of molecule {mol}, conformation {c} behind a swap: |gpu - f64| = {err:.3e}, bound 4 |f32 - f64| = {bound:.3e}")
            assert err <= bound, (name, mol, c, err, bound)
            checked += 1
    print(f"{name}: {checked} swapped replicas at the last attempt")
    # (the float64 restatement of s65_C3 accepts nothing at attempt 3, so that case may check none; of s9_65_C17 it moves 26 replicas)
    assert checked >= 1 or name != "s9_65_C17", "no replica was swapped at the last attempt: the ekin check ran on nothing"


# ------------------------------------------------------------------------------------------------ 4. bits
ALL = STATE + ("slots", "xs", "xe")


def test_the_same_call_twice_and_any_steps_per_call(hip):
    name = "s9_65_C17"
    b, m, k, v = _inputs(name)
    kw = dict(K=4, vel=v, n_steps=40, friction=mx.FRICTION, save_every=8, dt=0.001)
    first = _ladder_run(hip, b, m, k, mx.EXCHANGE_CASES[name], **kw)
    for spc in (1000, 1, 7, 64):          # with frames every 8 the run calls are cut at multiples of lcm(8, 4): 8, 8, 40 steps
        again = _ladder_run(hip, b, m, k, mx.EXCHANGE_CASES[name], steps_per_call=spc, **kw)
        for key in ALL + FRAMES:
            assert torch.equal(_bits(first[key]), _bits(again[key])), (spc, key)
    kw["save_every"] = 0          # without frames: multiples of K = 4 -- calls of 4, 4 and 40 steps
    plain = _ladder_run(hip, b, m, k, mx.EXCHANGE_CASES[name], **kw)
    for key in ("xs", "xe", "slots"):
        assert torch.equal(_bits(plain[key]), _bits(first[key])), key          # (frames change nothing of the run)
    for spc in (1, 7, 64):
        again = _ladder_run(hip, b, m, k, mx.EXCHANGE_CASES[name], steps_per_call=spc, **kw)
        for key in ALL:
            assert torch.equal(_bits(plain[key]), _bits(again[key])), (spc, key)


def test_run_calls_that_begin_off_an_attempts_boundary(hip, monkeypatch):
    """Without logs the library lets a run call begin anywhere.  The backend never cuts there, so for this test its alignment is
    switched off: run calls of 1, 3 and 7 steps with K = 4 give the bits of the run in one call, attempts included"""
    from grappa_amd import backend_mm
    name = "s9_65_C17"
    b, m, k, v = _inputs(name)
    kw = dict(K=4, vel=v, n_steps=40, friction=mx.FRICTION, dt=0.001)
    logged = _ladder_run(hip, b, m, k, mx.EXCHANGE_CASES[name], **kw)
    assert bool((logged["xs"][1:] != logged["xs"][:-1]).any()), "the case exchanges"
    monkeypatch.setattr(backend_mm.math, "lcm", lambda *a: 1)
    for spc in (1, 3, 7):
        got = _ladder_run(hip, b, m, k, mx.EXCHANGE_CASES[name], steps_per_call=spc, logs=False, **kw)
        for key in STATE + ("slots",):
            assert torch.equal(_bits(got[key]), _bits(logged[key])), (spc, key)
    with pytest.raises(GrappaHipError, match="GRAPPA_ERR_ARG"):          # ... and with a log such a call is refused
        _ladder_run(hip, b, m, k, mx.EXCHANGE_CASES[name], steps_per_call=3, **kw)


def test_a_run_continued_with_its_slots(hip):
    name = "s65_C3"
    b, m, k, v = _inputs(name)
    T, kw = mx.EXCHANGE_CASES[name], dict(K=2, friction=mx.FRICTION, dt=0.001)
    whole = _ladder_run(hip, b, m, k, T, vel=v, n_steps=20, **kw)
    half = _ladder_run(hip, b, m, k, T, vel=v, n_steps=10, **kw)
    rest = _ladder_run(hip, b, m, k, T, slots=half["slots"].numpy(), vel=half["vel"], xyz=half["xyz"], n_steps=10, first_step=10, **kw)
    for key in ("xyz", "vel", "epot", "ekin", "status", "slots"):
        assert torch.equal(_bits(whole[key]), _bits(rest[key])), key
    assert torch.equal(whole["xs"], torch.cat([half["xs"], rest["xs"]])) and torch.equal(_bits(whole["xe"]), _bits(torch.cat([half["xe"], rest["xe"]])))


def test_a_molecule_alone_and_in_the_mixed_batch(hip):
    b, m, k, v = _inputs(ms.MIXED)
    T, kw = mx.EXCHANGE_CASES[ms.MIXED], dict(K=4, n_steps=40, friction=mx.FRICTION, dt=0.001)
    mixed = _ladder_run(hip, b, m, k, T, vel=v, **kw)
    for mol in (0, 2):          # the 1-atom and the 17-atom molecule
        p0, p1 = int(b.ptr[mol]), int(b.ptr[mol + 1])
        alone = _ladder_run(hip, rr.Batch([b.mols[mol]]), m[p0:p1], k[mol:mol + 1], T, vel=v[p0:p1], **kw)
        assert torch.equal(_bits(alone["xyz"]), _bits(mixed["xyz"][p0:p1])) and torch.equal(_bits(alone["vel"]), _bits(mixed["vel"][p0:p1]))
        for key in ("epot", "ekin", "steps", "status", "slots"):
            assert torch.equal(_bits(alone[key][0]), _bits(mixed[key][mol])), (mol, key)
        assert torch.equal(alone["xs"][:, 0], mixed["xs"][:, mol]) and torch.equal(_bits(alone["xe"][:, 0]), _bits(mixed["xe"][:, mol]))


def test_without_a_ladder_the_entries_are_the_restraint_family(hip):
    c = mr.case("s65_C3")
    kw = dict(vel=c["vel"], n_steps=5, friction=5.0, save_every=5, dt=0.001, temperature=290.0)
    for rb in (c["rb"], None):
        got = _ladder_run(hip, c["batch"], c["masses"], c["keys"], None, rb=rb, **kw)
        sca = _scalar_run(hip, c["batch"], c["masses"], c["keys"], rb, **kw)
        for key in STATE + FRAMES + (("er", "phi", "frames_er", "frames_phi") if rb is not None else ()):
            assert torch.equal(_bits(got[key]), _bits(sca[key])), key
        assert torch.equal(got["slots"], torch.arange(3, dtype=torch.int32)[None])


def test_simulate_graph_continues_with_the_slots_it_returned(hip):
    """the continuation the front end prescribes: `ReplicaExchange(..., slots=result.slots)` -- a tensor on the graph's device --
    with velocities= and first_step=, against the uninterrupted run"""
    from grappa_amd import ReplicaExchange, backend
    from grappa_amd.dynamics import simulate_graph
    from grappa_amd.nonbonded import NonbondedBatch
    from grappa_amd.relax import graph_from_parameters
    from test_gpu_md_steps import _parameters
    b, m, k, v = _inputs("s65_C3")
    mol, T = b.mols[0], mx.EXCHANGE_CASES["s65_C3"]
    old = backend._BACKEND
    backend.set_backend(hip)
    try:
        g = graph_from_parameters(_parameters(mol), mol["xyz"].transpose(1, 0, 2)).to("cuda")
        nb = NonbondedBatch([mol["nb"]]).to("cuda")
        kw = dict(keys=k, stepwise="auto", friction=mx.FRICTION, dt=0.001)
        whole = simulate_graph(g, m, nb, velocities=v.to("cuda"), replicas=ReplicaExchange(T, 2), n_steps=20, **kw)
        half = simulate_graph(g, m, nb, velocities=v.to("cuda"), replicas=ReplicaExchange(T, 2), n_steps=10, **kw)
        assert half.slots.is_cuda and tuple(half.slots.shape) == (1, 3)
        g.nodes["n1"].data["xyz"] = half.xyz
        rest = simulate_graph(g, m, nb, velocities=half.velocities, replicas=ReplicaExchange(T, 2, slots=half.slots), n_steps=10, first_step=10, **kw)
        for f in ("xyz", "velocities", "potential_energy", "kinetic_energy", "status", "slots"):
            assert torch.equal(_bits(getattr(whole, f).cpu()), _bits(getattr(rest, f).cpu())), f
        assert torch.equal(whole.exchange_slots.cpu(), torch.cat([half.exchange_slots, rest.exchange_slots]).cpu())
        assert torch.equal(whole.exchange_energy.cpu(), torch.cat([half.exchange_energy, rest.exchange_energy]).cpu())
        assert bool((whole.exchange_slots[1:] != whole.exchange_slots[:-1]).any()), "the run exchanges"
    finally:
        backend.set_backend(old)


# ------------------------------------------------------------------------------------------------ 5. refusals and stops
def test_a_row_of_slots_that_is_no_permutation(hip):
    b, m, k, v = _inputs(ms.MIXED)
    T, kw = mx.EXCHANGE_CASES[ms.MIXED], dict(K=4, vel=v, n_steps=8, friction=mx.FRICTION, dt=0.001)
    good = np.tile(np.array([1, 0, 2]), (b.B, 1))
    ok = _ladder_run(hip, b, m, k, T, slots=good, **kw)
    for bad_row in ([0, 0, 2], [0, 1, 3], [-1, 1, 2]):
        slots = good.copy()
        slots[3] = bad_row
        got = _ladder_run(hip, b, m, k, T, slots=slots, **kw)
        p0, p1 = int(b.ptr[3]), int(b.ptr[4])
        assert bool((got["status"][3] == 5).all())
        assert bool((got["xyz"][p0:p1] == FILL).all()) and bool((got["vel"][p0:p1] == FILL).all()) and bool((got["xs"][:, 3] == FILL_I).all())
        for key in ("epot", "ekin"):
            assert bool((got[key][3] == FILL).all()), key
        assert bool((got["steps"][3] == FILL_I).all()) and bool((got["slots"][3] == FILL_I).all()) and bool((got["xe"][:, 3] == FILL).all())
        for mol in (0, 1, 2, 4, 5):
            q0, q1 = int(b.ptr[mol]), int(b.ptr[mol + 1])
            assert torch.equal(_bits(got["xyz"][q0:q1]), _bits(ok["xyz"][q0:q1])) and torch.equal(_bits(got["vel"][q0:q1]), _bits(ok["vel"][q0:q1]))
            assert torch.equal(got["slots"][mol], ok["slots"][mol]) and torch.equal(got["xs"][:, mol], ok["xs"][:, mol])


def test_a_temperature_the_ladder_refuses(hip):
    b, m, k, v = _inputs("s65_C3")
    for T, K in (([300.0, float("nan"), 320.0], 0), ([300.0, float("inf"), 320.0], 0), ([300.0, -1.0, 320.0], 0), ([300.0, 0.0, 320.0], 4)):
        got = _ladder_run(hip, b, m, k, np.array(T, dtype=np.float32), K=K, vel=v, n_steps=4, friction=5.0, unwritten=STATE + ("slots",))
        assert bool((got["status"] == 5).all()) and bool((got["xyz"] == FILL).all()), T
    got = _ladder_run(hip, b, m, k, np.array([300.0, 0.0, 320.0], dtype=np.float32), K=0, vel=v, n_steps=4, friction=5.0)
    assert not got["status"].any()          # without exchanges a slot at 0 K is a ladder


def test_a_stopped_replica_is_never_swapped(hip):
    base, m, k, v = _inputs(ms.MIXED)
    b = _with_coincident(base, 3, 0, 129, conf=1)
    T, kw = mx.EXCHANGE_CASES[ms.MIXED], dict(K=1, vel=v, n_steps=12, friction=mx.FRICTION, dt=0.001)
    got, ok = _ladder_run(hip, b, m, k, T, **kw), _ladder_run(hip, base, m, k, T, **kw)
    assert got["status"][3].tolist() == [0, 2, 0] and got["steps"][3, 0] == 12 and got["steps"][3, 2] == 12
    assert bool((got["xs"][:, 3, 1] == 1).all()) and got["slots"][3, 1] == 1 and bool(torch.isnan(got["xe"][:, 3, 1]).all())
    status = np.zeros((b.B, 3), dtype=np.int64)
    status[3, 1] = 2
    _check_decisions("stopped", got, T, k, 1, status=status)
    for mol in (0, 1, 2, 4, 5):
        q0, q1 = int(b.ptr[mol]), int(b.ptr[mol + 1])
        assert torch.equal(_bits(got["xyz"][q0:q1]), _bits(ok["xyz"][q0:q1])) and torch.equal(got["xs"][:, mol], ok["xs"][:, mol])


def test_arguments_the_library_refuses(hip):
    b, m, k, v = _inputs("s65_C3")
    T = mx.EXCHANGE_CASES["s65_C3"]
    for kw in (dict(K=4, friction=0.0, n_steps=8), dict(K=4, friction=5.0, n_steps=8, first_step=2)):
        with pytest.raises(GrappaHipError, match="GRAPPA_ERR_ARG"):
            _ladder_run(hip, b, m, k, T, vel=v, **kw)
        last = _ladder_run.last
        for key, t in last["out"].items():
            assert bool((t == (FILL_I if t.dtype == torch.int32 else FILL)).all()), f"{kw}: {key} was written"
        if kw["friction"] == 0.0:          # refused by the plan, before init: nothing launched
            assert bool((last["workspace"] == FILL_B).all()), "the workspace was written"
    lib = hip.lib
    assert lib.grappa_md_remd_init_f32(*([None] * 14), 0, 0, None, 0) == -1
    assert lib.grappa_md_remd_run_f32(*([None] * 13), 0, 0, None, 0, 0, 1, *([None] * 9)) == -1
    assert lib.grappa_md_remd_finish_f32(*([None] * 11), 0, 0, None, 0, *([None] * 10)) == -1


def test_launch_counts(hip):
    """what the header states: init gains one launch over the restrained call, finish one, a step none, a step with an attempt the
    energy launches of a frame plus two -- and only the two where the frame of the same step is written anyway"""
    c = mr.case("s65_C3")
    T = mx.EXCHANGE_CASES["s65_C3"]

    def count(fn, *a, **kw):
        before = hip.lib.grappa_launch_count(0)
        fn(hip, c["batch"], c["masses"], c["keys"], *a, vel=c["vel"], friction=5.0, dt=0.001, **kw)
        return hip.lib.grappa_launch_count(0) - before

    s0, s10, s10f = (count(_scalar_run, c["rb"], n_steps=n, save_every=e) for n, e in ((0, 0), (10, 0), (10, 5)))
    l0, l10, l10f = (count(_ladder_run, T, rb=c["rb"], n_steps=n, save_every=e) for n, e in ((0, 0), (10, 0), (10, 5)))
    x10, x10f = (count(_ladder_run, T, K=5, rb=c["rb"], n_steps=10, save_every=e) for e in (0, 5))
    per_frame = (s10f - s10) // 2
    print(f"launches: init + finish {s0} -> {l0}; 10 steps {s10 - s0} -> {l10 - l0}; a frame {per_frame}; an attempt {(x10 - l10) // 2}, beside a frame {(x10f - l10f) // 2}")
    assert l0 == s0 + 2 and l10 - l0 == s10 - s0 and l10f - l10 == s10f - s10
    assert x10 - l10 == 2 * (per_frame + 2) and x10f - l10f == 2 * 2


# ------------------------------------------------------------------------------------------------ 6. Grappa.simulate
def test_grappa_simulate_with_replicas(hip):
    """Grappa.simulate on the golden molecule: six slots, h-bonds, obc2, 200 steps of 2 fs, an attempt every 20.  Shapes, statuses and
    that the slots stay permutations; the acceptance per pair is printed, not gated"""
    import golden_utils as gu
    from grappa_amd import Grappa, GrappaModel, ReplicaExchange, acceptance, backend
    from grappa_amd.nonbonded import NonbondedParameters
    old = backend._BACKEND
    backend.set_backend(hip)
    try:
        fx = gu.load("ref_small_att.npz")
        model = GrappaModel(**gu.config_of(fx))
        model.load_state_dict(gu.state_dict_of(fx))
        wrapper = Grappa(model, device="cuda")
        mm = gu.molecules_of(fx)[0]
        mol = gu.molecule_of(mm)
        z = np.asarray(mol.atomic_numbers)
        q = np.asarray(mol.partial_charges, dtype=np.float64)
        pos = {int(a): i for i, a in enumerate(mol.atoms)}
        bonds = [(pos[int(a)], pos[int(b)]) for a, b in mol.bonds]
        nbp = NonbondedParameters.from_bonds(bonds, q, np.where(z == 1, 1.0, 3.2), np.where(z == 1, 0.02, 0.1))
        low = wrapper.relax(mol, np.ascontiguousarray(mm["xyz"].transpose(1, 0, 2)[:1]), nbp)
        xyz = np.ascontiguousarray(np.repeat(low.xyz, 6, axis=0))
        T = np.linspace(290.0, 390.0, 6)
        r = wrapper.simulate(mol, xyz, nbp, stepwise="auto", constraints="h-bonds", implicit_solvent="obc2",
                             replicas=ReplicaExchange(T, exchange_every=20), n_steps=200, dt=0.002, friction=5.0, seed=3)
        assert r.xyz.shape == xyz.shape and r.slots.shape == (6,) and r.exchange_slots.shape == (10, 6) and r.exchange_energy.shape == (10, 6)
        assert r.exchange_energy.dtype == np.float64 and not r.status.any() and bool((r.steps == 200).all())
        assert bool(np.isfinite(r.exchange_energy).all()) and bool(np.isfinite(r.xyz).all())
        assert sorted(r.slots.tolist()) == list(range(6)) and all(sorted(row.tolist()) == list(range(6)) for row in r.exchange_slots)
        assert np.array_equal(r.slots, r.exchange_slots[-1])
        print("acceptance per pair:", np.round(acceptance(r.exchange_slots[:, None], np.arange(6))[0], 2).tolist())
    finally:
        backend.set_backend(old)
