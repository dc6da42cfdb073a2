"""GPU: the stepwise dynamics with X-H bond constraints (csrc/dynamics_steps.hip through HipBackend.md_steps_cons and
grappa_amd/dynamics.py) against the restatement of tests/md_cons_refs.py on the cases of tests/md_steps_cons_refs.py, inside
sentinel-guarded output buffers and a guarded workspace.

Gates: those of tests/test_gpu_md_cons.py, used as they stand (its _gate_state: max_atoms |x_gpu - x_f64| <= 4 max_atoms |x_f32
restatement - x_f64| + 2^-20 A per item, the same for v with the floor 2^-20 max |v|, with the sibling rule; its _assert_constrained:
| |x_k - x_0| - d_k | <= tol d_k + 4 ulp32(max |x|) and |r_k . (v_k - v_0)| <= 2^-18 |r_k| max |v|).  Energy conservation:
D_gpu <= 2 max(D_f32, D_f64), the bound of tests/test_gpu_md.py."""
import numpy as np
import pytest
import torch

import golden_utils as gu
import md_cons_refs as mc
import md_refs as md
import md_steps_cons_refs as msc
import relax_refs as rr
import relax_steps_refs as rs
import test_gpu_md_cons as tc
from grappa_amd.constraints import ConstraintBatch, Constraints

pytestmark = pytest.mark.gpu

FILL, FILL_I, FILL_B, GUARD_B = tc.FILL, tc.FILL_I, 0xA5, 4096
OUTS, FRAMES = tc.OUTS, tc.FRAMES
_bits, _same_bits, _rows_of, _dev_keys = tc._bits, tc._same_bits, tc._rows_of, tc._dev_keys


@pytest.fixture(scope="module")
def hip():
    from grappa_amd.backend import HipBackend
    return HipBackend()


def _fill_of(buf):
    return FILL_I if buf.dtype == torch.int32 else FILL


def _run(hip, batch, cons, masses, keys, vel=None, xyz=None, tables=None, tolerance=mc.TOL, constrain_start=True, cutoff=None,
         steps_per_call=1000, short=0, seam="cons", **opts):
    """one call of the seam -> dict of CPU tensors (OUTS, and FRAMES when save_every > 0); asserts the guards around the outputs and the
    workspace.  cons: a list of Constraints or None per molecule; tables: a function that edits the ConstraintBatch; seam: "cons"
    (md_steps_cons), "cons_none" (md_steps_cons without constraints), "steps" (md_steps); short: bytes the workspace lacks"""
    o = {**md.MD_OPTS, **opts}
    plan = batch.plan("cuda")
    x = (batch.xyz if xyz is None else xyz).to("cuda")
    N, Cc, B = batch.N, x.shape[1], batch.B
    F = o["n_steps"] // o["save_every"] if o["save_every"] > 0 and o["n_steps"] > 0 else 0
    shapes = {"xyz": ((N, Cc, 3), torch.float32), "vel": ((N, Cc, 3), torch.float32), "epot": ((B, Cc), torch.float32),
              "ekin": ((B, Cc), torch.float32), "steps": ((B, Cc), torch.int32), "status": ((B, Cc), torch.int32)}
    if F:
        shapes.update({"frames_xyz": ((F, N, Cc, 3), torch.float32), "frames_epot": ((F, B, Cc), torch.float32),
                       "frames_ekin": ((F, B, Cc), torch.float32)})
    bufs = {k: tc._guarded(*v) for k, v in shapes.items()}
    out = {k: v[1] for k, v in bufs.items()}
    extra = {}
    K = 0
    if seam == "cons":
        cb = ConstraintBatch(cons, tolerance=tolerance)
        if tables is not None:
            tables(cb)
        K = int(cb.cluster_atoms.shape[0])
        extra = dict(constraints=cb.to("cuda"), constrain_start=constrain_start)
    need = int(hip.lib.grappa_md_steps_cons_workspace_bytes(N, Cc, B, rs.n_blocks(batch), K, int(cutoff is not None)))
    wbuf = torch.full((GUARD_B + need + GUARD_B,), FILL_B, dtype=torch.uint8, device="cuda")
    ws = wbuf[GUARD_B:GUARD_B + max(need - short, 0)]
    if cutoff is not None:
        extra["cutoff"] = cutoff
    call = hip.md_steps if seam == "steps" else hip.md_steps_cons
    args = (plan, x, [k.to("cuda") for k in batch.ks], [None if q is None else q.to("cuda") for q in batch.eqs], batch.n_per, False,
            batch.nonbonded().to("cuda"), o, torch.from_numpy(np.asarray(masses, dtype=np.float32)).to("cuda"), _dev_keys(keys),
            None if vel is None else vel.to("cuda"), out["xyz"], out["vel"], out["epot"], out["ekin"], out["steps"], out["status"])
    try:
        call(*args, frames_xyz=out.get("frames_xyz"), frames_epot=out.get("frames_epot"), frames_ekin=out.get("frames_ekin"),
             atom_counts_host=batch.counts, steps_per_call=steps_per_call, workspace=ws, **extra)
    except Exception:          # a refused call has written nothing
        torch.cuda.synchronize()
        for name, (buf, _) in bufs.items():
            assert bool((buf == _fill_of(buf)).all()), f"a refused call wrote {name}"
        assert bool((wbuf == FILL_B).all()), "a refused call wrote to the workspace"
        raise
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert bool((buf[:64] == _fill_of(buf)).all()) and bool((buf[-64:] == _fill_of(buf)).all()), f"written outside {k}"
    assert bool((wbuf[:GUARD_B] == FILL_B).all()) and bool((wbuf[-GUARD_B - short:] == FILL_B).all()), "written outside the workspace"
    return {k: v.cpu().clone() for k, v in out.items()}


def _case_run(hip, name, **kw):
    batch, cons, m, keys = msc.case(name)
    return _run(hip, batch, cons, m, keys, **kw)


def _live(batch):
    return torch.tensor([n > 0 for n in batch.counts])


def _assert_ran(batch, got, n_steps):
    live = _live(batch)
    assert bool((got["steps"][live] == n_steps).all()) and not got["status"][live].any(), (got["steps"].tolist(), got["status"].tolist())


# ------------------------------------------------------------------------------------------------ 1. trajectories
TRAJ = [(n, s) for n in msc.TRAJ_CASES for s in msc.TRAJ_STEPS]


@pytest.mark.parametrize("name,n_steps", TRAJ, ids=[f"{n}-{s}steps" for n, s in TRAJ])
def test_trajectory_without_thermostat(hip, name, n_steps):
    """friction 0, 2 fs, from the case coordinates (constrained first) with thermal velocities (projected first)"""
    batch = msc.case(name)[0]
    r64, r32s = msc.verlet(name)["snap"][n_steps], [r[n_steps] for r in msc.verlet32(name)]
    got = _case_run(hip, name, vel=msc.thermal_velocities(name), n_steps=n_steps, dt=msc.TRAJ_DT)
    _assert_ran(batch, got, n_steps)
    tc._gate_state(name, f"stepwise, {n_steps} steps, friction 0", batch, got, r64, r32s)
    tc._assert_constrained(name, msc.tables(name), batch, got["xyz"], got["vel"])


THERMO = dict(friction=50.0, temperature=300.0, dt=msc.TRAJ_DT, first_step=7)


@pytest.mark.parametrize("name", msc.TRAJ_CASES)
def test_trajectory_with_thermostat(hip, name):
    """40 steps at friction 50 / ps and 300 K, 2 fs; the restatements consume the noise md_noise wrote for these steps, so only the
    integrator is under test"""
    batch, cons, m, keys = msc.case(name)
    Cc, first, total = batch.xyz.shape[1], THERMO["first_step"], max(msc.TRAJ_STEPS)
    z = {first + k: tc._noise(hip, batch.counts, keys, Cc, first + k) for k in range(total)}
    common = dict(velocities=msc.thermal_velocities(name), noise=lambda step, purpose: z[step], n_steps=total, **THERMO)
    r64 = mc.gbaoab_ref(batch, m, cons, torch.float64, snapshots=(total,), **common)["snap"][total]
    r32s = [r[total] for r in mc.fp32_realisations(batch, m, cons, (total,), **common)]
    got = _case_run(hip, name, vel=msc.thermal_velocities(name), n_steps=total, **THERMO)
    _assert_ran(batch, got, total)
    tc._gate_state(name, f"stepwise, {total} steps, friction 50", batch, got, r64, r32s)
    tc._assert_constrained(name, msc.tables(name), batch, got["xyz"], got["vel"])


# ------------------------------------------------------------------------------------------------ 2. the same under the cutoff
@pytest.mark.parametrize("name", msc.CUT_CASES)
def test_trajectory_under_the_cutoff(hip, name):
    batch = msc.case(name)[0]
    for n_steps in msc.TRAJ_STEPS:
        r64, r32s = msc.verlet(name, True)["snap"][n_steps], [r[n_steps] for r in msc.verlet32(name, True)]
        got = _case_run(hip, name, vel=msc.thermal_velocities(name), n_steps=n_steps, dt=msc.TRAJ_DT, cutoff=msc.cutoff(name))
        _assert_ran(batch, got, n_steps)
        tc._gate_state(name, f"stepwise under the cutoff, {n_steps} steps", batch, got, r64, r32s)
        tc._assert_constrained(name, msc.tables(name), batch, got["xyz"], got["vel"])
        if n_steps == max(msc.TRAJ_STEPS):
            whole = _case_run(hip, name, vel=msc.thermal_velocities(name), n_steps=n_steps, dt=msc.TRAJ_DT, cutoff=msc.cutoff(name, False))
            _same_bits(got, whole, f"{name}: prune=True against prune=False")


# ------------------------------------------------------------------------------------------------ 3. constraints on every frame
@pytest.mark.parametrize("name,cut", [("span64", False), ("scattered130", False), ("k300", True)])
def test_every_frame_is_constrained(hip, name, cut):
    batch = msc.case(name)[0]
    opts = dict(n_steps=20, save_every=4, dt=msc.TRAJ_DT, friction=20.0, temperature=300.0, init_temperature=300.0)
    got = _case_run(hip, name, cutoff=msc.cutoff(name) if cut else None, **opts)          # velocities drawn, then projected
    _assert_ran(batch, got, 20)
    worst = [tc._assert_constrained(name, msc.tables(name), batch, got["xyz"], got["vel"], what="outputs")]
    for f in range(5):
        worst.append(tc._assert_constrained(name, msc.tables(name), batch, got["frames_xyz"][f], what=f"frame {f}"))
    print(f"{name}: largest bond error / bound {max(w[0] for w in worst):.3f}, |r.(vk - v0)| / (|r| max|v|) {worst[0][1]:.3e}")
    assert torch.equal(_bits(got["frames_xyz"][4]), _bits(got["xyz"])) and torch.equal(_bits(got["frames_ekin"][4]), _bits(got["ekin"]))
    assert torch.equal(_bits(got["frames_epot"][4]), _bits(got["epot"]))


# ------------------------------------------------------------------------------------------------ 4. bits
def test_the_same_call_twice_gives_the_same_bits(hip):
    opts = dict(vel=msc.thermal_velocities("scattered130"), n_steps=15, save_every=5, friction=10.0, temperature=300.0, dt=msc.TRAJ_DT)
    _same_bits(_case_run(hip, "scattered130", **opts), _case_run(hip, "scattered130", **opts), "scattered130 twice", keys=OUTS + FRAMES)


def test_a_molecule_alone_gives_the_bits_it_gives_in_the_batch(hip):
    batch, cons, m, keys = msc.case("mixed")
    vel = msc.thermal_velocities("mixed")
    opts = dict(n_steps=12, save_every=4, friction=10.0, temperature=300.0, dt=msc.TRAJ_DT)
    whole = _run(hip, batch, cons, m, keys, vel=vel, **opts)
    for b in range(batch.B):
        if batch.counts[b] == 0:
            continue
        p0, p1 = int(batch.ptr[b]), int(batch.ptr[b + 1])
        one = _run(hip, rr.Batch([batch.mols[b]]), [cons[b]], m[p0:p1], keys[b:b + 1], vel=vel[p0:p1], **opts)
        _same_bits(_rows_of(whole, batch, b), _rows_of(one, rr.Batch([batch.mols[b]]), 0), f"mixed molecule {b} alone", keys=OUTS + FRAMES)


def test_without_constraints_the_launches_and_the_bits_are_md_steps(hip):
    batch, cons, m, keys = msc.case("span64")
    vel = msc.thermal_velocities("span64")
    for cutoff in (None, msc.cutoff("span64")):
        opts = dict(vel=vel, n_steps=6, save_every=3, friction=5.0, temperature=300.0, cutoff=cutoff)
        runs, launches = {}, {}
        for seam, c in (("steps", cons), ("cons_none", cons), ("cons", [None])):          # md_steps; cons == NULL; K == 0
            before = hip.lib.grappa_launch_count(0)
            runs[seam] = _run(hip, batch, c, m, keys, seam=seam, **opts)
            launches[seam] = hip.lib.grappa_launch_count(0) - before
        assert launches["steps"] == launches["cons_none"] == launches["cons"], launches
        _same_bits(runs["cons_none"], runs["steps"], "cons == NULL", keys=OUTS + FRAMES)
        _same_bits(runs["cons"], runs["steps"], "K == 0", keys=OUTS + FRAMES)


@pytest.mark.parametrize("cut", [False, True], ids=["all_pairs", "cutoff"])
def test_the_bits_do_not_depend_on_how_steps_are_dealt_to_run_calls_or_on_frames(hip, cut):
    """40 steps as 40, 4 x 10 and 13 + 13 + 14, each with frames that match and without"""
    opts = dict(vel=msc.thermal_velocities("span64"), n_steps=40, friction=10.0, temperature=300.0, dt=msc.TRAJ_DT,
                cutoff=msc.cutoff("span64") if cut else None)
    runs = {(spc, every): _case_run(hip, "span64", steps_per_call=spc, save_every=every, **opts)
            for spc, every in ((1000, 0), (1000, 10), (10, 0), (10, 10), (13, 0), (13, 13))}
    for key, r in runs.items():
        _same_bits(r, runs[(1000, 0)], f"steps_per_call, save_every = {key}")
    _same_bits(runs[(10, 10)], runs[(1000, 10)], "the frames at 10, 20, 30, 40", keys=FRAMES)
    assert runs[(13, 13)]["frames_xyz"].shape[0] == 3 and bool(torch.isfinite(runs[(13, 13)]["frames_xyz"]).all())


def test_continuation(hip):
    """10 + 30 steps through finish and init with constrain_start = 0 and first_step + 10: the bits of 40 steps"""
    batch, cons, m, keys = msc.case("scattered130")
    opts = dict(friction=10.0, temperature=300.0, dt=msc.TRAJ_DT, first_step=3)
    whole = _run(hip, batch, cons, m, keys, vel=msc.thermal_velocities("scattered130"), n_steps=40, **opts)
    a = _run(hip, batch, cons, m, keys, vel=msc.thermal_velocities("scattered130"), n_steps=10, **opts)
    b = _run(hip, batch, cons, m, keys, vel=a["vel"], xyz=a["xyz"], n_steps=30, constrain_start=False, **{**opts, "first_step": 13})
    assert bool((a["steps"] == 10).all()) and bool((b["steps"] == 30).all())
    _same_bits(b, whole, "10 + 30 steps", keys=("xyz", "vel", "epot", "ekin", "status"))


# ------------------------------------------------------------------------------------------------ 5. launches
def test_a_step_is_three_launches_and_four_under_a_cutoff(hip):
    added = {}
    for name in ("span64", "k300"):
        batch, cons, m, keys = msc.case(name)
        for cut in (False, True):
            n = []
            for steps in (0, 10):
                before = hip.lib.grappa_launch_count(0)
                _run(hip, batch, cons, m, keys, vel=msc.thermal_velocities(name), n_steps=steps, cutoff=msc.cutoff(name) if cut else None)
                n.append(hip.lib.grappa_launch_count(0) - before)
            added[(name, cut)] = n[1] - n[0]          # init and finish launch the same with and without steps in between
    print(f"launches added by a run of 10 steps: {added}")
    assert added == {("span64", False): 30, ("k300", False): 30, ("span64", True): 40, ("k300", True): 40}


# ------------------------------------------------------------------------------------------------ 6. the two paths
@pytest.mark.parametrize("name", ["mix", "edge256"])
def test_the_two_paths_agree(hip, name):
    batch, cons, m, keys = mc.case(name)
    n_steps = max(msc.TRAJ_STEPS)
    r64, r32s = mc.verlet(name)["snap"][n_steps], [r[n_steps] for r in mc.verlet32(name)]
    opts = dict(vel=mc.thermal_velocities(name), n_steps=n_steps, dt=mc.TRAJ_DT)
    fused, steps = tc._run(hip, batch, cons, m, keys, **opts), _run(hip, batch, cons, m, keys, **opts)
    assert torch.equal(fused["steps"], steps["steps"]) and torch.equal(fused["status"], steps["status"])
    for label, got in (("fused", fused), ("stepwise", steps)):
        tc._gate_state(name, f"{label}, {n_steps} steps, friction 0", batch, got, r64, r32s)
    # an atom's noise is the same on both paths: one step from rest at 0 K start, the thermostat alone moves the atoms; the noise is
    # a function of (key, atom, conformation, step) that neither path's decomposition enters
    # (2^-12 of the largest velocity: the two paths' forces differ by fp32 rounding, some 2^-20 relative; another deviate would differ by
    # the size of the velocity itself)
    hot = dict(n_steps=1, dt=mc.TRAJ_DT, friction=50.0, temperature=300.0, init_temperature=0.0, first_step=11)
    f1, s1 = tc._run(hip, batch, cons, m, keys, **hot), _run(hip, batch, cons, m, keys, **hot)
    assert float(f1["vel"].abs().max()) > 0
    scale = mc.item_max(batch, f1["vel"]).max()
    assert float((f1["vel"].double() - s1["vel"].double()).norm(dim=-1).max()) <= 2.0 ** -12 * float(scale)


# ------------------------------------------------------------------------------------------------ 7. frozen atoms
def test_frozen_atoms(hip):
    """span64 with a frozen centre, a frozen leaf and a cluster frozen at both ends, 25 steps"""
    batch, cons, m, keys = msc.case("span64")
    rows = cons[0].clusters
    centre, leaf, both = int(rows[0, 0]), int(rows[1, 1]), (int(rows[2, 0]), int(rows[2, 1]))
    frozen = [centre, leaf, *both]
    mf = m.copy()
    mf[frozen] = 0.0
    vel = msc.thermal_velocities("span64")
    opts = dict(velocities=vel, snapshots=(25,), n_steps=25, dt=msc.TRAJ_DT)
    r64 = mc.gbaoab_ref(batch, mf, cons, torch.float64, **opts)["snap"][25]
    r32s = [r[25] for r in mc.fp32_realisations(batch, mf, cons, (25,), **{k: v for k, v in opts.items() if k != "snapshots"})]
    got = _run(hip, batch, cons, mf, keys, vel=vel, n_steps=25, dt=msc.TRAJ_DT, constrain_start=False)
    start = _run(hip, batch, cons, mf, keys, vel=vel, n_steps=0, constrain_start=False)
    _assert_ran(batch, got, 25)
    assert torch.equal(_bits(got["xyz"][frozen]), _bits(batch.xyz[frozen])), "a frozen atom moved"
    assert not got["vel"][frozen].any() and not start["vel"][frozen].any()
    got = _run(hip, batch, cons, mf, keys, vel=vel, n_steps=25, dt=msc.TRAJ_DT)
    _assert_ran(batch, got, 25)
    assert torch.equal(_bits(got["xyz"][frozen]), _bits(batch.xyz[frozen])), "a frozen atom moved"
    tc._gate_state("span64", "frozen atoms, 25 steps", batch, got, r64, r32s)
    # lengths are held where an end moves; the bond frozen at both ends keeps the length it came with
    tab = msc.tables("span64")
    keep = ~((tab.centre == both[0]))
    part = mc.Tables.__new__(mc.Tables)
    part.centre, part.leaf, part.d, part.mol, part.K, part.L = tab.centre[keep], tab.leaf[keep], tab.d[keep], tab.mol[keep], int(keep.sum()), tab.L
    tc._assert_constrained("span64", part, batch, got["xyz"], got["vel"], what="frozen atoms")


# ------------------------------------------------------------------------------------------------ 8. status 4
def test_a_constraint_that_cannot_be_met_ends_its_item_with_status_4(hip):
    """md_cons_refs.unsatisfiable() beside span64's first conformation: a constraint that cannot be met, not a device fault"""
    xh, cons, m, keys, v = mc.unsatisfiable()
    sb, scons, sm, skeys = msc.case("span64")
    calm_mol = dict(sb.mols[0], xyz=sb.mols[0]["xyz"][:, :1])
    calm = rr.Batch([calm_mol])
    calm_v = msc.thermal_velocities("span64")[:, :1].contiguous()
    both = rr.Batch([xh.mols[0], calm_mol])
    vel = torch.cat([v, calm_v])
    opts = dict(n_steps=6, save_every=1, dt=0.001, steps_per_call=2)          # three run calls: the status survives them and finish
    got = _run(hip, both, [cons[0], scons[0]], np.concatenate([m, sm]), np.concatenate([keys, skeys]), vel=vel, **opts)
    assert got["status"].flatten().tolist() == [4, 0] and got["steps"].flatten().tolist() == [0, 6]
    assert bool(torch.isfinite(got["xyz"]).all())
    alone = _run(hip, calm, scons, sm, skeys, vel=calm_v, **opts)
    _same_bits(_rows_of(got, both, 1), _rows_of(alone, calm, 0), "the neighbour of a failed item", keys=OUTS + FRAMES)
    # the status-2 rule for frames: the frame of the step that found the failure is written, no later one
    assert bool(torch.isfinite(got["frames_xyz"][0, :2]).all()) and not bool((got["frames_xyz"][0, :2] == FILL).all())
    assert bool((got["frames_xyz"][1:, :2] == FILL).all()) and bool((got["frames_epot"][1:, 0] == FILL).all())
    assert bool((got["frames_ekin"][1:, 0] == FILL).all())
    assert torch.equal(_bits(got["frames_xyz"][0, :2]), _bits(got["xyz"][:2])), "the failed item's state is not the one it held after that step"
    r = mc.gbaoab_ref(both, np.concatenate([m, sm]), [cons[0], scons[0]], torch.float32, velocities=vel, n_steps=6, dt=0.001)
    assert r["status"].flatten().tolist() == [4, 0] and r["steps"].flatten().tolist() == [0, 6]
    # the start's S failing: 0 steps as well, and no frame at all
    far = both.xyz.clone()
    far[1] = far[0]          # the leaf on its centre: no direction to restore the length along
    got = _run(hip, both, [cons[0], scons[0]], np.concatenate([m, sm]), np.concatenate([keys, skeys]), vel=torch.zeros_like(vel), xyz=far, **opts)
    assert got["status"].flatten().tolist() == [4, 0] and got["steps"].flatten().tolist() == [0, 6]
    assert bool((got["frames_xyz"][:, :2] == FILL).all())


# ------------------------------------------------------------------------------------------------ 9. status 5
def _edit(row, col, value, d=False):
    def apply(cb):
        (cb.cluster_d if d else cb.cluster_atoms)[row, col] = value
    return apply


def _two_blocks():
    """two clusters of scattered130 whose centres lie in different blocks -> (row a, row b)"""
    rows = msc.case("scattered130")[1][0].clusters
    blocks = rows[:, 0] // msc.BLOCK
    a = 0
    b = int(np.nonzero(blocks != blocks[a])[0][0])
    return a, b


BAD_TABLES = ["an atom in two clusters whose centres lie in different blocks", "an index equal to n", "a length of 0", "a leaf that is its centre",
              "a cluster without leaves"]


@pytest.mark.parametrize("what", BAD_TABLES)
def test_bad_tables_end_the_item_with_status_5_and_nothing_else(hip, what):
    """scattered130 beside mix's plain molecule, one table entry spoilt; the neighbour runs as before"""
    sb, scons, sm, skeys = msc.case("scattered130")
    mb, _, mm, mkeys = mc.case("mix")
    batch = rr.Batch([sb.mols[0], mb.mols[1]])
    cons, m, keys = [scons[0], None], np.concatenate([sm, mm[18:25]]), np.concatenate([skeys, mkeys[1:2]])
    rows = scons[0].clusters
    a, b = _two_blocks()
    assert rows[a, 0] // msc.BLOCK != rows[b, 0] // msc.BLOCK
    single = int(np.nonzero((rows[:, 1:] >= 0).sum(1) == 1)[0][0])
    edit = {BAD_TABLES[0]: _edit(b, 1, int(rows[a, 1])), BAD_TABLES[1]: _edit(a, 1, 136), BAD_TABLES[2]: _edit(a, 0, 0.0, d=True),
            BAD_TABLES[3]: _edit(b, 1, int(rows[b, 0])), BAD_TABLES[4]: _edit(single, 1, -1)}[what]
    opts = dict(n_steps=10, save_every=5, friction=20.0, temperature=300.0, init_temperature=300.0, steps_per_call=5)
    good = _run(hip, batch, cons, m, keys, **opts)
    assert good["status"].flatten().tolist() == [0] * 6
    got = _run(hip, batch, cons, m, keys, tables=edit, **opts)
    assert got["status"][0].tolist() == [5, 5, 5], what
    assert bool((got["xyz"][:136] == FILL).all()) and bool((got["vel"][:136] == FILL).all()) and bool((got["steps"][0] == FILL_I).all())
    assert bool((got["epot"][0] == FILL).all()) and bool((got["ekin"][0] == FILL).all()) and bool((got["frames_xyz"][:, :136] == FILL).all())
    assert bool((got["frames_epot"][:, 0] == FILL).all()) and bool((got["frames_ekin"][:, 0] == FILL).all())
    _same_bits(_rows_of(got, batch, 1), _rows_of(good, batch, 1), f"the neighbour of {what}", keys=OUTS + FRAMES)


# ------------------------------------------------------------------------------------------------ 10. bad arguments
def test_bad_arguments_are_refused_with_nothing_launched(hip, monkeypatch):
    from grappa_amd.backend import GrappaHipError
    batch, cons, m, keys = msc.case("span64")
    before = hip.lib.grappa_launch_count(0)
    for tol in (2.0 ** -21, 2.0 ** -6, float("nan")):
        def spoil(cb, tol=tol):
            cb.tolerance = tol
        with pytest.raises(GrappaHipError, match="GRAPPA_ERR_ARG"):
            _run(hip, batch, cons, m, keys, tables=spoil, n_steps=2)
    make = type(hip)._md_cons
    for field, value in (("K", -1), ("cluster_d", None), ("cluster_atoms", None), ("cluster_molptr", None)):
        def spoilt(*a, field=field, value=value, **kw):
            c = make(*a, **kw)
            setattr(c, field, value)
            return c
        monkeypatch.setattr(hip, "_md_cons", spoilt)
        with pytest.raises(GrappaHipError, match="GRAPPA_ERR_ARG"):
            _run(hip, batch, cons, m, keys, n_steps=2)
        monkeypatch.undo()
    for cut in (None, msc.cutoff("span64")):
        with pytest.raises(GrappaHipError, match="GRAPPA_ERR_WORKSPACE"):
            _run(hip, batch, cons, m, keys, n_steps=2, short=1, cutoff=cut)
    assert hip.lib.grappa_launch_count(0) == before, "a refused call launched something"
    _run(hip, batch, cons, m, keys, tolerance=2.0 ** -20, n_steps=2)
    _run(hip, batch, cons, m, keys, tolerance=2.0 ** -7, n_steps=2)


# ------------------------------------------------------------------------------------------------ 11. energy conservation
def test_energy_conservation(hip):
    """NVE on the 64 ethane replicas through the stepwise path: constrain_start, velocities drawn at 600 K, 2000 steps of 1 fs, a
    frame every 50.  D_gpu <= 2 max(D_f32, D_f64), the bound of tests/test_gpu_md.py"""
    batch, cons, m, keys = mc.case("ethane64")
    start = _run(hip, batch, cons, m, keys, **{**mc.NVE, "n_steps": 0, "save_every": 0})
    got = _run(hip, batch, cons, m, keys, **mc.NVE)
    assert not got["status"].any() and bool((got["steps"] == mc.NVE["n_steps"]).all())
    d_gpu = md.drift(start["epot"].double() + start["ekin"].double(), got["frames_epot"].double() + got["frames_ekin"].double())
    d32, d64 = mc.nve_drift(torch.float32), mc.nve_drift(torch.float64)
    print(f"energy conservation, stepwise with constraints: D_gpu {d_gpu:.4f}, D_f32 {d32:.4f}, D_f64 {d64:.4f} kcal/mol, "
          f"D_gpu / max = {d_gpu / max(d32, d64):.3f}")
    assert d_gpu <= 2 * max(d32, d64)
    for f in range(got["frames_xyz"].shape[0]):
        tc._assert_constrained("ethane64", mc.tables("ethane64"), batch, got["frames_xyz"][f], what=f"frame {f}")


# ------------------------------------------------------------------------------------------------ 12. the public door
def test_grappa_simulate_holds_the_hydrogen_bonds_on_the_stepwise_path(hip):
    from grappa_amd import Grappa, GrappaModel, backend
    from grappa_amd.constraints import hydrogen_constraints
    old = backend._BACKEND
    backend.set_backend(hip)
    try:
        fx = gu.load("ref_small_att.npz")
        model = GrappaModel(**gu.config_of(fx))
        model.load_state_dict(gu.state_dict_of(fx))
        wrapper = Grappa(model, device="cuda")
        mm = gu.molecules_of(fx)[0]
        mol = gu.molecule_of(mm)
        low = wrapper.relax(mol, np.ascontiguousarray(mm["xyz"].transpose(1, 0, 2)[:2]))
        assert bool((low.status != 2).all())
        xyz = np.ascontiguousarray(low.xyz)
        r = wrapper.simulate(mol, xyz, n_steps=200, dt=0.001, friction=0.0, init_temperature=300.0, seed=9, constraints="h-bonds", stepwise=True)
        assert r.xyz.shape == xyz.shape and not r.status.any() and bool((r.steps == 200).all()) and bool(np.isfinite(r.xyz).all())
        cons = hydrogen_constraints(wrapper.predict(mol), mol.atomic_numbers)
        c, l, d = cons.pairs()
        length = np.linalg.norm(r.xyz[:, l] - r.xyz[:, c], axis=-1)
        ulp = 2.0 ** (np.floor(np.log2(np.abs(r.xyz).max(axis=(1, 2)))) - 23)
        err = np.abs(length - d[None])
        print(f"Grappa.simulate, stepwise with h-bonds: {cons.n_constraints} constraints, largest | |r| - d | = {err.max():.3e} A")
        assert cons.n_constraints > 0 and bool((err <= mc.TOL * d[None] + 4 * ulp[:, None]).all())
    finally:
        backend.set_backend(old)


def test_simulate_auto_with_a_cutoff_and_constraints_runs_k300(hip):
    from grappa_amd import backend
    from grappa_amd.dynamics import simulate
    import test_host_md_steps_cons as th
    old = backend._BACKEND
    backend.set_backend(hip)
    try:
        batch, cons, m, keys = msc.case("k300")
        mol = batch.mols[0]
        vel = msc.thermal_velocities("k300")
        r = simulate(th._parameters(mol), mol["xyz"].transpose(1, 0, 2), m, mol["nb"], device="cuda", stepwise="auto", cutoff=msc.cutoff("k300"),
                     constraints=cons[0], velocities=vel.numpy().transpose(1, 0, 2), keys=keys, friction=0.0, dt=msc.TRAJ_DT, n_steps=5)
        assert r.status.tolist() == [0] and r.steps.tolist() == [5]
        got = {"xyz": torch.from_numpy(r.xyz.transpose(1, 0, 2)).float(), "vel": torch.from_numpy(r.velocities.transpose(1, 0, 2)).float()}
        tc._gate_state("k300", "simulate(stepwise='auto', cutoff=, constraints=), 5 steps", batch, got, msc.verlet("k300", True)["snap"][5],
                       [x[5] for x in msc.verlet32("k300", True)])
    finally:
        backend.set_backend(old)
