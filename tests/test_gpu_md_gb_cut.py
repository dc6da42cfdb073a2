"""GPU: the stepwise dynamics in GB/SA implicit solvent under the solvent's cutoff (grappa_md_steps_*_gbcut_f32 through
HipBackend.md_steps_gb with an `ImplicitSolvent(cutoff=)`) against the restatements of tests/md_gb_cut_refs.py: trajectories through
the gate of tests/test_gpu_md.py as it stands, the bits (two runs, chunk sizes, continuation, prune 0 against 1, gbcut = NULL against
the _gb_ entries), the energies against the library's own energy entries with and without the nonbonded cutoff, the launch budget, a
stopped conformation, refusals and the public door.  Every output and the workspace lie between guard words.
No energy-conservation test: a truncated pair sum is not conservative when a pair crosses the cutoff."""
import ctypes as C

import numpy as np
import pytest
import torch

import md_gb_cut_refs as mgc
import md_gb_refs as mg
import md_refs as md
import md_steps_refs as ms
import relax_steps_refs as rs
from grappa_amd import _lib
from grappa_amd.solvent import GBBatch, ImplicitSolvent
from test_gpu_md import _gate_state
from test_gpu_md_steps import FILL_B, GUARD_B, OUTS, _bits, _dev_keys, _fill_of, _guarded, _inputs, _noise, _output_buffers, _same_bits
from test_gpu_md_gb import GB_FRAMES, GB_OUTS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from grappa_amd.backend import HipBackend
    return HipBackend()


def _run(hip, batch, masses, keys, gbs, solvent, vel=None, xyz=None, steps_per_call=1000, cons=None, cutoff=None, **opts):
    """one call of the seam in the truncated solvent on a relax_refs.Batch -> dict of CPU tensors (GB_OUTS, and GB_FRAMES when
    save_every > 0); asserts the guards around the outputs and the workspace.  cutoff: the nonbonded cutoff or None"""
    o = {**md.MD_OPTS, **opts}
    plan = batch.plan("cuda")
    dnb = batch.nonbonded().to("cuda")
    x = (batch.xyz if xyz is None else xyz).to("cuda")
    Cc = x.shape[1]
    bufs = _output_buffers(batch, Cc, o)
    bufs["esolv"] = _guarded((batch.B, Cc))
    if "frames_epot" in bufs:
        bufs["frames_esolv"] = _guarded(tuple(bufs["frames_epot"][1].shape))
    out = {k: v[1] for k, v in bufs.items()}
    extra, K = {}, 0
    if cons is not None:
        from grappa_amd.constraints import ConstraintBatch
        import md_cons_refs as mc
        cb = ConstraintBatch(cons, tolerance=mc.TOL)
        K = int(cb.cluster_atoms.shape[0])
        extra = dict(constraints=cb.to("cuda"), constrain_start=True)
    if cutoff is not None:
        extra["cutoff"] = cutoff
    need = int(hip.lib.grappa_md_steps_gbcut_workspace_bytes(batch.N, Cc, batch.B, rs.n_blocks(batch), K))
    wbuf = torch.full((GUARD_B + need + GUARD_B,), FILL_B, dtype=torch.uint8, device="cuda")
    ks = [k.to("cuda") for k in batch.ks]
    eqs = [None if q is None else q.to("cuda") for q in batch.eqs]
    args = (plan, x, ks, eqs, batch.n_per, False, dnb, o, torch.from_numpy(np.asarray(masses, dtype=np.float32)).to("cuda"), _dev_keys(keys),
            None if vel is None else vel.to("cuda"), out["xyz"], out["vel"], out["epot"], out["ekin"], out["steps"], out["status"])
    kw = dict(frames_xyz=out.get("frames_xyz"), frames_epot=out.get("frames_epot"), frames_ekin=out.get("frames_ekin"),
              frames_esolv=out.get("frames_esolv"), esolv=out["esolv"])
    hip.md_steps_gb(*args, atom_counts_host=batch.counts, steps_per_call=steps_per_call, workspace=wbuf[GUARD_B:GUARD_B + need],
                    gb=GBBatch(gbs).to("cuda"), solvent=solvent, **kw, **extra)
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert bool((buf[:64] == _fill_of(buf)).all()) and bool((buf[-64:] == _fill_of(buf)).all()), f"written outside {k}"
    assert bool((wbuf[:GUARD_B] == FILL_B).all()) and bool((wbuf[-GUARD_B:] == FILL_B).all()), "written outside the workspace"
    for k in GB_OUTS:
        if out[k].numel():
            assert not bool((out[k] == _fill_of(out[k])).all()), f"{k} was not written"
    return {k: v.cpu().clone() for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ 1. trajectories
TRAJ = [(n, s) for n in mgc.CASES for s in mgc.TRAJ_STEPS]


@pytest.mark.parametrize("name,n_steps", TRAJ, ids=[f"{n}-{s}steps" for n, s in TRAJ])
def test_trajectory_without_thermostat(hip, name, n_steps):
    b, m, k, v = _inputs(name)
    r64, r32s = mgc.verlet(name)[n_steps], [r[n_steps] for r in mgc.verlet32(name)]
    got = _run(hip, b, m, k, mg.gb_params(name), mgc.solvent(name), vel=v, n_steps=n_steps, dt=0.001)
    live = torch.tensor([n > 0 for n in b.counts])
    assert bool((got["steps"][live] == n_steps).all()) and not got["status"].any()
    _gate_state(name, f"{n_steps} steps, friction 0, {mg.MODEL} cut at {mgc.placed(name)[0]:.3f} A", b, got, r64, r32s)


@pytest.mark.parametrize("name", mgc.CASES)
def test_trajectory_with_thermostat(hip, name):
    """friction 50 / ps at 300 K, 1, 5 and 40 steps; the restatements consume the noise md_noise wrote for these steps"""
    b, m, k, v = _inputs(name)
    Cc = b.xyz.shape[1]
    first, total = 7, max(mgc.TRAJ_STEPS)
    z = {first + s: _noise(hip, b.counts, k, Cc, first + s, 0).double() for s in range(total)}
    opts = dict(friction=50.0, temperature=300.0, dt=0.001, first_step=first)
    r32s = mgc.realisations(name, mgc.TRAJ_STEPS, velocities=v, noise=lambda step, purpose: z[step], n_steps=total, **opts)
    for n in mgc.TRAJ_STEPS:
        got = _run(hip, b, m, k, mg.gb_params(name), mgc.solvent(name), vel=v, n_steps=n, **opts)
        assert not got["status"].any()
        _gate_state(name, f"{n} steps, friction 50, {mg.MODEL} cut", b, got, r32s[0][n][1], [r[n] for r in r32s])


def test_trajectory_under_both_cutoffs(hip):
    """the solvent under its cutoff and the nonbonded term under Cutoff(rc, 0.8 rc, 1.0): 1, 5 and 40 steps without a thermostat"""
    name = mgc.BOTH_CASE
    b, m, k, v = _inputs(name)
    for n in mgc.TRAJ_STEPS:
        r64, r32s = mgc.verlet(name, True)[n], [r[n] for r in mgc.verlet32(name, True)]
        got = _run(hip, b, m, k, mg.gb_params(name), mgc.solvent(name), vel=v, cutoff=mgc.nb_cutoff(name), n_steps=n, dt=0.001)
        assert bool((got["steps"] == n).all()) and not got["status"].any()
        _gate_state(name, f"{n} steps, friction 0, both cutoffs", b, got, r64, r32s)


def test_constrained_trajectory(hip):
    """md_steps_cons_refs' star clusters across the block border in the truncated solvent: 1, 5 and 40 steps of 2 fs"""
    import md_steps_cons_refs as msc
    import test_gpu_md_cons as tc
    batch, cons, m, keys = msc.case(mgc.CONS_CASE)
    r64, r32 = mgc.cons_verlet()
    for n in msc.TRAJ_STEPS:
        got = _run(hip, batch, m, keys, list(mg.cons_gb()), mgc.solvent(mgc.CONS_CASE), vel=msc.thermal_velocities(mgc.CONS_CASE), cons=cons,
                   n_steps=n, dt=msc.TRAJ_DT)
        live = torch.tensor([c > 0 for c in batch.counts])
        assert bool((got["steps"][live] == n).all()) and not got["status"][live].any(), (got["steps"].tolist(), got["status"].tolist())
        tc._gate_state(mgc.CONS_CASE, f"stepwise, {n} steps, friction 0, {mg.MODEL} cut", batch, got, r64["snap"][n], [r[n] for r in r32])
        tc._assert_constrained(mgc.CONS_CASE, msc.tables(mgc.CONS_CASE), batch, got["xyz"], got["vel"])


# ------------------------------------------------------------------------------------------------ 2. launches
def test_a_step_gains_no_launch_over_the_all_pairs_solvent_step(hip):
    """the header's count: move (with the boxes), force, born, pair, chain = 5, as without the cutoff, with and without the nonbonded
    cutoff beside it; with constraints 7: the box launch behind the constrained move, which the nonbonded cutoff adds as well.  init
    gains the box launch, the finish the box launch of grappa_gb_obc_fwd_cut_f32"""
    import md_steps_cons_refs as msc
    from test_gpu_md_gb import _run as run_gb
    b, m, k, v = _inputs("s65_C3")
    gbs = mg.gb_params("s65_C3")
    n = {}
    for what in ("gb", "gbcut", "both"):
        for steps in (0, 10):
            before = hip.lib.grappa_launch_count(0)
            if what == "gb":
                run_gb(hip, b, m, k, gbs, vel=v, n_steps=steps)
            else:
                _run(hip, b, m, k, gbs, mgc.solvent("s65_C3"), vel=v, n_steps=steps, cutoff=mgc.nb_cutoff("s65_C3") if what == "both" else None)
            n[(what, steps)] = hip.lib.grappa_launch_count(0) - before
    batch, cons, mc_, keys = msc.case(mgc.CONS_CASE)
    vel = msc.thermal_velocities(mgc.CONS_CASE)
    for what in ("cons_gb", "cons_gbcut", "cons_both"):
        for steps in (0, 10):
            before = hip.lib.grappa_launch_count(0)
            if what == "cons_gb":
                run_gb(hip, batch, mc_, keys, list(mg.cons_gb()), vel=vel, cons=cons, n_steps=steps, dt=msc.TRAJ_DT)
            else:
                _run(hip, batch, mc_, keys, list(mg.cons_gb()), mgc.solvent(mgc.CONS_CASE), vel=vel, cons=cons, n_steps=steps, dt=msc.TRAJ_DT,
                     cutoff=mgc.nb_cutoff(mgc.CONS_CASE) if what == "cons_both" else None)
            n[(what, steps)] = hip.lib.grappa_launch_count(0) - before
    print(f"launches: {n}")
    per_step = {w: (n[(w, 10)] - n[(w, 0)]) // 10 for w in ("gb", "gbcut", "both", "cons_gb", "cons_gbcut", "cons_both")}
    assert per_step == {"gb": 5, "gbcut": 5, "both": 5, "cons_gb": 6, "cons_gbcut": 7, "cons_both": 7}, per_step
    assert n[("gbcut", 0)] == n[("gb", 0)] + 1 + 1 and n[("cons_gbcut", 0)] == n[("cons_gb", 0)] + 1 + 1
    assert n[("both", 0)] == n[("gbcut", 0)] + 1          # (the box launch of grappa_nonbonded_fwd_cut_f32 in the finish)


# ------------------------------------------------------------------------------------------------ 3. bits
THERMO = dict(friction=20.0, temperature=300.0, init_temperature=300.0)


def test_two_runs_chunks_continuation_and_pruning_give_the_same_bits(hip):
    b, m, k, _ = _inputs(ms.MIXED)
    gbs, sv = mg.gb_params(ms.MIXED), mgc.solvent(ms.MIXED)
    a = _run(hip, b, m, k, gbs, sv, n_steps=40, save_every=8, first_step=3, **THERMO)
    keys = GB_OUTS + GB_FRAMES
    _same_bits(a, _run(hip, b, m, k, gbs, sv, n_steps=40, save_every=8, first_step=3, **THERMO), "two runs", keys=keys)
    _same_bits(a, _run(hip, b, m, k, gbs, sv, n_steps=40, save_every=8, first_step=3, steps_per_call=8, **THERMO), "8 steps per call", keys=keys)
    _same_bits(a, _run(hip, b, m, k, gbs, mgc.solvent(ms.MIXED, prune=False), n_steps=40, save_every=8, first_step=3, **THERMO),
               "prune 0 against 1", keys=keys)
    one = _run(hip, b, m, k, gbs, sv, n_steps=16, save_every=8, first_step=3, **THERMO)
    two = _run(hip, b, m, k, gbs, sv, vel=one["vel"], xyz=one["xyz"], n_steps=24, save_every=8, first_step=19, **THERMO)
    _same_bits(a, two, "40 steps against 16 + 24", keys=("xyz", "vel", "epot", "ekin", "status", "esolv"))
    for key in GB_FRAMES:
        assert torch.equal(_bits(a[key]), _bits(torch.cat([one[key], two[key]]))), key
    from test_gpu_md_gb import _run as run_gb
    full = run_gb(hip, b, m, k, gbs, n_steps=40, save_every=8, first_step=3, **THERMO)
    assert not torch.equal(_bits(a["xyz"]), _bits(full["xyz"])), "the cutoff changed nothing"


def test_pruning_does_not_change_a_bit_on_the_long_chain_or_under_both_cutoffs(hip):
    b, m, k, v = _inputs("s513_C1")
    gbs = mg.gb_params("s513_C1")
    runs = [_run(hip, b, m, k, gbs, mgc.solvent("s513_C1", prune=p), vel=v, n_steps=40, save_every=20, cutoff=c)
            for p, c in ((True, None), (False, None), (True, mgc.nb_cutoff("s513_C1", True)), (False, mgc.nb_cutoff("s513_C1", False)))]
    _same_bits(runs[0], runs[1], "prune 0 against 1", keys=GB_OUTS + GB_FRAMES)
    _same_bits(runs[2], runs[3], "prune 0 against 1, both cutoffs", keys=GB_OUTS + GB_FRAMES)


def _raw(hip, name, n_steps=6):
    """what a direct call of the C entries needs"""
    b, m, k, v = _inputs(name)
    plan, x, dnb = b.plan("cuda"), b.xyz.to("cuda"), b.nonbonded().to("cuda")
    Cc = x.shape[1]
    ks, eqs = [t.to("cuda") for t in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    from grappa_amd.backend_mm import _nb_tables_desc, _opts_struct
    o = {**md.MD_OPTS, "n_steps": n_steps, "friction": 20.0, "temperature": 300.0}
    keep = (plan, x, dnb, ks, eqs)
    d = hip._mm_desc(plan, x, ks, eqs, b.n_per, False)
    nd = _nb_tables_desc(dnb, b.N, Cc, b.B, x.device, "test")
    mo = _opts_struct(_lib.MdOpts, o, "test")
    table, n_items, n_blocks, _ = hip.nonbonded_plan(dnb.atom_molptr_host, b.N, Cc, x.device)
    gb = GBBatch(mg.gb_params(name)).to("cuda")
    return dict(b=b, o=o, Cc=Cc, d=d, nd=nd, mo=mo, table=table, n_items=n_items, n_blocks=n_blocks, gb=gb, keep=keep,
                mass=torch.from_numpy(m).to("cuda"), key=_dev_keys(k), vel=v.to("cuda"))


def test_a_null_gbcut_is_the_gb_entry_point(hip):
    """grappa_md_steps_*_gbcut_f32 with gbcut == NULL against the _gb_ entries: the same launches, the same bits, and the same refusal
    of the nonbonded cutoff beside a solvent"""
    r = _raw(hip, "s129_C3")
    lib, b, Cc = hip.lib, r["b"], r["Cc"]
    g = _lib.GbDesc(radius=r["gb"].radius.data_ptr(), scale=r["gb"].scale.data_ptr(), **ImplicitSolvent().as_opts())
    outs = {}
    for which, sfx, more in (("gb", "_gb_f32", ()), ("null_gbcut", "_gbcut_f32", (None,))):
        ws = torch.zeros(int(lib.grappa_md_steps_gb_workspace_bytes(b.N, Cc, b.B, r["n_blocks"], 0)), dtype=torch.uint8, device="cuda")
        bufs = _output_buffers(b, Cc, r["o"])
        out = {kk: vv[1] for kk, vv in bufs.items()}
        es = torch.zeros(b.B, Cc, device="cuda")
        head = (None, C.byref(r["d"]), C.byref(r["nd"]), None, C.byref(r["mo"]), None, C.byref(g)) + more
        tail = (r["table"].data_ptr(), r["n_items"], r["n_blocks"], ws.data_ptr(), ws.numel())
        before = lib.grappa_launch_count(0)
        assert getattr(lib, "grappa_md_steps_init" + sfx)(*head, r["mass"].data_ptr(), r["key"].data_ptr(), r["vel"].data_ptr(), *tail) == 0
        assert getattr(lib, "grappa_md_steps_run" + sfx)(*head, r["mass"].data_ptr(), r["key"].data_ptr(), *tail, 0, 6, None, None, None, None) == 0
        assert getattr(lib, "grappa_md_steps_finish" + sfx)(*head, *tail, *[out[kk].data_ptr() for kk in OUTS], es.data_ptr()) == 0
        torch.cuda.synchronize()
        res = {kk: vv.cpu().clone() for kk, vv in out.items()}
        res["esolv"] = es.cpu()
        outs[which] = (res, lib.grappa_launch_count(0) - before)
    _same_bits(outs["gb"][0], outs["null_gbcut"][0], "gbcut == NULL against the _gb_ entry points", keys=OUTS + ("esolv",))
    assert outs["gb"][1] == outs["null_gbcut"][1]
    cut = _lib.NbCut(cutoff=9.0, switch_distance=0.0, rf_dielectric=1.0, prune=1)
    head = (None, C.byref(r["d"]), C.byref(r["nd"]), C.byref(cut), C.byref(r["mo"]), None, C.byref(g), None)
    assert lib.grappa_md_steps_init_gbcut_f32(*head, r["mass"].data_ptr(), r["key"].data_ptr(), r["vel"].data_ptr(), *tail) == -1


def test_refusals_launch_nothing(hip):
    """gbcut without gb, a cutoff or prune the energy entry refuses, refused options of the nonbonded cutoff, a solvent without nb:
    GRAPPA_ERR_ARG and no launch; a short workspace: GRAPPA_ERR_WORKSPACE"""
    r = _raw(hip, "s65_C3", 4)
    lib, b, Cc = hip.lib, r["b"], r["Cc"]
    need = int(lib.grappa_md_steps_gbcut_workspace_bytes(b.N, Cc, b.B, r["n_blocks"], 0))
    assert need > int(lib.grappa_md_steps_gb_workspace_bytes(b.N, Cc, b.B, r["n_blocks"], 0)) and lib.grappa_md_steps_gbcut_workspace_bytes(0, Cc, 1, 1, 0) == 0
    ws = torch.full((need,), FILL_B, dtype=torch.uint8, device="cuda")
    g = _lib.GbDesc(radius=r["gb"].radius.data_ptr(), scale=r["gb"].scale.data_ptr(), **ImplicitSolvent().as_opts())
    good = _lib.GbCut(cutoff=9.0, prune=1)
    nbc_bad = _lib.NbCut(cutoff=9.0, switch_distance=9.5, rf_dielectric=1.0, prune=1)
    nan = float("nan")
    torch.cuda.synchronize()
    before = lib.grappa_launch_count(0)
    tail = (r["table"].data_ptr(), r["n_items"], r["n_blocks"], ws.data_ptr(), ws.numel())
    for nbp, cutp, gp, gc_ in ((C.byref(r["nd"]), None, None, good), (C.byref(r["nd"]), None, C.byref(g), _lib.GbCut(cutoff=0.0, prune=1)),
                               (C.byref(r["nd"]), None, C.byref(g), _lib.GbCut(cutoff=nan, prune=1)),
                               (C.byref(r["nd"]), None, C.byref(g), _lib.GbCut(cutoff=1e20, prune=1)),
                               (C.byref(r["nd"]), None, C.byref(g), _lib.GbCut(cutoff=9.0, prune=2)),
                               (C.byref(r["nd"]), C.byref(nbc_bad), C.byref(g), good), (None, None, C.byref(g), good)):
        head = (None, C.byref(r["d"]), nbp, cutp, C.byref(r["mo"]), None, gp, C.byref(gc_))
        assert lib.grappa_md_steps_init_gbcut_f32(*head, r["mass"].data_ptr(), r["key"].data_ptr(), r["vel"].data_ptr(), *tail) == -1
        assert lib.grappa_md_steps_run_gbcut_f32(*head, r["mass"].data_ptr(), r["key"].data_ptr(), *tail, 0, 4, None, None, None, None) == -1
        assert lib.grappa_md_steps_finish_gbcut_f32(*head, *tail, None, None, None, None, None, None, None) == -1
    head = (None, C.byref(r["d"]), C.byref(r["nd"]), None, C.byref(r["mo"]), None, C.byref(g), C.byref(good))
    assert lib.grappa_md_steps_init_gbcut_f32(*head, r["mass"].data_ptr(), r["key"].data_ptr(), r["vel"].data_ptr(), r["table"].data_ptr(),
                                              r["n_items"], r["n_blocks"], ws.data_ptr(), need - 1) == -3
    assert lib.grappa_launch_count(0) == before, "a refused call launched something"
    torch.cuda.synchronize()
    assert bool((ws == FILL_B).all()), "a refused call wrote to the workspace"


# ------------------------------------------------------------------------------------------------ 4. energies
@pytest.mark.parametrize("both", [False, True], ids=["solvent cutoff", "both cutoffs"])
def test_epot_is_the_energy_entries_added_in_term_order(hip, both):
    """frame and final epot = the terms of grappa_mm_energy_fwd_f32, the nonbonded entry (planned, or _cut_ under the nonbonded cutoff)
    and grappa_gb_obc_fwd_cut_f32 at the frame's coordinates, added in double in term order, bit for bit; esolv = the solvent's two"""
    name = "s129_C3"
    b, m, k, v = _inputs(name)
    gbs, sv = mg.gb_params(name), mgc.solvent(name)
    nbc = mgc.nb_cutoff(name) if both else None
    got = _run(hip, b, m, k, gbs, sv, vel=v, n_steps=10, save_every=5, dt=0.001, cutoff=nbc)
    plan = b.plan("cuda")
    ks, eqs = [t.to("cuda") for t in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    nbd, gbd = b.nonbonded().to("cuda"), GBBatch(gbs).to("cuda")
    for x, epot, esolv, what in ((got["frames_xyz"][0], got["frames_epot"][0], got["frames_esolv"][0], "frame 0"),
                                 (got["frames_xyz"][1], got["frames_epot"][1], got["frames_esolv"][1], "frame 1"),
                                 (got["xyz"], got["epot"], got["esolv"], "final")):
        xd = x.to("cuda")
        Cc = xd.shape[1]
        e, t = torch.zeros(b.B, Cc, device="cuda"), torch.zeros(4, b.B, Cc, device="cuda")
        hip.mm_energy_fwd(plan, xd, ks, eqs, b.n_per, False, e, t)
        _, _, nt = nbd.evaluate(xd, terms=True, gradient=False, **({"cutoff": nbc} if both else {}))
        gt = gbd.evaluate(nbd, xd, sv, terms=True, gradient=False)["terms"]
        tot = torch.zeros(b.B, Cc, dtype=torch.float64)
        for row in torch.cat([t, nt]).cpu():
            tot = tot + row.double()
        es = gt[0].cpu().double() + gt[1].cpu().double()
        assert torch.equal(_bits(epot), _bits((tot + es).float())), f"{what}: epot {epot.tolist()} terms' sum {(tot + es).tolist()}"
        assert torch.equal(_bits(esolv), _bits(es.float())), what


def test_a_stopped_conformation_is_skipped_and_the_others_keep_their_bits(hip):
    """a NaN coordinate ends its item at step 0 (status 2): it is neither moved nor evaluated again, and every other item's bits are
    those of the clean run"""
    b, m, k, v = _inputs(ms.MIXED)
    gbs, sv = mg.gb_params(ms.MIXED), mgc.solvent(ms.MIXED)
    clean = _run(hip, b, m, k, gbs, sv, vel=v, n_steps=6, friction=20.0, temperature=300.0)
    x = b.xyz.clone()
    bad_mol, bad_conf = 3, 1
    x[int(b.ptr[bad_mol]) + 70, bad_conf, 1] = float("nan")
    got = _run(hip, b, m, k, gbs, sv, vel=v, xyz=x, n_steps=6, friction=20.0, temperature=300.0)
    assert int(got["status"][bad_mol, bad_conf]) == 2 and int(got["steps"][bad_mol, bad_conf]) == 0
    keep = torch.ones_like(got["status"], dtype=torch.bool)
    keep[bad_mol, bad_conf] = False
    assert not got["status"][keep].any()
    for key in ("epot", "ekin", "steps", "esolv"):
        assert torch.equal(_bits(got[key][keep]), _bits(clean[key][keep])), key
    atoms = torch.ones(b.N, b.xyz.shape[1], dtype=torch.bool)
    atoms[int(b.ptr[bad_mol]):int(b.ptr[bad_mol + 1]), bad_conf] = False
    for key in ("xyz", "vel"):
        assert torch.equal(_bits(got[key][atoms]), _bits(clean[key][atoms])), key


# ------------------------------------------------------------------------------------------------ 5. the public door
def test_grappa_simulate_under_the_solvents_cutoff_with_h_bond_constraints(hip):
    """Grappa.simulate(..., implicit_solvent=ImplicitSolvent(cutoff=...), constraints="h-bonds", stepwise="auto") end to end on a molecule
    of the golden fixture: a cutoff beyond the molecule gives the trajectory of the all-pairs solvent to rounding, a short one another;
    `cutoff=` beside it is taken, beside a solvent without a cutoff refused"""
    import golden_utils as gu
    from grappa_amd import Grappa, GrappaModel, backend
    from grappa_amd.nonbonded import Cutoff, NonbondedParameters
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
        nbp = NonbondedParameters.from_bonds([(pos[int(a)], pos[int(b)]) for a, b in mol.bonds], q, np.where(z == 1, 1.0, 3.2), np.where(z == 1, 0.02, 0.1))
        low = wrapper.relax(mol, np.ascontiguousarray(mm["xyz"].transpose(1, 0, 2)[:2]), nbp)
        assert bool((low.status != 2).all())
        xyz = np.ascontiguousarray(low.xyz)
        kw = dict(n_steps=20, save_every=10, dt=0.002, seed=9, constraints="h-bonds", stepwise="auto")
        full = wrapper.simulate(mol, xyz, nbp, implicit_solvent="obc2", **kw)
        wide = wrapper.simulate(mol, xyz, nbp, implicit_solvent=ImplicitSolvent("obc2", cutoff=100.0), **kw)
        short = wrapper.simulate(mol, xyz, nbp, implicit_solvent=ImplicitSolvent("obc2", cutoff=3.0), **kw)
        both = wrapper.simulate(mol, xyz, nbp, implicit_solvent=ImplicitSolvent("obc2", cutoff=3.0), cutoff=Cutoff(3.0, 2.4, 1.0), **kw)
        for r in (wide, short, both):
            assert r.xyz.shape == xyz.shape and bool(np.isfinite(r.xyz).all()) and bool(np.isfinite(r.potential_energy).all())
            assert bool((r.steps == 20).all()) and not r.status.any() and bool((r.esolv < 0).all())
            assert r.frames_esolv.shape == r.frame_potential_energy.shape and bool(np.isfinite(r.frames_esolv).all())
        assert float(np.abs(wide.xyz - full.xyz).max()) < 1e-3 and float(np.abs(wide.esolv - full.esolv).max()) < 1e-3 * float(np.abs(full.esolv).max())
        assert not np.array_equal(short.xyz, full.xyz) and not np.array_equal(both.xyz, short.xyz)
        print(f"Grappa.simulate under the solvent's cutoff: esolv all pairs {full.esolv.tolist()}, 100 A {wide.esolv.tolist()}, 3 A {short.esolv.tolist()}")
        with pytest.raises(ValueError, match="cutoff"):
            wrapper.simulate(mol, xyz, nbp, implicit_solvent="obc2", cutoff=9.0, **kw)
        with pytest.raises(ValueError, match="cutoff"):
            wrapper.relax(mol, xyz, nbp, implicit_solvent=ImplicitSolvent("obc2", cutoff=9.0), stepwise="auto")
    finally:
        backend.set_backend(old)
