"""GPU: the stepwise dynamics in GB/SA implicit solvent (grappa_md_steps_*_gb_f32 through HipBackend.md_steps_gb) against the
restatements of tests/md_gb_refs.py: trajectories through the gate of tests/test_gpu_md.py as it stands, the launch budget, the bits
(two runs, chunk sizes, continuation, gb = NULL against the _cons_ and plain entry points), the energies against the library's own
energy entries, a NaN coordinate, one constrained case, energy conservation and the public door.  Every output and the workspace lie
between guard words."""
import ctypes as C

import numpy as np
import pytest
import torch

import md_gb_refs as mg
import md_refs as md
import md_steps_refs as ms
import relax_steps_refs as rs
from grappa_amd import _lib
from grappa_amd.solvent import GBBatch, ImplicitSolvent
from test_gpu_md import _gate_state
from test_gpu_md_steps import (FILL_B, FRAMES, GUARD_B, OUTS, _bits, _dev_keys, _fill_of, _guarded, _inputs, _noise, _output_buffers, _parameters,
                               _rows_of, _same_bits)

pytestmark = pytest.mark.gpu

GB_OUTS, GB_FRAMES = OUTS + ("esolv",), FRAMES + ("frames_esolv",)


@pytest.fixture(scope="module")
def hip():
    from grappa_amd.backend import HipBackend
    return HipBackend()


def _run(hip, batch, masses, keys, gbs, vel=None, xyz=None, steps_per_call=1000, cons=None, constrain_start=True, solvent=mg.MODEL, **opts):
    """one call of the seam in the solvent on a relax_refs.Batch -> dict of CPU tensors (GB_OUTS, and GB_FRAMES when save_every > 0);
    asserts the guards around the outputs and the workspace.  gbs: the list of GBParameters; cons: a list of Constraints or None"""
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
        extra = dict(constraints=cb.to("cuda"), constrain_start=constrain_start)
    need = int(hip.lib.grappa_md_steps_gb_workspace_bytes(batch.N, Cc, batch.B, rs.n_blocks(batch), K))
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
TRAJ = [(n, s) for n in mg.CASES for s in mg.TRAJ_STEPS]


@pytest.mark.parametrize("name,n_steps", TRAJ, ids=[f"{n}-{s}steps" for n, s in TRAJ])
def test_trajectory_without_thermostat(hip, name, n_steps):
    b, m, k, v = _inputs(name)
    r64, r32s = mg.verlet(name)[n_steps], [r[n_steps] for r in mg.verlet32(name)]
    got = _run(hip, b, m, k, mg.gb_params(name), vel=v, n_steps=n_steps, dt=0.001)
    live = torch.tensor([n > 0 for n in b.counts])
    assert bool((got["steps"][live] == n_steps).all()) and not got["status"].any()
    _gate_state(name, f"{n_steps} steps, friction 0, {mg.MODEL}", b, got, r64, r32s)


@pytest.mark.parametrize("name", mg.CASES)
def test_trajectory_with_thermostat(hip, name):
    """friction 50 / ps at 300 K, 1, 5 and 40 steps; the restatements consume the noise md_noise wrote for these steps"""
    b, m, k, v = _inputs(name)
    Cc = b.xyz.shape[1]
    first, total = 7, max(mg.TRAJ_STEPS)
    z = {first + s: _noise(hip, b.counts, k, Cc, first + s, 0).double() for s in range(total)}
    opts = dict(friction=50.0, temperature=300.0, dt=0.001, first_step=first)
    r32s = mg.realisations(name, mg.TRAJ_STEPS, velocities=v, noise=lambda step, purpose: z[step], n_steps=total, **opts)
    for n in mg.TRAJ_STEPS:
        got = _run(hip, b, m, k, mg.gb_params(name), vel=v, n_steps=n, **opts)
        assert not got["status"].any()
        _gate_state(name, f"{n} steps, friction 50, {mg.MODEL}", b, got, r32s[0][n][1], [r[n] for r in r32s])


def test_constrained_trajectory(hip):
    """md_steps_cons_refs' star clusters across the block border with the solvent added: 1, 5 and 40 steps of 2 fs without a thermostat"""
    import md_steps_cons_refs as msc
    import test_gpu_md_cons as tc
    batch, cons, m, keys = msc.case(mg.CONS_CASE)
    r64, r32 = mg.cons_verlet()
    for n in msc.TRAJ_STEPS:
        got = _run(hip, batch, m, keys, list(mg.cons_gb()), vel=msc.thermal_velocities(mg.CONS_CASE), cons=cons, n_steps=n, dt=msc.TRAJ_DT)
        live = torch.tensor([c > 0 for c in batch.counts])
        assert bool((got["steps"][live] == n).all()) and not got["status"][live].any(), (got["steps"].tolist(), got["status"].tolist())
        tc._gate_state(mg.CONS_CASE, f"stepwise, {n} steps, friction 0, {mg.MODEL}", batch, got, r64["snap"][n], [r[n] for r in r32])
        tc._assert_constrained(mg.CONS_CASE, msc.tables(mg.CONS_CASE), batch, got["xyz"], got["vel"])


# ------------------------------------------------------------------------------------------------ 2. launches
def test_a_step_is_five_launches_six_with_constraints_and_init_gains_three(hip):
    """the header's count: move, force, born, pair, chain (+ close); init gains born, pair, chain; the finish gains the four launches
    of grappa_gb_obc_fwd_f32 without a gradient (born, pair, reduce) and the one that adds the eight terms"""
    import md_steps_cons_refs as msc
    from test_gpu_md_steps import _run as run_plain
    from test_gpu_md_steps_cons import _run as run_cons
    b, m, k, v = _inputs("s65_C3")
    n = {}
    for what in ("plain", "gb"):
        for steps in (0, 10):
            before = hip.lib.grappa_launch_count(0)
            if what == "plain":
                run_plain(hip, b, m, k, vel=v, n_steps=steps)
            else:
                _run(hip, b, m, k, mg.gb_params("s65_C3"), vel=v, n_steps=steps)
            n[(what, steps)] = hip.lib.grappa_launch_count(0) - before
    batch, cons, mc_, keys = msc.case(mg.CONS_CASE)
    vel = msc.thermal_velocities(mg.CONS_CASE)
    for what in ("cons", "cons_gb"):
        for steps in (0, 10):
            before = hip.lib.grappa_launch_count(0)
            if what == "cons":
                run_cons(hip, batch, cons, mc_, keys, vel=vel, n_steps=steps, dt=msc.TRAJ_DT)
            else:
                _run(hip, batch, mc_, keys, list(mg.cons_gb()), vel=vel, cons=cons, n_steps=steps, dt=msc.TRAJ_DT)
            n[(what, steps)] = hip.lib.grappa_launch_count(0) - before
    print(f"launches: {n}")
    assert n[("plain", 10)] - n[("plain", 0)] == 20 and n[("gb", 10)] - n[("gb", 0)] == 50
    assert n[("cons", 10)] - n[("cons", 0)] == 30 and n[("cons_gb", 10)] - n[("cons_gb", 0)] == 60
    assert n[("gb", 0)] == n[("plain", 0)] + 3 + 3 + 1 and n[("cons_gb", 0)] == n[("cons", 0)] + 3 + 3 + 1


# ------------------------------------------------------------------------------------------------ 3. bits
THERMO = dict(friction=20.0, temperature=300.0, init_temperature=300.0)


def test_two_runs_chunks_and_continuation_give_the_same_bits(hip):
    b, m, k, _ = _inputs(ms.MIXED)
    gbs = mg.gb_params(ms.MIXED)
    a = _run(hip, b, m, k, gbs, n_steps=40, save_every=8, first_step=3, **THERMO)
    _same_bits(a, _run(hip, b, m, k, gbs, n_steps=40, save_every=8, first_step=3, **THERMO), "two runs", keys=GB_OUTS + GB_FRAMES)
    _same_bits(a, _run(hip, b, m, k, gbs, n_steps=40, save_every=8, first_step=3, steps_per_call=8, **THERMO), "8 steps per call",
               keys=GB_OUTS + GB_FRAMES)
    one = _run(hip, b, m, k, gbs, n_steps=16, save_every=8, first_step=3, **THERMO)
    two = _run(hip, b, m, k, gbs, vel=one["vel"], xyz=one["xyz"], n_steps=24, save_every=8, first_step=19, **THERMO)
    _same_bits(a, two, "40 steps against 16 + 24", keys=("xyz", "vel", "epot", "ekin", "status", "esolv"))
    for key in GB_FRAMES:
        assert torch.equal(_bits(a[key]), _bits(torch.cat([one[key], two[key]]))), key
    from test_gpu_md_steps import _run as run_plain
    plain = run_plain(hip, b, m, k, n_steps=40, save_every=8, first_step=3, **THERMO)
    assert not torch.equal(_bits(a["xyz"]), _bits(plain["xyz"])), "the solvent changed nothing"


def test_a_molecule_alone_and_inside_the_mixed_batch_gives_the_same_bits(hip):
    b, m, k, v = _inputs(ms.MIXED)
    gbs = mg.gb_params(ms.MIXED)
    whole = _run(hip, b, m, k, gbs, vel=v, n_steps=12, save_every=6, friction=20.0, temperature=300.0)
    for i in (3, 5):
        p0, p1 = int(b.ptr[i]), int(b.ptr[i + 1])
        alone = _run(hip, rs.rr.Batch([b.mols[i]]), m[p0:p1], k[i:i + 1], [gbs[i]], vel=v[p0:p1], n_steps=12, save_every=6, friction=20.0, temperature=300.0)
        rows = _rows_of(whole, b, i)
        for key in ("xyz", "vel"):
            assert torch.equal(_bits(alone[key]), _bits(rows[key])), (i, key)
        for key in ("epot", "ekin"):
            assert torch.equal(_bits(alone[key][0]), _bits(rows[key])), (i, key)
        assert torch.equal(_bits(alone["esolv"][0]), _bits(whole["esolv"][i]))


def test_a_null_gb_is_the_cons_and_the_plain_entry_point(hip):
    """grappa_md_steps_*_gb_f32 with gb == NULL against the _cons_ entries (cons == NULL) and the plain ones: the same launches, the
    same bits"""
    b, m, k, v = _inputs("s129_C3")
    lib = hip.lib
    o = {**md.MD_OPTS, "n_steps": 6, "friction": 20.0, "temperature": 300.0}
    plan, x, dnb = b.plan("cuda"), b.xyz.to("cuda"), b.nonbonded().to("cuda")
    Cc = x.shape[1]
    ks, eqs = [t.to("cuda") for t in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    d = hip._mm_desc(plan, x, ks, eqs, b.n_per, False)
    from grappa_amd.backend_mm import _nb_tables_desc, _opts_struct
    nd = _nb_tables_desc(dnb, b.N, Cc, b.B, x.device, "test")
    mo = _opts_struct(_lib.MdOpts, o, "test")
    table, n_items, n_blocks, _ = hip.nonbonded_plan(dnb.atom_molptr_host, b.N, Cc, x.device)
    mass, key, vel = torch.from_numpy(m).to("cuda"), _dev_keys(k), v.to("cuda")
    outs = {}
    for which, mid, sfx, more in (("plain", (), "_f32", ()), ("null_cons", (None,), "_cons_f32", ()), ("null_gb", (None,), "_gb_f32", (None,))):
        ws = torch.zeros(int(lib.grappa_md_steps_workspace_bytes(b.N, Cc, b.B, n_blocks)), dtype=torch.uint8, device="cuda")
        bufs = _output_buffers(b, Cc, o)
        out = {kk: vv[1] for kk, vv in bufs.items()}
        # (stream, mm, nb[, cut], opts[, cons[, gb]])
        head = (None, C.byref(d), C.byref(nd)) + mid + (C.byref(mo),) + ((None,) if which != "plain" else ()) + ((None,) if which == "null_gb" else ())
        tail = (table.data_ptr(), n_items, n_blocks, ws.data_ptr(), ws.numel())
        before = lib.grappa_launch_count(0)
        assert getattr(lib, "grappa_md_steps_init" + sfx)(*head, mass.data_ptr(), key.data_ptr(), vel.data_ptr(), *tail) == 0
        assert getattr(lib, "grappa_md_steps_run" + sfx)(*head, mass.data_ptr(), key.data_ptr(), *tail, 0, 6, None, None, None, *more) == 0
        assert getattr(lib, "grappa_md_steps_finish" + sfx)(*head, *tail, *[out[kk].data_ptr() for kk in OUTS], *more) == 0
        torch.cuda.synchronize()
        outs[which] = ({kk: vv.cpu().clone() for kk, vv in out.items()}, lib.grappa_launch_count(0) - before)
    for which in ("null_cons", "null_gb"):
        _same_bits(outs["plain"][0], outs[which][0], f"{which} against the plain entry points")
        assert outs["plain"][1] == outs[which][1]


def test_refusals_launch_nothing(hip):
    """a cutoff together with the solvent, a solvent without nb, refused options, NULL radius: GRAPPA_ERR_ARG and no launch"""
    b, m, k, v = _inputs("s65_C3")
    lib = hip.lib
    plan, x, dnb = b.plan("cuda"), b.xyz.to("cuda"), b.nonbonded().to("cuda")
    Cc = x.shape[1]
    ks, eqs = [t.to("cuda") for t in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    d = hip._mm_desc(plan, x, ks, eqs, b.n_per, False)
    from grappa_amd.backend_mm import _nb_tables_desc, _opts_struct
    nd = _nb_tables_desc(dnb, b.N, Cc, b.B, x.device, "test")
    mo = _opts_struct(_lib.MdOpts, {**md.MD_OPTS, "n_steps": 4}, "test")
    table, n_items, n_blocks, _ = hip.nonbonded_plan(dnb.atom_molptr_host, b.N, Cc, x.device)
    gb = GBBatch(mg.gb_params("s65_C3")).to("cuda")
    need = int(lib.grappa_md_steps_gb_workspace_bytes(b.N, Cc, b.B, n_blocks, 0))
    assert need > int(lib.grappa_md_steps_workspace_bytes(b.N, Cc, b.B, n_blocks)) + 4 * 6 * b.N * Cc and lib.grappa_md_steps_gb_workspace_bytes(0, Cc, 1, 1, 0) == 0
    ws = torch.full((need,), FILL_B, dtype=torch.uint8, device="cuda")
    mass, key, vel = torch.from_numpy(m).to("cuda"), _dev_keys(k), v.to("cuda")
    good = ImplicitSolvent().as_opts()
    desc = lambda **over: _lib.GbDesc(radius=gb.radius.data_ptr(), scale=gb.scale.data_ptr(), **{**good, **over})      # noqa: E731
    cut = _lib.NbCut(cutoff=9.0, switch_distance=0.0, rf_dielectric=78.3, prune=1)
    no_r = desc()
    no_r.radius = None
    torch.cuda.synchronize()
    before = lib.grappa_launch_count(0)
    for nbp, cutp, g in ((C.byref(nd), C.byref(cut), desc()), (None, None, desc()), (C.byref(nd), None, desc(eps_out=0.0)),
                         (C.byref(nd), None, desc(alpha=float("nan"))), (C.byref(nd), None, no_r)):
        head = (None, C.byref(d), nbp, cutp, C.byref(mo), None, C.byref(g))
        tail = (table.data_ptr(), n_items, n_blocks, ws.data_ptr(), ws.numel())
        assert lib.grappa_md_steps_init_gb_f32(*head, mass.data_ptr(), key.data_ptr(), vel.data_ptr(), *tail) == -1
        assert lib.grappa_md_steps_run_gb_f32(*head, mass.data_ptr(), key.data_ptr(), *tail, 0, 4, None, None, None, None) == -1
        assert lib.grappa_md_steps_finish_gb_f32(*head, *tail, None, None, None, None, None, None, None) == -1
    head = (None, C.byref(d), C.byref(nd), None, C.byref(mo), None, C.byref(desc()))
    assert lib.grappa_md_steps_init_gb_f32(*head, mass.data_ptr(), key.data_ptr(), vel.data_ptr(), table.data_ptr(), n_items, n_blocks, ws.data_ptr(),
                                           need - 1) == -3
    assert lib.grappa_launch_count(0) == before, "a refused call launched something"
    torch.cuda.synchronize()
    assert bool((ws == FILL_B).all()), "a refused call wrote to the workspace"


# ------------------------------------------------------------------------------------------------ 4. energies
def test_epot_is_the_energy_entries_added_in_term_order(hip):
    """frame and final epot = the terms of grappa_mm_energy_fwd_f32, grappa_nonbonded_fwd_planned_f32 and grappa_gb_obc_fwd_f32 at the
    frame's coordinates, added in double in term order, bit for bit; esolv = the solvent's two terms"""
    b, m, k, v = _inputs("s129_C3")
    gbs = mg.gb_params("s129_C3")
    got = _run(hip, b, m, k, gbs, vel=v, n_steps=10, save_every=5, dt=0.001)
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
        _, _, nt = nbd.evaluate(xd, terms=True, gradient=False)
        gt = gbd.evaluate(nbd, xd, mg.MODEL, terms=True, gradient=False)["terms"]
        tot = torch.zeros(b.B, Cc, dtype=torch.float64)
        for row in torch.cat([t, nt]).cpu():
            tot = tot + row.double()
        es = gt[0].cpu().double() + gt[1].cpu().double()
        assert torch.equal(_bits(epot), _bits((tot + es).float())), f"{what}: epot {epot.tolist()} terms' sum {(tot + es).tolist()}"
        assert torch.equal(_bits(esolv), _bits(es.float())), what


def test_a_nan_coordinate_ends_its_item_and_leaves_the_others(hip):
    b, m, k, v = _inputs(ms.MIXED)
    gbs = mg.gb_params(ms.MIXED)
    clean = _run(hip, b, m, k, gbs, vel=v, n_steps=6, friction=20.0, temperature=300.0)
    x = b.xyz.clone()
    bad_mol, bad_conf = 3, 1
    x[int(b.ptr[bad_mol]) + 70, bad_conf, 1] = float("nan")
    got = _run(hip, b, m, k, gbs, vel=v, xyz=x, n_steps=6, friction=20.0, temperature=300.0)
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


def test_energy_conservation(hip):
    """NVE (md_steps_refs.NVE: 400 steps of 0.5 fs) on s2_130_9_C3 from its relaxed coordinates in the solvent:
    D_gpu <= 2 max(D_f32, D_f64) of the restatements in the same solvent (the factor of tests/test_gpu_md_steps.py)"""
    b, m, k, v = ms.nve_batch(), ms.masses(ms.NVE_CASE), ms.keys(ms.NVE_CASE), ms.thermal_velocities(ms.NVE_CASE)
    gbs = mg.gb_params("nve")
    start = _run(hip, b, m, k, gbs, vel=v, n_steps=0)
    got = _run(hip, b, m, k, gbs, vel=v, **ms.NVE)
    assert not got["status"].any() and bool((got["steps"] == ms.NVE["n_steps"]).all())
    d_gpu = md.drift(start["epot"].double() + start["ekin"].double(), got["frames_epot"].double() + got["frames_ekin"].double())
    d32, d64 = mg.nve_drift(torch.float32), mg.nve_drift(torch.float64)
    print(f"energy conservation, {mg.MODEL}: D_gpu {d_gpu:.4f}, D_f32 {d32:.4f}, D_f64 {d64:.4f} kcal/mol, D_gpu / max = {d_gpu / max(d32, d64):.3f}")
    assert d_gpu <= 2 * max(d32, d64)


# ------------------------------------------------------------------------------------------------ 5. the public door
def test_simulate_graph_against_the_seam(hip):
    from grappa_amd import backend
    from grappa_amd.dynamics import simulate_graph
    from grappa_amd.nonbonded import NonbondedBatch
    from grappa_amd.relax import graph_from_parameters
    old = backend._BACKEND
    backend.set_backend(hip)
    try:
        b, m, k, _ = _inputs("s65_C3")
        mol, gbs = b.mols[0], mg.gb_params("s65_C3")
        g = graph_from_parameters(_parameters(mol), mol["xyz"].transpose(1, 0, 2)).to("cuda")
        nb = NonbondedBatch([mol["nb"]]).to("cuda")
        opts = dict(n_steps=20, save_every=5, friction=20.0, temperature=300.0)
        runs = [simulate_graph(g, m, nb, keys=k, first_step=2, stepwise="auto", steps_per_launch=s, implicit_solvent="obc2",
                               gb=GBBatch(gbs).to("cuda"), **opts) for s in (10000, 7)]
        seam = _run(hip, b, m, k, gbs, first_step=2, init_temperature=300.0, **opts)
        for r in runs:
            assert bool((r.steps == 20).all()) and not r.status.any() and r.frames.shape == (4, 65, 3, 3)
            for f, key in (("xyz", "xyz"), ("velocities", "vel"), ("potential_energy", "epot"), ("kinetic_energy", "ekin"), ("frames", "frames_xyz"),
                           ("frame_potential_energy", "frames_epot"), ("frame_kinetic_energy", "frames_ekin"), ("esolv", "esolv"),
                           ("frames_esolv", "frames_esolv")):
                assert torch.equal(_bits(getattr(r, f).cpu()), _bits(seam[key])), f
    finally:
        backend.set_backend(old)


def test_grappa_simulate_in_implicit_solvent_with_h_bond_constraints(hip):
    """Grappa.simulate(..., implicit_solvent="obc2", constraints="h-bonds", stepwise="auto") end to end on a molecule of the golden
    fixture with its own partial charges: finite output, every item ran, esolv < 0, and the radii come from the molecule's elements"""
    import golden_utils as gu
    from grappa_amd import Grappa, GrappaModel, backend
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
        assert float(np.abs(q).max()) > 0.05, "the fixture molecule has no charges to solvate"
        pos = {int(a): i for i, a in enumerate(mol.atoms)}
        nbp = NonbondedParameters.from_bonds([(pos[int(a)], pos[int(b)]) for a, b in mol.bonds], q, np.where(z == 1, 1.0, 3.2), np.where(z == 1, 0.02, 0.1))
        low = wrapper.relax(mol, np.ascontiguousarray(mm["xyz"].transpose(1, 0, 2)[:2]), nbp)
        assert bool((low.status != 2).all())
        xyz = np.ascontiguousarray(low.xyz)
        kw = dict(n_steps=20, save_every=10, dt=0.002, seed=9, constraints="h-bonds", stepwise="auto")
        r = wrapper.simulate(mol, xyz, nbp, implicit_solvent="obc2", **kw)
        assert r.xyz.shape == xyz.shape and bool(np.isfinite(r.xyz).all()) and bool(np.isfinite(r.potential_energy).all())
        assert bool((r.steps == 20).all()) and not r.status.any()
        assert r.esolv.shape == r.potential_energy.shape and bool((r.esolv < 0).all())
        assert r.frames_esolv.shape == r.frame_potential_energy.shape and bool(np.isfinite(r.frames_esolv).all())
        print(f"Grappa.simulate in obc2 with h-bonds: esolv {r.esolv.tolist()} of epot {r.potential_energy.tolist()} kcal/mol")
        vac = wrapper.simulate(mol, xyz, nbp, **kw)
        assert vac.esolv is None and vac.frames_esolv is None and not np.array_equal(vac.xyz, r.xyz)
    finally:
        backend.set_backend(old)
