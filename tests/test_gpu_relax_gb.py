"""GPU: the stepwise FIRE minimiser in GB/SA implicit solvent (grappa_relax_steps_*_gb_f32 through HipBackend.relax_steps_gb and
grappa_amd/relax.py) against the restatements of tests/relax_gb_refs.py: step zero through the gates of tests/relax_refs.py and
tests/gb_refs.py, trajectories through the gate of tests/test_gpu_relax_steps.py as it stands, the bits (two runs, chunk sizes, a
molecule alone and in a batch, gb = NULL against the plain and the _cut_ entry points), the launch counts, convergence below the
vacuum minimum, the seam to the dynamics, a NaN coordinate, a radius below the offset, the refusals and the public doors.  Every output
and the workspace lie between guard words."""
import ctypes as C

import numpy as np
import pytest
import torch

import gb_refs as gr
import kernel_refs as kr
import relax_gb_refs as rg
import relax_refs as rr
import relax_steps_refs as rs
from grappa_amd import _lib
from grappa_amd.relax import RELAX_DEFAULTS
from grappa_amd.solvent import GBBatch, ImplicitSolvent
from test_gpu_relax_steps import FILL, FILL_B, FILL_I, GUARD_B, _guarded, _rows_of, _same_bits, _single, _traj_gate
from test_gpu_relax_steps import _run as run_vacuum

pytestmark = pytest.mark.gpu

OUTS = ("xyz", "energy", "gmax", "steps", "status", "terms", "grad", "esolv")


@pytest.fixture(scope="module")
def hip():
    from grappa_amd.backend import HipBackend
    return HipBackend()


def _shapes(N, Cc, B, rows=8):
    return {"xyz": ((N, Cc, 3), torch.float32), "energy": ((B, Cc), torch.float32), "gmax": ((B, Cc), torch.float32),
            "steps": ((B, Cc), torch.int32), "status": ((B, Cc), torch.int32), "terms": ((rows, B, Cc), torch.float32),
            "grad": ((N, Cc, 3), torch.float32), "esolv": ((B, Cc), torch.float32)}


def _fill_of(buf):
    return FILL_I if buf.dtype == torch.int32 else FILL


def _run(hip, batch, gbs, check_every=32, xyz=None, solvent=rg.MODEL, gb=None, **opts):
    """one call of the seam in the solvent on a relax_refs.Batch -> dict of CPU tensors (OUTS; terms (8,B,C)); asserts the guards around
    the outputs and the workspace.  gbs: the list of GBParameters; gb: a GBBatch on the device to use instead"""
    plan, dnb = batch.plan("cuda"), batch.nonbonded().to("cuda")
    x = (batch.xyz if xyz is None else xyz).to("cuda")
    N, Cc, B = batch.N, x.shape[1], batch.B
    bufs = {k: _guarded(*v) for k, v in _shapes(N, Cc, B).items()}
    o = {k: v[1] for k, v in bufs.items()}
    need = int(hip.lib.grappa_relax_steps_gb_workspace_bytes(N, Cc, B, rs.n_blocks(batch)))
    wbuf = torch.full((GUARD_B + need + GUARD_B,), FILL_B, dtype=torch.uint8, device="cuda")
    ks, eqs = [k.to("cuda") for k in batch.ks], [None if q is None else q.to("cuda") for q in batch.eqs]
    try:
        hip.relax_steps_gb(plan, x, ks, eqs, batch.n_per, False, dnb, {**RELAX_DEFAULTS, **opts}, o["xyz"], o["energy"], o["gmax"], o["steps"],
                           o["status"], term_energy=o["terms"], grad=o["grad"], atom_counts_host=batch.counts, check_every=check_every,
                           workspace=wbuf[GUARD_B:GUARD_B + need], gb=GBBatch(gbs).to("cuda") if gb is None else gb, solvent=solvent, esolv=o["esolv"])
    finally:
        torch.cuda.synchronize()
        for k, (buf, _) in bufs.items():
            assert bool((buf[:64] == _fill_of(buf)).all()) and bool((buf[-64:] == _fill_of(buf)).all()), f"written outside {k}"
        assert bool((wbuf[:GUARD_B] == FILL_B).all()) and bool((wbuf[-GUARD_B:] == FILL_B).all()), "written outside the workspace"
    for k, (buf, view) in bufs.items():
        if view.numel():
            assert not bool((view == _fill_of(buf)).all()), f"{k} was not written"
    return {k: v.cpu().clone() for k, v in o.items()}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _entries(hip, b, x):
    """the eight terms at x by the library's own energy entries -> (8, B, C) on the CPU"""
    plan, xd = b.plan("cuda"), x.to("cuda")
    ks, eqs = [k.to("cuda") for k in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    Cc = xd.shape[1]
    e, t = torch.zeros(b.B, Cc, device="cuda"), torch.zeros(4, b.B, Cc, device="cuda")
    hip.mm_energy_fwd(plan, xd, ks, eqs, b.n_per, False, e, t)
    nbd = b.nonbonded().to("cuda")
    _, _, nt = nbd.evaluate(xd, terms=True, gradient=False)
    return torch.cat([t, nt]).cpu(), nbd


# ------------------------------------------------------------------------------------------------ 1. step zero
@pytest.mark.parametrize("name", rg.TRAJ_CASES)
def test_forces_at_step_zero(hip, name):
    """max_steps = 0: the coordinates come back bit for bit; energy, the six terms and the total gradient pass the calibrated gate
    against the float64 solvent restatement; esolv and the solvent's two terms have the bits of grappa_gb_obc_fwd_f32 there (and pass
    gb_refs' gate), the six terms those of the existing energy entries"""
    b, gbs = rg.case(name), rg.gb_params(name)
    r64, r32 = rg.forces_of(name, torch.float64), rg.forces_of(name, torch.float32)
    got = _run(hip, b, gbs, max_steps=0, tolerance=0.0)
    assert torch.equal(_bits(got["xyz"]), _bits(b.xyz)), "xyz_out differs from the input"
    one = _single(b)[:, None].expand_as(got["status"])
    assert bool((got["steps"] == 0).all()) and torch.equal(got["status"], one.int())          # (a single atom: gmax = 0 <= 0, converged)
    rr.gate_forces(got["energy"], got["terms"][:6], got["grad"], r64, r32, name)
    gr.gate_all({"energy": got["esolv"], "terms": got["terms"][6:]}, r64["solv"], r32["solv"], f"{name}: solvent")
    want_gmax = torch.stack([got["grad"][int(b.ptr[k]):int(b.ptr[k + 1])].double().norm(dim=-1).max(0).values for k in range(b.B)])
    assert bool(((got["gmax"].double() - want_gmax).abs() <= 4 * kr.U32 * want_gmax).all()), "gmax is not the largest gradient norm"
    six, nbd = _entries(hip, b, b.xyz)
    assert torch.equal(_bits(got["terms"][:6]), _bits(six)), "the six terms are not the bits of the energy kernels"
    gt = GBBatch(gbs).to("cuda").evaluate(nbd, b.xyz.to("cuda"), rg.MODEL, terms=True, gradient=False)["terms"].cpu()
    assert torch.equal(_bits(got["terms"][6:]), _bits(gt)), "the solvent's terms are not the bits of grappa_gb_obc_fwd_f32"
    tot = torch.zeros(b.B, b.xyz.shape[1], dtype=torch.float64)
    for row in six:
        tot = tot + row.double()
    es = gt[0].double() + gt[1].double()
    assert torch.equal(_bits(got["esolv"]), _bits(es.float())) and torch.equal(_bits(got["energy"]), _bits((tot + es).float()))


# ------------------------------------------------------------------------------------------------ 2. trajectories
TRAJ = [(n, s) for n in rg.TRAJ_CASES for s in rr.TRAJ_STEPS]


@pytest.mark.parametrize("name,max_steps", TRAJ, ids=[f"{n}-{s}steps" for n, s in TRAJ])
def test_trajectory(hip, name, max_steps):
    """tolerance = 0: every item runs exactly max_steps steps; a conformation that keeps the branch margin ends within 4 x the fp32
    restatement's distance to float64 + 2^-20 A (test_gpu_relax_steps._traj_gate as it stands)"""
    b = rg.case(name)
    x64, x32 = rg.trajectory(name, torch.float64)["snap"][max_steps], rg.trajectory(name, torch.float32)["snap"][max_steps]
    ok = rg.margin_ok(name, max_steps)
    got = _run(hip, b, rg.gb_params(name), max_steps=max_steps, tolerance=0.0)
    one = _single(b)[:, None].expand_as(got["status"])
    assert torch.equal(got["steps"], torch.where(one, 0, max_steps).int()) and torch.equal(got["status"], one.int())
    _traj_gate(name, b, got["xyz"], x64, x32, ok, f"{max_steps} steps, {rg.MODEL}")


# ------------------------------------------------------------------------------------------------ 3. bits
def test_two_runs_and_every_chunk_size_give_the_same_bits(hip):
    b, gbs = rg.case(rg.MIXED), rg.gb_params(rg.MIXED)
    a = _run(hip, b, gbs, max_steps=40, tolerance=0.0)
    _same_bits(a, _run(hip, b, gbs, max_steps=40, tolerance=0.0), "two runs", keys=OUTS)
    for ce in (1, 7, 64):
        _same_bits(a, _run(hip, b, gbs, check_every=ce, max_steps=40, tolerance=0.0), f"check_every = {ce}", keys=OUTS)
    plain = run_vacuum(hip, b, max_steps=40, tolerance=0.0)
    assert not torch.equal(_bits(a["xyz"]), _bits(plain["xyz"])), "the solvent changed nothing"


def test_a_molecule_alone_and_inside_the_mixed_batch_gives_the_same_bits(hip):
    b, gbs = rg.case(rg.MIXED), rg.gb_params(rg.MIXED)          # sizes 1, 2, 17, 130, 5, 64
    whole = _run(hip, b, gbs, max_steps=60)
    for i in (2, 3, 5):
        sub = b.subset([i])
        alone = _run(hip, sub, [gbs[i]], max_steps=60)
        _same_bits(_rows_of(whole, b, i), _rows_of(alone, sub, 0), f"molecule {i} alone and in the batch")
        assert torch.equal(_bits(whole["esolv"][i]), _bits(alone["esolv"][0])), i


def _raw(hip, b, gbs=None, cut=None, sfx="_gb_f32", steps=6, **opts):
    """init, one run of `steps` steps and finish through the C entry points themselves -> (outputs on the CPU, [launches of init, of
    the run, of finish]); sfx "_f32": the plain calls, "_cut_f32": with `cut`, "_gb_f32": with `cut` and the solvent of gbs (None: NULL)"""
    from grappa_amd.backend_mm import _nb_tables_desc, _opts_struct
    lib = hip.lib
    plan, x, dnb = b.plan("cuda"), b.xyz.to("cuda"), b.nonbonded().to("cuda")
    N, Cc, B = b.N, x.shape[1], b.B
    ks, eqs = [t.to("cuda") for t in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    d = hip._mm_desc(plan, x, ks, eqs, b.n_per, False)
    nd = _nb_tables_desc(dnb, N, Cc, B, x.device, "test")
    o = _opts_struct(_lib.RelaxOpts, {**RELAX_DEFAULTS, **opts}, "test")
    table, n_items, n_blocks, _ = hip.nonbonded_plan(dnb.atom_molptr_host, N, Cc, x.device)
    gbd = None
    if gbs is not None:
        gb = GBBatch(gbs).to("cuda")
        gbd = _lib.GbDesc(radius=gb.radius.data_ptr(), scale=gb.scale.data_ptr(), **ImplicitSolvent().as_opts())
    size = lib.grappa_relax_steps_gb_workspace_bytes if gbd is not None else (lib.grappa_relax_steps_cut_workspace_bytes if cut is not None
                                                                                else lib.grappa_relax_steps_workspace_bytes)
    ws = torch.zeros(int(size(N, Cc, B, n_blocks)), dtype=torch.uint8, device="cuda")
    bufs = {k: _guarded(*v) for k, v in _shapes(N, Cc, B, 8 if gbd is not None else 6).items()}
    out = {k: v[1] for k, v in bufs.items()}
    cutp = C.byref(cut) if cut is not None else None
    mid = {"_f32": (), "_cut_f32": (cutp,), "_gb_f32": (cutp, C.byref(gbd) if gbd is not None else None)}[sfx]
    head = (None, C.byref(d), C.byref(nd)) + mid + (C.byref(o),)
    tail = (table.data_ptr(), n_items, n_blocks, ws.data_ptr(), ws.numel())
    nrun = torch.zeros(1, dtype=torch.int32, device="cuda")
    n = [lib.grappa_launch_count(0)]
    assert getattr(lib, "grappa_relax_steps_init" + sfx)(*head, *tail, nrun.data_ptr()) == 0
    n.append(lib.grappa_launch_count(0))
    assert getattr(lib, "grappa_relax_steps_run" + sfx)(*head, *tail, steps, nrun.data_ptr()) == 0
    n.append(lib.grappa_launch_count(0))
    more = (out["esolv"].data_ptr(),) if sfx == "_gb_f32" else ()
    assert getattr(lib, "grappa_relax_steps_finish" + sfx)(*head, *tail, *[out[k].data_ptr() for k in ("xyz", "energy", "terms", "grad", "gmax", "steps",
                                                                                                      "status")], *more) == 0
    n.append(lib.grappa_launch_count(0))
    torch.cuda.synchronize()
    return {k: v.cpu().clone() for k, v in out.items()}, [n[k + 1] - n[k] for k in range(3)]


def test_a_null_gb_is_the_plain_and_the_cut_entry_point(hip):
    """grappa_relax_steps_*_gb_f32 with gb == NULL against the plain entries and, with cut, the _cut_ entries: the same launches, the
    same bits (esolv is then not written)"""
    b = rg.case("s129_C3")
    keys = ("xyz", "energy", "gmax", "steps", "status", "terms", "grad")
    plain, null = _raw(hip, b, sfx="_f32", tolerance=0.0), _raw(hip, b, sfx="_gb_f32", tolerance=0.0)
    _same_bits(plain[0], null[0], "gb == NULL against the plain entry points", keys=keys)
    assert plain[1] == null[1] == [2, 24, 5] and bool((null[0]["esolv"] == FILL).all())
    cut = _lib.NbCut(cutoff=9.0, switch_distance=7.2, rf_dielectric=78.3, prune=1)
    cplain, cnull = _raw(hip, b, cut=cut, sfx="_cut_f32", tolerance=0.0), _raw(hip, b, cut=cut, sfx="_gb_f32", tolerance=0.0)
    _same_bits(cplain[0], cnull[0], "gb == NULL with a cut against the _cut_ entry points", keys=keys)
    assert cplain[1] == cnull[1] and cplain[1][1] == 24 and bool((cnull[0]["esolv"] == FILL).all())
    assert not torch.equal(_bits(plain[0]["xyz"]), _bits(cplain[0]["xyz"]))


# ------------------------------------------------------------------------------------------------ 4. launches
@pytest.mark.parametrize("name", ["s9_65_C17", "s513_C1"])
def test_launch_counts(hip, name):
    """the header's counts: init 5 (init, force, born, pair, chain), a step 7 (decide, vel, move, force, born, pair, chain), finish 9
    (decide, the bonded energy, the nonbonded pairs and their reduction, born, pair and reduction of grappa_gb_obc_fwd_f32, the copy
    kernel, the launch that adds the eight terms) -- whatever the shape; without solvent 2, 4 and 5"""
    b = rg.case(name)
    _, n = _raw(hip, b, rg.gb_params(name), steps=3, tolerance=0.0)
    _, m = _raw(hip, b, sfx="_f32", steps=3, tolerance=0.0)
    print(f"{name}: launches of init, three steps, finish: {n} in the solvent, {m} without")
    assert n == [5, 21, 9] and m == [2, 12, 5]


# ------------------------------------------------------------------------------------------------ 5. convergence
@pytest.mark.parametrize("name", rg.CONV_CASES)
def test_convergence_with_the_defaults(hip, name):
    """the assertions of test_gpu_relax_steps.test_convergence_with_the_defaults with the solvent restatement's forces, every item
    converged; and the reason the feature exists: the energy reached is below the start's and, on the molecules of
    relax_gb_refs.ORDERED, below the solvent energy at the coordinates the vacuum minimiser hands over"""
    b, gbs = rg.case(name), rg.gb_params(name)
    got = _run(hip, b, gbs, max_steps=rg.CONV_MAX_STEPS)
    print(f"{name}: steps {got['steps'].flatten().tolist()} status {got['status'].flatten().tolist()}")
    assert bool((got["status"] == 1).all()), got["status"].tolist()
    assert bool((got["steps"] <= rg.CONV_MAX_STEPS).all())
    r64, r32 = rg.forces(name, b, got["xyz"], torch.float64, scales=True), rg.forces(name, b, got["xyz"], torch.float32)
    per_mol = lambda t: torch.stack([t[int(b.ptr[k]):int(b.ptr[k + 1])].max(0).values for k in range(b.B)])      # noqa: E731
    gmax64, gmax32 = per_mol(r64["G"].norm(dim=-1)), per_mol(r32["G"].double().norm(dim=-1))
    floor = rr.C_GATE * kr.U32 * per_mol(r64["abs_f"])
    cal = torch.maximum(per_mol((r32["G"].double() - r64["G"]).norm(dim=-1)), (gmax32 - gmax64).abs())
    bound = floor + 2 * cal + 2 * kr.U32 * per_mol(rr.bond_rounding(b, got["xyz"]))
    fmt = lambda t: [f"{v:.2e}" for v in t.flatten().tolist()]      # noqa: E731
    print(f"  gmax gpu - f64 {fmt(got['gmax'].double() - gmax64)}\n  f64 gmax - tolerance {fmt(gmax64 - RELAX_DEFAULTS['tolerance'])}\n  bound {fmt(bound)}")
    assert bool((gmax64 <= RELAX_DEFAULTS["tolerance"] + bound).all()), "the float64 gradient at xyz_out is above the tolerance"
    rr.gate_forces(got["energy"], None, None, r64, r32, f"{name} at xyz_out")
    assert bool(((got["gmax"].double() - gmax64).abs() <= bound).all()), "gmax at xyz_out"
    e0 = rg.forces_of(name, torch.float64)["E"]
    vac = run_vacuum(hip, b, max_steps=rg.CONV_MAX_STEPS)
    ev = rg.forces(name, b, vac["xyz"], torch.float64)["E"]
    print(f"  solvent energy: start {fmt(e0)}, reached {fmt(got['energy'])}, at the vacuum minimiser's xyz_out {fmt(ev)} (its status {vac['status'].flatten().tolist()})")
    assert bool((r64["E"] < e0).all()) and bool((got["energy"].double() < e0).all()), "the energy went up"
    which = list(rg.ORDERED.get(name, ()))          # (the molecules whose float64 restatement shows the ordering with a margin)
    assert bool((got["energy"].double()[which] < ev[which]).all()) and bool((r64["E"][which] < ev[which]).all()), \
        "the vacuum minimum is as low on the solvent surface"


# ------------------------------------------------------------------------------------------------ 6. the seam to the dynamics
def test_the_dynamics_start_from_the_energy_the_minimiser_reports(hip):
    """md_steps_gb(n_steps = 0) from xyz_out: epot and esolv are the relaxation's energy and esolv bit for bit (the same entries at the
    same coordinates, added in the same order)"""
    import md_steps_refs as ms
    from test_gpu_md_gb import _run as run_md
    name = "s65_C3"
    b, gbs = rg.case(name), rg.gb_params(name)
    got = _run(hip, b, gbs, max_steps=25)
    md = run_md(hip, b, ms.masses(name), ms.keys(name), gbs, xyz=got["xyz"], n_steps=0, init_temperature=300.0)
    assert torch.equal(_bits(md["xyz"]), _bits(got["xyz"]))
    assert torch.equal(_bits(md["epot"]), _bits(got["energy"])) and torch.equal(_bits(md["esolv"]), _bits(got["esolv"]))


# ------------------------------------------------------------------------------------------------ 7. faults met, not provoked
def test_a_conformation_that_starts_at_nan_stops_and_leaves_the_others_their_bits(hip):
    clean, gbs = rg.case(rg.MIXED), rg.gb_params(rg.MIXED)
    M, cbad = 3, 1
    p0, p1 = int(clean.ptr[M]), int(clean.ptr[M + 1])
    x = clean.xyz.clone()
    x[p0 + 70, cbad, 1] = float("nan")
    a, c = _run(hip, clean, gbs, xyz=x, max_steps=3, tolerance=0.0), _run(hip, clean, gbs, max_steps=3, tolerance=0.0)
    assert int(a["status"][M, cbad]) == 2 and int(a["steps"][M, cbad]) == 0 and bool(torch.isinf(a["gmax"][M, cbad]))
    assert torch.equal(_bits(a["xyz"][p0:p1, cbad]), _bits(x[p0:p1, cbad])), "status 2 returns the coordinates it holds"
    keep = torch.ones(clean.N, x.shape[1], dtype=torch.bool)
    keep[p0:p1, cbad] = False
    item = torch.ones(clean.B, x.shape[1], dtype=torch.bool)
    item[M, cbad] = False
    for k in ("xyz", "grad"):
        assert torch.equal(_bits(a[k])[keep], _bits(c[k])[keep]), f"{k} of the other conformations"
    for k in ("energy", "gmax", "steps", "status", "esolv"):
        assert torch.equal(_bits(a[k])[item], _bits(c[k])[item]), f"{k} of the other conformations"
    assert torch.equal(_bits(a["terms"])[:, item], _bits(c["terms"])[:, item]), "terms of the other conformations"
    assert bool((a["steps"][M][item[M]] == 3).all()), "the molecule's other conformations did not run on"


def test_a_radius_below_the_offset_ends_its_molecule_and_leaves_the_others(hip):
    """a radius <= offset that reaches the kernels below GBParameters.validate (the table is changed on the device): the Born radii of
    that molecule are NaN, so its items end with status 2 at step 0; the other molecules keep their bits"""
    b, gbs = rg.case(rg.MIXED), rg.gb_params(rg.MIXED)
    M = 3
    gb = GBBatch(gbs).to("cuda")
    gb.radius[int(b.ptr[M]) + 5] = 0.05
    bad, good = _run(hip, b, gbs, gb=gb, max_steps=4, tolerance=0.0), _run(hip, b, gbs, max_steps=4, tolerance=0.0)
    assert bool((bad["status"][M] == 2).all()) and not bad["steps"][M].any() and bool(torch.isinf(bad["gmax"][M]).all())
    assert bool(torch.isnan(bad["energy"][M]).all()) and bool(torch.isnan(bad["esolv"][M]).all())
    p0, p1 = int(b.ptr[M]), int(b.ptr[M + 1])
    assert torch.equal(_bits(bad["xyz"][p0:p1]), _bits(b.xyz[p0:p1]))
    for k in (0, 1, 2, 4, 5):
        _same_bits(_rows_of(bad, b, k), _rows_of(good, b, k), f"molecule {k} beside one with a radius below the offset")
        assert torch.equal(_bits(bad["esolv"][k]), _bits(good["esolv"][k]))


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_launch_nothing_and_write_nothing(hip):
    """a cutoff together with the solvent, a solvent without nb or without charges, NULL radius or scale, options gb_consts refuses, a
    workspace of the plain size, a misaligned workspace: an error code, no launch, the workspace and every output untouched"""
    from grappa_amd.backend_mm import _nb_tables_desc, _opts_struct
    name = "s65_C3"
    b = rg.case(name)
    lib = hip.lib
    plan, x, dnb = b.plan("cuda"), b.xyz.to("cuda"), b.nonbonded().to("cuda")
    N, Cc, B = b.N, x.shape[1], b.B
    ks, eqs = [t.to("cuda") for t in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    d = hip._mm_desc(plan, x, ks, eqs, b.n_per, False)
    nd = _nb_tables_desc(dnb, N, Cc, B, x.device, "test")
    no_q = _nb_tables_desc(dnb, N, Cc, B, x.device, "test")
    no_q.charge = None
    o = _opts_struct(_lib.RelaxOpts, dict(RELAX_DEFAULTS), "test")
    table, n_items, n_blocks, _ = hip.nonbonded_plan(dnb.atom_molptr_host, N, Cc, x.device)
    gb = GBBatch(rg.gb_params(name)).to("cuda")
    need, plain = int(lib.grappa_relax_steps_gb_workspace_bytes(N, Cc, B, n_blocks)), int(lib.grappa_relax_steps_workspace_bytes(N, Cc, B, n_blocks))
    assert need > plain + 4 * 6 * N * Cc
    wbuf = torch.full((GUARD_B + need + GUARD_B,), FILL_B, dtype=torch.uint8, device="cuda")
    ws = wbuf[GUARD_B:GUARD_B + need]
    bufs = {k: _guarded(*v) for k, v in _shapes(N, Cc, B).items()}
    outs = [bufs[k][1].data_ptr() for k in ("xyz", "energy", "terms", "grad", "gmax", "steps", "status", "esolv")]
    nrun = torch.full((1,), FILL_I, dtype=torch.int32, device="cuda")
    good = ImplicitSolvent().as_opts()
    desc = lambda **over: _lib.GbDesc(radius=gb.radius.data_ptr(), scale=gb.scale.data_ptr(), **{**good, **over})      # noqa: E731
    cut = _lib.NbCut(cutoff=9.0, switch_distance=0.0, rf_dielectric=78.3, prune=1)
    no_r, no_s = desc(), desc()
    no_r.radius, no_s.scale = None, None
    torch.cuda.synchronize()
    before = lib.grappa_launch_count(0)

    def three(nbp, cutp, g, wptr, wbytes, want):
        head = (None, C.byref(d), nbp, cutp, C.byref(g), C.byref(o))
        tail = (table.data_ptr(), n_items, n_blocks, wptr, wbytes)
        assert lib.grappa_relax_steps_init_gb_f32(*head, *tail, nrun.data_ptr()) == want
        assert lib.grappa_relax_steps_run_gb_f32(*head, *tail, 4, nrun.data_ptr()) == want
        assert lib.grappa_relax_steps_finish_gb_f32(*head, *tail, *outs) == want

    for nbp, cutp, g in ((C.byref(nd), C.byref(cut), desc()), (None, None, desc()), (C.byref(no_q), None, desc()), (C.byref(nd), None, no_r),
                         (C.byref(nd), None, no_s), (C.byref(nd), None, desc(eps_out=0.0)), (C.byref(nd), None, desc(alpha=float("nan"))),
                         (C.byref(nd), None, desc(surface_tension=-1.0)), (C.byref(nd), None, desc(offset=float("inf")))):
        three(nbp, cutp, g, ws.data_ptr(), ws.numel(), -1)
    three(C.byref(nd), None, desc(), ws.data_ptr(), plain, -3)          # a workspace of the size a call without solvent needs
    three(C.byref(nd), None, desc(), ws.data_ptr(), need - 1, -3)
    three(C.byref(nd), None, desc(), ws.data_ptr() + 4, need - 4, -1)          # not 16-byte aligned
    assert lib.grappa_launch_count(0) == before, "a refused call launched something"
    torch.cuda.synchronize()
    assert bool((wbuf == FILL_B).all()), "a refused call wrote to the workspace"
    assert int(nrun[0]) == FILL_I
    for k, (buf, _) in bufs.items():
        assert bool((buf == _fill_of(buf)).all()), f"a refused call wrote to {k}"
    # the seam's own checks
    with pytest.raises(TypeError, match="GBBatch"):
        _run(hip, b, None, gb="obc2", max_steps=1)
    with pytest.raises(ValueError, match="offset"):
        _run(hip, b, rg.gb_params(name), solvent=ImplicitSolvent(offset=1.75), max_steps=1)


# ------------------------------------------------------------------------------------------------ 9. the public doors
def test_relax_and_relax_graph_against_the_seam(hip):
    from grappa_amd import backend
    from grappa_amd.nonbonded import NonbondedBatch
    from grappa_amd.relax import graph_from_parameters, relax, relax_graph
    from test_gpu_relax_steps import _parameters
    old = backend._BACKEND
    backend.set_backend(hip)
    try:
        name = "s65_C3"
        b, gbs = rg.case(name), rg.gb_params(name)
        mol = b.mols[0]
        p, xyz = _parameters(mol), mol["xyz"].transpose(1, 0, 2)
        seam = _run(hip, b, gbs, max_steps=200)
        r = relax(p, xyz, mol["nb"], stepwise="auto", max_steps=200, implicit_solvent="obc2", gb=gbs[0])
        g = graph_from_parameters(p, xyz).to("cuda")
        rg_ = relax_graph(g, NonbondedBatch([mol["nb"]]).to("cuda"), stepwise=True, max_steps=200, check_every=9, implicit_solvent=ImplicitSolvent(),
                          gb=GBBatch(gbs).to("cuda"))
        assert r.xyz.shape == xyz.shape and rg_.xyz.shape == (65, 3, 3) and bool((r.status != 2).all()) and r.esolv.shape == (3,)
        for f, key in (("xyz", "xyz"), ("energy", "energy"), ("gradient_max", "gmax"), ("steps", "steps"), ("status", "status"), ("esolv", "esolv")):
            assert torch.equal(_bits(getattr(rg_, f).cpu()), _bits(seam[key])), f
        assert np.array_equal(r.xyz.astype(np.float32), seam["xyz"].numpy().transpose(1, 0, 2))
        assert np.array_equal(r.energy.astype(np.float32), seam["energy"].numpy()[0]) and np.array_equal(r.esolv.astype(np.float32), seam["esolv"].numpy()[0])
        assert np.array_equal(r.steps, seam["steps"].numpy()[0]) and np.array_equal(r.status, seam["status"].numpy()[0])
        vac = relax(p, xyz, mol["nb"], stepwise="auto", max_steps=200)
        assert vac.esolv is None and not np.array_equal(vac.xyz, r.xyz)
    finally:
        backend.set_backend(old)


def test_grappa_relax_in_implicit_solvent(hip):
    """Grappa.relax(..., implicit_solvent="obc2", stepwise="auto") end to end on a molecule of the golden fixture with its own partial
    charges: finite output, esolv < 0 and part of the energy, the radii from the molecule's elements; the dynamics in the same solvent
    start at the energy it reports"""
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
        pos = {int(a): i for i, a in enumerate(mol.atoms)}
        nbp = NonbondedParameters.from_bonds([(pos[int(a)], pos[int(b)]) for a, b in mol.bonds], q, np.where(z == 1, 1.0, 3.2), np.where(z == 1, 0.02, 0.1))
        xyz = np.ascontiguousarray(mm["xyz"].transpose(1, 0, 2)[:2])
        r = wrapper.relax(mol, xyz, nbp, implicit_solvent="obc2", stepwise="auto")
        assert r.xyz.shape == xyz.shape and bool(np.isfinite(r.xyz).all()) and bool(np.isfinite(r.energy).all()) and bool((r.status != 2).all())
        assert r.esolv.shape == r.energy.shape and bool((r.esolv < 0).all())
        vac = wrapper.relax(mol, xyz, nbp, stepwise="auto")
        assert vac.esolv is None and not np.array_equal(vac.xyz, r.xyz)
        md = wrapper.simulate(mol, np.ascontiguousarray(r.xyz), nbp, implicit_solvent="obc2", stepwise="auto", n_steps=0)
        print(f"Grappa.relax in obc2: energy {r.energy.tolist()} of which esolv {r.esolv.tolist()} kcal/mol in {r.steps.tolist()} steps, status {r.status.tolist()}")
        assert np.array_equal(md.potential_energy, r.energy) and np.array_equal(md.esolv, r.esolv)
    finally:
        backend.set_backend(old)
