"""GPU: the stepwise minimiser under a nonbonded cutoff (grappa_relax_steps_*_cut_f32 through HipBackend.relax_steps(cutoff=) and
grappa_amd/relax.py) against the restatements of tests/relax_cut_refs.py: forces at step zero, trajectories through the gate of
tests/test_gpu_relax_steps.py as it stands, the bits (prune = 0 against prune = 1 over a converging run, two runs, chunk sizes, an item
alone against the same item in a batch, cut = NULL against the plain entry points), the launch counts, convergence, a conformation that
starts at NaN, the refusals and the public doors.  Every output and the workspace lie between guard words."""
import ctypes as C

import numpy as np
import pytest
import torch

import kernel_refs as kr
import md_steps_refs as ms
import relax_cut_refs as rc
import relax_refs as rr
import relax_steps_refs as rs
from grappa_amd import _lib
from grappa_amd.nonbonded import Cutoff
from grappa_amd.relax import RELAX_DEFAULTS
from test_gpu_md_cut import _run as _md_run
from test_gpu_relax_steps import FILL, FILL_B, FILL_I, GUARD_B, OUTS, _guarded, _parameters, _rows_of, _same_bits, _single, _traj_gate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from grappa_amd.backend import HipBackend
    return HipBackend()


def _sizes(hip, batch, Cc):
    """the workspace sizes (plain, cut) of the batch"""
    n = rs.n_blocks(batch)
    return (int(hip.lib.grappa_relax_steps_workspace_bytes(batch.N, Cc, batch.B, n)),
            int(hip.lib.grappa_relax_steps_cut_workspace_bytes(batch.N, Cc, batch.B, n)))


def _run(hip, batch, cut, nb=True, check_every=32, expect_written=True, short=0, **opts):
    """one call of the seam under `cut` (None: all pairs) on a relax_refs.Batch -> dict of CPU tensors (OUTS); asserts the guards around
    the outputs and the workspace (short: bytes the workspace handed over lacks)"""
    plan = batch.plan("cuda")
    dnb = batch.nonbonded().to("cuda") if nb else None
    x = batch.xyz.to("cuda")
    N, Cc, B = batch.N, x.shape[1], batch.B
    shapes = {"xyz": ((N, Cc, 3), torch.float32), "energy": ((B, Cc), torch.float32), "gmax": ((B, Cc), torch.float32),
              "steps": ((B, Cc), torch.int32), "status": ((B, Cc), torch.int32), "terms": ((6, B, Cc), torch.float32),
              "grad": ((N, Cc, 3), torch.float32)}
    bufs = {k: _guarded(*v) for k, v in shapes.items()}
    o = {k: bufs[k][1] for k in OUTS}
    need = _sizes(hip, batch, Cc)[0 if cut is None else 1]
    wbuf = torch.full((GUARD_B + need + GUARD_B,), FILL_B, dtype=torch.uint8, device="cuda")
    ws = wbuf[GUARD_B:GUARD_B + max(need - short, 0)]
    ks = [k.to("cuda") for k in batch.ks]
    eqs = [None if q is None else q.to("cuda") for q in batch.eqs]
    kw = {} if cut is None else {"cutoff": cut}

    def guards():
        torch.cuda.synchronize()
        for k, (buf, view) in bufs.items():
            fill = FILL_I if buf.dtype == torch.int32 else FILL
            assert bool((buf[:64] == fill).all()) and bool((buf[-64:] == fill).all()), f"written outside {k}"
        assert bool((wbuf[:GUARD_B] == FILL_B).all()) and bool((wbuf[-GUARD_B - short:] == FILL_B).all()), "written outside the workspace"
    try:
        hip.relax_steps(plan, x, ks, eqs, batch.n_per, False, dnb, {**RELAX_DEFAULTS, **opts}, o["xyz"], o["energy"], o["gmax"], o["steps"],
                        o["status"], term_energy=o["terms"], grad=o["grad"], atom_counts_host=batch.counts, check_every=check_every, workspace=ws,
                        **kw)
    finally:
        guards()
    if expect_written:
        for k, (buf, view) in bufs.items():
            if view.numel():
                assert not bool((view == (FILL_I if buf.dtype == torch.int32 else FILL)).all()), f"{k} was not written"
    else:
        for k, (buf, view) in bufs.items():
            assert bool((view == (FILL_I if buf.dtype == torch.int32 else FILL)).all()), f"a refused call wrote {k}"
        assert bool((wbuf == FILL_B).all()), "a refused call wrote to the workspace"
    return {k: v.cpu().clone() for k, v in o.items()}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


# ------------------------------------------------------------------------------------------------ 1. forces
@pytest.mark.parametrize("name", rc.TRAJ_CASES)
def test_forces_at_step_zero(hip, name):
    """max_steps = 0: the coordinates come back bit for bit; energy, the six terms and the gradient pass the calibrated gate against the
    cut restatement; the six terms are the bits of mm_energy_fwd and NonbondedBatch.evaluate(x, cutoff=cut)"""
    b, cut = rs.case(name), rc.cutoff(name)
    r64, r32 = rc.forces_of(name, torch.float64), rc.forces_of(name, torch.float32)
    got = _run(hip, b, cut, max_steps=0, tolerance=0.0)
    assert torch.equal(_bits(got["xyz"]), _bits(b.xyz)), "xyz_out differs from the input"
    one = _single(b)[:, None].expand_as(got["status"])
    assert bool((got["steps"] == 0).all()) and torch.equal(got["status"], one.int())
    rr.gate_forces(got["energy"], got["terms"], got["grad"], r64, r32, f"{name} under the cutoff")
    want_gmax = torch.stack([got["grad"][int(b.ptr[k]):int(b.ptr[k + 1])].double().norm(dim=-1).max(0).values for k in range(b.B)])
    assert bool(((got["gmax"].double() - want_gmax).abs() <= 4 * kr.U32 * want_gmax).all()), "gmax is not the largest gradient norm"
    plan, x = b.plan("cuda"), b.xyz.to("cuda")
    ks, eqs = [k.to("cuda") for k in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    Cc = x.shape[1]
    e, t = torch.zeros(b.B, Cc, device="cuda"), torch.zeros(4, b.B, Cc, device="cuda")
    hip.mm_energy_fwd(plan, x, ks, eqs, b.n_per, False, e, t)
    _, _, nt = b.nonbonded().to("cuda").evaluate(x, terms=True, gradient=False, cutoff=cut)
    want = torch.cat([t, nt]).cpu()
    assert torch.equal(_bits(got["terms"]), _bits(want)), "the six terms are not the bits of the energy kernels"
    # energy: the six terms added in double in term order
    tot = torch.zeros(b.B, Cc, dtype=torch.float64)
    for row in want:
        tot = tot + row.double()
    assert torch.equal(_bits(got["energy"]), _bits(tot.float()))
    _, _, nt_all = b.nonbonded().to("cuda").evaluate(x, terms=True, gradient=False)
    assert not torch.equal(_bits(nt.cpu()), _bits(nt_all.cpu())), "the cutoff changed nothing"


# ------------------------------------------------------------------------------------------------ 2. trajectories
TRAJ = [(n, s) for n in rc.TRAJ_CASES for s in rc.TRAJ_STEPS]


@pytest.mark.parametrize("name,max_steps", TRAJ, ids=[f"{n}-{s}steps" for n, s in TRAJ])
def test_trajectory(hip, name, max_steps):
    """tolerance = 0: every item runs exactly max_steps steps; a conformation that keeps the branch margin ends within 4 x the fp32
    restatement's distance to float64 + 2^-20 A (the gate of tests/test_gpu_relax_steps.py as it stands)"""
    b = rs.case(name)
    x64, x32 = rc.trajectory(name, torch.float64)["snap"][max_steps], rc.trajectory(name, torch.float32)["snap"][max_steps]
    ok = rc.margin_ok(name, max_steps)
    got = _run(hip, b, rc.cutoff(name), max_steps=max_steps, tolerance=0.0)
    one = _single(b)[:, None].expand_as(got["status"])
    assert torch.equal(got["steps"], torch.where(one, 0, max_steps).int()) and torch.equal(got["status"], one.int())
    _traj_gate(name, b, got["xyz"], x64, x32, ok, f"{max_steps} steps under the cutoff")


# ------------------------------------------------------------------------------------------------ 3. bits
@pytest.mark.parametrize("name,opts", [("s2_130_9_C3", dict(max_steps=1000)), (rc.MIXED, dict(max_steps=600)),
                                       ("s513_C1", dict(max_steps=40, tolerance=0.0))], ids=["s2_130_9_C3", "mixed", "s513_C1"])
def test_pruning_changes_no_bit(hip, name, opts):
    """prune = 1 against prune = 0.  With the default tolerance the conformations of one chunk stop at different steps (asserted), so
    this is the test of the margin and of "a stopped conformation keeps its box": a skipped tile that held a pair within the cutoff,
    or a box that moved on after its conformation stopped, would change a bit"""
    b = rs.case(name)
    on, off = _run(hip, b, rc.cutoff(name), **opts), _run(hip, b, rc.cutoff(name, False), **opts)
    print(f"{name}: steps {on['steps'].tolist()} status {on['status'].tolist()}")
    _same_bits(on, off, "prune = 1 against prune = 0")
    if "tolerance" not in opts:
        apart = [k for k in range(b.B) if bool((on["status"][k] == 1).all()) and len(set(on["steps"][k].tolist())) == on["steps"].shape[1]]
        assert apart, "no molecule whose conformations -- one chunk -- converge at different steps"


def test_two_runs_and_every_chunk_size_give_the_same_bits(hip):
    b, cut = rs.case(rc.MIXED), rc.cutoff(rc.MIXED)
    a = _run(hip, b, cut, max_steps=40, tolerance=0.0)
    _same_bits(a, _run(hip, b, cut, max_steps=40, tolerance=0.0), "two runs")
    for ce in (1, 7, 64):
        _same_bits(a, _run(hip, b, cut, check_every=ce, max_steps=40, tolerance=0.0), f"check_every = {ce}")
    # with the default tolerance items stop at different steps: steps enqueued after an item stopped touch neither it nor its box
    c = _run(hip, b, cut, check_every=1, max_steps=120)
    for ce in (7, 64):
        _same_bits(c, _run(hip, b, cut, check_every=ce, max_steps=120), f"default tolerance, check_every = {ce}")
    plain = _run(hip, b, None, max_steps=40, tolerance=0.0)
    assert not torch.equal(_bits(a["xyz"]), _bits(plain["xyz"])), "the cutoff changed nothing"


def test_an_item_alone_has_the_bits_it_has_inside_the_mixed_batch(hip):
    """under ONE cutoff (the mixed batch's): the 130-atom molecule (three blocks: other rows of the boxes and ranges behind its
    neighbours) and the 17-atom one"""
    mixed, cut = rs.case(rc.MIXED), rc.cutoff(rc.MIXED)
    a = _run(hip, mixed, cut, max_steps=300)
    for k in (2, 3):
        sub = mixed.subset([k])
        _same_bits(_rows_of(_run(hip, sub, cut, max_steps=300), sub, 0), _rows_of(a, mixed, k), f"molecule {k} alone against the batch")


def test_a_null_cut_is_the_plain_entry_point(hip):
    """grappa_relax_steps_*_cut_f32 with cut == NULL against grappa_relax_steps_*_f32: the same launches, the same bits, in a
    workspace of the plain size"""
    b = rs.case("s129_C3")
    lib = hip.lib
    plan, x, dnb = b.plan("cuda"), b.xyz.to("cuda"), b.nonbonded().to("cuda")
    Cc = x.shape[1]
    ks, eqs = [t.to("cuda") for t in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    d = hip._mm_desc(plan, x, ks, eqs, b.n_per, False)
    from grappa_amd.backend_mm import _nb_tables_desc, _opts_struct
    nd = _nb_tables_desc(dnb, b.N, Cc, b.B, x.device, "test")
    o = _opts_struct(_lib.RelaxOpts, {**RELAX_DEFAULTS, "max_steps": 6, "tolerance": 0.0}, "test")
    table, n_items, n_blocks, _ = hip.nonbonded_plan(dnb.atom_molptr_host, b.N, Cc, x.device)
    outs = {}
    for which in ("plain", "null_cut"):
        ws = torch.zeros(_sizes(hip, b, Cc)[0], dtype=torch.uint8, device="cuda")
        out = {"xyz": torch.empty_like(x), "energy": torch.zeros(b.B, Cc, device="cuda"), "terms": torch.zeros(6, b.B, Cc, device="cuda"),
               "grad": torch.empty_like(x), "gmax": torch.zeros(b.B, Cc, device="cuda"),
               "steps": torch.zeros(b.B, Cc, dtype=torch.int32, device="cuda"), "status": torch.zeros(b.B, Cc, dtype=torch.int32, device="cuda")}
        nrun = torch.zeros(1, dtype=torch.int32, device="cuda")
        head = (None, C.byref(d), C.byref(nd)) + ((None,) if which == "null_cut" else ()) + (C.byref(o),)
        sfx = "_cut_f32" if which == "null_cut" else "_f32"
        tail = (table.data_ptr(), n_items, n_blocks, ws.data_ptr(), ws.numel())
        before = lib.grappa_launch_count(0)
        assert getattr(lib, "grappa_relax_steps_init" + sfx)(*head, *tail, nrun.data_ptr()) == 0
        assert getattr(lib, "grappa_relax_steps_run" + sfx)(*head, *tail, 6, nrun.data_ptr()) == 0
        assert getattr(lib, "grappa_relax_steps_finish" + sfx)(*head, *tail, *[out[k].data_ptr() for k in ("xyz", "energy", "terms", "grad", "gmax",
                                                                                                            "steps", "status")]) == 0
        torch.cuda.synchronize()
        outs[which] = ({k: v.cpu().clone() for k, v in out.items()}, lib.grappa_launch_count(0) - before)
    _same_bits(outs["plain"][0], outs["null_cut"][0], "cut = NULL against the plain entry points")
    assert outs["plain"][1] == outs["null_cut"][1] == 2 + 6 * 4 + 5


# ------------------------------------------------------------------------------------------------ 4. launches
@pytest.mark.parametrize("name", ["s9_65_C17", "s513_C1"])
def test_launch_counts(hip, name):
    """with a cutoff: init 3 (init, boxes and ranges, force), a step 4 (decide, vel, move, force), finish 6 (decide, the bonded energy,
    boxes, pairs and reduce of the cut energy entry, out)"""
    b, cut = rs.case(name), rc.cutoff(name)
    lib = hip.lib
    plan, x, dnb = b.plan("cuda"), b.xyz.to("cuda"), b.nonbonded().to("cuda")
    Cc = x.shape[1]
    ks, eqs = [t.to("cuda") for t in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    d = hip._mm_desc(plan, x, ks, eqs, b.n_per, False)
    from grappa_amd.backend_mm import _cut_struct, _nb_tables_desc, _opts_struct
    nd = _nb_tables_desc(dnb, b.N, Cc, b.B, x.device, "test")
    o = _opts_struct(_lib.RelaxOpts, {**RELAX_DEFAULTS, "max_steps": 10, "tolerance": 0.0}, "test")
    cs = _cut_struct(cut, "test")
    table, n_items, n_blocks, _ = hip.nonbonded_plan(dnb.atom_molptr_host, b.N, Cc, x.device)
    ws = torch.zeros(_sizes(hip, b, Cc)[1], dtype=torch.uint8, device="cuda")
    out = [torch.empty_like(x), torch.zeros(b.B, Cc, device="cuda"), torch.zeros(6, b.B, Cc, device="cuda"), torch.empty_like(x),
           torch.zeros(b.B, Cc, device="cuda"), torch.zeros(b.B, Cc, dtype=torch.int32, device="cuda"),
           torch.zeros(b.B, Cc, dtype=torch.int32, device="cuda")]
    nrun = torch.zeros(1, dtype=torch.int32, device="cuda")
    head = (None, C.byref(d), C.byref(nd), C.byref(cs), C.byref(o))
    tail = (table.data_ptr(), n_items, n_blocks, ws.data_ptr(), ws.numel())
    n = [lib.grappa_launch_count(0)]
    assert lib.grappa_relax_steps_init_cut_f32(*head, *tail, nrun.data_ptr()) == 0
    n.append(lib.grappa_launch_count(0))
    assert lib.grappa_relax_steps_run_cut_f32(*head, *tail, 1, nrun.data_ptr()) == 0
    n.append(lib.grappa_launch_count(0))
    assert lib.grappa_relax_steps_run_cut_f32(*head, *tail, 9, nrun.data_ptr()) == 0
    n.append(lib.grappa_launch_count(0))
    assert lib.grappa_relax_steps_finish_cut_f32(*head, *tail, *[t.data_ptr() for t in out]) == 0
    n.append(lib.grappa_launch_count(0))
    torch.cuda.synchronize()
    counts = [n[k + 1] - n[k] for k in range(4)]
    print(f"{name}: launches of init, one step, nine steps, finish: {counts}")
    assert counts == [3, 4, 36, 6], counts
    assert bool((out[5].cpu()[~_single(b)] == 10).all())


# ------------------------------------------------------------------------------------------------ 5. convergence
@pytest.mark.parametrize("name", rc.CONV_CASES)
def test_convergence_with_the_defaults(hip, name):
    """the assertions of tests/test_gpu_relax_steps.py::test_convergence_with_the_defaults with the cut restatement's forces at xyz_out"""
    b = rs.case(name)
    got = _run(hip, b, rc.cutoff(name), max_steps=rc.CONV_MAX_STEPS)
    conv = got["status"] == 1
    assert bool(conv.any()) and bool(((got["status"] == 0) | conv).all()), got["status"].tolist()
    assert bool((got["steps"] <= rc.CONV_MAX_STEPS).all()) and bool((got["steps"][got["status"] == 0] == rc.CONV_MAX_STEPS).all())
    r64, r32 = rc.forces_at(name, got["xyz"], torch.float64), rc.forces_at(name, got["xyz"], torch.float32)
    per_mol = lambda t: torch.stack([t[int(b.ptr[k]):int(b.ptr[k + 1])].max(0).values for k in range(b.B)])      # noqa: E731
    gmax64, gmax32 = per_mol(r64["G"].norm(dim=-1)), per_mol(r32["G"].double().norm(dim=-1))
    floor = rr.C_GATE * kr.U32 * per_mol(r64["abs_f"])
    cal = torch.maximum(per_mol((r32["G"].double() - r64["G"]).norm(dim=-1)), (gmax32 - gmax64).abs())
    bound = floor + 2 * cal + 2 * kr.U32 * per_mol(rr.bond_rounding(b, got["xyz"]))
    fmt = lambda t: [f"{v:.2e}" for v in t.flatten().tolist()]      # noqa: E731
    print(f"{name}: steps {got['steps'].flatten().tolist()} status {got['status'].flatten().tolist()}\n  gmax gpu - f64 {fmt(got['gmax'].double() - gmax64)}"
          f"\n  f64 gmax - tolerance {fmt(gmax64 - RELAX_DEFAULTS['tolerance'])}\n  bound {fmt(bound)}")
    assert bool((gmax64 <= RELAX_DEFAULTS["tolerance"] + bound)[conv].all()), "the float64 gradient at xyz_out is above the tolerance"
    rr.gate_forces(got["energy"], None, None, r64, r32, f"{name} at xyz_out")
    assert bool(((got["gmax"].double() - gmax64).abs() <= bound).all()), "gmax at xyz_out"
    e0 = rc.forces_of(name, torch.float64)["E"]
    assert bool((r64["E"] <= e0)[conv].all()), "the float64 energy went up"


# ------------------------------------------------------------------------------------------------ 6. NaN
def test_a_conformation_that_starts_at_nan_stops_and_leaves_the_others_their_bits(hip):
    """one conformation of the 130-atom molecule starts with a NaN coordinate: the box of its block is NaN on that axis and compares as
    near.  It stops with status 2 at step zero with the coordinates it holds, and after three steps every other (molecule,
    conformation) -- its siblings in the chunk included -- has the bits it has without the NaN"""
    clean, cut = rs.case(rc.MIXED), rc.cutoff(rc.MIXED)
    M, cbad = 3, 1
    p0, p1 = int(clean.ptr[M]), int(clean.ptr[M + 1])
    mols = [dict(m) for m in clean.mols]
    xm = mols[M]["xyz"].copy()
    xm[70, cbad, 1] = float("nan")
    mols[M]["xyz"] = xm
    bad = rr.Batch(mols)
    keep = torch.ones(clean.N, clean.xyz.shape[1], dtype=torch.bool)
    keep[p0:p1, cbad] = False
    item = torch.ones(clean.B, clean.xyz.shape[1], dtype=torch.bool)
    item[M, cbad] = False
    a, c = _run(hip, bad, cut, max_steps=3, tolerance=0.0), _run(hip, clean, cut, max_steps=3, tolerance=0.0)
    assert int(a["status"][M, cbad]) == 2 and int(a["steps"][M, cbad]) == 0 and bool(torch.isinf(a["gmax"][M, cbad]))
    assert torch.equal(_bits(a["xyz"][p0:p1, cbad]), _bits(bad.xyz[p0:p1, cbad])), "status 2 returns the coordinates it holds"
    for k in ("xyz", "grad"):
        assert torch.equal(_bits(a[k])[keep], _bits(c[k])[keep]), f"{k} of the other conformations"
    for k in ("energy", "gmax", "steps", "status"):
        assert torch.equal(_bits(a[k])[item], _bits(c[k])[item]), f"{k} of the other conformations"
    assert torch.equal(_bits(a["terms"])[:, item], _bits(c["terms"])[:, item]), "terms of the other conformations"
    assert bool((a["steps"][M][item[M]] == 3).all()), "the molecule's other conformations did not run on"


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_launch_nothing_and_write_nothing(hip):
    from grappa_amd.backend import GrappaHipError
    b, cut = rs.case("s65_C3"), rc.cutoff("s65_C3")
    lib = hip.lib
    Cc = b.xyz.shape[1]
    plain, with_cut = _sizes(hip, b, Cc)
    assert with_cut > plain
    before = lib.grappa_launch_count(0)
    with pytest.raises(ValueError, match="a cutoff needs the nonbonded tables"):
        _run(hip, b, cut, nb=False, expect_written=False, max_steps=5)
    with pytest.raises(ValueError, match="distance"):
        _run(hip, b, -9.0, expect_written=False, max_steps=5)
    with pytest.raises(GrappaHipError, match="GRAPPA_ERR_WORKSPACE"):          # a workspace of the plain size
        _run(hip, b, cut, expect_written=False, short=with_cut - plain, max_steps=5)
    with pytest.raises(GrappaHipError, match="GRAPPA_ERR_WORKSPACE"):
        _run(hip, b, cut, expect_written=False, short=1, max_steps=5)
    assert lib.grappa_launch_count(0) == before, "a refused call launched something"
    # the C ABI itself
    plan, x, dnb = b.plan("cuda"), b.xyz.to("cuda"), b.nonbonded().to("cuda")
    ks, eqs = [t.to("cuda") for t in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    d = hip._mm_desc(plan, x, ks, eqs, b.n_per, False)
    from grappa_amd.backend_mm import _cut_struct, _nb_tables_desc, _opts_struct
    nd = _nb_tables_desc(dnb, b.N, Cc, b.B, x.device, "test")
    o = _opts_struct(_lib.RelaxOpts, dict(RELAX_DEFAULTS), "test")
    good = _cut_struct(cut, "test")
    table, n_items, n_blocks, _ = hip.nonbonded_plan(dnb.atom_molptr_host, b.N, Cc, x.device)
    big = rs.case("s513_C1")          # a table made for another batch: its nine blocks do not fit a batch of 65 atoms
    table9, n_items9, n_blocks9, _ = hip.nonbonded_plan(big.nonbonded().atom_molptr_host, big.N, Cc, x.device)
    wbuf = torch.full((GUARD_B + with_cut + GUARD_B,), FILL_B, dtype=torch.uint8, device="cuda")
    ws = wbuf[GUARD_B:GUARD_B + with_cut]
    xo, g = torch.full_like(x, FILL), torch.full_like(x, FILL)
    e, gm, te = torch.full((b.B, Cc), FILL, device="cuda"), torch.full((b.B, Cc), FILL, device="cuda"), torch.full((6, b.B, Cc), FILL, device="cuda")
    st, ss = (torch.full((b.B, Cc), FILL_I, dtype=torch.int32, device="cuda") for _ in range(2))
    nrun = torch.full((1,), FILL_I, dtype=torch.int32, device="cuda")
    neg = _lib.NbCut(cutoff=-9.0, switch_distance=0.0, rf_dielectric=78.3, prune=1)
    sw = _lib.NbCut(cutoff=9.0, switch_distance=9.5, rf_dielectric=78.3, prune=1)
    pr = _lib.NbCut(cutoff=9.0, switch_distance=0.0, rf_dielectric=78.3, prune=2)
    tail = (table.data_ptr(), n_items, n_blocks, ws.data_ptr(), ws.numel())
    cases = [("a cut without nb", None, good, tail, -1), ("a negative distance", nd, neg, tail, -1), ("a switch beyond the cutoff", nd, sw, tail, -1),
             ("prune = 2", nd, pr, tail, -1), ("a workspace of the plain size", nd, good, tail[:4] + (plain,), -3),
             ("a table made for another batch", nd, good, (table9.data_ptr(), n_items9, n_blocks9, ws.data_ptr(), ws.numel()), -1)]
    for what, ndx, cs, tl, want in cases:
        head = (None, C.byref(d), None if ndx is None else C.byref(ndx), C.byref(cs), C.byref(o))
        assert lib.grappa_relax_steps_init_cut_f32(*head, *tl, nrun.data_ptr()) == want, what
        assert lib.grappa_relax_steps_run_cut_f32(*head, *tl, 3, nrun.data_ptr()) == want, what
        assert lib.grappa_relax_steps_finish_cut_f32(*head, *tl, xo.data_ptr(), e.data_ptr(), te.data_ptr(), g.data_ptr(), gm.data_ptr(), st.data_ptr(),
                                                     ss.data_ptr()) == want, what
    torch.cuda.synchronize()
    assert lib.grappa_launch_count(0) == before, "a refused call launched something"
    assert bool((wbuf == FILL_B).all()), "a refused call wrote to the workspace"
    assert all(bool((t == FILL).all()) for t in (xo, g, e, gm, te)) and all(bool((t == FILL_I).all()) for t in (st, ss, nrun))


# ------------------------------------------------------------------------------------------------ 8. the public doors
def test_relax_with_a_cutoff_and_the_dynamics_that_follow(hip):
    from grappa_amd import backend
    from grappa_amd.relax import relax
    old = backend._BACKEND
    backend.set_backend(hip)
    try:
        name = "s513_C1"
        b, cut = rs.case(name), rc.cutoff(name)
        mol = b.mols[0]
        p, xyz = _parameters(mol), mol["xyz"].transpose(1, 0, 2)
        before = hip.lib.grappa_launch_count(0)
        for kw in ({}, {"stepwise": False}):
            with pytest.raises(ValueError, match='stepwise="auto"'):
                relax(p, xyz, mol["nb"], max_steps=5, tolerance=0.0, cutoff=9.0, **kw)
        assert hip.lib.grappa_launch_count(0) == before, "a refused call launched something"
        r = relax(p, xyz, mol["nb"], stepwise="auto", max_steps=5, tolerance=0.0, cutoff=cut)
        assert r.xyz.shape == xyz.shape and r.steps.tolist() == [5] and r.status.tolist() == [0]
        got = torch.from_numpy(np.ascontiguousarray(r.xyz.transpose(1, 0, 2))).float()
        _traj_gate(name, b, got, rc.trajectory(name, torch.float64)["snap"][5], rc.trajectory(name, torch.float32)["snap"][5], rc.margin_ok(name, 5),
                   "5 steps through relax(cutoff=, stepwise='auto')")
        seam = _run(hip, b, cut, max_steps=5, tolerance=0.0)
        assert torch.equal(_bits(got), _bits(seam["xyz"])) and np.array_equal(r.energy.astype(np.float32), seam["energy"].numpy()[0])
        plain = relax(p, xyz, mol["nb"], stepwise="auto", max_steps=5, tolerance=0.0, cutoff=float(cut.distance))          # a plain float is a Cutoff
        want = _run(hip, b, Cutoff(float(cut.distance)), max_steps=5, tolerance=0.0)
        assert np.array_equal(plain.xyz.transpose(1, 0, 2).astype(np.float32), want["xyz"].numpy())
        assert not np.array_equal(plain.xyz, r.xyz), "the switch changed nothing"
    finally:
        backend.set_backend(old)


@pytest.mark.parametrize("name", ["s513_C1", "s129_C3"])
def test_the_dynamics_start_at_the_energy_the_relaxation_ends_at(hip, name):
    """relax under the cutoff, then HipBackend.md_steps with the same cutoff and n_steps = 0 from xyz_out: epot has the bits of the
    relaxation's energy (ms_out_kernel keeps the arrangement of grappa_relax_steps_finish_f32: the six terms added in double in term
    order)"""
    b, cut = rs.case(name), rc.cutoff(name)
    got = _run(hip, b, cut, max_steps=20, tolerance=0.0)
    md = _md_run(hip, b, ms.masses(name), ms.keys(name), cut, vel=torch.zeros_like(b.xyz), xyz=got["xyz"], n_steps=0)
    assert torch.equal(_bits(md["xyz"]), _bits(got["xyz"]))
    assert torch.equal(_bits(md["epot"]), _bits(got["energy"])), (md["epot"].tolist(), got["energy"].tolist())
