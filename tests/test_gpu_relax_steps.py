"""GPU: the stepwise FIRE minimiser (csrc/relax_steps.hip through HipBackend.relax_steps and grappa_amd/relax.py) against the float64
restatement of tests/relax_refs.py on the cases of tests/relax_steps_refs.py.  Every output AND the workspace lie between guard regions
that must come back untouched.

Gates: those of tests/test_gpu_relax.py.  Forces and energies: |gpu - f64| <= 2 |fp32 restatement - f64| + 64 u32 scale.  Trajectories:
for every conformation that keeps the branch margin, max_atoms |x_gpu - x_f64| <= TRAJ_FACTOR max_atoms |x_f32 - x_f64| + 2^-20 A with
TRAJ_FACTOR = 4; the observed ratio is printed per case.  Convergence: the bound of test_convergence_with_the_defaults (the floor
64 u32 max_i abs_f_i + twice the fp32 restatement's distance to float64 at xyz_out + 2 u32 max_i sum_bonds k r)."""
import numpy as np
import pytest
import torch

import kernel_refs as kr
import relax_refs as rr
import relax_steps_refs as rs
from grappa_amd.relax import MAX_STEPS_CAP, RELAX_DEFAULTS

pytestmark = pytest.mark.gpu

FILL, FILL_I, FILL_B = 1024.0, 12345, 0xA5       # sentinels around (and, before the call, inside) every output buffer and the workspace
GUARD_B = 4096
TRAJ_FACTOR = 4
ULP_X = 2.0 ** -20
OUTS = ("xyz", "energy", "gmax", "steps", "status", "terms", "grad")


@pytest.fixture(scope="module")
def hip():
    from grappa_amd.backend import HipBackend
    return HipBackend()


def _guarded(shape, dtype=torch.float32, guard=64):
    n = int(np.prod(shape))
    buf = torch.full((guard + n + guard,), FILL_I if dtype == torch.int32 else FILL, dtype=dtype, device="cuda")
    return buf, buf[guard:guard + n].view(*shape)


def _workspace(hip, batch, Cc, short=0):
    need = int(hip.lib.grappa_relax_steps_workspace_bytes(batch.N, Cc, batch.B, rs.n_blocks(batch)))
    buf = torch.full((GUARD_B + need + GUARD_B,), FILL_B, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD_B:GUARD_B + max(need - short, 0)]


def _run(hip, batch, nb="full", check_every=32, expect_written=True, short=0, **opts):
    """one call of the seam on a relax_refs.Batch -> dict of CPU tensors (OUTS); asserts the guards.  nb: "full", "zero" (a table of
    all-zero charge and epsilon) or None"""
    plan = batch.plan("cuda")
    dnb = None if nb is None else batch.nonbonded(zero=nb == "zero").to("cuda")
    x = batch.xyz.to("cuda")
    N, Cc, B = batch.N, x.shape[1], batch.B
    shapes = {"xyz": ((N, Cc, 3), torch.float32), "energy": ((B, Cc), torch.float32), "gmax": ((B, Cc), torch.float32),
              "steps": ((B, Cc), torch.int32), "status": ((B, Cc), torch.int32), "terms": ((6, B, Cc), torch.float32),
              "grad": ((N, Cc, 3), torch.float32)}
    bufs = {k: _guarded(*v) for k, v in shapes.items()}
    o = {k: bufs[k][1] for k in OUTS}
    wbuf, ws = _workspace(hip, batch, Cc, short)
    ks = [k.to("cuda") for k in batch.ks]
    eqs = [None if q is None else q.to("cuda") for q in batch.eqs]

    def guards():
        torch.cuda.synchronize()
        for k, (buf, view) in bufs.items():
            fill = FILL_I if buf.dtype == torch.int32 else FILL
            assert bool((buf[:64] == fill).all()) and bool((buf[-64:] == fill).all()), f"written outside {k}"
        assert bool((wbuf[:GUARD_B] == FILL_B).all()) and bool((wbuf[-GUARD_B - short:] == FILL_B).all()), "written outside the workspace"
    try:
        hip.relax_steps(plan, x, ks, eqs, batch.n_per, False, dnb, {**RELAX_DEFAULTS, **opts}, o["xyz"], o["energy"], o["gmax"], o["steps"],
                        o["status"], term_energy=o["terms"], grad=o["grad"], atom_counts_host=batch.counts, check_every=check_every, workspace=ws)
    finally:
        guards()
    if expect_written:
        for k, (buf, view) in bufs.items():
            if view.numel():
                assert not bool((view == (FILL_I if buf.dtype == torch.int32 else FILL)).all()), f"{k} was not written"
    return {k: v.cpu().clone() for k, v in o.items()}


def _run_fused(hip, batch, **opts):
    """the fused kernel on the same batch -> xyz, steps, status"""
    plan, x = batch.plan("cuda"), batch.xyz.to("cuda")
    B, Cc = batch.B, x.shape[1]
    out = torch.empty_like(x)
    e, gm = torch.zeros(B, Cc, device="cuda"), torch.zeros(B, Cc, device="cuda")
    st, ss = torch.zeros(B, Cc, dtype=torch.int32, device="cuda"), torch.zeros(B, Cc, dtype=torch.int32, device="cuda")
    hip.relax_fire(plan, x, [k.to("cuda") for k in batch.ks], [None if q is None else q.to("cuda") for q in batch.eqs], batch.n_per, False,
                   batch.nonbonded().to("cuda"), {**RELAX_DEFAULTS, **opts}, out, e, gm, st, ss, atom_counts_host=batch.counts)
    torch.cuda.synchronize()
    return {"xyz": out.cpu(), "steps": st.cpu(), "status": ss.cpu()}


def _same_bits(a, b, what, keys=OUTS):
    for k in keys:
        assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                           b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), f"{what}: {k} differs"


def _rows_of(out, batch, b):
    """molecule b's part of every output"""
    p0, p1 = int(batch.ptr[b]), int(batch.ptr[b + 1])
    return {"xyz": out["xyz"][p0:p1], "grad": out["grad"][p0:p1], "terms": out["terms"][:, b], **{k: out[k][b] for k in ("energy", "gmax", "steps", "status")}}


def _single(batch):
    return torch.tensor([n == 1 for n in batch.counts])


def _dist(batch, x, x64):
    """(B, C): the farthest atom of every (molecule, conformation)"""
    return torch.stack([(x.double() - x64)[int(batch.ptr[k]):int(batch.ptr[k + 1])].norm(dim=-1).max(0).values for k in range(batch.B)])


def _traj_gate(name, b, got_xyz, x64, x32, ok, what):
    one = _single(b)[:, None].expand_as(ok)
    dg, dr = _dist(b, got_xyz, x64), _dist(b, x32, x64)
    ratio = ((dg - ULP_X).clamp_min(0) / dr.clamp_min(1e-300))[ok & ~one]
    print(f"{name} {what}: max |x_gpu - x_f64| {float(dg[ok].max()):.3e}, |x_f32 - x_f64| {float(dr[ok].max()):.3e}, "
          f"largest (|gpu| - 2^-20) / |f32| = {float(ratio.max()) if ratio.numel() else 0.0:.3f} over {int(ok.sum())} of {ok.numel()} conformations")
    assert bool(torch.isfinite(got_xyz).all())
    bad = ok & (dg > TRAJ_FACTOR * dr + ULP_X)
    assert not bool(bad.any()), f"{name} {what}: {int(bad.sum())} conformations outside {TRAJ_FACTOR} x fp32 + 2^-20: gpu {dg[bad].tolist()} fp32 {dr[bad].tolist()}"


# ------------------------------------------------------------------------------------------------ 1. forces
@pytest.mark.parametrize("name", rs.TRAJ_CASES)
def test_forces_at_step_zero(hip, name):
    """max_steps = 0: the coordinates come back bit for bit; energy, the six terms and the gradient pass the calibrated gate against
    float64; gmax is the largest gradient norm; the six terms are the bits of mm_energy_fwd and NonbondedBatch.evaluate"""
    b = rs.case(name)
    r64, r32 = rs.forces_of(name, torch.float64), rs.forces_of(name, torch.float32)
    got = _run(hip, b, max_steps=0, tolerance=0.0)
    assert torch.equal(got["xyz"].view(torch.int32), b.xyz.view(torch.int32)), "xyz_out differs from the input"
    one = _single(b)[:, None].expand_as(got["status"])
    assert bool((got["steps"] == 0).all()) and torch.equal(got["status"], one.int())          # (a single atom: gmax = 0 <= 0, converged)
    rr.gate_forces(got["energy"], got["terms"], got["grad"], r64, r32, name)
    want_gmax = torch.stack([got["grad"][int(b.ptr[k]):int(b.ptr[k + 1])].double().norm(dim=-1).max(0).values for k in range(b.B)])
    assert bool(((got["gmax"].double() - want_gmax).abs() <= 4 * kr.U32 * want_gmax).all()), "gmax is not the largest gradient norm"
    plan, x = b.plan("cuda"), b.xyz.to("cuda")
    ks, eqs = [k.to("cuda") for k in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    Cc = x.shape[1]
    e, t = torch.zeros(b.B, Cc, device="cuda"), torch.zeros(4, b.B, Cc, device="cuda")
    hip.mm_energy_fwd(plan, x, ks, eqs, b.n_per, False, e, t)
    _, _, nt = b.nonbonded().to("cuda").evaluate(x, terms=True, gradient=False)
    want = torch.cat([t, nt]).cpu()
    assert torch.equal(got["terms"].view(torch.int32), want.view(torch.int32)), "the six terms are not the bits of the energy kernels"


# ------------------------------------------------------------------------------------------------ 2. trajectories
TRAJ = [(n, s) for n in rs.TRAJ_CASES for s in rr.TRAJ_STEPS]


@pytest.mark.parametrize("name,max_steps", TRAJ, ids=[f"{n}-{s}steps" for n, s in TRAJ])
def test_trajectory(hip, name, max_steps):
    """tolerance = 0: every item runs exactly max_steps steps; a conformation that keeps the branch margin ends within
    TRAJ_FACTOR x the fp32 restatement's distance to float64 + one ulp of a coordinate"""
    b = rs.case(name)
    x64, x32 = rs.trajectory(name, torch.float64)["snap"][max_steps], rs.trajectory(name, torch.float32)["snap"][max_steps]
    ok = rs.margin_ok(name, max_steps)
    got = _run(hip, b, max_steps=max_steps, tolerance=0.0)
    one = _single(b)[:, None].expand_as(got["status"])
    assert torch.equal(got["steps"], torch.where(one, 0, max_steps).int()) and torch.equal(got["status"], one.int())
    _traj_gate(name, b, got["xyz"], x64, x32, ok, f"{max_steps} steps")


# ------------------------------------------------------------------------------------------------ 3. the two paths
@pytest.mark.parametrize("name", ["s65_C3", "mixed"])
def test_the_two_paths_agree(hip, name):
    """relax_steps and relax_fire: the same steps and status, both within the trajectory gate of float64 (their bits differ: they add in
    different orders)"""
    steps = max(rr.TRAJ_STEPS)
    if name == "mixed":
        b, ok = rr.case(name), rr.margin_ok(name, steps)
        x64, x32 = rr.trajectory(name, torch.float64)["snap"][steps], rr.trajectory(name, torch.float32)["snap"][steps]
    else:
        b, ok = rs.case(name), rs.margin_ok(name, steps)
        x64, x32 = rs.trajectory(name, torch.float64)["snap"][steps], rs.trajectory(name, torch.float32)["snap"][steps]
    a, f = _run(hip, b, max_steps=steps, tolerance=0.0), _run_fused(hip, b, max_steps=steps, tolerance=0.0)
    assert torch.equal(a["steps"], f["steps"]) and torch.equal(a["status"], f["status"])
    _traj_gate(name, b, a["xyz"], x64, x32, ok, "stepwise")
    _traj_gate(name, b, f["xyz"], x64, x32, ok, "fused")


# ------------------------------------------------------------------------------------------------ 4. bits
def test_two_runs_and_every_chunk_size_give_the_same_bits(hip):
    """check_every = 7 does not divide 40 and 64 exceeds it: the outputs do not depend on how the steps are dealt out to run calls"""
    b = rs.case(rs.MIXED)
    a = _run(hip, b, max_steps=40, tolerance=0.0)
    _same_bits(a, _run(hip, b, max_steps=40, tolerance=0.0), "two runs")
    for ce in (1, 7, 64):
        _same_bits(a, _run(hip, b, check_every=ce, max_steps=40, tolerance=0.0), f"check_every = {ce}")
    # with the default tolerance items stop at different steps: steps enqueued after an item stopped do not touch it
    c = _run(hip, b, check_every=1, max_steps=120)
    for ce in (7, 64, 200):
        _same_bits(c, _run(hip, b, check_every=ce, max_steps=120), f"default tolerance, check_every = {ce}")


@pytest.mark.parametrize("max_steps", [300, 600])
def test_same_bits_whatever_the_neighbours_do(hip, max_steps):
    """the 17-atom molecule gives the same bits alone, first and last in a batch, beside a neighbour that stops at step 0 (a single atom)
    and beside the 130-atom molecule.  With the case's seed the 17-atom molecule converges after 455 to 473 steps in float64 and the
    130-atom one after 1174 to 1669, so at max_steps = 300 both are cut off together; at 600 the 17-atom molecule has converged and
    its neighbour runs on, which is asserted there."""
    mixed = rs.case(rs.MIXED)          # sizes 1, 2, 17, 130, 5, 64
    opts = dict(max_steps=max_steps)
    a = _run(hip, mixed, **opts)
    print(f"status {a['status'].tolist()} steps {a['steps'].tolist()}")
    assert not a["steps"][0].any() and bool((a["status"][0] == 1).all())
    if max_steps == 600:
        assert bool((a["status"][2] == 1).all()), (a["status"].tolist(), a["steps"].tolist())
        assert bool((a["status"][3] == 0).all()) and bool((a["steps"][3] == max_steps).all()), "the 130-atom molecule does not run on"
    alone = _rows_of(_run(hip, mixed.subset([2]), **opts), mixed.subset([2]), 0)
    for order in ([2, 0, 3], [3, 0, 2], [0, 2], [2, 3]):
        sub = mixed.subset(order)
        _same_bits(_rows_of(_run(hip, sub, **opts), sub, order.index(2)), alone, f"molecule 2 in {order}")
    _same_bits(_rows_of(a, mixed, 2), alone, "molecule 2 in the whole batch")


def test_a_molecule_of_three_blocks_gives_the_same_bits_behind_another(hip):
    """behind another molecule its blocks take other rows of the plan and of the partials"""
    b = rs.case("s129_C3")
    alone = _rows_of(_run(hip, b, max_steps=40, tolerance=0.0), b, 0)
    two = rr.Batch([rs.case("s65_C3").mols[0], b.mols[0]])
    _same_bits(_rows_of(_run(hip, two, max_steps=40, tolerance=0.0), two, 1), alone, "129 atoms behind 65")


# ------------------------------------------------------------------------------------------------ 4b. the seam to the energy kernel
# the sizes of the mixed batch at C = 3; one molecule at C = 17, whose block is dealt out in two conformation chunks, and one of two
# blocks at C = 17 (five chunks and two)
SEAM_CASES = [rs.MIXED, "s9_C17", "s65_C17"]


def _nonbonded_kernel(hip, b, x):
    """energy terms and gradient of the nonbonded term alone by the planned energy kernel -> (terms (2,B,C), grad (N,C,3)) on the CPU"""
    nb, x = b.nonbonded().to("cuda"), x.to("cuda")
    Cc = x.shape[1]
    e, te, g = torch.full((b.B, Cc), FILL, device="cuda"), torch.full((2, b.B, Cc), FILL, device="cuda"), torch.full_like(x, FILL)
    hip.nonbonded(x, nb.atom_molptr, nb.charge, nb.sigma, nb.epsilon, nb.exc_ptr, nb.exc_atom, nb.exc_qq, nb.exc_sigma, nb.exc_eps, e, te, g,
                  plan=hip.nonbonded_plan(nb.atom_molptr_host, nb.N, Cc, x.device))
    torch.cuda.synchronize()
    return te.cpu(), g.cpu()


@pytest.mark.parametrize("name", SEAM_CASES)
def test_without_bonded_tuples_the_force_has_the_bits_of_the_nonbonded_kernel(hip, name):
    """T = 0 at every level: the gradient the stepwise path holds at step zero is that of the one pair loop (csrc/nb_loop.h) and of the
    same slice reduction, so it has the BITS of `nonbonded(plan=)`'s gradient, and the four bonded terms are zero"""
    b = rs.unbonded(name)
    assert all(int(i.shape[0]) == 0 for i in b.idx)
    got = _run(hip, b, max_steps=0, tolerance=0.0)
    te, g = _nonbonded_kernel(hip, b, b.xyz)
    diff = got["grad"].view(torch.int32) != g.view(torch.int32)
    print(f"{name}: {int(diff.sum())} of {diff.numel()} gradient words differ; largest |difference| {float((got['grad'] - g).abs().max()):.3e}")
    assert not bool(diff.any()), f"{name}: the stepwise force and the energy kernel's gradient differ in {int(diff.sum())} words"
    assert not got["terms"][:4].any() and torch.equal(got["terms"][4:].view(torch.int32), te.view(torch.int32))


def test_a_conformation_that_starts_at_nan_stops_and_leaves_the_others_their_bits(hip):
    """one conformation of the 130-atom molecule starts with a NaN coordinate.  At step zero its gradient is non-finite and every other
    (molecule, conformation) has the bits of the nonbonded kernel at the same coordinates; then it stops with status 2, the force
    launches of the steps that follow mask it (it is neither loaded nor asked for a verdict), and after three steps every other
    conformation has the bits it has without the NaN"""
    clean = rs.unbonded(rs.MIXED)
    M, cbad = 3, 1
    p0, p1 = int(clean.ptr[M]), int(clean.ptr[M + 1])
    x = clean.xyz.clone()
    x[p0 + 70, cbad, 1] = float("nan")
    bad = rr.Batch.from_tables(clean.counts, clean.idx, clean.mol_ptr, clean.ks, clean.eqs, clean.n_per, clean.params, x)
    keep = torch.ones(clean.N, x.shape[1], dtype=torch.bool)
    keep[p0:p1, cbad] = False
    item = torch.ones(clean.B, x.shape[1], dtype=torch.bool)
    item[M, cbad] = False
    got0 = _run(hip, bad, max_steps=0, tolerance=0.0)
    _, g = _nonbonded_kernel(hip, bad, x)
    assert torch.equal(got0["grad"].view(torch.int32)[keep], g.view(torch.int32)[keep]), "step zero: the other conformations' gradient"
    assert int(got0["status"][M, cbad]) == 2 and bool(torch.isinf(got0["gmax"][M, cbad]))
    a, c = _run(hip, bad, max_steps=3, tolerance=0.0), _run(hip, clean, max_steps=3, tolerance=0.0)
    assert int(a["status"][M, cbad]) == 2 and int(a["steps"][M, cbad]) == 0
    assert torch.equal(a["xyz"][p0:p1, cbad].view(torch.int32), x[p0:p1, cbad].view(torch.int32)), "status 2 returns the coordinates it holds"
    for k in ("xyz", "grad"):
        assert torch.equal(a[k].view(torch.int32)[keep], c[k].view(torch.int32)[keep]), f"{k} of the other conformations"
    for k in ("energy", "gmax", "steps", "status"):
        va, vc = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (a[k], c[k]))
        assert torch.equal(va[item], vc[item]), f"{k} of the other conformations"
    assert torch.equal(a["terms"].view(torch.int32)[:, item], c["terms"].view(torch.int32)[:, item]), "terms of the other conformations"
    assert bool((a["steps"][M][item[M]] == 3).all()), "the molecule's other conformations did not run on"


# ------------------------------------------------------------------------------------------------ 5. convergence
@pytest.mark.parametrize("name", rs.CONV_CASES)
def test_convergence_with_the_defaults(hip, name):
    b = rs.case(name)
    got = _run(hip, b, max_steps=rs.CONV_MAX_STEPS)
    conv = got["status"] == 1
    assert bool(conv.any()) and bool(((got["status"] == 0) | conv).all()), got["status"].tolist()
    assert bool((got["steps"] <= rs.CONV_MAX_STEPS).all()) and bool((got["steps"][got["status"] == 0] == rs.CONV_MAX_STEPS).all())
    r64, r32 = rr.forces(b, got["xyz"], torch.float64), rr.forces(b, got["xyz"], torch.float32)
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
    e0 = rs.forces_of(name, torch.float64)["E"]
    assert bool((r64["E"] <= e0)[conv].all()), "the float64 energy went up"


# ------------------------------------------------------------------------------------------------ 6. edges
def test_a_single_atom_and_an_empty_molecule_between_two_others(hip):
    nine, five = rr.case("n9_C3").mols[0], rr.case("mixed").mols[4]
    one = rr.case("n1_C3").mols[0]
    b = rr.Batch([nine, one, rr.gen_molecule(0, 3, np.random.default_rng(0)), five])
    got = _run(hip, b, max_steps=30)
    # the molecule without atoms: nothing written
    assert bool((got["energy"][2] == FILL).all()) and bool((got["gmax"][2] == FILL).all()) and bool((got["terms"][:, 2] == FILL).all())
    assert bool((got["steps"][2] == FILL_I).all()) and bool((got["status"][2] == FILL_I).all())
    # the single atom: converged at step 0 where it was
    assert bool((got["status"][1] == 1).all()) and not got["steps"][1].any()
    assert torch.equal(got["xyz"][9].view(torch.int32), torch.from_numpy(one["xyz"][0]).view(torch.int32))
    assert not got["energy"][1].any() and not got["gmax"][1].any() and not got["grad"][9].any()
    for k, m in ((0, nine), (3, five)):
        alone = rr.Batch([m])
        _same_bits(_rows_of(got, b, k), _rows_of(_run(hip, alone, max_steps=30), alone, 0), f"molecule {k} beside an empty one")


def test_no_table_equals_a_table_of_zero_charge_and_epsilon(hip):
    b = rs.case("s65_C3")
    none, zero = _run(hip, b, nb=None, max_steps=40, tolerance=0.0), _run(hip, b, nb="zero", max_steps=40, tolerance=0.0)
    x64 = rr.fire_ref(b, torch.float64, False, tolerance=0.0, max_steps=40)["xyz"]
    x32 = rr.fire_ref(b, torch.float32, False, tolerance=0.0, max_steps=40)["xyz"].double()
    dr = (x32 - x64).norm(dim=-1).max(0).values
    for what, o in (("nb = None", none), ("zero table", zero)):
        assert bool(((o["xyz"].double() - x64).norm(dim=-1).max(0).values <= TRAJ_FACTOR * dr + ULP_X).all()), what
    assert bool(((none["xyz"].double() - zero["xyz"].double()).norm(dim=-1).max(0).values <= TRAJ_FACTOR * dr + ULP_X).all())
    assert not none["terms"][4:].any() and not zero["terms"][4:].any()
    assert torch.equal(none["steps"], zero["steps"]) and torch.equal(none["status"], zero["status"])


def _with_coincident(batch, mol, i, j):
    mols = [dict(m) for m in batch.mols]
    x = mols[mol]["xyz"].copy()
    x[j] = x[i]
    mols[mol]["xyz"] = x
    return rr.Batch(mols)


def test_coincident_atoms(hip):
    base = rs.case(rs.MIXED)
    M = 3                                                        # the 130-atom molecule: atoms 0 and 129 lie in its first and third i-block
    p = base.params[M]
    pairs = {tuple(q) for q in p.exception_idx.tolist()}
    assert (0, 129) not in pairs and (129, 0) not in pairs          # they interact in full
    plain = _run(hip, base, max_steps=50)
    moved = _with_coincident(base, M, 0, 129)
    hit = _run(hip, moved, max_steps=50)
    assert bool((hit["status"][M] == 2).all()) and not hit["steps"][M].any() and bool(torch.isinf(hit["gmax"][M]).all())
    for k in (0, 1, 2, 4, 5):          # the other molecules: unaffected, bit for bit
        _same_bits(_rows_of(hit, base, k), _rows_of(plain, base, k), f"molecule {k} beside a non-finite one")
    p0 = int(base.ptr[M])
    assert torch.equal(hit["xyz"][p0:p0 + 130].view(torch.int32), moved.xyz[p0:p0 + 130].view(torch.int32)), "status 2 returns the coordinates it holds"
    # two EXCLUDED atoms on one point, in different i-blocks, relax normally
    excl = [(int(i), int(j)) for (i, j), q, e in zip(p.exception_idx.tolist(), p.exception_chargeprod, p.exception_epsilon)
            if q == 0 and e == 0 and min(i, j) < 64 <= max(i, j)]
    assert excl, "no exclusion crosses the first i-block's edge"
    i, j = excl[0]
    ex = _with_coincident(base, M, i, j)
    ok = _run(hip, ex, max_steps=50)
    assert bool((ok["status"][M] != 2).all()) and bool((ok["steps"][M] == 50).all()) and all(bool(torch.isfinite(ok[k][M]).all()) for k in ("energy", "gmax"))
    assert bool(torch.isfinite(ok["xyz"]).all())
    e_in, e_out = rr.forces(ex, ex.xyz)["E"][M], rr.forces(ex, ok["xyz"])["E"][M]
    assert bool((e_out < e_in).all()), (e_in.tolist(), e_out.tolist())


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_bad_options_and_a_short_workspace_are_refused(hip):
    from grappa_amd.backend import GrappaHipError
    b = rr.case("n9_C1")
    for bad in ({"max_steps": MAX_STEPS_CAP + 1}, {"max_steps": -1}, {"tolerance": -1.0}, {"dt_start": 0.0}, {"dt_max": -1.0}, {"max_disp": 0.0},
                {"dt_start": float("nan")}, {"n_min": -1}):
        with pytest.raises(GrappaHipError, match="GRAPPA_ERR_ARG"):
            _run(hip, b, expect_written=False, **bad)
    _run(hip, b, max_steps=MAX_STEPS_CAP, tolerance=1e6)          # the cap itself is accepted (and this call stops at step 0)
    before = hip.lib.grappa_launch_count(0)
    with pytest.raises(GrappaHipError, match="GRAPPA_ERR_WORKSPACE"):
        _run(hip, b, expect_written=False, short=1, max_steps=5)          # (the guards check that the workspace itself stayed untouched)
    assert hip.lib.grappa_launch_count(0) == before, "a call with a short workspace launched something"
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="check_every"):
            _run(hip, b, expect_written=False, check_every=bad)
    with pytest.raises(ValueError, match="atom_counts_host"):
        plan, x = b.plan("cuda"), b.xyz.to("cuda")
        z = lambda dt: torch.zeros(1, 1, dtype=dt, device="cuda")      # noqa: E731
        hip.relax_steps(plan, x, [k.to("cuda") for k in b.ks], [None if q is None else q.to("cuda") for q in b.eqs], b.n_per, False, None,
                        dict(RELAX_DEFAULTS), torch.empty_like(x), z(torch.float32), z(torch.float32), z(torch.int32), z(torch.int32))
    # the C ABI itself: n_steps < 1
    import ctypes as C
    from grappa_amd import _lib
    plan, x = b.plan("cuda"), b.xyz.to("cuda")
    ks, eqs = [k.to("cuda") for k in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    d = hip._mm_desc(plan, x, ks, eqs, b.n_per, False)
    o = _lib.RelaxOpts(**{k: (int(v) if k in ("max_steps", "n_min") else float(v)) for k, v in RELAX_DEFAULTS.items()})
    table, n_items, nblk, _ = hip.nonbonded_plan(torch.tensor([0, 9], dtype=torch.int32), 9, 1, x.device)
    wbuf, ws = _workspace(hip, b, 1)
    nrun = torch.zeros(1, dtype=torch.int32, device="cuda")
    for n_steps in (0, -1):
        rc = hip.lib.grappa_relax_steps_run_f32(hip._stream(), C.byref(d), None, C.byref(o), table.data_ptr(), n_items, nblk, ws.data_ptr(), ws.numel(),
                                                n_steps, nrun.data_ptr())
        assert rc == -1
    assert hip.lib.grappa_relax_steps_init_f32(hip._stream(), C.byref(d), None, C.byref(o), table.data_ptr(), n_items, nblk, ws.data_ptr(), ws.numel(),
                                               None) == -1
    torch.cuda.synchronize()
    assert bool((wbuf == FILL_B).all()), "a refused call wrote to the workspace"


# ------------------------------------------------------------------------------------------------ 8. launches
def test_four_launches_per_step_whatever_the_shape(hip):
    added = {}
    for name in ("s9_65_C17", "s513_C1"):
        b = rs.case(name)
        n = []
        for steps in (0, 10):
            before = hip.lib.grappa_launch_count(0)
            _run(hip, b, check_every=64, max_steps=steps, tolerance=0.0)
            n.append(hip.lib.grappa_launch_count(0) - before)
        added[name] = n[1] - n[0]          # init and finish launch the same with and without steps in between
    print(f"launches added by a run of 10 steps: {added}")
    assert added["s9_65_C17"] == added["s513_C1"] and 0 < added["s513_C1"] <= 40, added


# ------------------------------------------------------------------------------------------------ 9. front ends
def _parameters(mol):
    from grappa_amd.parameters import Parameters
    ids = np.arange(mol["n"])
    k3, k4 = mol["ks"][2].astype(np.float64), mol["ks"][3].astype(np.float64)
    return Parameters(atoms=ids, bonds=mol["idx"][0], bond_k=mol["ks"][0], bond_eq=mol["eqs"][0], angles=mol["idx"][1], angle_k=mol["ks"][1],
                      angle_eq=mol["eqs"][1], propers=mol["idx"][2], proper_ks=np.abs(k3), proper_phases=np.where(k3 >= 0, 0.0, np.pi),
                      impropers=mol["idx"][3], improper_ks=np.abs(k4), improper_phases=np.where(k4 >= 0, 0.0, np.pi))


def test_numpy_and_graph_front_ends_give_the_same_bits(hip):
    from grappa_amd import backend
    from grappa_amd.nonbonded import NonbondedBatch
    from grappa_amd.relax import graph_from_parameters, relax, relax_graph
    old = backend._BACKEND
    backend.set_backend(hip)
    try:
        mol = rs.case("s65_C3").mols[0]
        p, xyz = _parameters(mol), mol["xyz"].transpose(1, 0, 2)
        r = relax(p, xyz, mol["nb"], stepwise=True, max_steps=200)
        g = graph_from_parameters(p, xyz).to("cuda")
        rg = relax_graph(g, NonbondedBatch([mol["nb"]]).to("cuda"), stepwise=True, max_steps=200, check_every=9)
        assert r.xyz.shape == xyz.shape and rg.xyz.shape == (65, 3, 3) and bool((r.status != 2).all())
        assert np.array_equal(r.xyz.astype(np.float32), rg.xyz.cpu().numpy().transpose(1, 0, 2))
        assert np.array_equal(r.energy.astype(np.float32), rg.energy.cpu().numpy()[0]) and np.array_equal(r.steps, rg.steps.cpu().numpy()[0])
        assert np.array_equal(r.gradient_max.astype(np.float32), rg.gradient_max.cpu().numpy()[0]) and np.array_equal(r.status, rg.status.cpu().numpy()[0])
    finally:
        backend.set_backend(old)


def test_auto_relaxes_a_molecule_above_the_fused_limit(hip):
    from grappa_amd import backend
    from grappa_amd.relax import relax
    old = backend._BACKEND
    backend.set_backend(hip)
    try:
        b = rs.case("s513_C1")
        mol = b.mols[0]
        p, xyz = _parameters(mol), mol["xyz"].transpose(1, 0, 2)
        with pytest.raises(ValueError, match="above the limit"):
            relax(p, xyz, mol["nb"])
        r = relax(p, xyz, mol["nb"], stepwise="auto")
        assert r.xyz.shape == xyz.shape and bool(np.isfinite(r.xyz).all()) and bool((r.status != 2).all())
        e0 = rs.forces_of("s513_C1", torch.float64)["E"][0]
        e1 = rr.forces(b, torch.from_numpy(np.ascontiguousarray(r.xyz.transpose(1, 0, 2))))["E"][0]
        print(f"relax(stepwise='auto') on 513 atoms: E {e0.tolist()} -> {e1.tolist()} in {r.steps.tolist()} steps, status {r.status.tolist()}")
        assert bool((e1 < e0).all())
    finally:
        backend.set_backend(old)
