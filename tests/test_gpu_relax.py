"""GPU: the fused FIRE minimiser (csrc/relax.hip through HipBackend.relax_fire and grappa_amd/relax.py) against the float64
restatement of tests/relax_refs.py, inside sentinel-guarded output buffers.

Gates.  Forces, energies (1): the project's calibrated gate |gpu - f64| <= 2 |fp32 restatement - f64| + 64 u32 scale, with the scales
of the MM-energy and the nonbonded GPU tests added.  Trajectories (2): for every conformation that keeps the branch margin
(relax_refs.BRANCH_MARGIN), max_atoms |x_gpu - x_f64| <= TRAJ_FACTOR max_atoms |x_f32 - x_f64| + 2^-20 A: 2^-20 A is one ulp of a
coordinate below 16 A, and the factor is twice the elementwise gate's because the error accumulates over steps in another summation
order.  The observed ratio is printed per case; the largest seen on an MI355X was 0.98 (the molecule at the size limit), so the
factor 4 stands.

Convergence (3), a deviation from the issue: it bounds the float64 gmax at xyz_out by tolerance + 64 u32 max_i abs_f_i and gates the
reported gmax on the same scale.  Near a minimum that floor is 2e-7 to 9e-5 kcal/mol/A, while fp32 cannot hold a bond's force
k (r - eq) better than u32 k r = 4e-5 to 6e-5: on an MI355X |gmax_gpu - gmax_f64| was 3e-7 to 3.1e-5 and the fp32 restatement's own
distance 3e-7 to 4.3e-5 (2e-6 to 1.1e-4 over its gradient rows).  The test therefore adds to the issue's floor twice the fp32
restatement's distance to float64 at xyz_out (its farthest gradient row or its gmax, whichever is larger) and 2 u32 max_i sum_bonds k r
(relax_refs.bond_rounding: the square root and the sum under it), 1e-4 to 4e-4 in all: at most 0.2 % of the tolerance.  Each case
prints the figures and whether the issue's floor alone would have held."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_utils as gu
import kernel_refs as kr
import relax_refs as rr
from grappa_amd.relax import MAX_STEPS_CAP, RELAX_DEFAULTS

pytestmark = pytest.mark.gpu

FILL, FILL_I = 1024.0, 12345       # sentinels around (and, before the call, inside) every output buffer
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


def _run(hip, batch, nb="full", counts=False, expect_written=True, **opts):
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
    ks = [k.to("cuda") for k in batch.ks]
    eqs = [None if q is None else q.to("cuda") for q in batch.eqs]
    hip.relax_fire(plan, x, ks, eqs, batch.n_per, False, dnb, {**RELAX_DEFAULTS, **opts}, o["xyz"], o["energy"], o["gmax"], o["steps"], o["status"],
                   term_energy=o["terms"], grad=o["grad"], atom_counts_host=batch.counts if counts else None)
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        fill = FILL_I if buf.dtype == torch.int32 else FILL
        assert bool((buf[:64] == fill).all()) and bool((buf[-64:] == fill).all()), f"written outside {k}"
        if expect_written and view.numel():
            assert not bool((view == fill).all()), f"{k} was not written"
    return {k: v.cpu().clone() for k, v in o.items()}


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


# ------------------------------------------------------------------------------------------------ 1. forces
@pytest.mark.parametrize("name", sorted(rr.case_table()))
def test_forces_at_step_zero(hip, name):
    """max_steps = 0: the coordinates come back bit for bit; energy, the six terms and the gradient pass the calibrated gate against
    float64 and agree with HipBackend's own MM and nonbonded kernels within the same gate"""
    b = rr.case(name)
    r64, r32 = rr.forces_of(name, torch.float64), rr.forces_of(name, torch.float32)
    got = _run(hip, b, max_steps=0, tolerance=0.0)
    assert torch.equal(got["xyz"].view(torch.int32), b.xyz.view(torch.int32)), "xyz_out differs from the input"
    one = _single(b)[:, None].expand_as(got["status"])
    assert bool((got["steps"] == 0).all()) and torch.equal(got["status"], one.int())          # (a single atom: gmax = 0 <= 0, converged)
    rr.gate_forces(got["energy"], got["terms"], got["grad"], r64, r32, name)
    want_gmax = torch.stack([got["grad"][int(b.ptr[k]):int(b.ptr[k + 1])].double().norm(dim=-1).max(0).values for k in range(b.B)])
    assert bool(((got["gmax"].double() - want_gmax).abs() <= 4 * kr.U32 * want_gmax).all()), "gmax is not the largest gradient norm"
    # the existing kernels on the same input
    plan, x = b.plan("cuda"), b.xyz.to("cuda")
    ks, eqs = [k.to("cuda") for k in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    Cc = x.shape[1]
    e, t, g = torch.zeros(b.B, Cc, device="cuda"), torch.zeros(4, b.B, Cc, device="cuda"), torch.zeros(b.N, Cc, 3, device="cuda")
    hip.mm_energy_fwd(plan, x, ks, eqs, b.n_per, False, e, t)
    hip.mm_gradient_fwd(plan, x, ks, eqs, b.n_per, g)
    ne, ng, nt = b.nonbonded().to("cuda").evaluate(x, terms=True)
    other = dict(E=(e.double() + ne.double()).cpu(), G=(g.double() + ng.double()).cpu(), terms=torch.cat([t, nt]).double().cpu(),
                 abs_e=r64["abs_e"], abs_terms=r64["abs_terms"], abs_f=r64["abs_f"])
    close32 = {k: (r32[k].double() - r64[k] + other[k]) for k in ("E", "G", "terms")}          # the same calibration distance, around `other`
    rr.gate_forces(got["energy"], got["terms"], got["grad"], other, close32, f"{name} against mm_energy / mm_gradient / nonbonded")


# ------------------------------------------------------------------------------------------------ 2. trajectories
TRAJ = [(n, s) for n in rr.TRAJ_CASES for s in rr.TRAJ_STEPS] + [("max", 5)]


@pytest.mark.parametrize("name,max_steps", TRAJ, ids=[f"{n}-{s}steps" for n, s in TRAJ])
def test_trajectory(hip, name, max_steps):
    """tolerance = 0: every item runs exactly max_steps steps; a conformation that keeps the branch margin ends within
    TRAJ_FACTOR x the fp32 restatement's distance to float64 + one ulp of a coordinate"""
    b = rr.case(name)
    total = 5 if name == "max" else max(rr.TRAJ_STEPS)
    x64, x32 = rr.trajectory(name, torch.float64, total)["snap"][max_steps], rr.trajectory(name, torch.float32, total)["snap"][max_steps]
    ok = rr.margin_ok(name, max_steps, total)
    got = _run(hip, b, max_steps=max_steps, tolerance=0.0)
    one = _single(b)[:, None].expand_as(got["status"])
    assert torch.equal(got["steps"], torch.where(one, 0, max_steps).int()) and torch.equal(got["status"], one.int())
    dist = lambda x: torch.stack([(x.double() - x64)[int(b.ptr[k]):int(b.ptr[k + 1])].norm(dim=-1).max(0).values for k in range(b.B)])      # noqa: E731
    dg, dr = dist(got["xyz"]), dist(x32)
    ratio = ((dg - ULP_X).clamp_min(0) / dr.clamp_min(1e-300))[ok & ~one]
    print(f"{name} {max_steps} steps: max |x_gpu - x_f64| {float(dg[ok].max()):.3e}, |x_f32 - x_f64| {float(dr[ok].max()):.3e}, "
          f"largest (|gpu| - 2^-20) / |f32| = {float(ratio.max()) if ratio.numel() else 0.0:.3f} over {int(ok.sum())} of {ok.numel()} conformations")
    assert bool(torch.isfinite(got["xyz"]).all())
    bad = ok & (dg > TRAJ_FACTOR * dr + ULP_X)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} conformations outside {TRAJ_FACTOR} x fp32 + 2^-20: gpu {dg[bad].tolist()} fp32 {dr[bad].tolist()}"


# ------------------------------------------------------------------------------------------------ 3. convergence
@pytest.mark.parametrize("name", rr.CONV_CASES)
def test_convergence_with_the_defaults(hip, name):
    b = rr.case(name)
    got = _run(hip, b)
    conv = got["status"] == 1
    assert bool(conv.any()) and bool(((got["status"] == 0) | conv).all()), got["status"].tolist()
    assert bool((got["steps"] <= RELAX_DEFAULTS["max_steps"]).all()) and bool((got["steps"][got["status"] == 0] == RELAX_DEFAULTS["max_steps"]).all())
    r64, r32 = rr.forces(b, got["xyz"], torch.float64), rr.forces(b, got["xyz"], torch.float32)
    per_mol = lambda t: torch.stack([t[int(b.ptr[k]):int(b.ptr[k + 1])].max(0).values for k in range(b.B)])      # noqa: E731
    gmax64, gmax32 = per_mol(r64["G"].norm(dim=-1)), per_mol(r32["G"].double().norm(dim=-1))
    # the issue's floor 64 u32 max_i abs_f_i (abs_f: the scales of the MM and the nonbonded tests, added) + the calibration: twice the
    # fp32 restatement's own distance to float64 at xyz_out (its farthest gradient row, or its gmax) + two roundings of the bond lengths
    floor = rr.C_GATE * kr.U32 * per_mol(r64["abs_f"])
    cal = torch.maximum(per_mol((r32["G"].double() - r64["G"]).norm(dim=-1)), (gmax32 - gmax64).abs())
    bound = floor + 2 * cal + 2 * kr.U32 * per_mol(rr.bond_rounding(b, got["xyz"]))
    fmt = lambda t: [f"{v:.2e}" for v in t.flatten().tolist()]      # noqa: E731
    print(f"{name}: steps {got['steps'].flatten().tolist()} status {got['status'].flatten().tolist()}\n  gmax gpu - f64 {fmt(got['gmax'].double() - gmax64)}"
          f"\n  f64 gmax - tolerance {fmt(gmax64 - RELAX_DEFAULTS['tolerance'])}\n  fp32 restatement - f64 {fmt(cal)}\n  issue's floor {fmt(floor)}"
          f"\n  bound {fmt(bound)}; f64 gmax within tolerance + the issue's floor alone: {bool((gmax64 <= RELAX_DEFAULTS['tolerance'] + floor)[conv].all())}")
    assert bool((gmax64 <= RELAX_DEFAULTS["tolerance"] + bound)[conv].all()), "the float64 gradient at xyz_out is above the tolerance"
    rr.gate_forces(got["energy"], None, None, r64, r32, f"{name} at xyz_out")
    assert bool(((got["gmax"].double() - gmax64).abs() <= bound).all()), "gmax at xyz_out"
    e0 = rr.forces_of(name, torch.float64)["E"]
    assert bool((r64["E"] <= e0)[conv].all()), "the float64 energy went up"


# ------------------------------------------------------------------------------------------------ 4. known answers
def test_bonded_diatomic_ends_at_its_equilibrium_length(hip):
    b = rr.case("n2_C3")
    got = _run(hip, b, nb=None)
    assert bool((got["status"] == 1).all())
    r = (got["xyz"][0] - got["xyz"][1]).double().norm(dim=-1)
    k, eq = float(b.ks[0][0]), float(b.eqs[0][0])
    assert bool(((r - eq).abs() <= RELAX_DEFAULTS["tolerance"] / k + ULP_X).all()), (r.tolist(), eq)
    assert not got["terms"][4:].any()


def test_no_table_equals_a_table_of_zero_charge_and_epsilon(hip):
    b = rr.case("n9_C3")
    none, zero = _run(hip, b, nb=None, max_steps=40, tolerance=0.0), _run(hip, b, nb="zero", max_steps=40, tolerance=0.0)
    x64 = rr.fire_ref(b, torch.float64, False, tolerance=0.0, max_steps=40)["xyz"]
    x32 = rr.fire_ref(b, torch.float32, False, tolerance=0.0, max_steps=40)["xyz"].double()
    dr = (x32 - x64).norm(dim=-1).max(0).values
    for what, o in (("nb = None", none), ("zero table", zero)):
        assert bool(((o["xyz"].double() - x64).norm(dim=-1).max(0).values <= TRAJ_FACTOR * dr + ULP_X).all()), what
    assert bool(((none["xyz"].double() - zero["xyz"].double()).norm(dim=-1).max(0).values <= TRAJ_FACTOR * dr + ULP_X).all())
    assert not none["terms"][4:].any() and not zero["terms"][4:].any()


@pytest.mark.parametrize("name", ["n1_C1", "n1_C3"])
def test_single_atom(hip, name):
    b = rr.case(name)
    got = _run(hip, b)
    assert bool((got["status"] == 1).all()) and not got["steps"].any() and torch.equal(got["xyz"].view(torch.int32), b.xyz.view(torch.int32))
    assert not got["energy"].any() and not got["gmax"].any() and not got["grad"].any()


def test_a_molecule_without_atoms_writes_nothing(hip):
    nine, five = rr.case("n9_C3").mols[0], rr.case("mixed").mols[4]
    b = rr.Batch([nine, rr.gen_molecule(0, 3, np.random.default_rng(0)), five])
    got = _run(hip, b, max_steps=30)
    assert bool((got["energy"][1] == FILL).all()) and bool((got["gmax"][1] == FILL).all()) and bool((got["terms"][:, 1] == FILL).all())
    assert bool((got["steps"][1] == FILL_I).all()) and bool((got["status"][1] == FILL_I).all())
    for k, m in ((0, nine), (2, five)):
        alone = rr.Batch([m])
        _same_bits(_rows_of(got, b, k), _rows_of(_run(hip, alone, max_steps=30), alone, 0), f"molecule {k} beside an empty one")


# ------------------------------------------------------------------------------------------------ 5. bits
def test_same_input_same_bits_whatever_the_neighbours_do(hip):
    """two runs agree bit for bit, and a molecule's results are the same alone, first and last in a batch, beside a neighbour that
    stops at step 0 (a single atom) and one that runs to max_steps (65 atoms; the molecule itself converges earlier)"""
    mixed = rr.case("mixed")          # sizes 1, 2, 17, 65, 5
    opts = dict(max_steps=300)
    a, a2 = _run(hip, mixed, **opts), _run(hip, mixed, **opts)
    _same_bits(a, a2, "two runs")
    assert bool((a["status"][2] == 1).all()) and bool((a["status"][3] == 0).all()) and not a["steps"][0].any(), (a["status"].tolist(), a["steps"].tolist())
    alone = _rows_of(_run(hip, mixed.subset([2]), **opts), mixed.subset([2]), 0)
    for order in ([2, 0, 3], [3, 0, 2], [0, 2], [2, 3]):
        sub = mixed.subset(order)
        _same_bits(_rows_of(_run(hip, sub, **opts), sub, order.index(2)), alone, f"molecule 2 in {order}")
    _same_bits(_rows_of(a, mixed, 2), alone, "molecule 2 in the whole batch")


# ------------------------------------------------------------------------------------------------ 6. status 2
def _with_coincident(batch, mol, i, j):
    mols = [dict(m) for m in batch.mols]
    x = mols[mol]["xyz"].copy()
    x[j] = x[i]
    mols[mol]["xyz"] = x
    return rr.Batch(mols)


def test_coincident_atoms(hip):
    base = rr.case("mixed")
    pairs = {tuple(p) for p in base.params[2].exception_idx.tolist()}
    assert (0, 16) not in pairs and (0, 2) in pairs          # 0 and 16 interact in full; 0 and 2 (an angle's ends) are an exclusion
    plain = _run(hip, base, max_steps=50)
    hit = _run(hip, _with_coincident(base, 2, 0, 16), max_steps=50)
    assert bool((hit["status"][2] == 2).all()) and not hit["steps"][2].any() and bool(torch.isinf(hit["gmax"][2]).all())
    for k in (0, 1, 3, 4):          # the other molecules: unaffected, bit for bit
        _same_bits(_rows_of(hit, base, k), _rows_of(plain, base, k), f"molecule {k} beside a non-finite one")
    p0 = int(base.ptr[2])
    moved = _with_coincident(base, 2, 0, 16)
    assert torch.equal(hit["xyz"][p0:p0 + 17].view(torch.int32), moved.xyz[p0:p0 + 17].view(torch.int32)), "status 2 returns the coordinates it holds"
    # two EXCLUDED atoms on one point relax normally
    excl = _with_coincident(base, 2, 0, 2)
    ok = _run(hip, excl, max_steps=50)
    assert bool((ok["status"][2] != 2).all()) and bool((ok["steps"][2] == 50).all()) and all(bool(torch.isfinite(ok[k][2]).all()) for k in ("energy", "gmax"))
    assert bool(torch.isfinite(ok["xyz"]).all())
    e_in, e_out = rr.forces(excl, excl.xyz)["E"][2], rr.forces(excl, ok["xyz"])["E"][2]
    assert bool((e_out < e_in).all()), (e_in.tolist(), e_out.tolist())


# ------------------------------------------------------------------------------------------------ 7. limits
def test_a_molecule_above_the_limit_is_refused(hip):
    n = rr.max_atoms() + 1
    b = rr.Batch([rr.gen_molecule(n, 1, np.random.default_rng(5)), rr.case("n9_C1").mols[0]])
    with pytest.raises(ValueError, match="above the limit"):          # the caller knows the sizes on the host: nothing is launched
        before = hip.lib.grappa_launch_count(0)
        try:
            _run(hip, b, counts=True)
        finally:
            assert hip.lib.grappa_launch_count(0) == before
    # without host sizes the kernel marks the item: status 3 and nothing else written for it; its neighbour runs as if alone
    got = _run(hip, b, max_steps=20)
    assert got["status"].flatten().tolist() == [3, 0]
    assert bool((got["xyz"][:n] == FILL).all()) and bool((got["grad"][:n] == FILL).all()) and got["steps"][0, 0] == FILL_I
    assert got["energy"][0, 0] == FILL and got["gmax"][0, 0] == FILL and bool((got["terms"][:, 0] == FILL).all())
    nine = rr.case("n9_C1")
    _same_bits(_rows_of(got, b, 1), _rows_of(_run(hip, nine, max_steps=20), nine, 0), "the neighbour of a refused molecule")


def test_bad_options_and_pointers_are_refused(hip):
    from grappa_amd import _lib
    from grappa_amd.backend import GrappaHipError
    b = rr.case("n9_C1")
    for bad in ({"max_steps": MAX_STEPS_CAP + 1}, {"max_steps": -1}, {"tolerance": -1.0}, {"dt_start": 0.0}, {"dt_max": -1.0}, {"max_disp": 0.0},
                {"dt_start": float("nan")}, {"n_min": -1}):
        with pytest.raises(GrappaHipError, match="GRAPPA_ERR_ARG"):
            _run(hip, b, expect_written=False, **bad)
    _run(hip, b, max_steps=MAX_STEPS_CAP, tolerance=1e6)          # the cap itself is accepted (and this call stops at step 0)
    # the C ABI itself: NULL pointers and a nonbonded table of another shape
    plan, x = b.plan("cuda"), b.xyz.to("cuda")
    ks, eqs = [k.to("cuda") for k in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    d = hip._mm_desc(plan, x, ks, eqs, b.n_per, False)
    o = _lib.RelaxOpts(**{k: (int(v) if k in ("max_steps", "n_min") else float(v)) for k, v in RELAX_DEFAULTS.items()})
    out = {k: _guarded(s, t) for k, (s, t) in {"xyz": ((9, 1, 3), torch.float32), "e": ((1, 1), torch.float32), "g": ((1, 1), torch.float32),
                                                "s": ((1, 1), torch.int32), "st": ((1, 1), torch.int32)}.items()}
    ptr = {k: v[1].data_ptr() for k, v in out.items()}
    nd = _lib.NbDesc()
    nd.N, nd.C, nd.B = 9, 2, 1
    for args in ((None, C.byref(o), ptr["xyz"], ptr["e"], ptr["g"], ptr["s"], ptr["st"]), (None, None, ptr["xyz"], ptr["e"], ptr["g"], ptr["s"], ptr["st"]),
                 (None, C.byref(o), None, ptr["e"], ptr["g"], ptr["s"], ptr["st"]), (None, C.byref(o), ptr["xyz"], None, ptr["g"], ptr["s"], ptr["st"]),
                 (None, C.byref(o), ptr["xyz"], ptr["e"], None, ptr["s"], ptr["st"]), (None, C.byref(o), ptr["xyz"], ptr["e"], ptr["g"], None, ptr["st"]),
                 (None, C.byref(o), ptr["xyz"], ptr["e"], ptr["g"], ptr["s"], None), (C.byref(nd), C.byref(o), ptr["xyz"], ptr["e"], ptr["g"], ptr["s"], ptr["st"])):
        nb, op, xo, e, g, s, st = args
        rc = hip.lib.grappa_relax_fire_f32(hip._stream(), C.byref(d), nb, op, xo, e, None, None, g, s, st)
        if args[0] is None and all(a is not None for a in args[1:]):
            assert rc == 0          # the complete call is accepted
        else:
            assert rc == -1, args          # GRAPPA_ERR_ARG
    torch.cuda.synchronize()
    assert all(bool((buf[:64] == (FILL_I if buf.dtype == torch.int32 else FILL)).all()) for buf, _ in out.values())


def test_an_empty_batch_passes_every_seam_after_its_options_and_counts(hip):
    """the head the six entry families share (csrc/desc_check.h), in its observable order: with N = C = B = 0 and every output NULL a call
    returns 0 without a launch, but bad options -- and, on the stepwise paths, a negative n_items -- are refused first"""
    from grappa_amd import _lib
    lib, st = hip.lib, hip._stream()
    d = C.byref(_lib.MMDesc())          # all zero: an empty batch, every pointer NULL
    some = torch.zeros(4, dtype=torch.int32, device="cuda").data_ptr()          # (a pointer the struct checks accept; nothing reads it)
    ro = lambda **kw: C.byref(_lib.RelaxOpts(**{k: (int(v) if k in ("max_steps", "n_min") else float(v)) for k, v in {**RELAX_DEFAULTS, **kw}.items()}))      # noqa: E731
    mo = lambda **kw: C.byref(_lib.MdOpts(**{**dict(dt=0.001, temperature=300.0, friction=1.0, init_temperature=300.0, n_steps=4, save_every=0, first_step=0), **kw}))      # noqa: E731
    restr = C.byref(_lib.RelaxRestr(frozen=None, pos_k=None, dih_molptr=some, dih_atoms=some, dih_k=some, dih_target=some, R=1))
    cons = C.byref(_lib.MdCons(cluster_molptr=some, cluster_atoms=some, cluster_d=some, K=1, tolerance=1e-4, constrain_start=1))
    n7, n12 = [None] * 7, [None] * 12
    fused = {"relax_fire": lambda o: lib.grappa_relax_fire_f32(st, d, None, o, *n7),
             "relax_fire_restr": lambda o: lib.grappa_relax_fire_restr_f32(st, d, None, o, restr, *n7, some, None),      # (restraint_energy is required whatever the batch)
             "md_langevin": lambda o: lib.grappa_md_langevin_f32(st, d, None, o, *n12),
             "md_langevin_cons": lambda o: lib.grappa_md_langevin_cons_f32(st, d, None, o, cons, *n12)}
    steps = {"relax_steps_init": lambda o, ni: lib.grappa_relax_steps_init_f32(st, d, None, o, None, ni, 0, None, 0, None),
             "relax_steps_run": lambda o, ni: lib.grappa_relax_steps_run_f32(st, d, None, o, None, ni, 0, None, 0, 1, None),
             "relax_steps_finish": lambda o, ni: lib.grappa_relax_steps_finish_f32(st, d, None, o, None, ni, 0, None, 0, *n7),
             "md_steps_init": lambda o, ni: lib.grappa_md_steps_init_f32(st, d, None, o, None, None, None, None, ni, 0, None, 0),
             "md_steps_run": lambda o, ni: lib.grappa_md_steps_run_f32(st, d, None, o, None, None, None, ni, 0, None, 0, 0, 1, None, None, None),
             "md_steps_finish": lambda o, ni: lib.grappa_md_steps_finish_f32(st, d, None, o, None, ni, 0, None, 0, *[None] * 6)}
    before = lib.grappa_launch_count(0)
    for name, call in fused.items():
        good, bad = (mo(), mo(dt=0.0)) if name.startswith("md") else (ro(), ro(dt_start=0.0))
        assert call(good) == 0, f"{name}: an empty batch"
        assert call(bad) == -1, f"{name}: bad options with an empty batch"          # GRAPPA_ERR_ARG
    for name, call in steps.items():
        good, bad = (mo(), mo(dt=0.0)) if name.startswith("md") else (ro(), ro(dt_start=0.0))
        assert call(good, 0) == 0, f"{name}: an empty batch"
        assert call(bad, 0) == -1, f"{name}: bad options with an empty batch"
        assert call(good, -1) == -1, f"{name}: n_items = -1 with an empty batch"
    assert lib.grappa_launch_count(0) == before, "a call on an empty batch launched something"


# ------------------------------------------------------------------------------------------------ 8. front ends
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
        b = rr.case("n33_C3")
        mol = b.mols[0]
        p, xyz = _parameters(mol), mol["xyz"].transpose(1, 0, 2)
        r = relax(p, xyz, mol["nb"])
        g = graph_from_parameters(p, xyz).to("cuda")
        rg = relax_graph(g, NonbondedBatch([mol["nb"]]).to("cuda"))
        assert r.xyz.shape == xyz.shape and rg.xyz.shape == (33, 3, 3) and bool(r.converged.all())
        assert np.array_equal(r.xyz.astype(np.float32), rg.xyz.cpu().numpy().transpose(1, 0, 2))
        assert np.array_equal(r.energy.astype(np.float32), rg.energy.cpu().numpy()[0]) and np.array_equal(r.steps, rg.steps.cpu().numpy()[0])
        assert np.array_equal(r.gradient_max.astype(np.float32), rg.gradient_max.cpu().numpy()[0]) and np.array_equal(r.status, rg.status.cpu().numpy()[0])
        # the same molecule through the seam with the test's own incidence table: the same minimum within the convergence tolerance
        seam = _run(hip, b)
        assert bool((seam["status"] == 1).all())
        e64 = rr.forces(b, torch.from_numpy(r.xyz.transpose(1, 0, 2).copy()))["E"][0]
        assert bool((e64 <= rr.forces_of("n33_C3")["E"][0]).all())
    finally:
        backend.set_backend(old)


def test_grappa_relax_lowers_the_energy_of_a_golden_molecule(hip):
    from grappa_amd import Grappa, GrappaModel, backend
    from grappa_amd.relax import graph_from_parameters
    old = backend._BACKEND
    backend.set_backend(hip)
    try:
        fx = gu.load("ref_small_att.npz")
        model = GrappaModel(**gu.config_of(fx))
        model.load_state_dict(gu.state_dict_of(fx))
        wrapper = Grappa(model, device="cuda")
        m = gu.molecules_of(fx)[0]
        mol = gu.molecule_of(m)
        xyz = np.ascontiguousarray(m["xyz"].transpose(1, 0, 2)[:2])
        r = wrapper.relax(mol, xyz)
        assert r.xyz.shape == xyz.shape and bool(np.isfinite(r.xyz).all()) and bool((r.status != 2).all())

        def e64(x):
            g = graph_from_parameters(wrapper.predict(mol), x)
            pl = g.plan()
            ks = [g.nodes[lv].data["k"] for lv in rr.LEVELS]
            n_per = [0, 0, max(int(ks[2].shape[1]), 1), max(int(ks[3].shape[1]), 1)]
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32).transpose(1, 0, 2)))
            return kr.mm_ref64([pl.idx32[lv].long() for lv in rr.LEVELS], [pl.mol_ptr[lv] for lv in rr.LEVELS], 1, t, ks,
                               [g.nodes["n2"].data["eq"], g.nodes["n3"].data["eq"], None, None], n_per, False, torch.zeros(1, 2), torch.zeros(len(m["z"]), 2, 3))["E"][0]
        e_in, e_out = e64(xyz), e64(r.xyz)
        print(f"Grappa.relax: E {e_in.tolist()} -> {e_out.tolist()} in {r.steps.tolist()} steps, status {r.status.tolist()}")
        assert bool((e_out < e_in).all())
        assert np.allclose(r.energy, e_out.numpy(), rtol=1e-4, atol=1e-3)
    finally:
        backend.set_backend(old)
