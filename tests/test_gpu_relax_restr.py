"""GPU: the restrained fused FIRE minimiser (csrc/relax.hip through HipBackend.relax_fire(restraints=...) and grappa_amd/relax.py)
against the float64 restatement of tests/relax_restr_refs.py, inside sentinel-guarded output buffers.

Gates are those of tests/test_gpu_relax.py: the calibrated gate |gpu - f64| <= 2 |fp32 restatement - f64| + 64 u32 scale for what is
compared elementwise, TRAJ_FACTOR x the fp32 restatement's distance + 2^-20 A for trajectories of items inside the branch margin, and
test_convergence_with_the_defaults' bound (its floor, twice the fp32 calibration, the bond-rounding term) for the objective's gmax.
What the cases and these bounds rest on is decided on the CPU in tests/test_host_relax_restr.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_utils as gu
import kernel_refs as kr
import relax_refs as rr
import relax_restr_refs as rs
from grappa_amd.relax import RELAX_DEFAULTS
from grappa_amd.restraints import MAX_DIHEDRALS, RestraintBatch, Restraints

pytestmark = pytest.mark.gpu

FILL, FILL_I = 1024.0, 12345
TRAJ_FACTOR = 4
ULP_X = 2.0 ** -20
BASE = ("xyz", "energy", "gmax", "steps", "status", "terms", "grad")
OUTS = BASE + ("er", "phi")


@pytest.fixture(scope="module")
def hip():
    from grappa_amd.backend import HipBackend
    return HipBackend()


def _guarded(shape, dtype=torch.float32, guard=64):
    n = int(np.prod(shape))
    buf = torch.full((guard + n + guard,), FILL_I if dtype == torch.int32 else FILL, dtype=dtype, device="cuda")
    return buf, buf[guard:guard + n].view(*shape)


def _run(hip, batch, rb, nb=True, expect_written=True, unwritten=(), **opts):
    """one call of the seam -> dict of CPU tensors (OUTS; without rb: BASE, the unrestrained call); asserts the guards"""
    plan = batch.plan("cuda")
    dnb = batch.nonbonded().to("cuda") if nb else None
    x = batch.xyz.to("cuda")
    N, Cc, B = batch.N, x.shape[1], batch.B
    shapes = {"xyz": ((N, Cc, 3), torch.float32), "energy": ((B, Cc), torch.float32), "gmax": ((B, Cc), torch.float32),
              "steps": ((B, Cc), torch.int32), "status": ((B, Cc), torch.int32), "terms": ((6, B, Cc), torch.float32),
              "grad": ((N, Cc, 3), torch.float32)}
    if rb is not None:
        shapes.update(er=((B, Cc), torch.float32), phi=((rb.R, Cc), torch.float32))
    bufs = {k: _guarded(*v) for k, v in shapes.items()}
    o = {k: v[1] for k, v in bufs.items()}
    ks = [k.to("cuda") for k in batch.ks]
    eqs = [None if q is None else q.to("cuda") for q in batch.eqs]
    kw = {} if rb is None else dict(restraints=rb.to("cuda"), restraint_energy=o["er"], dihedral_out=o["phi"])
    hip.relax_fire(plan, x, ks, eqs, batch.n_per, False, dnb, {**RELAX_DEFAULTS, **opts}, o["xyz"], o["energy"], o["gmax"], o["steps"], o["status"],
                   term_energy=o["terms"], grad=o["grad"], **kw)
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        fill = FILL_I if buf.dtype == torch.int32 else FILL
        assert bool((buf[:64] == fill).all()) and bool((buf[-64:] == fill).all()), f"written outside {k}"
        if expect_written and view.numel() and k not in unwritten:
            assert not bool((view == fill).all()), f"{k} was not written"
    return {k: v.cpu().clone() for k, v in o.items()}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b, what, keys=OUTS):
    for k in keys:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs"


def _rows_of(out, batch, rb, b):
    """molecule b's part of every output"""
    p0, p1 = int(batch.ptr[b]), int(batch.ptr[b + 1])
    r0, r1 = int(rb.dih_molptr[b]), int(rb.dih_molptr[b + 1])
    return {"xyz": out["xyz"][p0:p1], "grad": out["grad"][p0:p1], "terms": out["terms"][:, b], "phi": out["phi"][r0:r1],
            **{k: out[k][b] for k in ("energy", "gmax", "steps", "status", "er")}}


def _per_mol(b, t):
    return torch.stack([t[int(b.ptr[k]):int(b.ptr[k + 1])].max(0).values for k in range(b.B)])


def _traj_gate(b, got_xyz, x64, x32, ok, what):
    one = torch.tensor([n == 1 for n in b.counts])[:, None].expand_as(ok)
    dist = lambda x: torch.stack([(x.double() - x64)[int(b.ptr[k]):int(b.ptr[k + 1])].norm(dim=-1).max(0).values for k in range(b.B)])      # noqa: E731
    dg, dr = dist(got_xyz), dist(x32)
    ratio = ((dg - ULP_X).clamp_min(0) / dr.clamp_min(1e-300))[ok & ~one]
    print(f"{what}: max |x_gpu - x_f64| {float(dg[ok].max()):.3e}, |x_f32 - x_f64| {float(dr[ok].max()):.3e}, "
          f"largest (|gpu| - 2^-20) / |f32| = {float(ratio.max()) if ratio.numel() else 0.0:.3f} over {int(ok.sum())} of {ok.numel()} conformations")
    assert bool(torch.isfinite(got_xyz).all())
    bad = ok & (dg > TRAJ_FACTOR * dr + ULP_X)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} conformations outside {TRAJ_FACTOR} x fp32 + 2^-20: gpu {dg[bad].tolist()} fp32 {dr[bad].tolist()}"


# ------------------------------------------------------------------------------------------------ 1. step zero
@pytest.mark.parametrize("name", sorted(rs.CASES))
def test_step_zero(hip, name):
    """max_steps = 0: grad, restraint_energy and dih_phi pass the calibrated gate against float64; energy and term_energy are those of
    the unrestrained kernel bit for bit; xyz_out is the input"""
    b, rb, nb = rs.case(name)
    r64, r32 = rs.objective_of(name, torch.float64), rs.objective_of(name, torch.float32)
    got = _run(hip, b, rb, nb, max_steps=0, tolerance=0.0)
    plain = _run(hip, b, None, nb, max_steps=0, tolerance=0.0)
    assert torch.equal(got["xyz"].view(torch.int32), b.xyz.view(torch.int32)) and not got["steps"].any()
    _same_bits(got, plain, f"{name}: the force field's energy", ("energy", "terms"))
    rows = lambda t, w: t.reshape(-1, w)      # noqa: E731
    kr.assert_calibrated(rows(got["grad"], 3), rows(r32["G"], 3), rows(r64["G"], 3), rr.C_GATE, r64["abs_f"].reshape(-1), f"{name}: gradient")
    kr.assert_calibrated(rows(got["er"], 1), rows(r32["Er"], 1), rows(r64["Er"], 1), rr.C_GATE, r64["abs_er"].reshape(-1), f"{name}: restraint energy")
    kr.assert_calibrated(rows(got["phi"], 1), rows(r32["phi"], 1), rows(r64["phi"], 1), rr.C_GATE, np.pi, f"{name}: dihedrals", period=2 * np.pi)
    want_gmax = _per_mol(b, got["grad"].double().norm(dim=-1))
    assert bool(((got["gmax"].double() - want_gmax).abs() <= 4 * kr.U32 * want_gmax).all()), "gmax is not the objective's largest gradient norm"
    tb = rs.Tables(b, rb)
    assert not got["grad"][tb.frozen].any(), "a frozen atom's gradient row is not 0"


# ------------------------------------------------------------------------------------------------ 2. trajectories
@pytest.mark.parametrize("name,max_steps", rs.TRAJ, ids=[f"{n}-{s}steps" for n, s in rs.TRAJ])
def test_trajectory(hip, name, max_steps):
    """tolerance = 0: every item runs exactly max_steps steps; the gate of test_gpu_relax.test_trajectory on items inside the margin"""
    b, rb, nb = rs.case(name)
    total = rs.total_steps(name)
    x64, x32 = rs.trajectory(name, torch.float64, total)["snap"][max_steps], rs.trajectory(name, torch.float32, total)["snap"][max_steps]
    ok = rs.margin_ok(name, max_steps)
    got = _run(hip, b, rb, nb, max_steps=max_steps, tolerance=0.0)
    one = torch.tensor([n == 1 for n in b.counts])[:, None].expand_as(got["status"])
    assert torch.equal(got["steps"], torch.where(one, 0, max_steps).int()) and torch.equal(got["status"], one.int())
    _traj_gate(b, got["xyz"], x64, x32, ok, f"{name} {max_steps} steps")
    tb = rs.Tables(b, rb)
    assert torch.equal(got["xyz"][tb.frozen].view(torch.int32), b.xyz[tb.frozen].view(torch.int32)), "a frozen atom moved"


# ------------------------------------------------------------------------------------------------ 3. convergence
@pytest.mark.parametrize("name", rs.CONV_CASES)
def test_convergence(hip, name):
    """the defaults (relax_restr_refs.CONV_OPTS is empty): status 1, and the objective's float64 gmax at xyz_out within the bound of
    test_gpu_relax.test_convergence_with_the_defaults"""
    b, rb, nb = rs.case(name)
    tb = rs.Tables(b, rb)
    got = _run(hip, b, rb, nb, **rs.CONV_OPTS)
    assert bool((got["status"] == 1).all()), got["status"].tolist()
    r64, r32 = rs.objective(b, tb, got["xyz"], b.xyz, torch.float64, nb), rs.objective(b, tb, got["xyz"], b.xyz, torch.float32, nb)
    gmax64, gmax32 = _per_mol(b, r64["G"].norm(dim=-1)), _per_mol(b, r32["G"].double().norm(dim=-1))
    floor = rr.C_GATE * kr.U32 * _per_mol(b, r64["abs_f"])
    cal = torch.maximum(_per_mol(b, (r32["G"].double() - r64["G"]).norm(dim=-1)), (gmax32 - gmax64).abs())
    bound = floor + 2 * cal + 2 * kr.U32 * _per_mol(b, rr.bond_rounding(b, got["xyz"]))
    fmt = lambda t: [f"{v:.2e}" for v in t.flatten().tolist()]      # noqa: E731
    print(f"{name}: steps {got['steps'].flatten().tolist()}\n  gmax gpu - f64 {fmt(got['gmax'].double() - gmax64)}\n  f64 gmax - tolerance "
          f"{fmt(gmax64 - RELAX_DEFAULTS['tolerance'])}\n  bound {fmt(bound)}")
    assert bool((gmax64 <= RELAX_DEFAULTS["tolerance"] + bound).all()), "the objective's float64 gradient at xyz_out is above the tolerance"
    assert bool(((got["gmax"].double() - gmax64).abs() <= bound).all()), "gmax at xyz_out"
    dev = torch.remainder(got["phi"].double() - rb.dih_target.double() + np.pi, 2 * np.pi) - np.pi
    print(f"  largest |phi - target| at convergence {float(dev.abs().max()) if dev.numel() else 0.0:.4f} rad")


# ------------------------------------------------------------------------------------------------ 4. known answer
def test_four_atom_chain_ends_on_its_torsion_series(hip):
    """bonded terms only, tolerance 0.01: at a restrained minimum of a 4-atom chain bonds and angles are at equilibrium, so energy is
    the torsion series at dih_phi within 1e-4 kcal/mol (residual strain <= tau^2 r^2 / (2 k_angle) = 2e-6 per angle, fp32 rounding
    1e-7) and k sin(phi - target) is minus the series' derivative within tolerance x 2 A"""
    b, rb, nb = rs.case("n4_C3")
    tol = 0.01
    got = _run(hip, b, rb, False, tolerance=tol)
    assert bool((got["status"] == 1).all()), got["status"].tolist()
    phi = got["phi"][0].double().numpy()
    e, de = rs.series(b.ks[2][0].numpy(), phi)
    torque = float(rb.dih_k[0]) * np.sin(phi - rb.dih_target[0].double().numpy())
    print(f"n4: energy - series {(got['energy'][0].double().numpy() - e).tolist()}, k sin(phi - target) + series' {(torque + de).tolist()}")
    assert np.abs(got["energy"][0].double().numpy() - e).max() <= 1e-4
    assert np.abs(torque + de).max() <= tol * 2.0
    assert not got["terms"][3:].any()


# ------------------------------------------------------------------------------------------------ 5. frozen atoms
def test_frozen_atoms_keep_their_bits_and_a_frozen_molecule_stops_at_once(hip):
    b, rb, nb = rs.case("n65_C1")
    tb = rs.Tables(b, rb)
    assert int(tb.frozen.sum()) >= 5
    got = _run(hip, b, rb, nb, max_steps=300)
    assert bool((got["steps"] > 40).all())
    assert torch.equal(got["xyz"][tb.frozen].view(torch.int32), b.xyz[tb.frozen].view(torch.int32)), "a frozen atom's coordinates changed"
    assert not torch.equal(got["xyz"][~tb.frozen], b.xyz[~tb.frozen]) and not got["grad"][tb.frozen].any()
    # all atoms frozen (with a restraint that pulls): step 0, status 1, the input bit for bit
    nine, rb9, _ = rs.case("n9_C3")
    allf = RestraintBatch([Restraints(frozen=np.ones(9, bool), dihedrals=rb9.items[0].dihedrals, dihedral_k=rb9.items[0].dihedral_k,
                                      dihedral_targets=rb9.items[0].dihedral_targets)], 3, atom_counts=[9])
    got = _run(hip, nine, allf, True)
    assert bool((got["status"] == 1).all()) and not got["steps"].any() and not got["gmax"].any() and not got["grad"].any()
    assert torch.equal(got["xyz"].view(torch.int32), nine.xyz.view(torch.int32)) and bool((got["er"] > 0).all())


# ------------------------------------------------------------------------------------------------ 6. bits
def test_same_input_same_bits_whatever_the_neighbours_do(hip):
    b, rb, nb = rs.case("mixed")
    opts = dict(max_steps=200)
    a, a2 = _run(hip, b, rb, nb, **opts), _run(hip, b, rb, nb, **opts)
    _same_bits(a, a2, "two runs")
    for which in ([2], [3], [3, 0, 2], [2, 3]):
        sb, srb, _ = rs.subset("mixed", which)
        out = _run(hip, sb, srb, nb, **opts)
        for pos, k in enumerate(which):
            if k in (2, 3):
                _same_bits(_rows_of(out, sb, srb, pos), _rows_of(a, b, rb, k), f"molecule {k} in {which}")


def test_no_restraints_is_the_unrestrained_call(hip):
    """r == NULL and an all-empty r against grappa_relax_fire_f32: all outputs equal, restraint_energy 0"""
    from grappa_amd import _lib
    b = rr.case("mixed")
    Cc = b.xyz.shape[1]
    plain = _run(hip, b, None, True, max_steps=60)
    empty = _run(hip, b, RestraintBatch([None] * b.B, Cc), True, max_steps=60)
    _same_bits(empty, plain, "an all-empty restraint batch", BASE)
    assert not empty["er"].any() and empty["phi"].numel() == 0
    # r == NULL through the C ABI
    plan, x = b.plan("cuda"), b.xyz.to("cuda")
    ks, eqs = [k.to("cuda") for k in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    d = hip._mm_desc(plan, x, ks, eqs, b.n_per, False)
    dnb = b.nonbonded().to("cuda")
    from grappa_amd.backend_mm import _nb_tables_desc
    nd = _nb_tables_desc(dnb, b.N, Cc, b.B, x.device, "test")
    o = _lib.RelaxOpts(**{k: (int(v) if k in ("max_steps", "n_min") else float(v)) for k, v in {**RELAX_DEFAULTS, "max_steps": 60}.items()})
    shapes = {"xyz": ((b.N, Cc, 3), torch.float32), "energy": ((b.B, Cc), torch.float32), "terms": ((6, b.B, Cc), torch.float32),
              "grad": ((b.N, Cc, 3), torch.float32), "gmax": ((b.B, Cc), torch.float32), "steps": ((b.B, Cc), torch.int32),
              "status": ((b.B, Cc), torch.int32), "er": ((b.B, Cc), torch.float32)}
    bufs = {k: _guarded(*v) for k, v in shapes.items()}
    p = {k: v[1].data_ptr() for k, v in bufs.items()}
    rc = hip.lib.grappa_relax_fire_restr_f32(hip._stream(), C.byref(d), C.byref(nd), C.byref(o), None, p["xyz"], p["energy"], p["terms"], p["grad"],
                                             p["gmax"], p["steps"], p["status"], p["er"], None)
    torch.cuda.synchronize()
    assert rc == 0
    null = {k: v[1].cpu().clone() for k, v in bufs.items()}
    _same_bits(null, plain, "r == NULL", BASE)
    assert not null["er"].any()


# ------------------------------------------------------------------------------------------------ 7. refusals
def _replace_tables(rb, **kw):
    out = rb.to("cpu")
    for k, v in kw.items():
        setattr(out, k, v)
    out.R = int(out.dih_atoms.shape[0])
    return out


def _refusal_cases():
    b, rb, _ = rs.case("mixed")          # molecule 2 (17 atoms) holds rows 0 .. 15
    at = rb.dih_atoms.clone()
    at[3, 1] = 17
    yield "an index equal to n", _replace_tables(rb, dih_atoms=at), 2
    at = rb.dih_atoms.clone()
    at[5, 2] = at[5, 0]
    yield "a repeated atom", _replace_tables(rb, dih_atoms=at), 2
    k = rb.dih_k.clone()
    k[0] = -1.0
    yield "a negative dih_k", _replace_tables(rb, dih_k=k), 2
    ptr = rb.dih_molptr.clone()
    ptr[3:] = 17
    yield "17 dihedrals on one molecule", _replace_tables(rb, dih_molptr=ptr, dih_atoms=torch.cat([rb.dih_atoms, rb.dih_atoms[:1]]),
                                                           dih_k=torch.cat([rb.dih_k, rb.dih_k[:1]]), dih_target=torch.cat([rb.dih_target, rb.dih_target[:1]])), 2
    pk = rb.pos_k.clone()
    pk[int(b.ptr[3]) + 1] = -2.0
    yield "a negative pos_k", _replace_tables(rb, pos_k=pk), 3


@pytest.mark.parametrize("what", ["an index equal to n", "a repeated atom", "a negative dih_k", "17 dihedrals on one molecule", "a negative pos_k",
                                  "a NaN target"])
def test_refused_tables_get_status_five(hip, what):
    """the item's outputs keep their fill (status 5 and nothing else), its neighbours' bits are those of the valid batch"""
    b, rb, nb = rs.case("mixed")
    good = _run(hip, b, rb, nb, max_steps=30)
    if what == "a NaN target":          # of conformation 1 only: the other conformations of the molecule run
        tg = rb.dih_target.clone()
        tg[7, 1] = float("nan")
        bad_rb, mol, confs = _replace_tables(rb, dih_target=tg), 2, [1]
    else:
        bad_rb, mol = next((r, m) for w, r, m in _refusal_cases() if w == what)
        confs = [0, 1, 2]
    got = _run(hip, b, bad_rb, nb, unwritten=("phi",) if mol == 2 and len(confs) == 3 else (), max_steps=30)          # (all dihedrals are molecule 2's)
    p0, p1 = int(b.ptr[mol]), int(b.ptr[mol + 1])
    r0, r1 = int(bad_rb.dih_molptr[mol]), int(bad_rb.dih_molptr[mol + 1])
    for c in confs:
        assert got["status"][mol, c] == 5, got["status"].tolist()
        assert bool((got["xyz"][p0:p1, c] == FILL).all()) and bool((got["grad"][p0:p1, c] == FILL).all()) and got["steps"][mol, c] == FILL_I
        assert got["energy"][mol, c] == FILL and got["gmax"][mol, c] == FILL and got["er"][mol, c] == FILL and bool((got["terms"][:, mol, c] == FILL).all())
        assert bool((got["phi"][r0:r1, c] == FILL).all())
    for k in range(b.B):
        for c in range(3):
            if k == mol and c in confs:
                continue
            for key in BASE + ("er",):
                sel = (lambda t: t[int(b.ptr[k]):int(b.ptr[k + 1]), c]) if key in ("xyz", "grad") else ((lambda t: t[:, k, c]) if key == "terms" else (lambda t: t[k, c]))
                assert torch.equal(_bits(sel(got[key])), _bits(sel(good[key]))), f"{what}: {key} of molecule {k}, conformation {c} changed"


def test_bad_arguments_are_refused_and_nothing_is_written(hip):
    from grappa_amd import _lib
    b, rb, nb = rs.case("n9_C3")
    dev_rb = rb.to("cuda")
    plan, x = b.plan("cuda"), b.xyz.to("cuda")
    ks, eqs = [k.to("cuda") for k in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    d = hip._mm_desc(plan, x, ks, eqs, b.n_per, False)
    o = _lib.RelaxOpts(**{k: (int(v) if k in ("max_steps", "n_min") else float(v)) for k, v in RELAX_DEFAULTS.items()})
    shapes = {"xyz": ((9, 3, 3), torch.float32), "e": ((1, 3), torch.float32), "g": ((1, 3), torch.float32), "s": ((1, 3), torch.int32),
              "st": ((1, 3), torch.int32), "er": ((1, 3), torch.float32), "phi": ((1, 3), torch.float32)}
    out = {k: _guarded(*v) for k, v in shapes.items()}
    ptr = {k: v[1].data_ptr() for k, v in out.items()}

    def restr(**kw):
        f = dict(frozen=None, pos_k=None, dih_molptr=dev_rb.dih_molptr.data_ptr(), dih_atoms=dev_rb.dih_atoms.data_ptr(), dih_k=dev_rb.dih_k.data_ptr(),
                 dih_target=dev_rb.dih_target.data_ptr(), R=1)
        f.update(kw)
        return _lib.RelaxRestr(**f)

    def call(r, mm=d, opts=o, **over):
        q = {**ptr, **over}
        return hip.lib.grappa_relax_fire_restr_f32(hip._stream(), C.byref(mm) if mm is not None else None, None, C.byref(opts) if opts is not None else None,
                                                   C.byref(r) if r is not None else None, q["xyz"], q["e"], None, None, q["g"], q["s"], q["st"], q["er"], q["phi"])

    bad_o = _lib.RelaxOpts(**{k: (int(v) if k in ("max_steps", "n_min") else float(v)) for k, v in {**RELAX_DEFAULTS, "dt_start": 0.0}.items()})
    for what, rc in (("R < 0", call(restr(R=-1))), ("NULL dih_molptr", call(restr(dih_molptr=None))), ("NULL dih_atoms", call(restr(dih_atoms=None))),
                     ("NULL dih_k", call(restr(dih_k=None))), ("NULL dih_target", call(restr(dih_target=None))),
                     ("NULL restraint_energy", call(restr(), er=None)), ("NULL restraint_energy, r NULL", call(None, er=None)),
                     ("R * C >= 2^31", call(restr(R=(1 << 31) // 3 + 1))), ("NULL mm", call(restr(), mm=None)), ("NULL opts", call(restr(), opts=None)),
                     ("bad options", call(restr(), opts=bad_o)), ("NULL xyz_out", call(restr(), xyz=None)), ("NULL energy", call(restr(), e=None)),
                     ("NULL gmax", call(restr(), g=None)), ("NULL steps", call(restr(), s=None)), ("NULL status", call(restr(), st=None)),
                     ("NULL xyz_out, r NULL", call(None, xyz=None))):
        assert rc == -1, what          # GRAPPA_ERR_ARG
    torch.cuda.synchronize()
    for k, (buf, _) in out.items():
        assert bool((buf == (FILL_I if buf.dtype == torch.int32 else FILL)).all()), f"{k} was written by a refused call"
    assert call(restr()) == 0          # the complete call is accepted
    torch.cuda.synchronize()
    assert bool((out["st"][1] != FILL_I).all()) and bool((out["er"][1] != FILL).all()) and hip.lib.grappa_relax_max_dihedrals() == MAX_DIHEDRALS


def test_a_molecule_above_the_limit_gets_status_three(hip):
    n = rr.max_atoms() + 1
    nine, rb9, _ = rs.case("n9_C3")
    big = rr.gen_molecule(n, 3, np.random.default_rng(5))
    b = rr.Batch([big, nine.mols[0]])
    rb = RestraintBatch([Restraints(dihedrals=[big["idx"][2][0]], dihedral_k=10.0, dihedral_targets=[0.3]), rb9.items[0]], 3, atom_counts=b.counts)
    got = _run(hip, b, rb, True, max_steps=20)
    assert got["status"][0].tolist() == [3, 3, 3] and bool((got["xyz"][:n] == FILL).all()) and bool((got["er"][0] == FILL).all())
    assert bool((got["phi"][0] == FILL).all()) and bool((got["steps"][0] == FILL_I).all())
    _same_bits(_rows_of(got, b, rb, 1), _rows_of(_run(hip, nine, rb9, True, max_steps=20), nine, rb9, 0), "the neighbour of a refused molecule")


# ------------------------------------------------------------------------------------------------ 8. the public door
def test_grappa_torsion_scan_on_a_golden_molecule(hip):
    from grappa_amd import Grappa, GrappaModel, backend
    from grappa_amd.relax import graph_from_parameters, relax, scan_starts
    from grappa_amd.restraints import rotating_side
    old = backend._BACKEND
    backend.set_backend(hip)
    try:
        fx = gu.load("ref_small_att.npz")
        model = GrappaModel(**gu.config_of(fx))
        model.load_state_dict(gu.state_dict_of(fx))
        wrapper = Grappa(model, device="cuda")
        m = gu.molecules_of(fx)[0]
        mol = gu.molecule_of(m)
        x0 = np.ascontiguousarray(m["xyz"].transpose(1, 0, 2)[0]).astype(np.float64)
        p = wrapper.predict(mol)
        atoms = np.asarray(p.atoms).reshape(-1)
        pos = {int(a): k for k, a in enumerate(atoms.tolist())}
        bonds = np.array([[pos[int(a)], pos[int(c)]] for a, c in np.asarray(p.bonds).reshape(-1, 2).tolist()])
        dih = next(row for row in np.asarray(p.propers).reshape(-1, 4).tolist() if rotating_side(len(atoms), bonds, pos[row[1]], pos[row[2]]) is not None)
        angles = -np.pi + np.deg2rad(30.0) * np.arange(12)
        s = wrapper.torsion_scan(mol, x0, dih, angles, max_steps=40, tolerance=0.0)
        n = len(atoms)
        assert s.xyz.shape == (12, n, 3) and all(getattr(s, k).shape == (12,) for k in ("angles", "dihedrals", "energy", "restraint_energy", "steps", "status"))
        assert bool(np.isin(s.status, (0, 1)).all()) and bool((s.restraint_energy >= 0).all()) and bool(np.isfinite(s.energy).all())
        # the scan IS a restrained relax call on the rotated starts
        starts, idx = scan_starts(p, x0, dih, angles)
        r = relax(p, starts, restraints=Restraints(dihedrals=[idx], dihedral_k=[239.0], dihedral_targets=angles[None, :]), max_steps=40, tolerance=0.0)
        assert np.array_equal(r.xyz, s.xyz) and np.array_equal(r.energy, s.energy) and np.array_equal(r.dihedrals[0], s.dihedrals)
        # the achieved dihedrals against the float64 restatement after 40 steps, by the trajectory gate
        g = graph_from_parameters(p, starts)
        pl = g.plan()
        ks = [g.nodes[lv].data["k"] for lv in rr.LEVELS]
        n_per = [0, 0, max(int(ks[2].shape[1]), 1), max(int(ks[3].shape[1]), 1)]
        b = rr.Batch.from_tables([n], [pl.idx32[lv].long() for lv in rr.LEVELS], [pl.mol_ptr[lv] for lv in rr.LEVELS], ks,
                                 [g.nodes["n2"].data["eq"], g.nodes["n3"].data["eq"], None, None], n_per, None, g.nodes["n1"].data["xyz"])
        rb = RestraintBatch([Restraints(dihedrals=[idx], dihedral_k=[239.0], dihedral_targets=angles[None, :])], 12, atom_counts=[n])
        t64 = rs.fire_restr_ref(b, rb, torch.float64, False, max_steps=40, tolerance=0.0)
        t32 = rs.fire_restr_ref(b, rb, torch.float32, False, max_steps=40, tolerance=0.0)
        ok = torch.ones(1, 12, dtype=torch.bool)
        for t in t64["margin"][1:40]:
            ok &= ~(t.abs() < rr.BRANCH_MARGIN)
        got_xyz = torch.from_numpy(s.xyz.transpose(1, 0, 2).astype(np.float32))
        if bool(ok.any()):
            _traj_gate(b, got_xyz, t64["xyz"], t32["xyz"], ok, "torsion scan, 40 steps")
        tb = rs.Tables(b, rb)
        phi64, phi32 = rs.dihedral_t(t64["xyz"], tb.ix)[0], rs.dihedral_t(t32["xyz"].double(), tb.ix)[0]
        wrap = lambda a: torch.remainder(a + np.pi, 2 * np.pi) - np.pi      # noqa: E731
        dg, dr = wrap(torch.from_numpy(s.dihedrals) - phi64).abs(), wrap(phi32 - phi64).abs()
        okc = ok[0]
        print(f"torsion scan: |phi_gpu - phi_f64| {float(dg[okc].max()) if okc.any() else 0:.3e}, |phi_f32 - phi_f64| {float(dr[okc].max()) if okc.any() else 0:.3e}; "
              f"|phi - target| after 40 steps {np.abs(wrap(torch.from_numpy(s.dihedrals - angles)).numpy()).max():.4f} rad")
        assert bool((dg <= TRAJ_FACTOR * dr + rr.C_GATE * kr.U32 * np.pi)[okc].all())
        # at convergence: no bound on |phi - target| (nobody has measured it) -- printed
        full = wrapper.torsion_scan(mol, x0, dih, angles)
        print(f"torsion scan to convergence: status {full.status.tolist()}, steps {full.steps.tolist()}, "
              f"largest |phi - target| {np.abs(wrap(torch.from_numpy(full.dihedrals - angles)).numpy()).max():.4f} rad")
        assert bool(np.isin(full.status, (0, 1)).all()) and bool((full.restraint_energy >= 0).all())
    finally:
        backend.set_backend(old)
