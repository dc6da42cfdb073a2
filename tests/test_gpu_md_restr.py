"""GPU: restraints on the stepwise dynamics (csrc/md_restr.h and csrc/dynamics_steps.hip through HipBackend.md_steps_restr and
grappa_amd/dynamics.py) against the restatements of tests/md_restr_refs.py.  Every output AND the workspace lie between guard regions
that must come back untouched.

Gates: step zero by the calibrated gate of tests/test_gpu_relax_restr.py (kernel_refs.assert_calibrated with relax_refs.C_GATE: energy
against its absolute sum, dihedrals against pi, periodic); trajectories by test_gpu_md._gate_state as it stands (factor 4, floor 2^-20),
whose calibration tests/test_host_md_restr.py bounds from the restatement alone; conservation by the bound of
test_gpu_md_steps.test_energy_conservation with E_r counted in the total.

Observed on an MI355X (largest (|gpu| - floor) / |f32| over the steady items of each group, the gate being 4): see DESIGN.md section 23."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_utils as gu
import kernel_refs as kr
import md_cons_refs as mc
import md_cut_refs as mcut
import md_gb_cut_refs as mgc
import md_gb_refs as mg
import md_refs as md
import md_restr_refs as mr
import md_steps_cons_refs as msc
import md_steps_refs as ms
import relax_refs as rr
import relax_restr_refs as rs
import relax_steps_refs as rst
from grappa_amd.restraints import RestraintBatch, Restraints
from grappa_amd.solvent import GBBatch
from test_gpu_md import _gate_state
from test_gpu_md_steps import FILL, FILL_B, FILL_I, GUARD_B, OUTS, _bits, _dev_keys, _fill_of, _guarded, _noise, _same_bits, _with_coincident

pytestmark = pytest.mark.gpu

R_OUTS = OUTS + ("er", "phi")
FRAMES = ("frames_xyz", "frames_epot", "frames_ekin")
R_FRAMES = FRAMES + ("frames_er", "frames_phi")
THERMO = dict(friction=20.0, temperature=300.0, init_temperature=300.0)


@pytest.fixture(scope="module")
def hip():
    from grappa_amd.backend import HipBackend
    return HipBackend()


def _run(hip, batch, masses, keys, rb, ref=None, vel=None, xyz=None, cons=None, cutoff=None, gbs=None, solvent=None, steps_per_call=1000,
         unwritten=(), **opts):
    """one call of a seam on a relax_refs.Batch -> dict of CPU tensors; asserts the guards around the outputs and, with restraints, the
    workspace.  rb: a RestraintBatch (md_steps_restr) or None: the call WITHOUT restraints that the same Hamiltonian makes today
    (md_steps, md_steps_cons, md_steps_gb).  cons: a list of Constraints; cutoff: a Cutoff; gbs + solvent: the GB parameters and model"""
    o = {**md.MD_OPTS, **opts}
    plan = batch.plan("cuda")
    x = (batch.xyz if xyz is None else xyz).to("cuda")
    N, B, Cc = batch.N, batch.B, x.shape[1]
    F = o["n_steps"] // o["save_every"] if o["save_every"] > 0 and o["n_steps"] > 0 else 0
    shapes = {"xyz": ((N, Cc, 3), torch.float32), "vel": ((N, Cc, 3), torch.float32), "epot": ((B, Cc), torch.float32),
              "ekin": ((B, Cc), torch.float32), "steps": ((B, Cc), torch.int32), "status": ((B, Cc), torch.int32)}
    if F:
        shapes.update({"frames_xyz": ((F, N, Cc, 3), torch.float32), "frames_epot": ((F, B, Cc), torch.float32), "frames_ekin": ((F, B, Cc), torch.float32)})
    if gbs is not None:
        shapes["esolv"] = ((B, Cc), torch.float32)
    if rb is not None:
        shapes.update(er=((B, Cc), torch.float32), phi=((rb.R, Cc), torch.float32))
        if F:
            shapes.update(frames_er=((F, B, Cc), torch.float32), frames_phi=((F, rb.R, Cc), torch.float32))
    bufs = {k: _guarded(*v) for k, v in shapes.items()}
    out = {k: v[1] for k, v in bufs.items()}
    ks = [k.to("cuda") for k in batch.ks]
    eqs = [None if q is None else q.to("cuda") for q in batch.eqs]
    args = (plan, x, ks, eqs, batch.n_per, False, batch.nonbonded().to("cuda"), o, torch.from_numpy(np.asarray(masses, dtype=np.float32)).to("cuda"),
            _dev_keys(keys), None if vel is None else vel.to("cuda"), out["xyz"], out["vel"], out["epot"], out["ekin"], out["steps"], out["status"])
    kw = dict(frames_xyz=out.get("frames_xyz"), frames_epot=out.get("frames_epot"), frames_ekin=out.get("frames_ekin"), atom_counts_host=batch.counts,
              steps_per_call=steps_per_call)
    K = 0
    if cons is not None:
        from grappa_amd.constraints import ConstraintBatch
        cb = ConstraintBatch(cons, tolerance=mc.TOL)
        K = int(cb.cluster_atoms.shape[0])
        kw.update(constraints=cb.to("cuda"), constrain_start=True)
    if cutoff is not None:
        kw["cutoff"] = cutoff
    if gbs is not None:
        kw.update(gb=GBBatch(gbs).to("cuda"), solvent=solvent, esolv=out["esolv"])
    wbuf = None
    if rb is None:
        (hip.md_steps_gb if gbs is not None else (hip.md_steps_cons if cons is not None else hip.md_steps))(*args, **kw)
    else:
        from grappa_amd.solvent import as_implicit_solvent
        gbcut = gbs is not None and as_implicit_solvent(solvent).cutoff is not None
        need = int(hip.lib.grappa_md_steps_restr_workspace_bytes(N, Cc, B, rst.n_blocks(batch), K, int(cutoff is not None), int(gbs is not None), int(gbcut)))
        wbuf = torch.full((GUARD_B + need + GUARD_B,), FILL_B, dtype=torch.uint8, device="cuda")
        hip.md_steps_restr(*args, **kw, workspace=wbuf[GUARD_B:GUARD_B + need], restraints=rb.to("cuda"),
                           restraint_reference=None if ref is None else ref.to("cuda"), restraint_energy=out["er"], dihedral_out=out["phi"],
                           frames_restraint_energy=out.get("frames_er"), frames_dihedrals=out.get("frames_phi"))
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert bool((buf[:64] == _fill_of(buf)).all()) and bool((buf[-64:] == _fill_of(buf)).all()), f"written outside {k}"
    if wbuf is not None:
        assert bool((wbuf[:GUARD_B] == FILL_B).all()) and bool((wbuf[-GUARD_B:] == FILL_B).all()), "written outside the workspace"
    for k in R_OUTS if rb is not None else OUTS:
        if out[k].numel() and k not in unwritten:
            assert not bool((out[k] == _fill_of(out[k])).all()), f"{k} was not written"
    return {k: v.cpu().clone() for k, v in out.items()}


def _case_run(hip, name, rb="case", **opts):
    c = mr.case(name)
    rb = c["rb"] if isinstance(rb, str) else rb
    ref = None if c["offset"] is None or rb is None else mr.reference_of(c["batch"], offset=c["offset"])
    return _run(hip, c["batch"], c["masses"], c["keys"], rb, ref=ref, vel=c["vel"], **opts)


def _rows_of(out, batch, rb, b):
    """molecule b's part of every output"""
    p0, p1 = int(batch.ptr[b]), int(batch.ptr[b + 1])
    r0, r1 = int(rb.dih_molptr[b]), int(rb.dih_molptr[b + 1])
    rows = {"xyz": out["xyz"][p0:p1], "vel": out["vel"][p0:p1], "phi": out["phi"][r0:r1], **{k: out[k][b] for k in ("epot", "ekin", "steps", "status", "er")}}
    if "frames_xyz" in out:
        rows.update({"frames_xyz": out["frames_xyz"][:, p0:p1], "frames_phi": out["frames_phi"][:, r0:r1],
                     **{k: out[k][:, b] for k in ("frames_epot", "frames_ekin", "frames_er")}})
    return rows


# ------------------------------------------------------------------------------------------------ 1. step zero
@pytest.mark.parametrize("name", mr.CASES)
def test_step_zero(hip, name):
    """n_steps = 0: restraint_energy and dihedrals pass the calibrated gate of tests/test_gpu_relax_restr.py against float64 at the
    input; epot, ekin, coordinates and velocities are, bit for bit, those of the call without restraints"""
    c = mr.case(name)
    b = c["batch"]
    got = _case_run(hip, name, n_steps=0)
    plain = _case_run(hip, name, rb=None, n_steps=0)
    _same_bits(got, plain, f"{name}: what the force field alone decides")
    assert torch.equal(_bits(got["xyz"]), _bits(b.xyz)) and not got["steps"].any() and not got["status"].any()
    with mr.restr_force(c["rb"], offset=c["offset"]):
        r64, r32 = rr.forces(b, b.xyz, torch.float64, True), rr.forces(b, b.xyz, torch.float32, True)
    rows = lambda t, w: t.reshape(-1, w)      # noqa: E731
    kr.assert_calibrated(rows(got["er"], 1), rows(r32["Er"], 1), rows(r64["Er"], 1), rr.C_GATE, r64["abs_er"].reshape(-1), f"{name}: restraint energy")
    kr.assert_calibrated(rows(got["phi"], 1), rows(r32["phi"], 1), rows(r64["phi"], 1), rr.C_GATE, np.pi, f"{name}: dihedrals", period=2 * np.pi)


# ------------------------------------------------------------------------------------------------ 2. trajectories
@pytest.mark.parametrize("name,n_steps", mr.TRAJ, ids=[f"{n}-{s}steps" for n, s in mr.TRAJ])
def test_trajectory_without_thermostat(hip, name, n_steps):
    """friction = 0 (velocity Verlet), dt = 1 fs, from the case coordinates with thermal velocities"""
    b = mr.case(name)["batch"]
    r64, r32s = mr.verlet(name)[n_steps], [r[n_steps] for r in mr.verlet32(name)]
    got = _case_run(hip, name, n_steps=n_steps, dt=0.001)
    assert bool((got["steps"] == n_steps).all()) and not got["status"].any()
    _gate_state(name, f"{n_steps} steps, friction 0, restrained", b, got, r64, r32s)
    er, phi = mr.energy_at(b, mr.case(name)["rb"], got["xyz"].double(), offset=mr.case(name)["offset"])
    # (a consistency check, not the gate -- that is step zero's: fp32 holds a dihedral to a few u32 pi and a displacement of these
    # molecules to a few u32 x 100 A, which moves a row by at most 239 x 1e-6 and a tether by 50 x 0.5 x 1e-5 kcal/mol: 1e-4 relative
    # to 1 + E_r lies two orders above both for every case here)
    assert bool(((got["er"].double() - er).abs() <= 1e-4 * (1.0 + er.abs())).all()), "restraint_energy is E_r at xyz_out"
    d = torch.remainder(got["phi"].double() - phi + np.pi, 2 * np.pi) - np.pi
    assert bool((d.abs() <= 1e-4).all()), "dihedrals are the restrained dihedrals at xyz_out"


def test_trajectory_with_thermostat(hip):
    """friction 50 / ps at 300 K, 40 steps on the three-block case: the restatements consume the noise md_noise wrote"""
    name = "s129_C3"
    c = mr.case(name)
    b, m, k, v = c["batch"], c["masses"], c["keys"], c["vel"]
    first, total = 7, max(ms.TRAJ_STEPS)
    z = {first + s: _noise(hip, b.counts, k, b.xyz.shape[1], first + s, 0).double() for s in range(total)}
    opts = dict(friction=50.0, temperature=300.0, dt=0.001, first_step=first)
    with mr.restr_force(c["rb"]):
        r32s = md.fp32_realisations(b, m, (total,), velocities=v, noise=lambda step, purpose: z[step], n_steps=total, **opts)
    got = _case_run(hip, name, n_steps=total, **opts)
    assert bool((got["steps"] == total).all()) and not got["status"].any()
    _gate_state(name, f"{total} steps, friction 50, restrained", b, got, r32s[0][total][1], [r[total] for r in r32s])


# ------------------------------------------------------------------------------------------------ 3. every Hamiltonian
def _span64_restraints():
    batch = msc.case("span64")[0]
    rng = np.random.default_rng(64)
    return RestraintBatch([rs._restraints_of(batch.mols[0], batch.xyz.shape[1], rng, 2, 0, 4)], batch.xyz.shape[1], atom_counts=batch.counts)


def _zero_strength_is_the_call_without(hip, what, batch, m, keys, rb, vel, **kw):
    zero = _run(hip, batch, m, keys, mr.zero_strength(rb, batch), vel=vel, **kw)
    plain = _run(hip, batch, m, keys, None, vel=vel, **kw)
    _same_bits(zero, plain, f"{what}: zero-strength tables", keys=("xyz", "vel", "epot", "ekin", "steps", "status") + (("esolv",) if "esolv" in plain else ()))
    assert not zero["er"].any(), f"{what}: restraint_energy of zero-strength tables"
    _, phi = mr.energy_at(batch, rb, zero["xyz"].double())
    d = torch.remainder(zero["phi"].double() - phi + np.pi, 2 * np.pi) - np.pi
    assert bool((d.abs() <= 1e-4).all()), f"{what}: dihedrals are reported"


def test_under_a_cutoff(hip):
    name = "s129_C3"
    c = mr.case(name)
    cut = mcut.cutoff(name)
    with mcut.cut_force(cut), mr.restr_force(c["rb"]):
        r32s = md.fp32_realisations(c["batch"], c["masses"], (5,), velocities=c["vel"], n_steps=5)
    got = _case_run(hip, name, cutoff=cut, n_steps=5, dt=0.001)
    assert bool((got["steps"] == 5).all()) and not got["status"].any()
    _gate_state(name, "5 steps, cutoff, restrained", c["batch"], got, r32s[0][5][1], [r[5] for r in r32s])
    _zero_strength_is_the_call_without(hip, "cutoff", c["batch"], c["masses"], c["keys"], c["rb"], c["vel"], cutoff=cut, n_steps=5, dt=0.001)


@pytest.mark.parametrize("cut", [False, True], ids=["all_pairs", "cutoff"])
def test_with_constraints(hip, cut):
    name = "span64"
    batch, cons, m, keys = msc.case(name)
    rb, v = _span64_restraints(), msc.thermal_velocities(name)
    kw = dict(velocities=v, n_steps=5, dt=msc.TRAJ_DT)
    with msc.force_of(name, cut), mr.restr_force(rb):
        r64 = mc.gbaoab_ref(batch, m, cons, torch.float64, snapshots=(5,), **kw)
        r32s = mc.fp32_realisations(batch, m, cons, (5,), **kw)
    assert not r64["status"].any()
    run = dict(cons=cons, cutoff=msc.cutoff(name) if cut else None, n_steps=5, dt=msc.TRAJ_DT)
    got = _run(hip, batch, m, keys, rb, vel=v, **run)
    assert bool((got["steps"] == 5).all()) and not got["status"].any()
    _gate_state(name, f"5 steps of 2 fs, constraints{', cutoff' if cut else ''}, restrained", batch, got, r64["snap"][5], [r[5] for r in r32s])
    _zero_strength_is_the_call_without(hip, "constraints", batch, m, keys, rb, v, **run)


def test_in_implicit_solvent(hip):
    name = "s65_C3"
    c = mr.case(name)
    gbs = mg.gb_params(name)
    with mg.gb_force(gbs), mr.restr_force(c["rb"]):
        r32s = md.fp32_realisations(c["batch"], c["masses"], (5,), velocities=c["vel"], n_steps=5)
    got = _case_run(hip, name, gbs=gbs, solvent=mg.MODEL, n_steps=5, dt=0.001)
    assert bool((got["steps"] == 5).all()) and not got["status"].any() and bool((got["esolv"] < 0).all())
    _gate_state(name, "5 steps, obc2, restrained", c["batch"], got, r32s[0][5][1], [r[5] for r in r32s])
    _zero_strength_is_the_call_without(hip, "obc2", c["batch"], c["masses"], c["keys"], c["rb"], c["vel"], gbs=gbs, solvent=mg.MODEL, n_steps=5, dt=0.001)


def test_in_cut_off_solvent_under_a_cutoff_with_constraints(hip):
    name = mgc.CONS_CASE
    batch, cons, m, keys = msc.case(name)
    rb, v, gbs, sv, nbc = _span64_restraints(), msc.thermal_velocities(name), list(mg.cons_gb()), mgc.solvent(name), mgc.nb_cutoff(name)
    kw = dict(velocities=v, n_steps=5, dt=msc.TRAJ_DT)
    with mgc.gb_cut_force(gbs, sv, nbc), mr.restr_force(rb):
        r64 = mc.gbaoab_ref(batch, m, cons, torch.float64, snapshots=(5,), **kw)
        r32s = mc.fp32_realisations(batch, m, cons, (5,), **kw)
    run = dict(cons=cons, cutoff=nbc, gbs=gbs, solvent=sv, n_steps=5, dt=msc.TRAJ_DT)
    got = _run(hip, batch, m, keys, rb, vel=v, **run)
    assert bool((got["steps"] == 5).all()) and not got["status"].any()
    _gate_state(name, "5 steps of 2 fs, cut-off obc2 + cutoff + constraints, restrained", batch, got, r64["snap"][5], [r[5] for r in r32s])
    _zero_strength_is_the_call_without(hip, "cut-off obc2 + cutoff + constraints", batch, m, keys, rb, v, **run)


# ------------------------------------------------------------------------------------------------ 4. energy conservation
def test_energy_conservation(hip):
    """NVE on md_steps_refs.nve_batch with tethers and dihedrals (md_restr_refs.nve_case): D = max over frames and items of
    |E_tot - E_tot at step 0| with E_tot = epot + E_r + ekin; D_gpu <= 2 max(D_f32, D_f64), the bound of
    test_gpu_md_steps.test_energy_conservation.  The force is the gradient of the energy reported, or this fails"""
    b, rb = mr.nve_case()
    m, k, v = ms.masses(ms.NVE_CASE), ms.keys(ms.NVE_CASE), ms.thermal_velocities(ms.NVE_CASE)
    start = _run(hip, b, m, k, rb, vel=v, n_steps=0)
    got = _run(hip, b, m, k, rb, vel=v, **ms.NVE)
    assert not got["status"].any() and bool((got["steps"] == ms.NVE["n_steps"]).all())
    tot = lambda r, p="": r[p + "epot"].double() + r[p + "er"].double() + r[p + "ekin"].double()      # noqa: E731
    d_gpu = md.drift(tot(start), tot(got, "frames_"))
    without = md.drift(start["epot"].double() + start["ekin"].double(), got["frames_epot"].double() + got["frames_ekin"].double())
    d32, d64 = mr.nve_drift(torch.float32), mr.nve_drift(torch.float64)
    print(f"energy conservation, restrained: D_gpu {d_gpu:.4f}, D_f32 {d32:.4f}, D_f64 {d64:.4f} kcal/mol, D_gpu / max = {d_gpu / max(d32, d64):.3f}; "
          f"without E_r in the sum {without:.2f}")
    assert d_gpu <= 2 * max(d32, d64)


# ------------------------------------------------------------------------------------------------ 5. frames
def test_frames_are_the_states_of_shorter_runs(hip):
    name = mr.MIXED
    whole = _case_run(hip, name, n_steps=20, save_every=5, **THERMO)
    assert whole["frames_er"].shape[0] == 4 and whole["frames_phi"].shape == (4, 18, 3)
    for f in range(4):
        part = _case_run(hip, name, n_steps=5 * (f + 1), **THERMO)
        for fk, pk in (("frames_xyz", "xyz"), ("frames_epot", "epot"), ("frames_ekin", "ekin"), ("frames_er", "er"), ("frames_phi", "phi")):
            assert torch.equal(_bits(whole[fk][f]), _bits(part[pk])), f"frame {f}: {fk}"


def test_a_stopped_item_writes_no_later_frame(hip):
    """atoms 0 and 129 of the 130-atom molecule on one point in conformation 1: status 2; its later frames of E_r and of its dihedrals
    keep the sentinel (the front end's NaN), every other item is bit-equal to the run without the defect"""
    c = mr.case(mr.MIXED)
    b, M = c["batch"], 3
    ref = mr.reference_of(b, offset=c["offset"])
    opts = dict(n_steps=20, save_every=5, **THERMO)
    plain = _run(hip, b, c["masses"], c["keys"], c["rb"], ref=ref, **opts)
    moved = _with_coincident(b, M, 0, 129, conf=1)
    hit = _run(hip, moved, c["masses"], c["keys"], c["rb"], ref=ref, **opts)
    assert int(hit["status"][M, 1]) == 2 and int(hit["status"].sum()) == 2
    stop = int(hit["steps"][M, 1])
    later = [f for f in range(4) if 5 * (f + 1) > stop]
    r0, r1 = int(c["rb"].dih_molptr[M]), int(c["rb"].dih_molptr[M + 1])
    assert later and r1 > r0 and bool((hit["frames_er"][later][:, M, 1] == FILL).all()) and bool((hit["frames_phi"][later][:, r0:r1, 1] == FILL).all())
    for key in ("er", "frames_er"):
        a, g = hit[key].clone(), plain[key].clone()
        a[..., M, 1], g[..., M, 1] = 0, 0
        assert torch.equal(_bits(a), _bits(g)), key
    for key in ("phi", "frames_phi"):
        a, g = hit[key].clone(), plain[key].clone()
        a[..., r0:r1, 1], g[..., r0:r1, 1] = 0, 0
        assert torch.equal(_bits(a), _bits(g)), key


# ------------------------------------------------------------------------------------------------ 6. bits
def test_two_runs_and_every_chunk_size_give_the_same_bits(hip):
    name = mr.MIXED
    a = _case_run(hip, name, n_steps=64, save_every=8, **THERMO)
    _same_bits(a, _case_run(hip, name, n_steps=64, save_every=8, **THERMO), "two runs", keys=R_OUTS + R_FRAMES)
    for spc in (1, 7, 64):
        _same_bits(a, _case_run(hip, name, n_steps=64, steps_per_call=spc, **THERMO), f"steps_per_call = {spc}", keys=R_OUTS)
    _same_bits(a, _case_run(hip, name, n_steps=64, save_every=8, steps_per_call=7, **THERMO), "frames, 7 per call", keys=R_OUTS + R_FRAMES)


def test_continuation_needs_the_original_reference(hip):
    """20 = 10 + 10 with first_step advanced and the ORIGINAL reference passed explicitly: the bits of 20.  With the default reference
    on the second half the tethers move to its start and the bits differ: the documented hazard"""
    c = mr.case("s65_C3")
    b, m, k = c["batch"], c["masses"], c["keys"]
    opts = dict(save_every=5, **THERMO)
    whole = _run(hip, b, m, k, c["rb"], n_steps=20, first_step=3, **opts)
    one = _run(hip, b, m, k, c["rb"], n_steps=10, first_step=3, **opts)
    two = _run(hip, b, m, k, c["rb"], ref=b.xyz, vel=one["vel"], xyz=one["xyz"], n_steps=10, first_step=13, **opts)
    _same_bits(whole, two, "20 steps against 10 + 10", keys=("xyz", "vel", "epot", "ekin", "status", "er", "phi"))
    for key in R_FRAMES:
        assert torch.equal(_bits(whole[key]), _bits(torch.cat([one[key], two[key]]))), key
    moved = _run(hip, b, m, k, c["rb"], vel=one["vel"], xyz=one["xyz"], n_steps=10, first_step=13, **opts)
    assert not torch.equal(_bits(moved["xyz"]), _bits(whole["xyz"])) and not torch.equal(_bits(moved["er"]), _bits(whole["er"]))


def test_a_molecule_gives_the_same_bits_alone_and_in_the_batch(hip):
    c = mr.case(mr.MIXED)
    b, rb = c["batch"], c["rb"]
    ref = mr.reference_of(b, offset=c["offset"])
    opts = dict(n_steps=20, save_every=10, **THERMO)
    mixed = _run(hip, b, c["masses"], c["keys"], rb, ref=ref, **opts)
    for j in (2, 3):          # the 17 atoms with 16 dihedrals, the 130 atoms in three blocks
        p0, p1 = int(b.ptr[j]), int(b.ptr[j + 1])
        sub = b.subset([j])
        srb = RestraintBatch([rb.items[j]], rb.C, atom_counts=sub.counts)
        alone = _run(hip, sub, c["masses"][p0:p1], c["keys"][[j]], srb, ref=ref[p0:p1], **opts)
        _same_bits(_rows_of(mixed, b, rb, j), _rows_of(alone, sub, srb, 0), f"molecule {j} alone and in the batch",
                   keys=R_OUTS + R_FRAMES)


def _abi(hip, b, m, k, o):
    from grappa_amd import _lib
    from grappa_amd.backend_mm import _nb_tables_desc
    plan, x = b.plan("cuda"), b.xyz.to("cuda")
    Cc = x.shape[1]
    ks, eqs = [t.to("cuda") for t in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    d = hip._mm_desc(plan, x, ks, eqs, b.n_per, False)
    dnb = b.nonbonded().to("cuda")
    nd = _nb_tables_desc(dnb, b.N, Cc, b.B, x.device, "test")
    mo = _lib.MdOpts(**{**md.MD_OPTS, **o})
    table, n_items, n_blocks, _ = hip.nonbonded_plan(torch.from_numpy(b.ptr.astype(np.int32)), b.N, Cc, x.device)
    keep = (plan, x, ks, eqs, dnb, table)
    return dict(d=d, nd=nd, mo=mo, table=table, n_items=n_items, n_blocks=n_blocks, keep=keep, Cc=Cc,
                mass=torch.from_numpy(np.asarray(m, dtype=np.float32)).to("cuda"), key=_dev_keys(k))


def test_no_restraints_is_the_call_without(hip):
    """r == NULL and all-empty tables through the C ABI against grappa_md_steps_*_gbcut_f32 (with everything else NULL: the plain
    calls), and an all-empty RestraintBatch through the seam: all outputs equal, restraint_energy 0 for molecules with atoms"""
    from grappa_amd import _lib
    name = "s65_C3"
    c = mr.case(name)
    b, m, k = c["batch"], c["masses"], c["keys"]
    o = dict(n_steps=12, save_every=0, **THERMO)
    plain = _run(hip, b, m, k, None, **o)
    empty = _run(hip, b, m, k, RestraintBatch([None], 3, atom_counts=b.counts), unwritten=("phi",), **o)
    _same_bits(empty, plain, "an all-empty restraint batch")
    assert not empty["er"].any() and empty["phi"].numel() == 0
    a = _abi(hip, b, m, k, o)
    lib, st = hip.lib, hip._stream()
    for r in (None, _lib.MdRestr(R=0)):
        ws = torch.zeros(int(lib.grappa_md_steps_restr_workspace_bytes(b.N, a["Cc"], b.B, a["n_blocks"], 0, 0, 0, 0)), dtype=torch.uint8, device="cuda")
        shapes = {"xyz": ((b.N, 3, 3), torch.float32), "vel": ((b.N, 3, 3), torch.float32), "epot": ((1, 3), torch.float32), "ekin": ((1, 3), torch.float32),
                  "steps": ((1, 3), torch.int32), "status": ((1, 3), torch.int32), "er": ((1, 3), torch.float32)}
        bufs = {kk: _guarded(*v) for kk, v in shapes.items()}
        p = {kk: v[1].data_ptr() for kk, v in bufs.items()}
        rp = None if r is None else C.byref(r)
        head = (st, C.byref(a["d"]), C.byref(a["nd"]), None, C.byref(a["mo"]), None, None, None, rp)
        tail = (a["table"].data_ptr(), a["n_items"], a["n_blocks"], ws.data_ptr(), ws.numel())
        assert lib.grappa_md_steps_init_restr_f32(*head, a["mass"].data_ptr(), a["key"].data_ptr(), None, *tail) == 0
        assert lib.grappa_md_steps_run_restr_f32(*head, a["mass"].data_ptr(), a["key"].data_ptr(), *tail, 0, 12, None, None, None, None, None, None) == 0
        assert lib.grappa_md_steps_finish_restr_f32(*head, *tail, p["xyz"], p["vel"], p["epot"], p["ekin"], p["steps"], p["status"], None, p["er"], None) == 0
        torch.cuda.synchronize()
        got = {kk: v[1].cpu().clone() for kk, v in bufs.items()}
        _same_bits(got, plain, "r == NULL" if r is None else "R == 0 and pos_k == NULL")
        assert not got["er"].any()


# ------------------------------------------------------------------------------------------------ 7. frozen atoms
def test_frozen_atoms_through_the_front_end(hip):
    """Restraints.frozen through simulate_graph: the frozen atoms keep their input bits over 25 steps, their velocities are 0, and the
    temperature divides by the reduced count of moving atoms"""
    from grappa_amd import backend
    from grappa_amd.dynamics import KB, simulate_graph
    from grappa_amd.nonbonded import NonbondedBatch
    from grappa_amd.relax import graph_from_parameters
    from test_gpu_md_steps import _parameters
    c = mr.case("s65_C3")
    b, mol = c["batch"], c["batch"].mols[0]
    old = backend._BACKEND
    backend.set_backend(hip)
    try:
        g = graph_from_parameters(_parameters(mol), mol["xyz"].transpose(1, 0, 2)).to("cuda")
        nb = NonbondedBatch([mol["nb"]]).to("cuda")
        r = simulate_graph(g, c["masses_in"], nb, keys=c["keys"], velocities=c["vel"].to("cuda"), stepwise="auto", restraints=c["rb_frozen"].to("cuda"),
                           n_steps=25, save_every=5, friction=20.0, temperature=300.0)
        assert bool((r.steps == 25).all()) and not r.status.any()
        fz = list(c["frozen"])
        assert len(fz) == 3 and torch.equal(_bits(r.xyz.cpu()[fz]), _bits(b.xyz[fz])) and not _bits(r.velocities.cpu()[fz]).any()
        rest = [a for a in range(65) if a not in fz]
        assert bool((r.xyz.cpu()[rest] != b.xyz[rest]).any(-1).all())
        want = 2.0 * r.kinetic_energy.double() / (3.0 * KB * 62)
        assert torch.allclose(r.temperature.double(), want, rtol=1e-6), "the temperature divides by the 62 moving atoms"
        # ... and it is the seam's run with the folded masses, bit for bit
        seam = _run(hip, b, c["masses"], c["keys"], c["rb"], vel=c["vel"], n_steps=25, save_every=5, friction=20.0, temperature=300.0, init_temperature=300.0)
        for f, key in (("xyz", "xyz"), ("velocities", "vel"), ("potential_energy", "epot"), ("kinetic_energy", "ekin"), ("restraint_energy", "er"),
                       ("dihedrals", "phi"), ("frames", "frames_xyz"), ("frames_restraint_energy", "frames_er"), ("frames_dihedrals", "frames_phi")):
            assert torch.equal(_bits(getattr(r, f).cpu()), _bits(seam[key])), f
    finally:
        backend.set_backend(old)


# ------------------------------------------------------------------------------------------------ 8. status 5 and refused arguments
def _replace_tables(rb, **kw):
    out = rb.to("cpu")
    for k, v in kw.items():
        setattr(out, k, v)
    out.R = int(out.dih_atoms.shape[0])
    return out


def _refusal(what):
    """-> (bad RestraintBatch, molecule, refused conformations): molecule 2 of the mixed case (17 atoms) holds rows 0 .. 15"""
    c = mr.case(mr.MIXED)
    b, rb = c["batch"], c["rb"]
    if what == "an index equal to n":
        at = rb.dih_atoms.clone()
        at[3, 1] = 17
        return _replace_tables(rb, dih_atoms=at), 2, [0, 1, 2]
    if what == "a repeated atom":
        at = rb.dih_atoms.clone()
        at[5, 2] = at[5, 0]
        return _replace_tables(rb, dih_atoms=at), 2, [0, 1, 2]
    if what == "a negative dih_k":
        k = rb.dih_k.clone()
        k[0] = -1.0
        return _replace_tables(rb, dih_k=k), 2, [0, 1, 2]
    if what == "17 rows":          # molecule 2 takes the first row of molecule 3 as its seventeenth
        ptr = rb.dih_molptr.clone()
        ptr[3] = 17
        return _replace_tables(rb, dih_molptr=ptr), 2, [0, 1, 2]
    if what == "a negative pos_k":
        pk = rb.pos_k.clone()
        pk[int(b.ptr[3]) + 1] = -2.0
        return _replace_tables(rb, pos_k=pk), 3, [0, 1, 2]
    tg = rb.dih_target.clone()          # a NaN target of conformation 1 only
    tg[7, 1] = float("nan")
    return _replace_tables(rb, dih_target=tg), 2, [1]


@pytest.mark.parametrize("what", ["an index equal to n", "a repeated atom", "a negative dih_k", "17 rows", "a negative pos_k", "a NaN target"])
def test_refused_tables_get_status_five(hip, what):
    """the refused item gets status 5 and nothing else (its outputs keep their fill, as the constraint vet leaves them); every
    neighbour's bits -- the molecule's other conformations included -- are those of the valid batch"""
    c = mr.case(mr.MIXED)
    b, rb = c["batch"], c["rb"]
    ref = mr.reference_of(b, offset=c["offset"])
    opts = dict(n_steps=10, save_every=5, **THERMO)
    good = _run(hip, b, c["masses"], c["keys"], rb, ref=ref, **opts)
    bad_rb, mol, confs = _refusal(what)
    got = _run(hip, b, c["masses"], c["keys"], bad_rb, ref=ref, **opts)
    p0, p1 = int(b.ptr[mol]), int(b.ptr[mol + 1])
    r0, r1 = int(rb.dih_molptr[mol]), int(rb.dih_molptr[mol + 1])
    for cc in confs:
        assert got["status"][mol, cc] == 5, got["status"].tolist()
        assert bool((got["xyz"][p0:p1, cc] == FILL).all()) and bool((got["vel"][p0:p1, cc] == FILL).all()) and got["steps"][mol, cc] == FILL_I
        assert got["epot"][mol, cc] == FILL and got["ekin"][mol, cc] == FILL and got["er"][mol, cc] == FILL
        assert bool((got["phi"][r0:r1, cc] == FILL).all()) and bool((got["frames_xyz"][:, p0:p1, cc] == FILL).all())
        assert bool((got["frames_er"][:, mol, cc] == FILL).all()) and bool((got["frames_phi"][:, r0:r1, cc] == FILL).all())
    rows = r1 - r0
    for j in range(b.B):
        for cc in range(3):
            if j == mol and cc in confs:
                continue
            if what == "17 rows" and j == 3:
                continue          # (its first row was given to molecule 2: another table, another run)
            a, g = _rows_of(got, b, rb, j), _rows_of(good, b, rb, j)
            for key in R_OUTS + R_FRAMES:
                sel = (lambda t: t[:, cc]) if key in ("xyz", "vel", "phi") else ((lambda t: t[:, :, cc]) if key in ("frames_xyz", "frames_phi") else (lambda t: t[..., cc]))
                assert torch.equal(_bits(sel(a[key])), _bits(sel(g[key]))), f"{what}: {key} of molecule {j}, conformation {cc} changed"
    assert rows >= 0


def test_bad_arguments_are_refused_and_nothing_is_written(hip):
    from grappa_amd import _lib
    c = mr.case("s65_C3")
    b, m, k = c["batch"], c["masses"], c["keys"]
    rb = c["rb"].to("cuda")
    o = dict(n_steps=4, save_every=2, **THERMO)
    a = _abi(hip, b, m, k, o)
    lib, st = hip.lib, hip._stream()
    need = int(lib.grappa_md_steps_restr_workspace_bytes(b.N, 3, 1, a["n_blocks"], 0, 0, 0, 0))
    wbuf = torch.full((GUARD_B + need + GUARD_B,), FILL_B, dtype=torch.uint8, device="cuda")
    ws = wbuf[GUARD_B:GUARD_B + need]
    shapes = {"xyz": ((b.N, 3, 3), torch.float32), "vel": ((b.N, 3, 3), torch.float32), "epot": ((1, 3), torch.float32), "ekin": ((1, 3), torch.float32),
              "steps": ((1, 3), torch.int32), "status": ((1, 3), torch.int32), "er": ((1, 3), torch.float32), "phi": ((1, 3), torch.float32),
              "frames_er": ((2, 1, 3), torch.float32), "frames_phi": ((2, 1, 3), torch.float32)}
    bufs = {kk: _guarded(*v) for kk, v in shapes.items()}
    p = {kk: v[1].data_ptr() for kk, v in bufs.items()}
    ref = b.xyz.to("cuda")

    def restr(**kw):
        f = dict(pos_k=rb.pos_k.data_ptr(), pos_ref=None, dih_molptr=rb.dih_molptr.data_ptr(), dih_atoms=rb.dih_atoms.data_ptr(), dih_k=rb.dih_k.data_ptr(),
                 dih_target=rb.dih_target.data_ptr(), R=1)
        f.update(kw)
        return _lib.MdRestr(**f)

    def finish(r, er=p["er"]):
        head = (st, C.byref(a["d"]), C.byref(a["nd"]), None, C.byref(a["mo"]), None, None, None, C.byref(r))
        tail = (a["table"].data_ptr(), a["n_items"], a["n_blocks"], ws.data_ptr(), ws.numel())
        return lib.grappa_md_steps_finish_restr_f32(*head, *tail, p["xyz"], p["vel"], p["epot"], p["ekin"], p["steps"], p["status"], None, er, p["phi"])

    def calls(r, er=p["er"]):
        head = (st, C.byref(a["d"]), C.byref(a["nd"]), None, C.byref(a["mo"]), None, None, None, C.byref(r))
        tail = (a["table"].data_ptr(), a["n_items"], a["n_blocks"], ws.data_ptr(), ws.numel())
        return (lib.grappa_md_steps_init_restr_f32(*head, a["mass"].data_ptr(), a["key"].data_ptr(), None, *tail),
                lib.grappa_md_steps_run_restr_f32(*head, a["mass"].data_ptr(), a["key"].data_ptr(), *tail, 0, 4, None, None, None, None, p["frames_er"],
                                                  p["frames_phi"]),
                lib.grappa_md_steps_finish_restr_f32(*head, *tail, p["xyz"], p["vel"], p["epot"], p["ekin"], p["steps"], p["status"], None, er, p["phi"]))

    before = lib.grappa_launch_count(0)
    for what, r in (("R < 0", restr(R=-1)), ("NULL dih_molptr", restr(dih_molptr=None)), ("NULL dih_atoms", restr(dih_atoms=None)),
                    ("NULL dih_k", restr(dih_k=None)), ("NULL dih_target", restr(dih_target=None)),
                    ("pos_ref without pos_k", restr(pos_k=None, pos_ref=ref.data_ptr())), ("R * C >= 2^31", restr(R=(1 << 31) // 3 + 1))):
        assert calls(r) == (-1, -1, -1), what
    assert finish(restr(), er=None) == -1, "NULL erestr"
    gbcut_alone = _lib.GbCut(cutoff=9.0, prune=1)          # a refusal of the _gbcut_ family holds here too: gbcut without gb
    head = (st, C.byref(a["d"]), C.byref(a["nd"]), None, C.byref(a["mo"]), None, None, C.byref(gbcut_alone), C.byref(restr()))
    assert lib.grappa_md_steps_init_restr_f32(*head, a["mass"].data_ptr(), a["key"].data_ptr(), None, a["table"].data_ptr(), a["n_items"], a["n_blocks"],
                                              ws.data_ptr(), ws.numel()) == -1
    short = (st, C.byref(a["d"]), C.byref(a["nd"]), None, C.byref(a["mo"]), None, None, None, C.byref(restr()))
    assert lib.grappa_md_steps_init_restr_f32(*short, a["mass"].data_ptr(), a["key"].data_ptr(), None, a["table"].data_ptr(), a["n_items"], a["n_blocks"],
                                              ws.data_ptr(), ws.numel() - 1) == -3, "a workspace one byte short"
    torch.cuda.synchronize()
    assert lib.grappa_launch_count(0) == before, "a refused call launched something"
    for kk, (buf, _) in bufs.items():
        assert bool((buf == _fill_of(buf)).all()), f"{kk} was written by a refused call"
    assert bool((wbuf == FILL_B).all()), "a refused call wrote to the workspace"
    assert calls(restr(pos_ref=ref.data_ptr())) == (0, 0, 0)          # the complete sequence is accepted
    torch.cuda.synchronize()
    assert bool((bufs["status"][1] == 0).all()) and not bool((bufs["frames_er"][1] == FILL).any()) and not bool((bufs["er"][1] == FILL).any())
    assert bool((wbuf[:GUARD_B] == FILL_B).all()) and bool((wbuf[-GUARD_B:] == FILL_B).all())


# ------------------------------------------------------------------------------------------------ 9. the public door
def test_grappa_simulate_runs_umbrella_windows(hip):
    """Grappa.simulate on the golden molecule: C = 6 windows of one dihedral, 200 steps of 2 fs with h-bonds in obc2, frames every 20"""
    from grappa_amd import Grappa, GrappaModel, backend
    from grappa_amd.constants import ATOMIC_MASSES
    from grappa_amd.constraints import hydrogen_constraints
    from grappa_amd.dynamics import simulate
    from grappa_amd.nonbonded import NonbondedParameters
    from grappa_amd.restraints import rotating_side
    from grappa_amd.solvent import GBParameters
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
        p = wrapper.predict(mol)
        n = len(z)
        heavy = lambda row: all(z[pos[int(a)]] > 1 for a in row)      # noqa: E731
        dih = next(row for row in np.asarray(p.propers).reshape(-1, 4).tolist()
                   if heavy(row) and rotating_side(n, np.asarray(bonds), pos[row[1]], pos[row[2]]) is not None)
        idx = [pos[int(a)] for a in dih]
        low = wrapper.relax(mol, np.ascontiguousarray(mm["xyz"].transpose(1, 0, 2)[:1]), nbp)
        xyz = np.ascontiguousarray(np.repeat(low.xyz, 6, axis=0))
        from grappa_amd.restraints import dihedral_angle
        phi0 = dihedral_angle(xyz[0], *idx)
        targets = np.mod(phi0 + np.deg2rad(10.0) * np.arange(6) + np.pi, 2 * np.pi) - np.pi
        res = Restraints(dihedrals=[idx], dihedral_k=[239.0], dihedral_targets=targets[None, :])
        kw = dict(n_steps=200, save_every=20, dt=0.002, seed=9, stepwise="auto", implicit_solvent="obc2")
        r = wrapper.simulate(mol, xyz, nbp, constraints="h-bonds", restraints=res, **kw)
        assert r.xyz.shape == xyz.shape and bool((r.steps == 200).all()) and not r.status.any()
        assert r.restraint_energy.shape == (6,) and bool((r.restraint_energy >= 0).all()) and r.dihedrals.shape == (1, 6)
        assert r.frames_restraint_energy.shape == (6, 10) and r.frames_dihedrals.shape == (1, 6, 10) and bool(np.isfinite(r.frames_dihedrals).all())
        assert r.esolv.shape == (6,) and bool(np.isfinite(r.potential_energy).all())
        masses = [ATOMIC_MASSES[int(a)] for a in z]
        gbp = GBParameters.from_elements(mol.atomic_numbers, bonds)
        s = simulate(p, xyz, masses, nbp, device="cuda", constraints=hydrogen_constraints(p, mol.atomic_numbers), restraints=res, gb=gbp, **kw)
        for f in ("xyz", "velocities", "potential_energy", "kinetic_energy", "restraint_energy", "dihedrals", "frames", "frames_restraint_energy",
                  "frames_dihedrals", "esolv"):
            assert np.array_equal(getattr(r, f), getattr(s, f)), f
        wrap = lambda a: np.mod(a + np.pi, 2 * np.pi) - np.pi      # noqa: E731
        off = np.abs(wrap(r.frames_dihedrals[0] - targets[:, None])).mean(axis=1)
        print(f"umbrella windows at {np.round(targets, 3).tolist()} rad: time-averaged |phi - target| per window {np.round(off, 4).tolist()} rad; "
              f"E_r at the end {np.round(r.restraint_energy, 3).tolist()} kcal/mol")
    finally:
        backend.set_backend(old)
