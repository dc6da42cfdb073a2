"""GPU: the fused Langevin dynamics (csrc/dynamics.hip through HipBackend.md_langevin / md_noise and grappa_amd/dynamics.py) against
the restatement of tests/md_refs.py, inside sentinel-guarded output buffers.

Gates.  Noise: |z_gpu - z_f64| <= 2^-16 (r <= 5.9; the angle is exact in half turns and sincospi is good to a few ulp: below 3e-6;
the logarithm's error: below 1e-6; 2^-16 = 1.5e-5 leaves margin).  Trajectories: per (molecule, conformation),
max_atoms |x_gpu - x_f64| <= 4 max_atoms |x_f32 restatement - x_f64| + 2^-20 A, and the same for v with the floor 2^-20 max_atoms |v|:
the gate of tests/test_gpu_relax.py (one ulp of a coordinate below 16 A; the factor is twice the elementwise gate's because the error
accumulates over steps in another summation order).  That gate is asserted as it stands wherever the fp32 restatement is a steady
yardstick: where its own siblings (md_refs.fp32_realisations: the same input turned rigidly about the centroid, so the same
magnitudes and other roundings) all lie within the gate of the unturned fp32 run.  Where one of them does not -- the gate would refuse
the restatement itself, because the trajectory amplifies roundings too strongly for one fp32 run to say how far fp32 strays -- the
farthest sibling calibrates instead, with the same factor and floor (a deviation from the issue, confined to those items; DESIGN.md
section 12 has the figures).  The ratios are printed per case.  Energies: relax_refs.gate_forces.
Kinetic energy and start velocities: 8 u32 relative to float64.  The conservation and equipartition bounds are stated at their tests."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_utils as gu
import kernel_refs as kr
import md_refs as md
import relax_refs as rr

pytestmark = pytest.mark.gpu

FILL, FILL_I = 1024.0, 12345       # sentinels around (and, before the call, inside) every output buffer
TRAJ_FACTOR = 4
ULP_X = 2.0 ** -20
NOISE_TOL = 2.0 ** -16
OUTS = ("xyz", "vel", "epot", "ekin", "steps", "status")
FRAMES = ("frames_xyz", "frames_epot", "frames_ekin")


@pytest.fixture(scope="module")
def hip():
    from grappa_amd.backend import HipBackend
    return HipBackend()


def _guarded(shape, dtype=torch.float32, guard=64):
    n = int(np.prod(shape))
    buf = torch.full((guard + n + guard,), FILL_I if dtype == torch.int32 else FILL, dtype=dtype, device="cuda")
    return buf, buf[guard:guard + n].view(*shape)


def _guards_hold(bufs):
    for k, (buf, _) in bufs.items():
        fill = FILL_I if buf.dtype == torch.int32 else FILL
        assert bool((buf[:64] == fill).all()) and bool((buf[-64:] == fill).all()), f"written outside {k}"


def _dev_keys(keys):
    return torch.from_numpy(np.asarray(keys, dtype=np.uint64).view(np.int64).copy()).to("cuda")


def _run(hip, batch, masses, keys, vel=None, xyz=None, nb="full", counts=False, expect_written=True, **opts):
    """one call of the seam on a relax_refs.Batch -> dict of CPU tensors (OUTS, and FRAMES when save_every > 0); asserts the guards.
    vel: (N,C,3) CPU tensor or None (velocities drawn at init_temperature); xyz: start coordinates other than the batch's"""
    o = {**md.MD_OPTS, **opts}
    plan = batch.plan("cuda")
    dnb = None if nb is None else batch.nonbonded(zero=nb == "zero").to("cuda")
    x = (batch.xyz if xyz is None else xyz).to("cuda")
    N, Cc, B = batch.N, x.shape[1], batch.B
    F = o["n_steps"] // o["save_every"] if o["save_every"] > 0 and o["n_steps"] > 0 else 0
    shapes = {"xyz": ((N, Cc, 3), torch.float32), "vel": ((N, Cc, 3), torch.float32), "epot": ((B, Cc), torch.float32),
              "ekin": ((B, Cc), torch.float32), "steps": ((B, Cc), torch.int32), "status": ((B, Cc), torch.int32)}
    if F:
        shapes.update({"frames_xyz": ((F, N, Cc, 3), torch.float32), "frames_epot": ((F, B, Cc), torch.float32),
                       "frames_ekin": ((F, B, Cc), torch.float32)})
    bufs = {k: _guarded(*v) for k, v in shapes.items()}
    out = {k: v[1] for k, v in bufs.items()}
    ks = [k.to("cuda") for k in batch.ks]
    eqs = [None if q is None else q.to("cuda") for q in batch.eqs]
    try:
        hip.md_langevin(plan, x, ks, eqs, batch.n_per, False, dnb, o, torch.from_numpy(np.asarray(masses, dtype=np.float32)).to("cuda"),
                        _dev_keys(keys), None if vel is None else vel.to("cuda"), out["xyz"], out["vel"], out["epot"], out["ekin"], out["steps"],
                        out["status"], frames_xyz=out.get("frames_xyz"), frames_epot=out.get("frames_epot"), frames_ekin=out.get("frames_ekin"),
                        atom_counts_host=batch.counts if counts else None)
    except Exception:          # a refused call has written nothing
        torch.cuda.synchronize()
        for name, (buf, _) in bufs.items():
            assert bool((buf == (FILL_I if buf.dtype == torch.int32 else FILL)).all()), f"a refused call wrote {name}"
        raise
    torch.cuda.synchronize()
    _guards_hold(bufs)
    if expect_written:
        for k in OUTS:
            if out[k].numel():
                assert not bool((out[k] == (FILL_I if out[k].dtype == torch.int32 else FILL)).all()), f"{k} was not written"
    return {k: v.cpu().clone() for k, v in out.items()}


def _noise(hip, counts, keys, Cc, step, purpose):
    """md_noise on a batch with `counts` atoms per molecule -> (N, Cc, 3) CPU tensor; asserts the guards"""
    ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to("cuda")
    buf, view = _guarded((int(sum(counts)), Cc, 3))
    hip.md_noise(_dev_keys(keys), ptr, Cc, step, purpose, view)
    torch.cuda.synchronize()
    _guards_hold({"noise": (buf, view)})
    return view.cpu().clone()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b, what, keys=OUTS):
    for k in keys:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs"


def _rows_of(out, batch, b):
    """molecule b's part of every output"""
    p0, p1 = int(batch.ptr[b]), int(batch.ptr[b + 1])
    rows = {"xyz": out["xyz"][p0:p1], "vel": out["vel"][p0:p1], **{k: out[k][b] for k in ("epot", "ekin", "steps", "status")}}
    if "frames_xyz" in out:
        rows.update({"frames_xyz": out["frames_xyz"][:, p0:p1], "frames_epot": out["frames_epot"][:, b], "frames_ekin": out["frames_ekin"][:, b]})
    return rows


def _item_max(batch, t):
    """(N, C, 3) -> (B, C): the largest row norm of each (molecule, conformation)"""
    return torch.stack([t[int(batch.ptr[k]):int(batch.ptr[k + 1])].double().norm(dim=-1).max(0).values for k in range(batch.B)])


def _gate_state(name, what, batch, got, r64, r32s):
    """x and v of a run against the float64 restatement's (xyz, vel) through the trajectory gate.  r32s: md_refs.fp32_realisations at
    that step (pairs of an fp32 state and the float64 state of the same input; the first is the input as it is, the others its
    rotations).  An item whose rotated siblings all pass the gate of the unturned fp32 run is held to that run alone, as the issue
    states the gate; any other item to the farthest of them."""
    for k, label, idx in (("xyz", "x", 0), ("vel", "v", 1)):
        dg = _item_max(batch, got[k].double() - r64[idx])
        each = torch.stack([_item_max(batch, r32[idx].double() - own64[idx]) for r32, own64 in r32s])
        floor = ULP_X * (1.0 if k == "xyz" else _item_max(batch, r64[idx])) * torch.ones_like(dg)
        steady = (each[1:] <= TRAJ_FACTOR * each[0] + floor).all(0)
        dr = torch.where(steady, each[0], each.max(0).values)
        ratio = (dg - floor).clamp_min(0) / dr.clamp_min(1e-300)
        alone = (dg - floor).clamp_min(0) / each[0].clamp_min(1e-300)
        print(f"{name} {what}: max |{label}_gpu - {label}_f64| {float(dg.max()):.3e}, |{label}_f32 - {label}_f64| {float(each[0].max()):.3e}; "
              f"{int(steady.sum())} of {steady.numel()} items steady, largest (|gpu| - floor) / |f32| = "
              f"{float(ratio[steady].max()) if bool(steady.any()) else 0.0:.3f}; the others against the farthest sibling "
              f"{float(ratio[~steady].max()) if bool((~steady).any()) else 0.0:.3f} (against the unturned run {float(alone[~steady].max()) if bool((~steady).any()) else 0.0:.3f})")
        assert bool(torch.isfinite(got[k]).all())
        bad = dg > TRAJ_FACTOR * dr + floor
        assert not bool(bad.any()), (f"{name} {what}: {int(bad.sum())} items' {label} outside {TRAJ_FACTOR} x fp32 + floor: gpu {dg[bad].tolist()} "
                                     f"fp32 {dr[bad].tolist()} steady {steady[bad].tolist()}")


# ------------------------------------------------------------------------------------------------ 1. noise
@pytest.mark.parametrize("name", ["mixed", "edge256", "n9_C64"])
def test_noise_against_the_restatement(hip, name):
    b = md.case(name)
    Cc = b.xyz.shape[1]
    for step, purpose in ((0, 0), (0, 1), (12345, 0), (2 ** 32 - 1, 1)):
        got = _noise(hip, b.counts, md.keys(name), Cc, step, purpose)
        want = md.noise_ref(b.counts, md.keys(name), Cc, step, purpose)
        err = float((got.double() - want).abs().max())
        print(f"{name} step {step} purpose {purpose}: max |z_gpu - z_f64| = {err:.3e}")
        assert err <= NOISE_TOL


def test_noise_is_standard_normal_and_keyed(hip):
    """98,304 values (512 atoms x 64 conformations): |mean| <= 5 / sqrt(n), |var - 1| <= 5 sqrt(2 / n) (the restatement itself is inside
    both: tests/test_md_refs.py); purposes, steps and keys give different tensors"""
    k = md.keys("max")
    z = _noise(hip, [512], k, 64, 3, 0)
    assert float((z.double() - md.noise_ref([512], k, 64, 3, 0)).abs().max()) <= NOISE_TOL
    flat = z.double().reshape(-1)
    n = flat.numel()
    print(f"n = {n}: mean {float(flat.mean()):.3e} (bound {5 / np.sqrt(n):.3e}), var - 1 {float(flat.var()) - 1:.3e} (bound {5 * np.sqrt(2 / n):.3e})")
    assert n == 98304 and abs(float(flat.mean())) <= 5 / np.sqrt(n) and abs(float(flat.var(unbiased=False)) - 1) <= 5 * np.sqrt(2 / n)
    others = [_noise(hip, [512], k, 64, 3, 1), _noise(hip, [512], k, 64, 4, 0), _noise(hip, [512], md.keys("mixed")[:1], 64, 3, 0)]
    for o in others:
        assert not bool((o == z).any())
    assert torch.equal(_bits(z), _bits(_noise(hip, [512], k, 64, 3, 0)))


# ------------------------------------------------------------------------------------------------ 2. step zero
@pytest.mark.parametrize("name", md.CASES)
def test_step_zero(hip, name):
    """n_steps = 0: coordinates and velocities come back bit for bit, epot passes the calibrated gate, ekin is float64's within 8 u32"""
    b, m, v = md.case(name), md.masses(name), md.thermal_velocities(name)
    got = _run(hip, b, m, md.keys(name), vel=v, n_steps=0, friction=5.0)
    assert torch.equal(_bits(got["xyz"]), _bits(b.xyz)) and torch.equal(_bits(got["vel"]), _bits(v))
    assert not got["steps"].any() and not got["status"].any()
    rr.gate_forces(got["epot"], None, None, md.forces_of(name, torch.float64), md.forces_of(name, torch.float32), name)
    want = md.kinetic(b, torch.from_numpy(m).double(), v)
    assert bool(((got["ekin"].double() - want).abs() <= 8 * kr.U32 * want).all()), (got["ekin"].tolist(), want.tolist())


@pytest.mark.parametrize("name", ["mixed", "edge256", "max"])
def test_step_zero_potential_energy_has_the_minimiser_s_bits(hip, name):
    """n_steps = 0 against relax_fire at max_steps = 0 on the same coordinates: both kernels take the energy from the one sum of
    csrc/rx_force.h (rx_energies), so epot and energy are the same bits, with the nonbonded tables and without them"""
    from grappa_amd.relax import RELAX_DEFAULTS
    b, m = md.case(name), md.masses(name)
    plan, x = b.plan("cuda"), b.xyz.to("cuda")
    ks, eqs = [k.to("cuda") for k in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    for nb in ("full", None):
        got = _run(hip, b, m, md.keys(name), vel=md.thermal_velocities(name), nb=nb, n_steps=0)
        xo, e, gm = torch.empty_like(x), torch.zeros(b.B, x.shape[1], device="cuda"), torch.zeros(b.B, x.shape[1], device="cuda")
        st, ss = torch.zeros_like(e, dtype=torch.int32), torch.zeros_like(e, dtype=torch.int32)
        hip.relax_fire(plan, x, ks, eqs, b.n_per, False, None if nb is None else b.nonbonded().to("cuda"),
                       {**RELAX_DEFAULTS, "max_steps": 0, "tolerance": 0.0}, xo, e, gm, st, ss)
        assert torch.equal(_bits(got["epot"]), _bits(e.cpu())), f"{name} nb={nb}: epot {got['epot'].tolist()} energy {e.cpu().tolist()}"


# ------------------------------------------------------------------------------------------------ 3. trajectories, no thermostat
TRAJ = [(n, s) for n in md.CASES for s in md.TRAJ_STEPS]


@pytest.mark.parametrize("name,n_steps", TRAJ, ids=[f"{n}-{s}steps" for n, s in TRAJ])
def test_trajectory_without_thermostat(hip, name, n_steps):
    """friction = 0 (velocity Verlet), dt = 1 fs, from the case coordinates with thermal velocities"""
    b = md.case(name)
    r64, r32s = md.verlet(name)[n_steps], [r[n_steps] for r in md.verlet32(name)]
    got = _run(hip, b, md.masses(name), md.keys(name), vel=md.thermal_velocities(name), n_steps=n_steps, dt=0.001)
    assert bool((got["steps"] == n_steps).all()) and not got["status"].any()
    _gate_state(name, f"{n_steps} steps, friction 0", b, got, r64, r32s)


# ------------------------------------------------------------------------------------------------ 4. trajectories with the thermostat
@pytest.mark.parametrize("name", md.CASES)
def test_trajectory_with_thermostat(hip, name):
    """friction 50 / ps at 300 K: the restatements consume the noise md_noise wrote for these steps (gated in 1.), so only the integrator
    is under test"""
    b, Cc = md.case(name), md.case(name).xyz.shape[1]
    first, total = 7, max(md.TRAJ_STEPS)
    z = {first + k: _noise(hip, b.counts, md.keys(name), Cc, first + k, 0).double() for k in range(total)}
    opts = dict(friction=50.0, temperature=300.0, dt=0.001, first_step=first)
    common = dict(velocities=md.thermal_velocities(name), noise=lambda step, purpose: z[step], n_steps=total, **opts)
    r64 = md.baoab_ref(b, md.masses(name), torch.float64, snapshots=md.TRAJ_STEPS, **common)["snap"]
    r32s = md.fp32_realisations(b, md.masses(name), md.TRAJ_STEPS, **common)
    for n_steps in md.TRAJ_STEPS:
        got = _run(hip, b, md.masses(name), md.keys(name), vel=md.thermal_velocities(name), n_steps=n_steps, **opts)
        assert bool((got["steps"] == n_steps).all()) and not got["status"].any()
        _gate_state(name, f"{n_steps} steps, friction 50", b, got, r64[n_steps], [r[n_steps] for r in r32s])


# ------------------------------------------------------------------------------------------------ 5. start velocities
@pytest.mark.parametrize("name", ["mixed", "edge256"])
def test_start_velocities(hip, name):
    b, m, Cc = md.case(name), md.masses(name), md.case(name).xyz.shape[1]
    first = 11
    got = _run(hip, b, m, md.keys(name), n_steps=0, init_temperature=250.0, first_step=first)
    z = _noise(hip, b.counts, md.keys(name), Cc, first, 1).double()
    want = torch.sqrt(md.ACC * md.KB * 250.0 / torch.from_numpy(m).double())[:, None, None] * z
    assert torch.equal(_bits(got["xyz"]), _bits(b.xyz))
    assert bool(((got["vel"].double() - want).abs() <= 8 * kr.U32 * want.abs()).all())
    ke = md.kinetic(b, torch.from_numpy(m).double(), got["vel"])
    assert bool(((got["ekin"].double() - ke).abs() <= 8 * kr.U32 * ke).all())
    cold = _run(hip, b, m, md.keys(name), n_steps=0, init_temperature=0.0)
    assert not _bits(cold["vel"]).any() and not _bits(cold["ekin"]).any()


# ------------------------------------------------------------------------------------------------ 6. continuation
@pytest.mark.parametrize("friction", [0.0, 20.0])
@pytest.mark.parametrize("name", ["mixed", "edge256"])
def test_continuation(hip, name, friction):
    """40 steps in one call = 20 + 20 with vel_in = vel_out, xyz = xyz_out, first_step advanced: the same bits, frames included"""
    b, m, k = md.case(name), md.masses(name), md.keys(name)
    opts = dict(friction=friction, temperature=300.0, init_temperature=300.0, save_every=5)
    whole = _run(hip, b, m, k, n_steps=40, first_step=3, **opts)
    one = _run(hip, b, m, k, n_steps=20, first_step=3, **opts)
    two = _run(hip, b, m, k, vel=one["vel"], xyz=one["xyz"], n_steps=20, first_step=23, **opts)
    _same_bits(whole, two, "40 steps against 20 + 20", keys=("xyz", "vel", "epot", "ekin", "status"))
    assert bool((one["steps"] == 20).all()) and bool((two["steps"] == 20).all()) and bool((whole["steps"] == 40).all())
    for key in FRAMES:
        assert torch.equal(_bits(whole[key]), _bits(torch.cat([one[key], two[key]]))), key
    assert not torch.equal(_bits(whole["xyz"]), _bits(one["xyz"]))


def _parameters(mol):
    from grappa_amd.parameters import Parameters
    ids = np.arange(mol["n"])
    k3, k4 = mol["ks"][2].astype(np.float64), mol["ks"][3].astype(np.float64)
    return Parameters(atoms=ids, bonds=mol["idx"][0], bond_k=mol["ks"][0], bond_eq=mol["eqs"][0], angles=mol["idx"][1], angle_k=mol["ks"][1],
                      angle_eq=mol["eqs"][1], propers=mol["idx"][2], proper_ks=np.abs(k3), proper_phases=np.where(k3 >= 0, 0.0, np.pi),
                      impropers=mol["idx"][3], improper_ks=np.abs(k4), improper_phases=np.where(k4 >= 0, 0.0, np.pi))


RESULT_FIELDS = ("xyz", "velocities", "potential_energy", "kinetic_energy", "temperature", "steps", "status", "frames", "frame_potential_energy",
                 "frame_kinetic_energy")


def test_simulate_graph_does_not_depend_on_steps_per_launch(hip):
    from grappa_amd import backend
    from grappa_amd.dynamics import simulate_graph
    from grappa_amd.nonbonded import NonbondedBatch
    from grappa_amd.relax import graph_from_parameters
    old = backend._BACKEND
    backend.set_backend(hip)
    try:
        mol = md.case("n33_C3").mols[0]
        g = graph_from_parameters(_parameters(mol), mol["xyz"].transpose(1, 0, 2)).to("cuda")
        nb = NonbondedBatch([mol["nb"]]).to("cuda")
        runs = [simulate_graph(g, md.masses("n33_C3"), nb, seed=5, n_steps=40, save_every=5, friction=20.0, steps_per_launch=s) for s in (10, 40, 13)]
        assert bool((runs[0].steps == 40).all()) and not runs[0].status.any() and runs[0].frames.shape == (8, 33, 3, 3)
        assert bool(torch.isfinite(runs[0].frames).all()) and bool(torch.isfinite(runs[0].frame_kinetic_energy).all())
        for r in runs[1:]:
            for f in RESULT_FIELDS:
                assert torch.equal(_bits(getattr(r, f)), _bits(getattr(runs[0], f))), f
    finally:
        backend.set_backend(old)


# ------------------------------------------------------------------------------------------------ 7. frames
def test_frames_are_the_states_of_shorter_runs(hip):
    b, m, k = md.case("mixed"), md.masses("mixed"), md.keys("mixed")
    opts = dict(friction=20.0, temperature=300.0, init_temperature=300.0)
    whole = _run(hip, b, m, k, n_steps=40, save_every=5, **opts)
    assert whole["frames_xyz"].shape[0] == 8
    for f in range(8):
        part = _run(hip, b, m, k, n_steps=5 * (f + 1), **opts)
        assert torch.equal(_bits(whole["frames_xyz"][f]), _bits(part["xyz"])), f"frame {f}: coordinates"
        assert torch.equal(_bits(whole["frames_epot"][f]), _bits(part["epot"])), f"frame {f}: potential energy"
        assert torch.equal(_bits(whole["frames_ekin"][f]), _bits(part["ekin"])), f"frame {f}: kinetic energy"
    assert torch.equal(_bits(whole["frames_ekin"][7]), _bits(whole["ekin"])) and torch.equal(_bits(whole["frames_xyz"][7]), _bits(whole["xyz"]))
    # 42 steps: still 8 frames, and the run goes on after the last one
    longer = _run(hip, b, m, k, n_steps=42, save_every=5, **opts)
    _same_bits(longer, whole, "the frames of 42 and of 40 steps", keys=FRAMES)
    assert not torch.equal(_bits(longer["xyz"]), _bits(whole["xyz"]))


# ------------------------------------------------------------------------------------------------ 8. bits
def test_same_input_same_bits_whatever_the_neighbours_do(hip):
    mixed, m, k = md.case("mixed"), md.masses("mixed"), md.keys("mixed")          # sizes 1, 2, 17, 65, 5
    opts = dict(n_steps=30, save_every=10, friction=20.0, temperature=300.0, init_temperature=300.0)
    a, a2 = _run(hip, mixed, m, k, **opts), _run(hip, mixed, m, k, **opts)
    _same_bits(a, a2, "two runs", keys=OUTS + FRAMES)
    ptr = mixed.ptr
    sub_m = lambda order: np.concatenate([m[int(ptr[j]):int(ptr[j + 1])] for j in order])      # noqa: E731
    alone = _rows_of(_run(hip, mixed.subset([2]), sub_m([2]), k[[2]], **opts), mixed.subset([2]), 0)
    for order in ([2, 0, 3], [3, 0, 2], [4, 2]):
        sub = mixed.subset(order)
        _same_bits(_rows_of(_run(hip, sub, sub_m(order), k[order], **opts), sub, order.index(2)), alone, f"molecule 2 in {order}", keys=OUTS + FRAMES)
    _same_bits(_rows_of(a, mixed, 2), alone, "molecule 2 in the whole batch", keys=OUTS + FRAMES)
    # another key: another trajectory
    other = _run(hip, mixed.subset([2]), sub_m([2]), k[[3]], **opts)
    assert not torch.equal(_bits(other["xyz"]), _bits(alone["xyz"]))


# ------------------------------------------------------------------------------------------------ 9. frozen atoms
def test_frozen_atoms(hip):
    b, m, v = md.case("n9_C3"), md.masses("n9_C3").copy(), md.thermal_velocities("n9_C3")
    m[[0, 4]] = 0.0
    for friction in (0.0, 20.0):
        got = _run(hip, b, m, md.keys("n9_C3"), vel=v, n_steps=25, friction=friction, temperature=300.0)
        assert not got["status"].any() and bool((got["steps"] == 25).all())
        for a in (0, 4):
            assert torch.equal(_bits(got["xyz"][a]), _bits(b.xyz[a])) and not _bits(got["vel"][a]).any()
        rest = [a for a in range(9) if a not in (0, 4)]
        assert bool((got["xyz"][rest] != b.xyz[rest]).all()) and bool(torch.isfinite(got["xyz"]).all()) and bool(torch.isfinite(got["epot"]).all())
        if friction == 0.0:
            r64 = md.baoab_ref(b, m, velocities=v, n_steps=25, snapshots=(25,))["snap"][25]
            _gate_state("n9_C3", "25 steps, two frozen atoms", b, got, r64, [r[25] for r in md.fp32_realisations(b, m, (25,), velocities=v, n_steps=25)])


# ------------------------------------------------------------------------------------------------ 10. failure and refusals
def _with_coincident(batch, mol, i, j):
    mols = [dict(mm) for mm in batch.mols]
    x = mols[mol]["xyz"].copy()
    x[j] = x[i]
    mols[mol]["xyz"] = x
    return rr.Batch(mols)


def test_coincident_atoms(hip):
    base, m, k = md.case("mixed"), md.masses("mixed"), md.keys("mixed")
    pairs = {tuple(p) for p in base.params[2].exception_idx.tolist()}
    assert (0, 16) not in pairs          # 0 and 16 of molecule 2 interact in full
    opts = dict(n_steps=20, save_every=5, friction=20.0, temperature=300.0, init_temperature=300.0)
    plain = _run(hip, base, m, k, **opts)
    moved = _with_coincident(base, 2, 0, 16)
    hit = _run(hip, moved, m, k, **opts)
    assert bool((hit["status"][2] == 2).all()) and not hit["steps"][2].any()
    assert hit["status"][[0, 1, 3, 4]].any().item() is False
    for j in (0, 1, 3, 4):          # the other molecules: unaffected, bit for bit
        _same_bits(_rows_of(hit, base, j), _rows_of(plain, base, j), f"molecule {j} beside a non-finite one", keys=OUTS + FRAMES)
    p0 = int(base.ptr[2])
    assert torch.equal(_bits(hit["xyz"][p0:p0 + 17]), _bits(moved.xyz[p0:p0 + 17])), "status 2 returns the coordinates it holds"
    # its frames were never reached: the guard pattern stands
    assert bool((hit["frames_xyz"][:, p0:p0 + 17] == FILL).all()) and bool((hit["frames_epot"][:, 2] == FILL).all()) and bool((hit["frames_ekin"][:, 2] == FILL).all())


def test_a_molecule_above_the_limit_is_refused(hip):
    from grappa_amd import backend
    from grappa_amd.dynamics import simulate_graph
    from grappa_amd.relax import graph_from_parameters
    n = rr.max_atoms() + 1
    big = rr.gen_molecule(n, 1, np.random.default_rng(5))
    b = rr.Batch([big, md.case("n9_C1").mols[0]])
    m = np.concatenate([np.full(n, 12.011, dtype=np.float32), md.masses("n9_C1")])
    k = md.keys("mixed")[:2]
    before = hip.lib.grappa_launch_count(0)
    with pytest.raises(ValueError, match="above the limit"):          # the caller knows the sizes on the host: nothing is launched
        _run(hip, b, m, k, counts=True, n_steps=5)
    old = backend._BACKEND
    backend.set_backend(hip)
    try:
        g = graph_from_parameters(_parameters(big), big["xyz"].transpose(1, 0, 2)).to("cuda")
        with pytest.raises(ValueError, match="above the limit"):
            simulate_graph(g, m[:n], n_steps=5)
    finally:
        backend.set_backend(old)
    assert hip.lib.grappa_launch_count(0) == before
    # without host sizes the kernel marks the item: status 3 and nothing else written for it; its neighbour runs as if alone
    got = _run(hip, b, m, k, n_steps=5, save_every=5)
    assert got["status"].flatten().tolist() == [3, 0]
    assert bool((got["xyz"][:n] == FILL).all()) and bool((got["vel"][:n] == FILL).all()) and got["steps"][0, 0] == FILL_I
    assert got["epot"][0, 0] == FILL and got["ekin"][0, 0] == FILL and bool((got["frames_xyz"][:, :n] == FILL).all())
    nine = md.case("n9_C1")
    _same_bits(_rows_of(got, b, 1), _rows_of(_run(hip, nine, md.masses("n9_C1"), k[1:], n_steps=5, save_every=5), nine, 0),
               "the neighbour of a refused molecule", keys=OUTS + FRAMES)


def test_bad_options_and_pointers_are_refused(hip):
    from grappa_amd import _lib
    from grappa_amd.backend import GrappaHipError
    b, m, k = md.case("n9_C1"), md.masses("n9_C1"), md.keys("n9_C1")
    for bad in ({"dt": 0.0}, {"dt": -0.001}, {"dt": float("nan")}, {"dt": float("inf")}, {"temperature": -1.0}, {"temperature": float("nan")},
                {"temperature": float("inf")}, {"friction": -1.0}, {"friction": float("nan")}, {"init_temperature": -1.0},
                {"init_temperature": float("inf")}, {"n_steps": -1}, {"n_steps": 1000001}, {"save_every": -1},
                {"first_step": 2 ** 32 - 1, "n_steps": 1}, {"first_step": 2 ** 32 - 5, "n_steps": 5}):
        with pytest.raises(GrappaHipError, match="GRAPPA_ERR_ARG"):
            _run(hip, b, m, k, **{"n_steps": 3, **bad})
    _run(hip, b, m, k, first_step=2 ** 32 - 5, n_steps=4)          # the last admissible step index is accepted
    # the C ABI itself: NULL pointers, a nonbonded table of another shape, B * C = 2^31
    plan, x = b.plan("cuda"), b.xyz.to("cuda")
    ks, eqs = [t.to("cuda") for t in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    d = hip._mm_desc(plan, x, ks, eqs, b.n_per, False)
    o = _lib.MdOpts(dt=0.001, temperature=300.0, friction=1.0, init_temperature=300.0, n_steps=3, save_every=0, first_step=0)
    mass, key = torch.from_numpy(m).to("cuda"), _dev_keys(k)
    out = {n: _guarded(s, t) for n, (s, t) in {"x": ((9, 1, 3), torch.float32), "v": ((9, 1, 3), torch.float32), "ep": ((1, 1), torch.float32),
                                                "ek": ((1, 1), torch.float32), "s": ((1, 1), torch.int32), "st": ((1, 1), torch.int32)}.items()}
    full = [C.byref(o), mass.data_ptr(), key.data_ptr(), None] + [out[n][1].data_ptr() for n in ("x", "v", "ep", "ek", "s", "st")]

    def call(args, desc=d, nb=None):
        return hip.lib.grappa_md_langevin_f32(hip._stream(), C.byref(desc), nb, *args, None, None, None)

    for drop in (0, 1, 2, 4, 5, 6, 7, 8, 9):          # o and every required array in turn (3 is vel_in, which may be NULL)
        args = list(full)
        args[drop] = None
        assert call(args) == -1, drop
    assert hip.lib.grappa_md_langevin_f32(hip._stream(), None, None, *full, None, None, None) == -1          # mm == NULL
    for shape in ((9, 2, 1), (8, 1, 1), (9, 1, 2)):          # nb disagreeing with mm in C, in N, in B
        nd = _lib.NbDesc()
        nd.N, nd.C, nd.B = shape
        assert call(full, nb=C.byref(nd)) == -1, shape
    wide = _lib.MMDesc.from_buffer_copy(d)
    wide.B, wide.C = 1 << 16, 1 << 15
    assert call(full, desc=wide) == -1
    torch.cuda.synchronize()
    for buf, view in out.values():
        assert bool((buf == (FILL_I if buf.dtype == torch.int32 else FILL)).all()), "a refused call wrote"
    assert call(full) == 0          # the complete call is accepted
    torch.cuda.synchronize()
    _guards_hold(out)
    assert int(out["s"][1][0, 0]) == 3 and int(out["st"][1][0, 0]) == 0


# ------------------------------------------------------------------------------------------------ 11. energy conservation
def test_energy_conservation(hip):
    """NVE on the 64 replicas: 2000 steps of 0.5 fs, a frame every 50.  D = max over frames and items of |E_tot - E_tot at step 0|;
    D_gpu <= 2 max(D of the fp32 restatement, D of the float64 restatement): D is the integrator's O(dt^2) band, the same in all
    three, and the factor covers the different summation orders of kernel and restatement"""
    b, m, k, v = md.case("n9_C64"), md.masses("n9_C64"), md.keys("n9_C64"), md.thermal_velocities("n9_C64")
    start = _run(hip, b, m, k, vel=v, n_steps=0)
    got = _run(hip, b, m, k, vel=v, **md.NVE)
    assert not got["status"].any() and bool((got["steps"] == md.NVE["n_steps"]).all())
    d_gpu = md.drift(start["epot"].double() + start["ekin"].double(), got["frames_epot"].double() + got["frames_ekin"].double())
    d32, d64 = md.nve_drift(torch.float32), md.nve_drift(torch.float64)
    print(f"energy conservation: D_gpu {d_gpu:.4f}, D_f32 {d32:.4f}, D_f64 {d64:.4f} kcal/mol, D_gpu / max = {d_gpu / max(d32, d64):.3f}")
    assert d_gpu <= 2 * max(d32, d64)


# ------------------------------------------------------------------------------------------------ 12. equipartition
def test_equipartition(hip):
    """the 64 replicas at 300 K, friction 10 / ps, 2000 steps, frames before step 500 discarded: the kinetic temperature, averaged over
    frames and then over replicas, is the float64 restatement's within 5 sqrt(2) of its standard error across replicas (two
    independent means of that error each; here the two share the random stream, which only brings them closer)"""
    b, m, k = md.case("n9_C64"), md.masses("n9_C64"), md.keys("n9_C64")
    got = _run(hip, b, m, k, **md.NVT)
    assert not got["status"].any()
    mean_gpu, se_gpu = md.replica_temperature(got["frames_ekin"], 9)
    mean64, se = md.replica_temperature(md.nvt()["frame_ekin"], 9)
    print(f"equipartition: kinetic temperature gpu {mean_gpu:.2f} +- {se_gpu:.2f} K, float64 restatement {mean64:.2f} +- {se:.2f} K")
    assert abs(mean_gpu - mean64) <= 5 * np.sqrt(2) * se


# ------------------------------------------------------------------------------------------------ 13. front ends
def test_numpy_and_graph_front_ends_give_the_same_bits(hip):
    from grappa_amd import backend
    from grappa_amd.dynamics import simulate, simulate_graph
    from grappa_amd.nonbonded import NonbondedBatch
    from grappa_amd.relax import graph_from_parameters
    old = backend._BACKEND
    backend.set_backend(hip)
    try:
        mol, m = md.case("n33_C3").mols[0], md.masses("n33_C3")
        p, xyz = _parameters(mol), mol["xyz"].transpose(1, 0, 2)
        opts = dict(seed=3, n_steps=30, save_every=10, friction=5.0)
        r = simulate(p, xyz, m, mol["nb"], **opts)
        rg = simulate_graph(graph_from_parameters(p, xyz).to("cuda"), m, NonbondedBatch([mol["nb"]]).to("cuda"), **opts)
        assert r.xyz.shape == xyz.shape and r.frames.shape == (3, 3, 33, 3) and rg.frames.shape == (3, 33, 3, 3) and not r.status.any()
        f32 = lambda a: np.asarray(a, dtype=np.float32)      # noqa: E731
        assert np.array_equal(f32(r.xyz), rg.xyz.cpu().numpy().transpose(1, 0, 2)) and np.array_equal(f32(r.velocities), rg.velocities.cpu().numpy().transpose(1, 0, 2))
        assert np.array_equal(f32(r.frames), rg.frames.cpu().numpy().transpose(2, 0, 1, 3))
        for a, t in ((r.potential_energy, rg.potential_energy), (r.kinetic_energy, rg.kinetic_energy), (r.temperature, rg.temperature)):
            assert np.array_equal(f32(a), t.cpu().numpy()[0])
        assert np.array_equal(f32(r.frame_potential_energy), rg.frame_potential_energy.cpu().numpy()[:, 0].T)
        assert np.array_equal(r.steps, rg.steps.cpu().numpy()[0]) and bool((r.steps == 30).all())
        # given velocities and a continued run through the numpy front end
        half = simulate(p, xyz, m, mol["nb"], seed=3, n_steps=10, friction=5.0)
        rest = simulate(p, half.xyz, m, mol["nb"], velocities=half.velocities, first_step=10, seed=3, n_steps=20, friction=5.0)
        assert np.array_equal(f32(rest.xyz), f32(r.xyz)) and np.array_equal(f32(rest.velocities), f32(r.velocities))
    finally:
        backend.set_backend(old)


def test_grappa_simulate_conserves_the_energy_of_a_golden_molecule(hip):
    """friction 0, 200 steps of 0.5 fs under predicted parameters, from the conformations `Grappa.relax` returns, velocities drawn at
    300 K: |E_tot - E_tot at step 0| below D of item 11 (the larger of the two restatements' D, 9 atoms) scaled by the atom count: the
    band of velocity Verlet grows with the number of oscillators.  Not from the golden conformations themselves: they lie far above the
    minimum of the small golden model's force field, from there the molecule heats from 300 K to 13,000 K within 200 steps, and item
    11's D describes a molecule at 300 K (figures: DESIGN.md section 12)."""
    from grappa_amd import Grappa, GrappaModel, backend
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
        opts = dict(friction=0.0, dt=0.0005, init_temperature=300.0, seed=9)
        start = wrapper.simulate(mol, xyz, n_steps=0, **opts)
        r = wrapper.simulate(mol, xyz, n_steps=200, **opts)
        assert r.xyz.shape == xyz.shape and not r.status.any() and bool((r.steps == 200).all())
        assert bool(np.isfinite(r.potential_energy).all()) and bool(np.isfinite(r.kinetic_energy).all()) and bool(np.isfinite(r.xyz).all())
        assert bool((r.xyz != xyz).any()) and np.array_equal(start.xyz.astype(np.float32), xyz.astype(np.float32))
        d = np.abs(r.potential_energy + r.kinetic_energy - start.potential_energy - start.kinetic_energy)
        n = xyz.shape[1]
        bound = max(md.nve_drift(torch.float32), md.nve_drift(torch.float64)) * n / 9
        print(f"Grappa.simulate: {n} atoms, relaxed in {low.steps.tolist()} steps (status {low.status.tolist()}), |E_tot - E_tot,0| = {d.tolist()} "
              f"kcal/mol after 200 steps, bound {bound:.3f}; temperature {start.temperature.tolist()} -> {r.temperature.tolist()} K")
        assert bool((d <= bound).all())
    finally:
        backend.set_backend(old)
