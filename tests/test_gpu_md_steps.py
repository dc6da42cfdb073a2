"""GPU: the stepwise Langevin dynamics (csrc/dynamics_steps.hip through HipBackend.md_steps and grappa_amd/dynamics.py) against the
float64 restatement of tests/md_refs.py on the cases of tests/md_steps_refs.py.  Every output AND the workspace lie between guard
regions that must come back untouched.

Gates: those of tests/test_gpu_md.py, as they stand there (`_gate_state` is imported, not copied): per (molecule, conformation)
max_atoms |x_gpu - x_f64| <= 4 max_atoms |x_f32 restatement - x_f64| + 2^-20 A, the same for v with the floor 2^-20 max_atoms |v|; an
item whose rotated fp32 siblings do not all pass that gate themselves is held to the farthest sibling instead
(tests/test_host_md_steps.py bounds how many such items there are: 4 of 198 for x, 5 of 198 for v).  Kinetic energy and start
velocities: 8 u32 relative to float64.  The conservation bound is stated at its test."""
import ctypes as C

import numpy as np
import pytest
import torch

import kernel_refs as kr
import md_refs as md
import md_steps_refs as ms
import relax_refs as rr
import relax_steps_refs as rs
from test_gpu_md import _gate_state

pytestmark = pytest.mark.gpu

FILL, FILL_I, FILL_B = 1024.0, 12345, 0xA5       # sentinels around (and, before the call, inside) every output buffer and the workspace
GUARD_B = 4096
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


def _fill_of(buf):
    return FILL_I if buf.dtype == torch.int32 else FILL


def _workspace(hip, batch, Cc, short=0):
    need = int(hip.lib.grappa_md_steps_workspace_bytes(batch.N, Cc, batch.B, rs.n_blocks(batch)))
    buf = torch.full((GUARD_B + need + GUARD_B,), FILL_B, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD_B:GUARD_B + max(need - short, 0)]


def _dev_keys(keys):
    return torch.from_numpy(np.asarray(keys, dtype=np.uint64).view(np.int64).copy()).to("cuda")


def _output_buffers(batch, Cc, o):
    N, B = batch.N, batch.B
    F = o["n_steps"] // o["save_every"] if o["save_every"] > 0 and o["n_steps"] > 0 else 0
    shapes = {"xyz": ((N, Cc, 3), torch.float32), "vel": ((N, Cc, 3), torch.float32), "epot": ((B, Cc), torch.float32),
              "ekin": ((B, Cc), torch.float32), "steps": ((B, Cc), torch.int32), "status": ((B, Cc), torch.int32)}
    if F:
        shapes.update({"frames_xyz": ((F, N, Cc, 3), torch.float32), "frames_epot": ((F, B, Cc), torch.float32),
                       "frames_ekin": ((F, B, Cc), torch.float32)})
    return {k: _guarded(*v) for k, v in shapes.items()}


def _run(hip, batch, masses, keys, vel=None, xyz=None, nb="full", fused=False, steps_per_call=1000, short=0, expect_written=True, **opts):
    """one call of the seam (md_steps; fused=True: md_langevin) on a relax_refs.Batch -> dict of CPU tensors (OUTS, and FRAMES when
    save_every > 0); asserts the guards around the outputs and the workspace.  vel: (N,C,3) CPU tensor or None (velocities drawn at
    init_temperature); xyz: start coordinates other than the batch's"""
    o = {**md.MD_OPTS, **opts}
    plan = batch.plan("cuda")
    dnb = None if nb is None else batch.nonbonded(zero=nb == "zero").to("cuda")
    x = (batch.xyz if xyz is None else xyz).to("cuda")
    Cc = x.shape[1]
    bufs = _output_buffers(batch, Cc, o)
    out = {k: v[1] for k, v in bufs.items()}
    wbuf, ws = _workspace(hip, batch, Cc, short)
    ks = [k.to("cuda") for k in batch.ks]
    eqs = [None if q is None else q.to("cuda") for q in batch.eqs]
    args = (plan, x, ks, eqs, batch.n_per, False, dnb, o, torch.from_numpy(np.asarray(masses, dtype=np.float32)).to("cuda"), _dev_keys(keys),
            None if vel is None else vel.to("cuda"), out["xyz"], out["vel"], out["epot"], out["ekin"], out["steps"], out["status"])
    kw = dict(frames_xyz=out.get("frames_xyz"), frames_epot=out.get("frames_epot"), frames_ekin=out.get("frames_ekin"))
    try:
        if fused:
            hip.md_langevin(*args, atom_counts_host=batch.counts, **kw)
        else:
            hip.md_steps(*args, atom_counts_host=batch.counts, steps_per_call=steps_per_call, workspace=ws, **kw)
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
    if expect_written:
        for k in OUTS:
            if out[k].numel():
                assert not bool((out[k] == _fill_of(out[k])).all()), f"{k} was not written"
    return {k: v.cpu().clone() for k, v in out.items()}


def _noise(hip, counts, keys, Cc, step, purpose):
    ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to("cuda")
    buf, view = _guarded((int(sum(counts)), Cc, 3))
    hip.md_noise(_dev_keys(keys), ptr, Cc, step, purpose, view)
    torch.cuda.synchronize()
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


def _inputs(name):
    return ms.case(name), ms.masses(name), ms.keys(name), ms.thermal_velocities(name)


def _sub(name, order):
    """the molecules `order` of a case as a batch of their own -> (batch, masses, keys, velocities)"""
    b, m, k, v = _inputs(name)
    rows = np.concatenate([np.arange(int(b.ptr[j]), int(b.ptr[j + 1])) for j in order])
    return b.subset(order), m[rows], k[list(order)], v[rows]


# ------------------------------------------------------------------------------------------------ 1. step zero
@pytest.mark.parametrize("name", ms.TRAJ_CASES)
def test_step_zero(hip, name):
    """n_steps = 0: coordinates and velocities come back bit for bit; epot is, bit for bit, the sum in double in term order of what the
    energy entry points give at the input; ekin is float64's within 8 u32"""
    b, m, k, v = _inputs(name)
    got = _run(hip, b, m, k, vel=v, n_steps=0, friction=5.0)
    assert torch.equal(_bits(got["xyz"]), _bits(b.xyz)) and torch.equal(_bits(got["vel"]), _bits(v))
    assert not got["steps"].any() and not got["status"].any()
    plan, x = b.plan("cuda"), b.xyz.to("cuda")
    ks, eqs = [t.to("cuda") for t in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    Cc = x.shape[1]
    e, t = torch.zeros(b.B, Cc, device="cuda"), torch.zeros(4, b.B, Cc, device="cuda")
    hip.mm_energy_fwd(plan, x, ks, eqs, b.n_per, False, e, t)
    _, _, nt = b.nonbonded().to("cuda").evaluate(x, terms=True, gradient=False)
    tot = torch.zeros(b.B, Cc, dtype=torch.float64)
    for row in torch.cat([t, nt]).cpu():
        tot = tot + row.double()
    assert torch.equal(_bits(got["epot"]), _bits(tot.float())), f"{name}: epot {got['epot'].tolist()} terms' sum {tot.tolist()}"
    want = md.kinetic(b, torch.from_numpy(m).double(), v)
    assert bool(((got["ekin"].double() - want).abs() <= 8 * kr.U32 * want).all()), (got["ekin"].tolist(), want.tolist())


# ------------------------------------------------------------------------------------------------ 2. trajectories, no thermostat
TRAJ = [(n, s) for n in ms.TRAJ_CASES for s in ms.TRAJ_STEPS]


@pytest.mark.parametrize("name,n_steps", TRAJ, ids=[f"{n}-{s}steps" for n, s in TRAJ])
def test_trajectory_without_thermostat(hip, name, n_steps):
    """friction = 0 (velocity Verlet), dt = 1 fs, from the case coordinates with thermal velocities"""
    b, m, k, v = _inputs(name)
    r64, r32s = ms.verlet(name)[n_steps], [r[n_steps] for r in ms.verlet32(name)]
    got = _run(hip, b, m, k, vel=v, n_steps=n_steps, dt=0.001)
    assert bool((got["steps"] == n_steps).all()) and not got["status"].any()
    _gate_state(name, f"{n_steps} steps, friction 0, stepwise", b, got, r64, r32s)


# ------------------------------------------------------------------------------------------------ 3. with the thermostat
@pytest.mark.parametrize("name", ms.TRAJ_CASES)
def test_trajectory_with_thermostat(hip, name):
    """friction 50 / ps at 300 K, 40 steps: the restatements consume the noise md_noise wrote for these steps -- what the fused kernel
    draws (tests/test_gpu_md.py gates it against the restated generator) -- so the stepwise path must draw the same numbers for
    (atom within molecule, conformation, step).  Start velocities drawn at init_temperature: 8 u32 of sqrt(ACC kB T0 / m) md_noise(first_step, 1)"""
    b, m, k, v = _inputs(name)
    Cc = b.xyz.shape[1]
    first, total = 7, max(ms.TRAJ_STEPS)
    z = {first + s: _noise(hip, b.counts, k, Cc, first + s, 0).double() for s in range(total)}
    opts = dict(friction=50.0, temperature=300.0, dt=0.001, first_step=first)
    common = dict(velocities=v, noise=lambda step, purpose: z[step], n_steps=total, **opts)
    r32s = md.fp32_realisations(b, m, (total,), **common)
    got = _run(hip, b, m, k, vel=v, n_steps=total, **opts)
    assert bool((got["steps"] == total).all()) and not got["status"].any()
    _gate_state(name, f"{total} steps, friction 50, stepwise", b, got, r32s[0][total][1], [r[total] for r in r32s])
    start = _run(hip, b, m, k, n_steps=0, init_temperature=250.0, first_step=first)
    z1 = _noise(hip, b.counts, k, Cc, first, 1).double()
    want = torch.sqrt(md.ACC * md.KB * 250.0 / torch.from_numpy(m).double())[:, None, None] * z1
    assert torch.equal(_bits(start["xyz"]), _bits(b.xyz))
    assert bool(((start["vel"].double() - want).abs() <= 8 * kr.U32 * want.abs()).all())
    cold = _run(hip, b, m, k, n_steps=0, init_temperature=0.0)
    assert not _bits(cold["vel"]).any() and not _bits(cold["ekin"]).any()


# ------------------------------------------------------------------------------------------------ 4. the two paths
@pytest.mark.parametrize("name", ["s65_C3", ms.MIXED])
def test_the_two_paths_agree(hip, name):
    """md_steps and md_langevin: the same steps and status, both within the trajectory gate of the same float64 state (their bits
    differ: they add in different orders)"""
    b, m, k, v = _inputs(name)
    n = max(ms.TRAJ_STEPS)
    assert max(b.counts) <= rr.max_atoms()
    r64, r32s = ms.verlet(name)[n], [r[n] for r in ms.verlet32(name)]
    a, f = _run(hip, b, m, k, vel=v, n_steps=n, dt=0.001), _run(hip, b, m, k, vel=v, n_steps=n, dt=0.001, fused=True)
    assert torch.equal(a["steps"], f["steps"]) and torch.equal(a["status"], f["status"])
    _gate_state(name, "the two paths: stepwise", b, a, r64, r32s)
    _gate_state(name, "the two paths: fused", b, f, r64, r32s)


# ------------------------------------------------------------------------------------------------ 5. bits
THERMO = dict(friction=20.0, temperature=300.0, init_temperature=300.0)


def test_two_runs_and_every_chunk_size_give_the_same_bits(hip):
    """1, 7 and 40 steps per run call (7 does not divide 40): the outputs do not depend on how the steps are dealt out, frames included"""
    b, m, k, _ = _inputs(ms.MIXED)
    a = _run(hip, b, m, k, n_steps=40, **THERMO)
    _same_bits(a, _run(hip, b, m, k, n_steps=40, **THERMO), "two runs")
    for spc in (1, 7, 40):
        _same_bits(a, _run(hip, b, m, k, n_steps=40, steps_per_call=spc, **THERMO), f"steps_per_call = {spc}")
    one = _run(hip, b, m, k, n_steps=40, save_every=1, steps_per_call=1, **THERMO)
    _same_bits(one, _run(hip, b, m, k, n_steps=40, save_every=1, steps_per_call=40, **THERMO), "a frame every step, 1 and 40 per call", keys=OUTS + FRAMES)
    five = _run(hip, b, m, k, n_steps=40, save_every=5, steps_per_call=7, **THERMO)
    _same_bits(five, _run(hip, b, m, k, n_steps=40, save_every=5, steps_per_call=40, **THERMO), "a frame every 5 steps, 7 and 40 per call", keys=OUTS + FRAMES)
    _same_bits(a, one, "with and without frames")
    _same_bits(a, five, "with and without frames")
    assert torch.equal(_bits(one["frames_xyz"][4::5]), _bits(five["frames_xyz"])) and torch.equal(_bits(one["frames_epot"][4::5]), _bits(five["frames_epot"]))


@pytest.mark.parametrize("friction", [0.0, 20.0])
def test_continuation(hip, friction):
    """40 steps = 16 + 24 with vel_in = vel_out, xyz = xyz_out and first_step advanced: the same bits, frames included"""
    b, m, k, _ = _inputs(ms.MIXED)
    opts = dict(friction=friction, temperature=300.0, init_temperature=300.0, save_every=8)
    whole = _run(hip, b, m, k, n_steps=40, first_step=3, **opts)
    one = _run(hip, b, m, k, n_steps=16, first_step=3, **opts)
    two = _run(hip, b, m, k, vel=one["vel"], xyz=one["xyz"], n_steps=24, first_step=19, **opts)
    _same_bits(whole, two, "40 steps against 16 + 24", keys=("xyz", "vel", "epot", "ekin", "status"))
    assert bool((one["steps"] == 16).all()) and bool((two["steps"] == 24).all()) and bool((whole["steps"] == 40).all())
    for key in FRAMES:
        assert torch.equal(_bits(whole[key]), _bits(torch.cat([one[key], two[key]]))), key
    assert not torch.equal(_bits(whole["xyz"]), _bits(one["xyz"]))


def test_frames_are_the_states_of_shorter_runs(hip):
    b, m, k, _ = _inputs(ms.MIXED)
    whole = _run(hip, b, m, k, n_steps=40, save_every=5, **THERMO)
    assert whole["frames_xyz"].shape[0] == 8
    for f in range(8):
        part = _run(hip, b, m, k, n_steps=5 * (f + 1), **THERMO)
        assert torch.equal(_bits(whole["frames_xyz"][f]), _bits(part["xyz"])), f"frame {f}: coordinates"
        assert torch.equal(_bits(whole["frames_epot"][f]), _bits(part["epot"])), f"frame {f}: potential energy"
        assert torch.equal(_bits(whole["frames_ekin"][f]), _bits(part["ekin"])), f"frame {f}: kinetic energy"
    longer = _run(hip, b, m, k, n_steps=42, save_every=5, **THERMO)          # still 8 frames, and the run goes on after the last one
    _same_bits(longer, whole, "the frames of 42 and of 40 steps", keys=FRAMES)
    assert not torch.equal(_bits(longer["xyz"]), _bits(whole["xyz"]))


def _with_coincident(batch, mol, i, j, conf=None):
    mols = [dict(mm) for mm in batch.mols]
    x = mols[mol]["xyz"].copy()
    if conf is None:
        x[j] = x[i]
    else:
        x[j, conf] = x[i, conf]
    mols[mol]["xyz"] = x
    return rr.Batch(mols)


def test_a_molecule_of_three_blocks_gives_the_same_bits_whatever_its_neighbours_do(hip):
    """alone, behind another molecule (its blocks take other rows of the plan and of the partials) with the same key, and beside a
    neighbour that stops at once"""
    b, m, k, _ = _inputs("s129_C3")
    opts = dict(n_steps=30, save_every=10, **THERMO)
    alone = _rows_of(_run(hip, b, m, k, **opts), b, 0)
    assert bool((alone["steps"] == 30).all())
    front, mf = ms.case("s65_C3").mols[0], ms.masses("s65_C3")
    keys2 = np.concatenate([ms.keys("s65_C3"), k])
    two = rr.Batch([front, b.mols[0]])
    _same_bits(_rows_of(_run(hip, two, np.concatenate([mf, m]), keys2, **opts), two, 1), alone, "129 atoms behind 65", keys=OUTS + FRAMES)
    hit = _with_coincident(two, 0, 0, 64)          # atoms of the neighbour's two blocks on one point: it stops at step 0
    pairs = {tuple(p) for p in two.params[0].exception_idx.tolist()}
    assert (0, 64) not in pairs and (64, 0) not in pairs
    got = _run(hip, hit, np.concatenate([mf, m]), keys2, **opts)
    assert bool((got["status"][0] == 2).all()) and not got["steps"][0].any()
    _same_bits(_rows_of(got, hit, 1), alone, "129 atoms beside a molecule that stops", keys=OUTS + FRAMES)
    other = _rows_of(_run(hip, b, m, ms.keys("s65_C3"), **opts), b, 0)          # another key: another trajectory
    assert not torch.equal(_bits(other["xyz"]), _bits(alone["xyz"]))


def _parameters(mol):
    from grappa_amd.parameters import Parameters
    ids = np.arange(mol["n"])
    k3, k4 = mol["ks"][2].astype(np.float64), mol["ks"][3].astype(np.float64)
    return Parameters(atoms=ids, bonds=mol["idx"][0], bond_k=mol["ks"][0], bond_eq=mol["eqs"][0], angles=mol["idx"][1], angle_k=mol["ks"][1],
                      angle_eq=mol["eqs"][1], propers=mol["idx"][2], proper_ks=np.abs(k3), proper_phases=np.where(k3 >= 0, 0.0, np.pi),
                      impropers=mol["idx"][3], improper_ks=np.abs(k4), improper_phases=np.where(k4 >= 0, 0.0, np.pi))


def test_simulate_graph_agrees_with_the_seam(hip):
    from grappa_amd import backend
    from grappa_amd.dynamics import simulate_graph
    from grappa_amd.nonbonded import NonbondedBatch
    from grappa_amd.relax import graph_from_parameters
    old = backend._BACKEND
    backend.set_backend(hip)
    try:
        b, m, k, _ = _inputs("s65_C3")
        mol = b.mols[0]
        g = graph_from_parameters(_parameters(mol), mol["xyz"].transpose(1, 0, 2)).to("cuda")
        nb = NonbondedBatch([mol["nb"]]).to("cuda")
        opts = dict(n_steps=20, save_every=5, friction=20.0, temperature=300.0)
        runs = [simulate_graph(g, m, nb, keys=k, first_step=2, stepwise=True, steps_per_launch=s, **opts) for s in (10000, 7)]
        seam = _run(hip, b, m, k, first_step=2, init_temperature=300.0, **opts)
        for r in runs:
            assert bool((r.steps == 20).all()) and not r.status.any() and r.frames.shape == (4, 65, 3, 3)
            for f, key in (("xyz", "xyz"), ("velocities", "vel"), ("potential_energy", "epot"), ("kinetic_energy", "ekin"), ("frames", "frames_xyz"),
                           ("frame_potential_energy", "frames_epot"), ("frame_kinetic_energy", "frames_ekin")):
                assert torch.equal(_bits(getattr(r, f).cpu()), _bits(seam[key])), f
    finally:
        backend.set_backend(old)


# ------------------------------------------------------------------------------------------------ 6. launches
def test_the_same_launches_per_step_whatever_the_shape(hip):
    added = {}
    for name in ("s9_65_C17", "s513_C1"):
        b, m, k, v = _inputs(name)
        n = []
        for steps in (0, 10):
            before = hip.lib.grappa_launch_count(0)
            _run(hip, b, m, k, vel=v, n_steps=steps)
            n.append(hip.lib.grappa_launch_count(0) - before)
        added[name] = n[1] - n[0]          # init and finish launch the same with and without steps in between
    print(f"launches added by a run of 10 steps: {added}")
    assert added["s9_65_C17"] == added["s513_C1"] and added["s513_C1"] % 10 == 0 and 0 < added["s513_C1"] <= 30, added


# ------------------------------------------------------------------------------------------------ 7. a non-finite gradient
def test_coincident_atoms(hip):
    """atoms 0 and 129 of the 130-atom molecule (its first and third i-block; they interact in full) on one point in conformation 1
    only: that item stops with status 2 at the step the float64 restatement stops it, holding its coordinates; its frames keep the
    sentinel; every other item -- the molecule's other conformations included -- is bit-equal to the run without the defect"""
    base, m, k, _ = _inputs(ms.MIXED)
    M = 3
    pairs = {tuple(q) for q in base.params[M].exception_idx.tolist()}
    assert base.counts[M] == 130 and (0, 129) not in pairs and (129, 0) not in pairs
    opts = dict(n_steps=20, save_every=5, **THERMO)
    plain = _run(hip, base, m, k, **opts)
    moved = _with_coincident(base, M, 0, 129, conf=1)
    hit = _run(hip, moved, m, k, **opts)
    want = md.baoab_ref(moved, m, torch.float64, keys=k, **opts)
    assert int(want["status"][M, 1]) == 2 and int(want["status"].sum()) == 2
    assert torch.equal(hit["status"].long(), want["status"].long()) and torch.equal(hit["steps"].long(), want["steps"])
    p0 = int(base.ptr[M])
    assert torch.equal(_bits(hit["xyz"][p0:p0 + 130, 1]), _bits(moved.xyz[p0:p0 + 130, 1])), "status 2 returns the coordinates it holds"
    stop = int(want["steps"][M, 1])
    later = [f for f in range(4) if 5 * (f + 1) > stop]
    assert later and bool((hit["frames_xyz"][later][:, p0:p0 + 130, 1] == FILL).all())
    assert bool((hit["frames_epot"][later][:, M, 1] == FILL).all()) and bool((hit["frames_ekin"][later][:, M, 1] == FILL).all())
    for key in OUTS + FRAMES:          # every other item: unaffected, bit for bit
        a, b_ = hit[key].clone(), plain[key].clone()
        if key in ("xyz", "vel"):
            a[p0:p0 + 130, 1], b_[p0:p0 + 130, 1] = 0, 0
        elif key == "frames_xyz":
            a[:, p0:p0 + 130, 1], b_[:, p0:p0 + 130, 1] = 0, 0
        elif key in ("frames_epot", "frames_ekin"):
            a[:, M, 1], b_[:, M, 1] = 0, 0
        else:
            a[M, 1], b_[M, 1] = 0, 0
        assert torch.equal(_bits(a), _bits(b_)), f"{key} of an item beside the non-finite one differs"


# ------------------------------------------------------------------------------------------------ 8. frozen atoms
def test_frozen_atoms(hip):
    """masses 0 on both sides of the second block's edge: their coordinates come back bit for bit and their velocities are 0, whatever
    vel_in holds; the other atoms stay inside the gate against the restatement with the same masses"""
    b, m, k, v = _inputs("s129_C3")
    m = m.copy()
    frozen = [63, 64, 65]
    m[frozen] = 0.0
    assert bool((v[frozen] != 0).all())
    for friction in (0.0, 20.0):
        got = _run(hip, b, m, k, vel=v, n_steps=25, friction=friction, temperature=300.0)
        assert not got["status"].any() and bool((got["steps"] == 25).all())
        for a in frozen:
            assert torch.equal(_bits(got["xyz"][a]), _bits(b.xyz[a])) and not _bits(got["vel"][a]).any()
        rest = [a for a in range(129) if a not in frozen]
        assert bool((got["xyz"][rest] != b.xyz[rest]).any(-1).all()) and bool(torch.isfinite(got["xyz"]).all()) and bool(torch.isfinite(got["epot"]).all())
        if friction == 0.0:
            r32s = md.fp32_realisations(b, m, (25,), velocities=v, n_steps=25)
            _gate_state("s129_C3", "25 steps, three frozen atoms, stepwise", b, got, r32s[0][25][1], [r[25] for r in r32s])
    zero = _run(hip, b, m, k, vel=v, n_steps=0)
    assert not _bits(zero["vel"][frozen]).any() and torch.equal(_bits(zero["vel"][:63]), _bits(v[:63]))


# ------------------------------------------------------------------------------------------------ 9. degenerate members
def test_a_single_atom_drifts_and_an_empty_molecule_writes_nothing(hip):
    b, m, k, v = _inputs(ms.MIXED)
    assert b.counts[0] == 1
    got = _run(hip, b, m, k, vel=v, n_steps=10, dt=0.001)
    # the single atom: no force, so v is untouched and x moves by dt v per step (two half drifts: at most one ulp of x each)
    want = md.baoab_ref(b.subset([0]), m[:1], torch.float64, velocities=v[:1], n_steps=10, dt=0.001)
    assert torch.equal(_bits(got["vel"][0]), _bits(v[0])) and bool((got["steps"][0] == 10).all()) and not got["status"][0].any()
    # 20 fp32 additions of at most one unit roundoff of |x| each (|x| <= |x_0| + 10 dt |v| throughout), the products' roundings far below
    scale = b.xyz[0].double().abs() + 10 * 0.001 * v[0].double().abs()
    assert bool(((got["xyz"][0].double() - want["xyz"][0]).abs() <= 24 * kr.U32 * scale).all())
    drift = got["xyz"][0].double() - b.xyz[0].double()
    assert bool(((drift - 10 * float(np.float32(0.001)) * v[0].double()).abs() <= 24 * kr.U32 * scale).all()) and bool((drift != 0).any())
    assert not got["epot"][0].any()
    # a molecule without atoms between two others: nothing is written for it, and its neighbours run as if alone
    order = [2, 4]
    sub, sm, sk, sv = _sub(ms.MIXED, order)
    mols = [sub.mols[0], rr.gen_molecule(0, 3, np.random.default_rng(0)), sub.mols[1]]
    e = rr.Batch(mols)
    keys3 = np.array([sk[0], 99, sk[1]], dtype=np.uint64)
    opts = dict(n_steps=15, save_every=5, **THERMO)
    gote = _run(hip, e, sm, keys3, **opts)
    for key in ("epot", "ekin"):
        assert bool((gote[key][1] == FILL).all()) and bool((gote["frames_" + key][:, 1] == FILL).all()), key
    assert bool((gote["steps"][1] == FILL_I).all()) and bool((gote["status"][1] == FILL_I).all())
    for pos, j in ((0, 0), (2, 1)):
        one = sub.subset([j])
        rows = np.arange(int(sub.ptr[j]), int(sub.ptr[j + 1]))
        _same_bits(_rows_of(gote, e, pos), _rows_of(_run(hip, one, sm[rows], sk[[j]], **opts), one, 0), f"molecule {pos} beside an empty one",
                   keys=OUTS + FRAMES)


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals_launch_nothing_and_write_nothing(hip):
    from grappa_amd import _lib
    from grappa_amd.backend import GrappaHipError
    b, m, k = rr.case("n9_C1"), md.masses("n9_C1"), md.keys("n9_C1")
    before = hip.lib.grappa_launch_count(0)
    # through the seam: the options of grappa_md_langevin_f32, a short workspace, the seam's own arguments
    for bad in ({"dt": 0.0}, {"dt": float("nan")}, {"temperature": -1.0}, {"friction": float("inf")}, {"init_temperature": -1.0}, {"n_steps": -1},
                {"n_steps": 1000001}, {"save_every": -1}, {"first_step": 2 ** 32 - 1, "n_steps": 1}, {"first_step": 2 ** 32 - 5, "n_steps": 5}):
        with pytest.raises(GrappaHipError, match="GRAPPA_ERR_ARG"):
            _run(hip, b, m, k, **{"n_steps": 3, **bad})
    with pytest.raises(GrappaHipError, match="GRAPPA_ERR_WORKSPACE"):
        _run(hip, b, m, k, short=1, n_steps=3)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="steps_per_call"):
            _run(hip, b, m, k, steps_per_call=bad, n_steps=3)
    assert hip.lib.grappa_launch_count(0) == before, "a refused call launched something"
    _run(hip, b, m, k, first_step=2 ** 32 - 5, n_steps=4)          # the last admissible step index is accepted
    # the C ABI itself
    plan, x = b.plan("cuda"), b.xyz.to("cuda")
    ks, eqs = [t.to("cuda") for t in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    d = hip._mm_desc(plan, x, ks, eqs, b.n_per, False)
    mk = lambda **kw: _lib.MdOpts(**{**dict(dt=0.001, temperature=300.0, friction=1.0, init_temperature=300.0, n_steps=6, save_every=2, first_step=0), **kw})      # noqa: E731
    o = mk()
    table, n_items, nblk, _ = hip.nonbonded_plan(torch.tensor([0, 9], dtype=torch.int32), 9, 1, x.device)
    wbuf, ws = _workspace(hip, b, 1)
    mass, key = torch.from_numpy(m).to("cuda"), _dev_keys(k)
    bufs = _output_buffers(b, 1, dict(n_steps=6, save_every=2))
    outs = [bufs[n][1].data_ptr() for n in OUTS]
    frames = [bufs[n][1].data_ptr() for n in FRAMES]
    st, lib = hip._stream(), hip.lib

    def init(mm=C.byref(d), nb=None, opt=None, ms_=mass.data_ptr(), ky=key.data_ptr(), tb=table.data_ptr(), ni=n_items, nbk=nblk, w=ws.data_ptr(),
             wb=ws.numel()):
        return lib.grappa_md_steps_init_f32(st, mm, nb, C.byref(opt or o), ms_, ky, None, tb, ni, nbk, w, wb)

    def run(mm=C.byref(d), nb=None, opt=None, ms_=mass.data_ptr(), ky=key.data_ptr(), tb=table.data_ptr(), ni=n_items, nbk=nblk, w=ws.data_ptr(),
            wb=ws.numel(), step0=0, n=2, fr=(None, None, None)):
        return lib.grappa_md_steps_run_f32(st, mm, nb, C.byref(opt or o), ms_, ky, tb, ni, nbk, w, wb, step0, n, *fr)

    def finish(mm=C.byref(d), nb=None, opt=None, tb=table.data_ptr(), ni=n_items, nbk=nblk, w=ws.data_ptr(), wb=ws.numel(), out=outs):
        return lib.grappa_md_steps_finish_f32(st, mm, nb, C.byref(opt or o), tb, ni, nbk, w, wb, *out)

    before = lib.grappa_launch_count(0)
    wide = [_lib.MMDesc.from_buffer_copy(d) for _ in range(3)]
    wide[0].B, wide[0].C = 1 << 16, 1 << 15                          # B * C = 2^31
    wide[1].C = 1 << 28                                              # N * C * 3 >= 2^31
    wide[2].N, wide[2].B, wide[2].C = 64, (1 << 16) - 1, 1 << 15     # n_blocks * C = 2^31 with n_blocks = N / 64 + B
    for call in (init, run, finish):
        assert call(mm=None) == -1 and call(tb=None) == -1 and call(w=None) == -1, call.__name__
        assert call(tb=table.data_ptr() + 4) == -1 and call(w=ws.data_ptr() + 8) == -1, f"{call.__name__}: a misaligned table or workspace"
        assert call(ni=-1) == -1 and call(nbk=-1) == -1 and call(nbk=9 // 64 + 1 + 1) == -1, f"{call.__name__}: counts"
        assert call(mm=C.byref(wide[0])) == -1 and call(mm=C.byref(wide[1])) == -1, f"{call.__name__}: sizes at 2^31"
        assert call(mm=C.byref(wide[2]), nbk=1 << 16) == -1, f"{call.__name__}: n_blocks * C at 2^31"
        assert call(wb=ws.numel() - 1) == -3, f"{call.__name__}: a workspace one byte short"
        assert call(opt=mk(first_step=2 ** 32 - 6)) == -1 and call(opt=mk(dt=-1.0)) == -1, f"{call.__name__}: options"
        for shape in ((9, 2, 1), (8, 1, 1), (9, 1, 2)):          # nb disagreeing with mm in C, in N, in B
            nd = _lib.NbDesc()
            nd.N, nd.C, nd.B = shape
            assert call(nb=C.byref(nd)) == -1, shape
    for call in (init, run):
        assert call(ms_=None) == -1 and call(ky=None) == -1, call.__name__
    assert lib.grappa_md_steps_init_f32(st, C.byref(d), None, None, mass.data_ptr(), key.data_ptr(), None, table.data_ptr(), n_items, nblk,
                                        ws.data_ptr(), ws.numel()) == -1
    for drop in range(6):          # every output of finish in turn
        assert finish(out=[None if j == drop else p for j, p in enumerate(outs)]) == -1, drop
    assert run(n=0) == -1 and run(n=-1) == -1 and run(step0=-1) == -1 and run(step0=5, n=2) == -1 and run(step0=0, n=7) == -1
    assert run(step0=1, n=2, fr=frames) == -1 and run(step0=1, n=2, fr=(None, None, frames[2])) == -1          # frames from a step0 off the period
    torch.cuda.synchronize()
    assert lib.grappa_launch_count(0) == before, "a refused call launched something"
    for name, (buf, _) in bufs.items():
        assert bool((buf == _fill_of(buf)).all()), f"a refused call wrote {name}"
    assert bool((wbuf == FILL_B).all()), "a refused call wrote to the workspace"
    # the complete sequence is accepted, with run calls off the period as long as no frame is asked for; the frame pointer of a run call is
    # the slice of ITS first frame (here frame 1: step0 = 2, save_every = 2)
    assert init() == 0 and run(step0=0, n=1) == 0 and run(step0=1, n=1) == 0 and run(step0=2, n=4, fr=[frames[0] + 1 * 9 * 3 * 4, None, None]) == 0 and finish() == 0
    torch.cuda.synchronize()
    assert int(bufs["steps"][1][0, 0]) == 6 and int(bufs["status"][1][0, 0]) == 0
    assert bool((bufs["frames_xyz"][1][0] == FILL).all()) and not bool((bufs["frames_xyz"][1][1:] == FILL).any())
    assert bool((wbuf[:GUARD_B] == FILL_B).all()) and bool((wbuf[-GUARD_B:] == FILL_B).all())
    # an empty batch returns 0 without a launch
    empty = _lib.MMDesc.from_buffer_copy(d)
    empty.N = 0
    before = lib.grappa_launch_count(0)
    assert init(mm=C.byref(empty)) == 0 and run(mm=C.byref(empty)) == 0 and finish(mm=C.byref(empty)) == 0
    assert lib.grappa_launch_count(0) == before
    with pytest.raises(ValueError, match="atom_counts_host"):
        z = lambda dt: torch.zeros(1, 1, dtype=dt, device="cuda")      # noqa: E731
        hip.md_steps(plan, x, ks, eqs, b.n_per, False, None, {**md.MD_OPTS, "n_steps": 2}, mass, key, None, torch.empty_like(x), torch.empty_like(x),
                     z(torch.float32), z(torch.float32), z(torch.int32), z(torch.int32))


# ------------------------------------------------------------------------------------------------ 11. energy conservation
def test_energy_conservation(hip):
    """NVE on s2_130_9_C3 from its relaxed coordinates with 300 K velocities: 400 steps of 0.5 fs, a frame every 50.  D = max over frames
    and items of |E_tot - E_tot at step 0|; D_gpu <= 2 max(D of the fp32 restatement, D of the float64 restatement): D is the
    integrator's O(dt^2) band, the same in all three (the bound of tests/test_gpu_md.py test_energy_conservation)"""
    b, m, k, v = ms.nve_batch(), ms.masses(ms.NVE_CASE), ms.keys(ms.NVE_CASE), ms.thermal_velocities(ms.NVE_CASE)
    start = _run(hip, b, m, k, vel=v, n_steps=0)
    got = _run(hip, b, m, k, vel=v, **ms.NVE)
    assert not got["status"].any() and bool((got["steps"] == ms.NVE["n_steps"]).all())
    d_gpu = md.drift(start["epot"].double() + start["ekin"].double(), got["frames_epot"].double() + got["frames_ekin"].double())
    d32, d64 = ms.nve_drift(torch.float32), ms.nve_drift(torch.float64)
    print(f"energy conservation, stepwise: D_gpu {d_gpu:.4f}, D_f32 {d32:.4f}, D_f64 {d64:.4f} kcal/mol, D_gpu / max = {d_gpu / max(d32, d64):.3f}")
    assert d_gpu <= 2 * max(d32, d64)


# ------------------------------------------------------------------------------------------------ 12. the public door
def test_auto_runs_a_molecule_above_the_fused_limit(hip):
    from grappa_amd import backend
    from grappa_amd.dynamics import simulate
    old = backend._BACKEND
    backend.set_backend(hip)
    try:
        name = "s513_C1"
        b, m, k, v = _inputs(name)
        mol = b.mols[0]
        p, xyz = _parameters(mol), mol["xyz"].transpose(1, 0, 2)
        vel = v.numpy().transpose(1, 0, 2)
        before = hip.lib.grappa_launch_count(0)
        for kw in ({}, {"stepwise": False}):
            with pytest.raises(ValueError, match="above the limit.*stepwise"):
                simulate(p, xyz, m, mol["nb"], velocities=vel, n_steps=5, friction=0.0, **kw)
        assert hip.lib.grappa_launch_count(0) == before, "a refused call launched something"
        r = simulate(p, xyz, m, mol["nb"], velocities=vel, keys=k, stepwise="auto", n_steps=5, friction=0.0, dt=0.001)
        assert r.xyz.shape == xyz.shape and bool((r.steps == 5).all()) and not r.status.any()
        assert all(bool(np.isfinite(getattr(r, f)).all()) for f in ("xyz", "velocities", "potential_energy", "kinetic_energy", "temperature"))
        got = {"xyz": torch.from_numpy(np.ascontiguousarray(r.xyz.transpose(1, 0, 2))).float(),
               "vel": torch.from_numpy(np.ascontiguousarray(r.velocities.transpose(1, 0, 2))).float()}
        _gate_state(name, "5 steps through simulate(stepwise='auto')", b, got, ms.verlet(name)[5], [q[5] for q in ms.verlet32(name)])
    finally:
        backend.set_backend(old)
