"""GPU: the stepwise dynamics under a nonbonded cutoff (grappa_md_steps_*_cut_f32 through HipBackend.md_steps(cutoff=)) against the
restatements of tests/md_cut_refs.py: trajectories through the gate of tests/test_gpu_md.py as it stands, the launch budget, the bits
(two runs, chunk sizes, continuation, prune = 0 against prune = 1, cut = NULL against the plain entry points), the energies against the
cut energy kernel, energy conservation and the public door.  Every output and the workspace lie between guard words."""
import ctypes as C

import numpy as np
import pytest
import torch

import md_cut_refs as mc
import md_refs as md
import md_steps_refs as ms
import relax_steps_refs as rs
from grappa_amd import _lib
from grappa_amd.nonbonded import Cutoff, NonbondedBatch
from test_gpu_md import _gate_state
from test_gpu_md_steps import (FILL_B, FRAMES, GUARD_B, OUTS, _bits, _dev_keys, _fill_of, _inputs, _noise, _output_buffers, _parameters,
                               _same_bits)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from grappa_amd.backend import HipBackend
    return HipBackend()


def _run(hip, batch, masses, keys, cut, vel=None, xyz=None, steps_per_call=1000, **opts):
    """one call of the seam under `cut` (None: all pairs) on a relax_refs.Batch -> dict of CPU tensors (OUTS, and FRAMES when
    save_every > 0); asserts the guards around the outputs and the workspace"""
    o = {**md.MD_OPTS, **opts}
    plan = batch.plan("cuda")
    dnb = batch.nonbonded().to("cuda")
    x = (batch.xyz if xyz is None else xyz).to("cuda")
    Cc = x.shape[1]
    bufs = _output_buffers(batch, Cc, o)
    out = {k: v[1] for k, v in bufs.items()}
    size = hip.lib.grappa_md_steps_workspace_bytes if cut is None else hip.lib.grappa_md_steps_cut_workspace_bytes
    need = int(size(batch.N, Cc, batch.B, rs.n_blocks(batch)))
    wbuf = torch.full((GUARD_B + need + GUARD_B,), FILL_B, dtype=torch.uint8, device="cuda")
    ks = [k.to("cuda") for k in batch.ks]
    eqs = [None if q is None else q.to("cuda") for q in batch.eqs]
    args = (plan, x, ks, eqs, batch.n_per, False, dnb, o, torch.from_numpy(np.asarray(masses, dtype=np.float32)).to("cuda"), _dev_keys(keys),
            None if vel is None else vel.to("cuda"), out["xyz"], out["vel"], out["epot"], out["ekin"], out["steps"], out["status"])
    kw = dict(frames_xyz=out.get("frames_xyz"), frames_epot=out.get("frames_epot"), frames_ekin=out.get("frames_ekin"))
    if cut is not None:
        kw["cutoff"] = cut
    hip.md_steps(*args, atom_counts_host=batch.counts, steps_per_call=steps_per_call, workspace=wbuf[GUARD_B:GUARD_B + need], **kw)
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert bool((buf[:64] == _fill_of(buf)).all()) and bool((buf[-64:] == _fill_of(buf)).all()), f"written outside {k}"
    assert bool((wbuf[:GUARD_B] == FILL_B).all()) and bool((wbuf[-GUARD_B:] == FILL_B).all()), "written outside the workspace"
    for k in OUTS:
        if out[k].numel():
            assert not bool((out[k] == _fill_of(out[k])).all()), f"{k} was not written"
    return {k: v.cpu().clone() for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ 1. trajectories
TRAJ = [(n, s) for n in mc.CASES for s in mc.TRAJ_STEPS]


@pytest.mark.parametrize("name,n_steps", TRAJ, ids=[f"{n}-{s}steps" for n, s in TRAJ])
def test_trajectory_without_thermostat(hip, name, n_steps):
    b, m, k, v = _inputs(name)
    r64, r32s = mc.verlet(name)[n_steps], [r[n_steps] for r in mc.verlet32(name)]
    got = _run(hip, b, m, k, mc.cutoff(name), vel=v, n_steps=n_steps, dt=0.001)
    assert bool((got["steps"] == n_steps).all()) and not got["status"].any()
    _gate_state(name, f"{n_steps} steps, friction 0, cutoff {mc.cutoff(name).distance:.4f}", b, got, r64, r32s)


@pytest.mark.parametrize("name", mc.CASES)
def test_trajectory_with_thermostat(hip, name):
    """friction 50 / ps at 300 K, 1, 5 and 40 steps; the restatements consume the noise md_noise wrote for these steps"""
    b, m, k, v = _inputs(name)
    Cc = b.xyz.shape[1]
    first, total = 7, max(mc.TRAJ_STEPS)
    z = {first + s: _noise(hip, b.counts, k, Cc, first + s, 0).double() for s in range(total)}
    opts = dict(friction=50.0, temperature=300.0, dt=0.001, first_step=first)
    r32s = mc.realisations(name, mc.TRAJ_STEPS, velocities=v, noise=lambda step, purpose: z[step], n_steps=total, **opts)
    for n in mc.TRAJ_STEPS:
        got = _run(hip, b, m, k, mc.cutoff(name), vel=v, n_steps=n, **opts)
        assert bool((got["steps"] == n).all()) and not got["status"].any()
        _gate_state(name, f"{n} steps, friction 50, cutoff", b, got, r32s[0][n][1], [r[n] for r in r32s])


# ------------------------------------------------------------------------------------------------ 2. launches
def test_a_step_stays_two_launches_and_init_gains_one(hip):
    added, base = {}, {}
    for name in ("s65_C3", "s513_C1"):
        b, m, k, v = _inputs(name)
        for cut in (None, mc.cutoff(name)):
            n = []
            for steps in (0, 10):
                before = hip.lib.grappa_launch_count(0)
                _run(hip, b, m, k, cut, vel=v, n_steps=steps)
                n.append(hip.lib.grappa_launch_count(0) - before)
            added[(name, cut is not None)], base[(name, cut is not None)] = n[1] - n[0], n[0]
    print(f"launches added by 10 steps: {added}; by init + finish: {base}")
    assert all(a == 20 for a in added.values()), added
    for name in ("s65_C3", "s513_C1"):
        # init gains the launch of the boxes and ranges; the finish's cut energy entry has one launch more than the planned one
        assert base[(name, True)] == base[(name, False)] + 2, base


# ------------------------------------------------------------------------------------------------ 3. bits
THERMO = dict(friction=20.0, temperature=300.0, init_temperature=300.0)


def test_two_runs_chunks_and_continuation_give_the_same_bits(hip):
    b, m, k, _ = _inputs(ms.MIXED)
    cut = mc.cutoff(ms.MIXED)
    a = _run(hip, b, m, k, cut, n_steps=40, save_every=8, first_step=3, **THERMO)
    _same_bits(a, _run(hip, b, m, k, cut, n_steps=40, save_every=8, first_step=3, **THERMO), "two runs", keys=OUTS + FRAMES)
    _same_bits(a, _run(hip, b, m, k, cut, n_steps=40, save_every=8, first_step=3, steps_per_call=8, **THERMO), "8 steps per call", keys=OUTS + FRAMES)
    one = _run(hip, b, m, k, cut, n_steps=16, save_every=8, first_step=3, **THERMO)
    two = _run(hip, b, m, k, cut, vel=one["vel"], xyz=one["xyz"], n_steps=24, save_every=8, first_step=19, **THERMO)
    _same_bits(a, two, "40 steps against 16 + 24", keys=("xyz", "vel", "epot", "ekin", "status"))
    for key in FRAMES:
        assert torch.equal(_bits(a[key]), _bits(torch.cat([one[key], two[key]]))), key
    plain = _run(hip, b, m, k, None, n_steps=40, save_every=8, first_step=3, **THERMO)
    assert not torch.equal(_bits(a["xyz"]), _bits(plain["xyz"])), "the cutoff changed nothing"


def test_steps_per_launch_through_simulate_graph(hip):
    from grappa_amd import backend
    from grappa_amd.dynamics import simulate_graph
    from grappa_amd.relax import graph_from_parameters
    old = backend._BACKEND
    backend.set_backend(hip)
    try:
        b, m, k, _ = _inputs("s65_C3")
        mol = b.mols[0]
        cut = mc.cutoff("s65_C3")
        g = graph_from_parameters(_parameters(mol), mol["xyz"].transpose(1, 0, 2)).to("cuda")
        nb = NonbondedBatch([mol["nb"]]).to("cuda")
        opts = dict(n_steps=20, save_every=5, friction=20.0, temperature=300.0)
        runs = [simulate_graph(g, m, nb, keys=k, first_step=2, stepwise="auto", steps_per_launch=s, cutoff=cut, **opts) for s in (10000, 7)]
        seam = _run(hip, b, m, k, cut, first_step=2, init_temperature=300.0, **opts)
        for r in runs:
            assert bool((r.steps == 20).all()) and not r.status.any() and r.frames.shape == (4, 65, 3, 3)
            for f, key in (("xyz", "xyz"), ("velocities", "vel"), ("potential_energy", "epot"), ("kinetic_energy", "ekin"), ("frames", "frames_xyz"),
                           ("frame_potential_energy", "frames_epot"), ("frame_kinetic_energy", "frames_ekin")):
                assert torch.equal(_bits(getattr(r, f).cpu()), _bits(seam[key])), f
    finally:
        backend.set_backend(old)


@pytest.mark.parametrize("name", ["s513_C1", ms.MIXED])
def test_pruning_changes_no_bit_over_forty_steps(hip, name):
    b, m, k, _ = _inputs(name)
    on = _run(hip, b, m, k, mc.cutoff(name), n_steps=40, save_every=8, **THERMO)
    off = _run(hip, b, m, k, mc.cutoff(name, prune=False), n_steps=40, save_every=8, **THERMO)
    _same_bits(on, off, "prune = 1 against prune = 0", keys=OUTS + FRAMES)


def test_a_null_cut_is_the_plain_entry_point(hip):
    """grappa_md_steps_*_cut_f32 with cut == NULL against grappa_md_steps_*_f32: the same launches, the same bits"""
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
    for which in ("plain", "null_cut"):
        ws = torch.zeros(int(lib.grappa_md_steps_workspace_bytes(b.N, Cc, b.B, n_blocks)), dtype=torch.uint8, device="cuda")
        bufs = _output_buffers(b, Cc, o)
        out = {kk: vv[1] for kk, vv in bufs.items()}
        head = (None, C.byref(d), C.byref(nd)) + ((None,) if which == "null_cut" else ()) + (C.byref(mo),)
        sfx = "_cut_f32" if which == "null_cut" else "_f32"
        tail = (table.data_ptr(), n_items, n_blocks, ws.data_ptr(), ws.numel())
        before = lib.grappa_launch_count(0)
        assert getattr(lib, "grappa_md_steps_init" + sfx)(*head, mass.data_ptr(), key.data_ptr(), vel.data_ptr(), *tail) == 0
        assert getattr(lib, "grappa_md_steps_run" + sfx)(*head, mass.data_ptr(), key.data_ptr(), *tail, 0, 6, None, None, None) == 0
        assert getattr(lib, "grappa_md_steps_finish" + sfx)(*head, *tail, *[out[kk].data_ptr() for kk in OUTS]) == 0
        torch.cuda.synchronize()
        outs[which] = ({kk: vv.cpu().clone() for kk, vv in out.items()}, lib.grappa_launch_count(0) - before)
    _same_bits(outs["plain"][0], outs["null_cut"][0], "cut = NULL against the plain entry points")
    assert outs["plain"][1] == outs["null_cut"][1]


# ------------------------------------------------------------------------------------------------ 4. energies
def test_epot_is_the_cut_energy_kernel_plus_the_bonded_one(hip):
    """frame and final epot = the terms of grappa_mm_energy_fwd_f32 and of grappa_nonbonded_fwd_cut_f32 at the frame's coordinates,
    added in double in term order, bit for bit"""
    b, m, k, v = _inputs("s129_C3")
    cut = mc.cutoff("s129_C3")
    got = _run(hip, b, m, k, cut, vel=v, n_steps=10, save_every=5, dt=0.001)
    plan = b.plan("cuda")
    ks, eqs = [t.to("cuda") for t in b.ks], [None if q is None else q.to("cuda") for q in b.eqs]
    nbd = b.nonbonded().to("cuda")
    for x, epot, what in ((got["frames_xyz"][0], got["frames_epot"][0], "frame 0"), (got["frames_xyz"][1], got["frames_epot"][1], "frame 1"),
                          (got["xyz"], got["epot"], "final")):
        xd = x.to("cuda")
        Cc = xd.shape[1]
        e, t = torch.zeros(b.B, Cc, device="cuda"), torch.zeros(4, b.B, Cc, device="cuda")
        hip.mm_energy_fwd(plan, xd, ks, eqs, b.n_per, False, e, t)
        _, _, nt = nbd.evaluate(xd, terms=True, gradient=False, cutoff=cut)
        tot = torch.zeros(b.B, Cc, dtype=torch.float64)
        for row in torch.cat([t, nt]).cpu():
            tot = tot + row.double()
        assert torch.equal(_bits(epot), _bits(tot.float())), f"{what}: epot {epot.tolist()} terms' sum {tot.tolist()}"


def test_energy_conservation(hip):
    """NVE (md_steps_refs.NVE: 400 steps of 0.5 fs) on s2_130_9_C3 from its relaxed coordinates under the cutoff:
    D_gpu <= 2 max(D_f32, D_f64) of the restatements under the same cutoff (the factor of tests/test_gpu_md_steps.py)"""
    b, m, k, v = ms.nve_batch(), ms.masses(ms.NVE_CASE), ms.keys(ms.NVE_CASE), ms.thermal_velocities(ms.NVE_CASE)
    cut = mc.cutoff("nve")
    start = _run(hip, b, m, k, cut, vel=v, n_steps=0)
    got = _run(hip, b, m, k, cut, vel=v, **ms.NVE)
    assert not got["status"].any() and bool((got["steps"] == ms.NVE["n_steps"]).all())
    d_gpu = md.drift(start["epot"].double() + start["ekin"].double(), got["frames_epot"].double() + got["frames_ekin"].double())
    d32, d64 = mc.nve_drift(torch.float32), mc.nve_drift(torch.float64)
    print(f"energy conservation, cutoff {cut.distance:.4f}: D_gpu {d_gpu:.4f}, D_f32 {d32:.4f}, D_f64 {d64:.4f} kcal/mol, D_gpu / max = {d_gpu / max(d32, d64):.3f}")
    assert d_gpu <= 2 * max(d32, d64)


# ------------------------------------------------------------------------------------------------ 5. the public door
def test_simulate_with_a_cutoff(hip):
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
        cut = mc.cutoff(name)
        before = hip.lib.grappa_launch_count(0)
        with pytest.raises(ValueError, match='stepwise="auto"'):
            simulate(p, xyz, m, mol["nb"], velocities=vel, n_steps=5, friction=0.0, stepwise=False, cutoff=9.0)
        assert hip.lib.grappa_launch_count(0) == before, "a refused call launched something"
        r = simulate(p, xyz, m, mol["nb"], velocities=vel, keys=k, stepwise="auto", n_steps=5, friction=0.0, dt=0.001, cutoff=cut)
        assert r.xyz.shape == xyz.shape and bool((r.steps == 5).all()) and not r.status.any()
        got = {"xyz": torch.from_numpy(np.ascontiguousarray(r.xyz.transpose(1, 0, 2))).float(),
               "vel": torch.from_numpy(np.ascontiguousarray(r.velocities.transpose(1, 0, 2))).float()}
        _gate_state(name, "5 steps through simulate(cutoff=, stepwise='auto')", b, got, mc.verlet(name)[5], [q[5] for q in mc.verlet32(name)])
        plain = simulate(p, xyz, m, mol["nb"], velocities=vel, keys=k, stepwise="auto", n_steps=5, friction=0.0, dt=0.001, cutoff=9.0)
        assert bool(np.isfinite(plain.xyz).all()) and bool((plain.steps == 5).all())          # a plain float is a Cutoff
    finally:
        backend.set_backend(old)
