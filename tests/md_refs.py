"""The dynamics of include/grappa_hip.h (grappa_md_langevin_f32) restated in numpy and torch, never imported by the product: the
generator (Philox4x32-10 in uint64 arithmetic, the Box-Muller map in float64), the BAOAB loop for every (molecule, conformation) of a
batch at once with per-item state (`baoab_ref`, forces from relax_refs.forces in float64 -- the truth -- or float32 -- what calibrates
the trajectory gates), and the inputs of tests/test_md_refs.py (CPU) and tests/test_gpu_md.py.

Cases: those of relax_refs.case_table plus "edge256" (255, 256 and 257 atoms in one batch: the switch from several slices to one slice
and two atoms per thread) and "n9_C64" (9 atoms x 64 conformations: the replicas of the conservation and equipartition tests).  The
replicas start within 0.01 A of the molecule's minimum (relax_refs.fire_ref in float64): relax_refs' chain geometry lies 20 to 35
kcal/mol above it, three times the molecule's thermal energy at 300 K, and a run of 2000 steps from there measures the decay of that
excess, not the thermostat.  The thermostat test draws its start velocities at twice its temperature, which a harmonic system started
at its minimum shares out into the thermostat's energy within a vibration.  Masses are those of
constants.ATOMIC_MASSES for atomic numbers drawn from {1, 6, 7, 8}."""
import functools

import numpy as np
import torch

import relax_refs as rr
from grappa_amd import constants

ACC = 418.4
KB = 0.0019872041
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
MD_OPTS = {"dt": 0.001, "temperature": 300.0, "friction": 0.0, "init_temperature": 0.0, "n_steps": 0, "save_every": 0, "first_step": 0}
TRAJ_STEPS = (1, 5, 40)
# Philox4x32-10 known answers of Random123 (kat_vectors): (counter, key) -> output
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


# ---------------------------------------------------------------------------------------------------------------------- the generator
def philox(key, c0, c1, c2, c3):
    """Philox4x32-10: key (uint64), counter words (< 2^32), arrays that broadcast -> (..., 4) uint64 holding the four 32-bit words"""
    key = np.asarray(key, dtype=np.uint64)
    k0, k1 = key & MASK, key >> np.uint64(32)
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in (c0, c1, c2, c3)]
    k0, k1, *c = np.broadcast_arrays(k0, k1, *c)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # (32 x 32 bits: no overflow of uint64)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(c, axis=-1)


def normal3(key, atom, conf, step, purpose):
    """the three normal deviates of (key, atom in molecule, conformation, step, purpose) in float64 -> (..., 3)"""
    w = philox(key, atom, conf, step, purpose) >> np.uint64(8)
    u = lambda k: (w[..., k].astype(np.float64) + 0.5) * 2.0 ** -24      # noqa: E731
    r = lambda k: np.sqrt(-2.0 * np.log(u(k)))      # noqa: E731
    a = lambda k: 2.0 * np.pi * w[..., k].astype(np.float64) * 2.0 ** -24      # noqa: E731
    return np.stack([r(0) * np.cos(a(1)), r(0) * np.sin(a(1)), r(2) * np.cos(a(3))], axis=-1)


def noise_ref(counts, keys, C, step, purpose):
    """z of every (atom, conformation) of a batch with `counts` atoms per molecule -> (N, C, 3) float64 tensor"""
    keys = np.asarray(keys, dtype=np.uint64)
    key = np.repeat(keys, counts)[:, None]
    atom = np.concatenate([np.arange(n) for n in counts] + [np.zeros(0, dtype=np.int64)])[:, None]
    return torch.from_numpy(normal3(key, atom, np.arange(C)[None, :], step, purpose))


# ------------------------------------------------------------------------------------------------------------------------- the loop
def _per_item(batch, t, op):
    return rr._per_mol(batch, t, op)


def kinetic(batch, m, v):
    """(B, C) float64: 0.5 / ACC sum m v^2"""
    return _per_item(batch, (m[:, None] * (v.double() ** 2).sum(-1)), "sum") * (0.5 / ACC)


def baoab_ref(batch, masses, dtype=torch.float64, nonbonded=True, velocities=None, noise=None, keys=None, snapshots=(), **opts):
    """the loop of grappa_md_langevin_f32 for all items at once.  masses (N,) (0: frozen); velocities (N,C,3) or None (drawn at
    init_temperature from purpose-1 noise); noise(step, purpose) -> (N,C,3) float64 (default: the restated generator with `keys`).
    The step's constants are formed in float64 and rounded once to `dtype`, as the library does.  -> dict: xyz, vel (N,C,3), epot,
    ekin (B,C float64: ekin from the velocities held in `dtype`), steps, status (B,C), frame_xyz (F,N,C,3), frame_epot, frame_ekin
    (F,B,C), written (F,B,C) bool, snap {k: (xyz, vel) after k steps}"""
    o = {**MD_OPTS, **opts}
    B, C, counts = batch.B, batch.xyz.shape[1], batch.counts
    if noise is None:
        noise = lambda step, purpose: noise_ref(counts, keys, C, step, purpose)      # noqa: E731
    c = lambda val: torch.tensor(val, dtype=torch.float64).to(dtype)      # noqa: E731
    dt = float(np.float32(o["dt"]))          # (the options reach the library as float32)
    fr, T, T0 = (float(np.float32(o[k])) for k in ("friction", "temperature", "init_temperature"))
    c1d = np.exp(-fr * dt)
    h2, hk, c1, c2, kt, kt0 = c(0.5 * dt), c(0.5 * dt * ACC), c(c1d), c(np.sqrt(1.0 - c1d * c1d)), c(ACC * KB * T), c(ACC * KB * T0)
    m = torch.as_tensor(np.asarray(masses, dtype=np.float32)).to(dtype)
    moving = m > 0
    w = torch.where(moving, 1.0 / torch.where(moving, m, torch.ones_like(m)), torch.zeros_like(m))
    kw, sg = (hk * w)[:, None, None], (c2 * torch.sqrt(kt * w))[:, None, None]
    mv = moving[:, None, None]
    am = batch.atom_mol
    x = batch.xyz.to(dtype).clone()
    if velocities is not None:
        v = torch.where(mv, velocities.to(dtype), torch.zeros_like(x))
    elif T0 > 0:
        v = torch.sqrt(kt0 * w)[:, None, None] * noise(o["first_step"], 1).to(dtype)
    else:
        v = torch.zeros_like(x)

    def evaluate(xx):
        f = rr.forces(batch, xx, dtype, nonbonded)
        return f["G"], f["E"].double(), ~torch.isfinite(_per_item(batch, f["G"].norm(dim=-1), "max"))

    g, E, bad = evaluate(x)
    empty = torch.tensor([n == 0 for n in counts])[:, None].expand(B, C)
    status = torch.where(bad & ~empty, 2, 0)
    run = ~bad & ~empty
    steps = torch.zeros(B, C, dtype=torch.long)
    every = o["save_every"]
    F = o["n_steps"] // every if every > 0 else 0
    fx, fe, fk = torch.zeros(F, *x.shape, dtype=dtype), torch.zeros(F, B, C, dtype=torch.float64), torch.zeros(F, B, C, dtype=torch.float64)
    written = torch.zeros(F, B, C, dtype=torch.bool)
    snap = {0: (x.clone(), v.clone())} if 0 in snapshots else {}
    for k in range(o["n_steps"]):
        if not bool(run.any()):
            break
        ra = run[am][..., None]
        upd = ra & mv
        v1 = v - kw * g
        x1 = x + h2 * v1
        if fr > 0:
            v1 = c1 * v1 + sg * noise(o["first_step"] + k, 0).to(dtype)
        x1 = x1 + h2 * v1
        x, v = torch.where(upd, x1, x), torch.where(upd, v1, v)
        gn, En, badn = evaluate(x)
        g, E = torch.where(ra, gn, g), torch.where(run, En, E)
        v = torch.where(upd, v - kw * g, v)
        steps = steps + run.long()
        if every > 0 and (k + 1) % every == 0:
            f = (k + 1) // every - 1
            fx[f], fe[f], fk[f], written[f] = torch.where(ra, x, fx[f]), torch.where(run, E, fe[f]), torch.where(run, kinetic(batch, m.double(), v), fk[f]), run
        status = torch.where(run & badn, 2, status)
        run = run & ~badn
        if k + 1 in snapshots:
            snap[k + 1] = (x.clone(), v.clone())
    return dict(xyz=x, vel=v, epot=E, ekin=kinetic(batch, m.double(), v), steps=steps, status=status, frame_xyz=fx, frame_epot=fe,
                frame_ekin=fk, written=written, snap=snap)


# ------------------------------------------------------------------------------------------------------------------------- cases
EXTRA = {"edge256": ((255, 256, 257), 1), "n9_C64": ((9,), 64)}
REPLICA_JITTER = 0.01         # Angstrom around the minimum: see the module text
CASES = [f"n{n}_C{C}" for n in (2, 3, 9, 33, 65) for C in (1, 3)] + ["mixed", "max", "edge256", "n9_C64"]


@functools.lru_cache(maxsize=None)
def case(name) -> rr.Batch:
    """computed once and shared: treat as read-only"""
    if name not in EXTRA:
        return rr.case(name)
    sizes, C = EXTRA[name]
    rng = np.random.default_rng(sum(map(ord, name)) * 7919 + C)
    if name == "n9_C64":
        mol = rr.gen_molecule(sizes[0], 1, rng)
        low = rr.fire_ref(rr.Batch([mol]), torch.float64)
        assert int(low["status"][0, 0]) == 1, "the replicas' start did not converge"
        mol["xyz"] = (low["xyz"].numpy() + rng.uniform(-REPLICA_JITTER, REPLICA_JITTER, size=(sizes[0], C, 3))).astype(np.float32)
        return rr.Batch([mol])
    return rr.Batch([rr.gen_molecule(n, C, rng) for n in sizes])


@functools.lru_cache(maxsize=None)
def masses(name) -> np.ndarray:
    """(N,) float32 in amu"""
    rng = np.random.default_rng(sum(map(ord, name)) * 104729 + 17)
    z = rng.choice([1, 6, 7, 8], size=case(name).N)
    return np.array([constants.ATOMIC_MASSES[int(a)] for a in z], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def keys(name) -> np.ndarray:
    from grappa_amd.dynamics import mol_keys
    return mol_keys(sum(map(ord, name)), case(name).B)


@functools.lru_cache(maxsize=None)
def thermal_velocities(name, temperature=300.0) -> torch.Tensor:
    """(N, C, 3) float32: sqrt(ACC kB T / m) times normal deviates of the case's own rng"""
    b = case(name)
    rng = np.random.default_rng(sum(map(ord, name)) * 15485863 + 3)
    s = np.sqrt(ACC * KB * temperature / masses(name).astype(np.float64))
    return torch.from_numpy((s[:, None, None] * rng.standard_normal((b.N, b.xyz.shape[1], 3))).astype(np.float32))


@functools.lru_cache(maxsize=None)
def forces_of(name, dtype=torch.float64):
    """relax_refs.forces at the case coordinates"""
    b = case(name)
    return rr.forces(b, b.xyz, dtype, True)


# Sibling fp32 restatements of one trajectory: the same input turned rigidly about each conformation's centroid (velocities and noise
# turned with it).  The physics is the same and so are the coordinates' magnitudes -- hence their ulps -- but every rounding differs.
# Rounding errors of a molecule in motion grow exponentially at a rate that differs from trajectory to trajectory, so the distance of ONE
# fp32 run to float64 is one draw of that; the siblings show, from the restatement alone, where that draw can serve as a yardstick
# (tests/test_gpu_md.py _gate_state).  Each sibling is measured against the float64 restatement of its own turned input, so rounding
# the turned input to fp32 does not enter, and distances do not change under the rotation, so nothing is turned back.
ROTATIONS = (((1.0, 2.0, 3.0), 0.7), ((-2.0, 1.0, 0.5), 1.9), ((0.3, -1.0, 2.0), 2.6))          # (axis, angle in radians)


def _rotation(axis, angle):
    """Rodrigues' formula -> (3, 3) float64"""
    k = torch.tensor(axis, dtype=torch.float64)
    k = k / k.norm()
    K = torch.tensor([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def fp32_realisations(batch, m, snapshots, velocities, noise=None, **kw):
    """-> list of {k: ((xyz, vel) of the fp32 restatement, (xyz, vel) of the float64 one) after k steps}: first the input as it is,
    then its ROTATIONS (`velocities` (N,C,3), `noise` and `kw` as for baoab_ref)"""
    out = []
    for R in [None] + [_rotation(*r) for r in ROTATIONS]:
        moved, vel, nz = batch, velocities, noise
        if R is not None:
            mols = []
            for mol in batch.mols:
                x = torch.from_numpy(mol["xyz"]).double()
                c = x.mean(0, keepdim=True)
                mols.append(dict(mol, xyz=((x - c) @ R.T + c).float().numpy()))
            moved, vel = rr.Batch(mols), (velocities.double() @ R.T).float()
            if noise is not None:
                nz = lambda step, purpose, R=R: noise(step, purpose).double() @ R.T      # noqa: E731
        r32, r64 = (baoab_ref(moved, m, dt, velocities=vel, noise=nz, snapshots=snapshots, **kw)["snap"] for dt in (torch.float32, torch.float64))
        out.append({k: (r32[k], r64[k]) for k in r32})
    return out


@functools.lru_cache(maxsize=None)
def verlet(name, steps=max(TRAJ_STEPS)):
    """friction 0 from the case coordinates with thermal_velocities, snapshots after TRAJ_STEPS: the float64 restatement"""
    return baoab_ref(case(name), masses(name), torch.float64, velocities=thermal_velocities(name), snapshots=TRAJ_STEPS, n_steps=steps)["snap"]


@functools.lru_cache(maxsize=None)
def verlet32(name, steps=max(TRAJ_STEPS)):
    return fp32_realisations(case(name), masses(name), TRAJ_STEPS, velocities=thermal_velocities(name), n_steps=steps)


# the replicas: energy conservation and equipartition on n9_C64
NVE = dict(dt=0.0005, friction=0.0, n_steps=2000, save_every=50)
# (dt: at 0.0005 the stiffest bond of this molecule gives harmonic_bias = 0.069 > 0.03, so the step is halved: 0.017)
NVT = dict(dt=0.00025, friction=10.0, temperature=300.0, init_temperature=600.0, n_steps=2000, save_every=50)
NVT_DISCARD = 500 // 50          # frames before step 500


@functools.lru_cache(maxsize=None)
def nve(dtype):
    return baoab_ref(case("n9_C64"), masses("n9_C64"), dtype, velocities=thermal_velocities("n9_C64"), **NVE)


@functools.lru_cache(maxsize=None)
def nvt():
    """the float64 restatement with its own restated generator"""
    return baoab_ref(case("n9_C64"), masses("n9_C64"), torch.float64, keys=keys("n9_C64"), **NVT)


def drift(e0, frame_e):
    """D = max over frames and items of |E_tot - E_tot,0|"""
    return float((frame_e - e0[None]).abs().max())


@functools.lru_cache(maxsize=None)
def nve_drift(dtype):
    """D of the restatement in `dtype`, against its own total energy at step 0"""
    start = baoab_ref(case("n9_C64"), masses("n9_C64"), dtype, velocities=thermal_velocities("n9_C64"), n_steps=0)
    r = nve(dtype)
    return drift(start["epot"] + start["ekin"], r["frame_epot"] + r["frame_ekin"])


def replica_temperature(frame_ekin, n_moving):
    """frames (F,B,C) of kinetic energy -> (mean over replicas of the frame-averaged kinetic temperature, its standard error)"""
    t = (2.0 * frame_ekin[NVT_DISCARD:].double() / (3.0 * n_moving * KB)).mean(0).reshape(-1)
    return float(t.mean()), float(t.std(unbiased=True) / np.sqrt(t.numel()))


def harmonic_bias(name, dt):
    """a = dt^2 max_bonds ACC k (1/m_i + 1/m_j) / 2: twice BAOAB's harmonic bias (omega dt)^2 / 4 of the stiffest bond"""
    b, m = case(name), masses(name).astype(np.float64)
    ix = b.idx[0].numpy()
    return float(dt * dt * (ACC * b.ks[0].numpy().astype(np.float64) * (1.0 / m[ix[:, 0]] + 1.0 / m[ix[:, 1]])).max() / 2.0)
