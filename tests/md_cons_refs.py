"""The constrained dynamics of include/grappa_hip.h (grappa_md_langevin_cons_f32) restated in torch, never imported by the product: the
velocity projection P, the cluster-wise Newton iteration S with the library's iteration rule, cap and tolerance, and the g-BAOAB loop
for every (molecule, conformation) of a batch at once (`gbaoab_ref`; forces from relax_refs.forces, noise from md_refs.noise_ref), in
float64 -- the truth -- or float32 -- what calibrates the trajectory gates -- and the inputs of tests/test_md_cons_refs.py,
tests/test_host_md_cons.py (CPU) and tests/test_gpu_md_cons.py.

Cases: molecules of relax_refs.gen_molecule with leaves of mass 1.008 attached to some of their atoms (bond 1.09 A, placed within
0.03 A of it, so that the start's S has something to do), the force field drawn as gen_molecule draws it over the bonds of the whole
molecule.  The leaves come last in the atom order, except in "scattered".
    xh_C1, xh_C3  2 atoms: the molecule is one cluster, no free atom
    xh4       5 atoms: one cluster of four leaves
    mix       a molecule of 18 atoms with clusters of 1, 2 and 3 leaves next to free atoms, a molecule without constraints and a
              molecule without atoms, 3 conformations
    scattered mix with the atom order of its first molecule permuted: no leaf's ordinary owner is its cluster's thread
    edge256   255, 256 and 257 atoms; in the last a cluster's leaf has index 256 and its centre an index below
    k256      512 atoms, 256 one-leaf clusters: every thread owns one
    ethane64  8 atoms x 64 conformations, two clusters of three leaves: the replicas of the conservation and equipartition tests,
              started as md_refs starts n9_C64 (the float64 FIRE minimum plus 0.01 A of jitter)"""
import functools
import math

import numpy as np
import torch

import md_refs as md
import relax_refs as rr
from grappa_amd import _hostlib
from grappa_amd.constraints import MAX_LEAVES, Constraints
from grappa_amd.nonbonded import NonbondedParameters

ACC, KB = md.ACC, md.KB
MAX_ITER = 8                   # GRAPPA_MD_CONS_MAX_ITER
TOL = 2.0 ** -19
M_H = 1.008
D_XH = 1.09
TRAJ_STEPS = md.TRAJ_STEPS
TRAJ_DT = 0.002


# --------------------------------------------------------------------------------------------------------------------- the tables
class Tables:
    """the constraints of a batch (a list of Constraints or None per molecule) with batch-global atom indices: centre (K,), leaf
    (K, 4; -1 = none), d (K, 4), mol (K,)"""

    def __init__(self, batch, cons):
        ce, le, dd, mol = [], [], [], []
        for b, c in enumerate(cons):
            if c is None or c.n_clusters == 0:
                continue
            off = int(batch.ptr[b])
            ce.append(c.clusters[:, 0].astype(np.int64) + off)
            le.append(np.where(c.clusters[:, 1:] >= 0, c.clusters[:, 1:].astype(np.int64) + off, -1))
            dd.append(c.lengths.astype(np.float64))
            mol.append(np.full(c.n_clusters, b, dtype=np.int64))
        cat = lambda v, shape: torch.from_numpy(np.concatenate(v) if v else np.zeros(shape))      # noqa: E731
        self.centre, self.leaf = cat(ce, (0,)).long(), cat(le, (0, MAX_LEAVES)).long()
        self.d, self.mol = cat(dd, (0, MAX_LEAVES)).double(), cat(mol, (0,)).long()
        self.K = int(self.centre.shape[0])
        self.L = int((self.leaf >= 0).sum(1).max()) if self.K else 0          # the widest cluster: the systems solved are L x L


def solve(M, b):
    """M y = b by elimination without pivoting, written out as the kernel writes it.  M (..., L, L), b (..., L)"""
    L = M.shape[-1]
    M, b = M.clone(), b.clone()
    for i in range(L):
        inv = 1.0 / M[..., i, i]
        for j in range(i + 1, L):
            f = M[..., j, i] * inv
            M[..., j, i + 1:] = M[..., j, i + 1:] - f[..., None] * M[..., i, i + 1:]
            b[..., j] = b[..., j] - f * b[..., i]
    y = torch.zeros_like(b)
    for i in range(L - 1, -1, -1):
        y[..., i] = (b[..., i] - (M[..., i, i + 1:] * y[..., i + 1:]).sum(-1)) / M[..., i, i]
    return y


class Clusters:
    """P and S on state tensors x, v (N, C, 3) of one dtype.  w (N,): inverse masses (0: frozen)"""

    def __init__(self, tab: Tables, w, dtype, tolerance=TOL):
        self.t, self.dtype, L = tab, dtype, tab.L
        self.leaf = tab.leaf[:, :L]
        self.li = self.leaf.clamp_min(0)
        self.w0 = w[tab.centre]                                        # (K,)
        self.wl = torch.where(self.leaf >= 0, w[self.li], torch.zeros((), dtype=dtype))          # (K, L)
        self.act = (self.leaf >= 0) & (self.w0[:, None] + self.wl > 0)      # a leaf with both ends frozen is absent
        self.d2 = torch.where(self.act, (tab.d[:, :L].to(torch.float32).to(dtype)) ** 2, torch.ones((), dtype=dtype))
        self.tol2 = torch.tensor(2.0 * tolerance, dtype=torch.float64).to(dtype)
        self.eye = torch.eye(L, dtype=dtype)
        self.pair = self.act[:, :, None] & self.act[:, None, :]          # (K, L, L)
        self.c_k = torch.nonzero(self.w0 > 0)[:, 0]                      # the clusters with a moving centre, and those centres
        self.c_idx = tab.centre[self.c_k]
        self.l_k, self.l_j = torch.nonzero(self.act & (self.wl > 0), as_tuple=True)          # the moving leaves
        self.l_idx = self.li[self.l_k, self.l_j]

    def rel(self, x):
        """leaf - centre -> (K, C, L, 3), zero for an absent leaf"""
        r = x[self.li].permute(0, 2, 1, 3) - x[self.t.centre][:, :, None, :]
        return torch.where(self.act[:, None, :, None], r, torch.zeros((), dtype=self.dtype))

    def _system(self, a, b):
        """w_0 (a_k . b_l) + delta_kl w_k (a_k . b_k), identity rows for absent leaves -> (K, C, L, L)"""
        G = (a[:, :, :, None, :] * b[:, :, None, :, :]).sum(-1)
        M = self.w0[:, None, None, None] * G + self.eye * (self.wl[:, None, :] * (a * b).sum(-1))[..., None]
        return torch.where(self.pair[:, None], M, self.eye.expand_as(M))

    def _scatter(self, t, d_centre, d_leaf):
        """t + the clusters' displacements (K, C, 3) and (K, C, L, 3); a frozen or absent atom gets none (an atom is in one cluster
        only, so every index occurs once)"""
        out = t.clone()
        out[self.c_idx] = t[self.c_idx] + d_centre[self.c_k]
        out[self.l_idx] = t[self.l_idx] + d_leaf[self.l_k, :, self.l_j]
        return out

    def project(self, x, v):
        """P(x, v) -> v"""
        if self.t.K == 0:
            return v
        r, dv = self.rel(x), self.rel(v)
        mu = solve(self._system(r, r), (r * dv).sum(-1))
        mu = torch.where(self.act[:, None], mu, torch.zeros((), dtype=self.dtype))
        s = (mu[..., None] * r).sum(2)
        return self._scatter(v, self.w0[:, None, None] * s, -(self.wl[:, None, :] * mu)[..., None] * r)

    def shake(self, xref, x, v, h2):
        """S(xref, x, v) -> x, v, failed (K, C) bool, updates (K, C): the Newton updates each cluster took.  v None: positions only"""
        K, C = self.t.K, x.shape[1]
        if K == 0:
            return x, v, torch.zeros(0, C, dtype=torch.bool), torch.zeros(0, C, dtype=torch.long)
        rref, rt = self.rel(xref), self.rel(x)
        lam = torch.zeros(K, C, self.t.L, dtype=self.dtype)
        done = torch.zeros(K, C, dtype=torch.bool)
        updates = torch.zeros(K, C, dtype=torch.long)
        for it in range(MAX_ITER + 1):
            s = (lam[..., None] * rref).sum(2)
            r = rt - (self.wl[:, None, :] * lam)[..., None] * rref - self.w0[:, None, None, None] * s[:, :, None, :]
            sig = torch.where(self.act[:, None], (r * r).sum(-1) - self.d2[:, None], torch.zeros((), dtype=self.dtype))
            done = (sig.abs() <= self.tol2 * self.d2[:, None]).all(-1)          # (a sigma that is not finite: not converged)
            if it == MAX_ITER or bool(done.all()):
                break
            J = -2.0 * self._system(r, rref)
            J = torch.where(self.pair[:, None], J, self.eye.expand_as(J))
            lam = torch.where(done[..., None], lam, lam - solve(J, sig))
            updates = updates + (~done).long()
        finite = torch.isfinite(lam).all(-1)
        apply = (finite[..., None] & torch.ones_like(s, dtype=torch.bool))
        dc = torch.where(apply, self.w0[:, None, None] * s, torch.zeros((), dtype=self.dtype))
        x0_new = x[self.t.centre] + torch.where((self.w0 > 0)[:, None, None], dc, torch.zeros((), dtype=self.dtype))
        # x_k = x_0 (new) + r_k: stated as a displacement of the old x_k that gives those bits in exact arithmetic is not possible, so
        # the leaves are written, not added
        out = x.clone()
        out[self.t.centre] = x0_new
        mv = self.act & (self.wl > 0)
        kk, ll = torch.nonzero(mv, as_tuple=True)
        new_leaf = x0_new[:, :, None, :] + r
        keep = x[self.li].permute(0, 2, 1, 3)
        new_leaf = torch.where(apply[:, :, None, :], new_leaf, keep)
        out[self.li[kk, ll]] = new_leaf[kk, :, ll]
        if v is not None:
            ih = 1.0 / h2
            zero = torch.zeros((), dtype=self.dtype)
            v = self._scatter(v, torch.where(apply, self.w0[:, None, None] * s * ih, zero),
                              torch.where(apply[:, :, None, :], -((self.wl[:, None, :] * lam) * ih)[..., None] * rref, zero))
        return out, v, ~done, updates


# ------------------------------------------------------------------------------------------------------------------------- the loop
def gbaoab_ref(batch, masses, cons, dtype=torch.float64, nonbonded=True, velocities=None, noise=None, keys=None, snapshots=(),
               tolerance=TOL, constrain_start=True, **opts):
    """the loop of grappa_md_langevin_cons_f32 for all items at once; arguments and result as md_refs.baoab_ref, plus cons (a list of
    Constraints or None per molecule), tolerance and constrain_start, and in the result `updates`: the most Newton updates any S took"""
    o = {**md.MD_OPTS, **opts}
    B, C, counts = batch.B, batch.xyz.shape[1], batch.counts
    if noise is None:
        noise = lambda step, purpose: md.noise_ref(counts, keys, C, step, purpose)      # noqa: E731
    c = lambda val: torch.tensor(val, dtype=torch.float64).to(dtype)      # noqa: E731
    dt = float(np.float32(o["dt"]))
    fr, T, T0 = (float(np.float32(o[k])) for k in ("friction", "temperature", "init_temperature"))
    c1d = np.exp(-fr * dt)
    h2, hk, c1, c2, kt, kt0 = c(0.5 * dt), c(0.5 * dt * ACC), c(c1d), c(np.sqrt(1.0 - c1d * c1d)), c(ACC * KB * T), c(ACC * KB * T0)
    m = torch.as_tensor(np.asarray(masses, dtype=np.float32)).to(dtype)
    moving = m > 0
    w = torch.where(moving, 1.0 / torch.where(moving, m, torch.ones_like(m)), torch.zeros_like(m))
    kw, sg = (hk * w)[:, None, None], (c2 * torch.sqrt(kt * w))[:, None, None]
    mv = moving[:, None, None]
    am = batch.atom_mol
    tab = Tables(batch, cons)
    cl = Clusters(tab, w, dtype, tolerance)
    most = 0

    def failed_items(f):
        out = torch.zeros(B, C, dtype=torch.bool)
        if tab.K:
            out.index_put_((tab.mol[:, None].expand_as(f), torch.arange(C)[None, :].expand_as(f)), f, accumulate=True)
        return out

    x = batch.xyz.to(dtype).clone()
    fail = torch.zeros(B, C, dtype=torch.bool)
    if constrain_start:
        x, _, f, u = cl.shake(x, x, None, h2)
        fail, most = failed_items(f), max(most, int(u.max()) if u.numel() else 0)
    if velocities is not None:
        v = torch.where(mv, velocities.to(dtype), torch.zeros_like(x))
    elif T0 > 0:
        v = torch.sqrt(kt0 * w)[:, None, None] * noise(o["first_step"], 1).to(dtype)
    else:
        v = torch.zeros_like(x)
    if constrain_start or velocities is None:
        v = cl.project(x, v)

    def evaluate(xx):
        f = rr.forces(batch, xx, dtype, nonbonded)
        return f["G"], f["E"].double(), ~torch.isfinite(md._per_item(batch, f["G"].norm(dim=-1), "max"))

    g, E, bad = evaluate(x)
    empty = torch.tensor([n == 0 for n in counts])[:, None].expand(B, C)
    status = torch.where(fail, 4, torch.where(bad, 2, 0))
    status = torch.where(empty, 0, status)
    run = ~bad & ~fail & ~empty
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
        v1 = cl.project(x, v - kw * g)
        x1, v1, f1, u1 = cl.shake(x, x + h2 * v1, v1, h2)
        v1 = cl.project(x1, v1)
        if fr > 0:
            v1 = cl.project(x1, c1 * v1 + sg * noise(o["first_step"] + k, 0).to(dtype))
        x2, v1, f2, u2 = cl.shake(x1, x1 + h2 * v1, v1, h2)
        v1 = cl.project(x2, v1)
        x, v = torch.where(upd, x2, x), torch.where(upd, v1, v)
        failn = failed_items(f1 | f2) & run
        if tab.K:
            in_run = run[tab.mol]
            most = max([most] + [int(u[in_run].max()) for u in (u1, u2) if bool(in_run.any())])
        gn, En, badn = evaluate(x)
        g, E = torch.where(ra, gn, g), torch.where(run, En, E)
        v = torch.where(upd, cl.project(x, v - kw * g), v)
        steps = steps + (run & ~failn).long()          # a step whose constraint did not converge is completed but not counted
        if every > 0 and (k + 1) % every == 0:
            f = (k + 1) // every - 1
            fx[f], fe[f], fk[f], written[f] = torch.where(ra, x, fx[f]), torch.where(run, E, fe[f]), torch.where(run, md.kinetic(batch, m.double(), v), fk[f]), run
        status = torch.where(run & failn, 4, torch.where(run & badn, 2, status))
        run = run & ~badn & ~failn
        if k + 1 in snapshots:
            snap[k + 1] = (x.clone(), v.clone())
    return dict(xyz=x, vel=v, epot=E, ekin=md.kinetic(batch, m.double(), v), steps=steps, status=status, frame_xyz=fx, frame_epot=fe,
                frame_ekin=fk, written=written, snap=snap, updates=most)


def fp32_realisations(batch, m, cons, snapshots, velocities, noise=None, **kw):
    """md_refs.fp32_realisations' scheme for the constrained loop: the input as it is, then its md_refs.ROTATIONS, each as (fp32 state,
    float64 state of the same input) per snapshot"""
    out = []
    for R in [None] + [md._rotation(*r) for r in md.ROTATIONS]:
        moved, vel, nz = batch, velocities, noise
        if R is not None:
            mols = []
            for mol in batch.mols:
                x = torch.from_numpy(mol["xyz"]).double()
                ctr = x.mean(0, keepdim=True) if mol["n"] else x
                mols.append(dict(mol, xyz=((x - ctr) @ R.T + ctr).float().numpy()))
            moved, vel = rr.Batch(mols), (velocities.double() @ R.T).float()
            if noise is not None:
                nz = lambda step, purpose, R=R: noise(step, purpose).double() @ R.T      # noqa: E731
        r32, r64 = (gbaoab_ref(moved, m, cons, dt, velocities=vel, noise=nz, snapshots=snapshots, **kw)["snap"] for dt in (torch.float32, torch.float64))
        out.append({k: (r32[k], r64[k]) for k in r32})
    return out


# ------------------------------------------------------------------------------------------------------------------------- measures
def item_max(batch, t):
    """(N, C, 3) -> (B, C) float64: the largest row norm of each (molecule, conformation); 0 for a molecule without atoms"""
    zero = torch.zeros(t.shape[1], dtype=torch.float64)
    return torch.stack([t[int(batch.ptr[k]):int(batch.ptr[k + 1])].double().norm(dim=-1).max(0).values if batch.counts[k] else zero
                        for k in range(batch.B)])


def bond_errors(tab: Tables, x):
    """| |x_k - x_0| - d_k | / d_k of every constrained bond -> (n_bonds, C) float64, with the bond's molecule (n_bonds,)"""
    k, j = torch.nonzero(tab.leaf >= 0, as_tuple=True)
    r = (x.double()[tab.leaf[k, j]] - x.double()[tab.centre[k]]).norm(dim=-1)
    d = tab.d[k, j].float().double()[:, None]
    return (r - d).abs() / d, tab.mol[k]


def velocity_errors(tab: Tables, x, v):
    """|r_k . (v_k - v_0)| / |r_k| of every constrained bond -> (n_bonds, C) float64"""
    k, j = torch.nonzero(tab.leaf >= 0, as_tuple=True)
    r = x.double()[tab.leaf[k, j]] - x.double()[tab.centre[k]]
    return ((r * (v.double()[tab.leaf[k, j]] - v.double()[tab.centre[k]])).sum(-1)).abs() / r.norm(dim=-1)


# ------------------------------------------------------------------------------------------------------------------------- cases
TET = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) / math.sqrt(3.0)
CONE = math.radians(70.53)
_K = np.arange(96) + 0.5
SPHERE = np.stack([np.sqrt(1 - (1 - 2 * _K / 96) ** 2) * np.cos(math.pi * (1 + 5 ** 0.5) * _K),
                   np.sqrt(1 - (1 - 2 * _K / 96) ** 2) * np.sin(math.pi * (1 + 5 ** 0.5) * _K), 1 - 2 * _K / 96], axis=1)


def attach_leaves(mol, leaves, rng, perm=None):
    """a molecule of relax_refs.gen_molecule with leaves[centre] hydrogens attached to its atoms -> (molecule dict, Constraints, masses
    (n,) float32).  The new atoms come last; perm (n,): new index of every atom, applied to everything"""
    n0, C = mol["n"], mol["xyz"].shape[1]
    bonds0 = mol["idx"][0].reshape(-1, 2)
    nbrs = [[] for _ in range(n0)]
    for a, b in bonds0.tolist():
        nbrs[a].append(b)
        nbrs[b].append(a)
    new_bonds, pos = [], [mol["xyz"].astype(np.float64)]
    placed = pos[0][:, 0]                                                    # conformation 0 decides the directions of all
    n = n0
    for centre in sorted(leaves):
        xc = pos[0][centre]                                                  # (C, 3)
        for j in range(leaves[centre]):
            if not nbrs[centre]:
                u = TET[j]
            elif len(nbrs[centre]) == 1:          # an end atom: its leaves on a cone about the bond's continuation
                away = xc[0] - pos[0][nbrs[centre][0]][0]
                away = away / np.linalg.norm(away)
                e1 = np.cross(away, np.array([0.3, -0.4, 1.0]))
                e1 = e1 / np.linalg.norm(e1)
                phi = 2.0 * math.pi * j / leaves[centre] + 0.4 * centre
                u = math.cos(CONE) * away + math.sin(CONE) * (math.cos(phi) * e1 + math.sin(phi) * np.cross(away, e1))
            else:          # of the directions of a Fibonacci sphere the one that keeps the new atom farthest from all others
                others = np.delete(placed, centre, axis=0)
                gap = np.linalg.norm((xc[0] + D_XH * SPHERE)[:, None, :] - others[None, :, :], axis=-1).min(1)
                u = SPHERE[int(np.argmax(gap))]
            new = xc + D_XH * u + rng.uniform(-0.03, 0.03, size=(C, 3))
            pos.append(new[None])
            placed = np.concatenate([placed, new[None, 0]])
            new_bonds.append([centre, n])
            n += 1
    xyz = np.concatenate(pos, axis=0)
    bonds = np.concatenate([bonds0, np.array(new_bonds, dtype=np.int64).reshape(-1, 2)])
    is_h = np.arange(n) >= n0
    if perm is not None:
        perm = np.asarray(perm)
        bonds = perm[bonds]
        inv = np.argsort(perm)
        xyz, is_h = xyz[inv], is_h[inv]
    if n >= 3:
        angles, propers = _hostlib.enumerate_tuples(bonds)
        angles, propers = np.asarray(angles, dtype=np.int64).reshape(-1, 3), np.asarray(propers, dtype=np.int64).reshape(-1, 4)
    else:
        angles, propers = np.zeros((0, 3), np.int64), np.zeros((0, 4), np.int64)
    nb2 = [[] for _ in range(n)]
    for a, b in bonds.tolist():
        nb2[a].append(b)
        nb2[b].append(a)
    impropers = np.array([[v[0], v[1], a, v[2]] for a, v in enumerate(nb2) if len(v) == 3], dtype=np.int64).reshape(-1, 4)
    idx = [bonds, angles, propers, impropers]
    T = [a.shape[0] for a in idx]
    f32 = lambda a: np.asarray(a, dtype=np.float32)      # noqa: E731
    ks = [f32(rng.uniform(400, 700, T[0])), f32(rng.uniform(80, 140, T[1])),
          f32(rng.uniform(-1, 1, (T[2], 3)) * np.array([1.0, 0.5, 0.3])), f32(rng.uniform(-1, 1, (T[3], 2)) * np.array([1.0, 0.5]))]
    xh = is_h[bonds[:, 0]] != is_h[bonds[:, 1]]
    # an angle with a leaf in it rests where conformation 0 has it: the leaves were placed for room, not at 111 degrees
    p0 = xyz[:, 0]
    u1, u2 = p0[angles[:, 0]] - p0[angles[:, 1]], p0[angles[:, 2]] - p0[angles[:, 1]]
    here = np.arccos(np.clip((u1 * u2).sum(-1) / (np.linalg.norm(u1, axis=-1) * np.linalg.norm(u2, axis=-1)), -1.0, 1.0)) if T[1] else np.zeros(0)
    eqs = [f32(np.where(xh, D_XH, 1.53)), f32(np.where(is_h[angles].any(1), here, math.radians(111.0))), None, None]
    q = rng.uniform(-0.3, 0.3, n)
    q = q - q.mean()
    q *= 0.3 / max(np.abs(q).max(), 0.3)
    nb = NonbondedParameters.from_bonds(bonds, q, np.where(is_h, 1.5, rng.uniform(3.0, 3.5, n)), np.where(is_h, 0.02, rng.uniform(0.05, 0.15, n)))
    masses = np.where(is_h, M_H, rng.choice([12.011, 14.007, 15.999], size=n)).astype(np.float32)
    cons = Constraints.from_bonds(bonds, is_h, eqs[0])
    return dict(n=n, idx=idx, ks=ks, eqs=eqs, nb=nb, xyz=xyz.astype(np.float32)), cons, masses


def _plain(n, C, rng):
    mol = rr.gen_molecule(n, C, rng)
    return mol, None, rng.choice([12.011, 14.007, 15.999], size=n).astype(np.float32)


def _build(name):
    rng = np.random.default_rng(sum(map(ord, name)) * 7919 + 11)
    if name in ("xh_C1", "xh_C3"):
        return [attach_leaves(rr.gen_molecule(1, int(name[-1]), rng), {0: 1}, rng)]
    if name == "xh4":
        return [attach_leaves(rr.gen_molecule(1, 1, rng), {0: 4}, rng)]
    if name in ("mix", "scattered"):
        rng = np.random.default_rng(sum(map(ord, "mix")) * 7919 + 11)          # the same molecules in both
        base = rr.gen_molecule(12, 3, rng)
        # 11 ends the chain (one bond: room for three leaves), 9 is a side atom (one bond), 4 a chain atom with two bonds
        perm = None
        if name == "scattered":          # atoms 0, 1, 2 (whose ordinary owners are the three clusters' threads) are made heavy atoms
            perm = np.concatenate([[3, 5, 8], np.random.default_rng(5).permutation([0, 1, 2, 4, 6, 7] + list(range(9, 18)))])
            perm = np.argsort(perm)
        first = attach_leaves(base, {4: 1, 9: 2, 11: 3}, rng, perm)
        return [first, _plain(7, 3, rng), _plain(0, 3, rng)]
    if name == "edge256":
        return [attach_leaves(rr.gen_molecule(n - 57, 1, rng), {3 * k + 1: 1 for k in range(57)}, rng) for n in (255, 256, 257)]
    if name == "k256":
        return [attach_leaves(rr.gen_molecule(256, 1, rng), {k: 1 for k in range(256)}, rng)]
    if name == "ethane64":
        mol, cons, m = attach_leaves(rr.gen_molecule(2, 1, rng), {0: 3, 1: 3}, rng)
        low = rr.fire_ref(rr.Batch([mol]), torch.float64)
        assert int(low["status"][0, 0]) == 1, "the replicas' start did not converge"
        mol["xyz"] = (low["xyz"].numpy() + rng.uniform(-md.REPLICA_JITTER, md.REPLICA_JITTER, size=(8, 64, 3))).astype(np.float32)
        return [(mol, cons, m)]
    raise KeyError(name)


def unsatisfiable():
    """xh with d = the input length and a leaf velocity of 4000 A/ps across the bond at 1 fs: the half drift moves the leaf 2 A
    sideways, and no multiplier along the old bond brings it back"""
    batch, cons, m, keys = case("xh_C1")
    x = batch.xyz[:, 0].double()
    r = x[1] - x[0]
    d = float(np.float32(r.norm()))
    side = torch.linalg.cross(r, torch.tensor([0.3, -0.4, 1.0], dtype=torch.float64))
    v = torch.zeros(2, 1, 3)
    v[1, 0] = (4000.0 * side / side.norm()).float()
    return batch, [Constraints(cons[0].clusters, [[d, 0, 0, 0]])], m, keys, v


TRAJ_CASES = ["xh_C1", "xh_C3", "xh4", "mix", "scattered", "edge256", "k256"]
CASES = TRAJ_CASES + ["ethane64"]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (relax_refs.Batch, [Constraints or None per molecule], masses (N,) float32, keys (B,) uint64); computed once, read-only"""
    from grappa_amd.dynamics import mol_keys
    parts = _build(name)
    batch = rr.Batch([p[0] for p in parts])
    return batch, [p[1] for p in parts], np.concatenate([p[2] for p in parts]), mol_keys(sum(map(ord, name)), batch.B)


@functools.lru_cache(maxsize=None)
def tables(name) -> Tables:
    batch, cons, _, _ = case(name)
    return Tables(batch, cons)


@functools.lru_cache(maxsize=None)
def thermal_velocities(name, temperature=300.0) -> torch.Tensor:
    """(N, C, 3) float32: sqrt(ACC kB T / m) times normal deviates of the case's own rng (not projected: the start's P does that)"""
    batch, _, m, _ = case(name)
    rng = np.random.default_rng(sum(map(ord, name)) * 15485863 + 3)
    s = np.sqrt(ACC * KB * temperature / m.astype(np.float64))
    return torch.from_numpy((s[:, None, None] * rng.standard_normal((batch.N, batch.xyz.shape[1], 3))).astype(np.float32))


@functools.lru_cache(maxsize=None)
def verlet(name):
    """friction 0, 2 fs, from the case coordinates with thermal_velocities, snapshots after TRAJ_STEPS: the float64 restatement"""
    batch, cons, m, _ = case(name)
    return gbaoab_ref(batch, m, cons, torch.float64, velocities=thermal_velocities(name), snapshots=TRAJ_STEPS, n_steps=max(TRAJ_STEPS), dt=TRAJ_DT)


@functools.lru_cache(maxsize=None)
def verlet32(name):
    batch, cons, m, _ = case(name)
    return fp32_realisations(batch, m, cons, TRAJ_STEPS, velocities=thermal_velocities(name), n_steps=max(TRAJ_STEPS), dt=TRAJ_DT)


# the replicas: energy conservation and equipartition on ethane64
NVE = dict(dt=0.001, friction=0.0, n_steps=2000, save_every=50, init_temperature=600.0)
NVT = dict(dt=0.001, friction=10.0, temperature=300.0, init_temperature=300.0, n_steps=2000, save_every=50)
NVT_DISCARD = 500 // 50


@functools.lru_cache(maxsize=None)
def nve(dtype):
    """velocities drawn at 600 K by the restated generator"""
    batch, cons, m, keys = case("ethane64")
    return gbaoab_ref(batch, m, cons, dtype, keys=keys, **NVE)


@functools.lru_cache(maxsize=None)
def nve_drift(dtype):
    batch, cons, m, keys = case("ethane64")
    start = gbaoab_ref(batch, m, cons, dtype, keys=keys, **{**NVE, "n_steps": 0, "save_every": 0})
    r = nve(dtype)
    return md.drift(start["epot"] + start["ekin"], r["frame_epot"] + r["frame_ekin"])


@functools.lru_cache(maxsize=None)
def nvt():
    batch, cons, m, keys = case("ethane64")
    return gbaoab_ref(batch, m, cons, torch.float64, keys=keys, **NVT)


def degrees_of_freedom(name):
    """(B,) 3 n_moving - n_constraints with a moving end"""
    batch, cons, m, _ = case(name)
    return np.array([3 * int((m[batch.ptr[b]:batch.ptr[b + 1]] > 0).sum()) - (0 if c is None else c.n_constraints_moving(m[batch.ptr[b]:batch.ptr[b + 1]]))
                     for b, c in enumerate(cons)])


def replica_temperature(frame_ekin, dof):
    t = (2.0 * frame_ekin[NVT_DISCARD:].double() / (dof * KB)).mean(0).reshape(-1)
    return float(t.mean()), float(t.std(unbiased=True) / np.sqrt(t.numel()))
