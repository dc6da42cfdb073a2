"""The FIRE loop of include/grappa_hip.h (grappa_relax_fire_f32) restated in torch, the input generator and the case tables of
tests/test_host_relax.py (CPU) and tests/test_gpu_relax.py.

fire_ref runs the loop for every (molecule, conformation) of a batch at once with per-item state; gradients come from
kernel_refs.mm_ref64 plus nonbonded_refs.nb_ref, in float64 (the truth) or float32 (what calibrates the trajectory bound).  It returns
snapshots of the coordinates and, per step, P / (Fn vn): a conformation whose |P| / (Fn vn) stays above BRANCH_MARGIN takes the same
branch of FIRE in every arithmetic, so its trajectory can be compared elementwise.

Molecules are branched zig-zag chains (bond 1.53 A, angle 111 degrees, a side atom on every third chain atom) with k_bond 400-700,
k_angle 80-140, propers of three periodicities (|k| <= 1, 0.5, 0.3), impropers of two on the branch points, charges in +-0.3 summing
to 0, sigma 3-3.5, eps 0.05-0.15, exceptions from NonbondedParameters.from_bonds, and a jitter of 0.15 A per conformation."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

import kernel_refs as kr
import nonbonded_refs as nr
from grappa_amd import _hostlib, _lib
from grappa_amd.nonbonded import NonbondedBatch, NonbondedParameters
from grappa_amd.relax import RELAX_DEFAULTS

LEVELS = ("n2", "n3", "n4", "n4_improper")
ARITY = (2, 3, 4, 4)
N_PER = [0, 0, 3, 2]
BRANCH_MARGIN = 0.01
C_GATE = 64
TRAJ_STEPS = (1, 5, 40)


# ------------------------------------------------------------------------------------------------------------------------- inputs
def _place(p1, p2, p3, r, theta, phi):
    """a point at distance r from p3, angle theta at p3 towards p2 and dihedral phi about p2-p3 relative to p1"""
    bc = (p3 - p2) / np.linalg.norm(p3 - p2)
    nrm = np.cross(p2 - p1, bc)
    nrm /= np.linalg.norm(nrm)
    m = np.stack([bc, np.cross(nrm, bc), nrm], axis=1)
    return p3 + m @ np.array([-r * math.cos(theta), r * math.sin(theta) * math.cos(phi), r * math.sin(theta) * math.sin(phi)])


def gen_molecule(n, C, rng):
    """-> dict(n, idx (4 int64 arrays (T, s)), ks, eqs (float32 arrays), nb (NonbondedParameters), xyz (n, C, 3) float32)"""
    r0, th0 = 1.53, math.radians(111.0)
    parent, chain = [-1], [0]
    for i in range(1, n):
        if i >= 3 and i % 3 == 0 and len(chain) >= 3:
            parent.append(chain[-2])              # a side atom on the chain atom before the last
        else:
            parent.append(chain[-1])
            chain.append(i)
    pos = np.zeros((n, 3))
    on_chain = set(chain)
    sign = 1.0
    for i in range(1, n):
        p = parent[i]
        if p == 0:
            pos[i] = [r0, 0.0, 0.0]
        elif parent[p] == 0 and i in on_chain:
            pos[i] = pos[p] + r0 * np.array([-math.cos(th0), math.sin(th0), 0.0])
        else:
            gp = parent[p]
            ggp = parent[gp] if parent[gp] >= 0 else None
            ref = pos[ggp] if ggp is not None else pos[gp] + np.array([0.3, -0.4, 1.0])
            if i in on_chain:
                pos[i] = _place(ref, pos[gp], pos[p], r0, th0, math.pi)
            else:
                pos[i] = _place(ref, pos[gp], pos[p], r0, th0, sign * math.pi / 3)
                sign = -sign
    bonds = np.array([[parent[i], i] for i in range(1, n)], dtype=np.int64).reshape(-1, 2)
    if n >= 2:
        angles, propers = _hostlib.enumerate_tuples(bonds)
        angles, propers = np.asarray(angles, dtype=np.int64).reshape(-1, 3), np.asarray(propers, dtype=np.int64).reshape(-1, 4)
    else:
        angles, propers = np.zeros((0, 3), np.int64), np.zeros((0, 4), np.int64)
    nbrs = [[] for _ in range(n)]
    for a, b in bonds:
        nbrs[a].append(int(b))
        nbrs[b].append(int(a))
    impropers = np.array([[v[0], v[1], a, v[2]] for a, v in enumerate(nbrs) if len(v) == 3], dtype=np.int64).reshape(-1, 4)
    idx = [bonds, angles, propers, impropers]
    T = [a.shape[0] for a in idx]
    f32 = lambda a: np.asarray(a, dtype=np.float32)      # noqa: E731
    ks = [f32(rng.uniform(400, 700, T[0])), f32(rng.uniform(80, 140, T[1])),
          f32(rng.uniform(-1, 1, (T[2], 3)) * np.array([1.0, 0.5, 0.3])), f32(rng.uniform(-1, 1, (T[3], 2)) * np.array([1.0, 0.5]))]
    eqs = [f32(np.full(T[0], r0)), f32(np.full(T[1], th0)), None, None]
    q = rng.uniform(-0.3, 0.3, n)
    if n:
        q = q - q.mean()
        q *= 0.3 / max(np.abs(q).max(), 0.3)
    nb = NonbondedParameters.from_bonds(bonds, q, rng.uniform(3.0, 3.5, n), rng.uniform(0.05, 0.15, n))
    xyz = pos[:, None, :] + rng.uniform(-0.15, 0.15, size=(n, C, 3))
    return dict(n=n, idx=idx, ks=ks, eqs=eqs, nb=nb, xyz=xyz.astype(np.float32))


class Batch:
    """molecules concatenated: what the kernel's seam (HipBackend.relax_fire) and the float64 restatement read"""

    def __init__(self, mols):
        self.mols = mols
        self.B = len(mols)
        self.counts = [m["n"] for m in mols]
        self.ptr = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.N = int(self.ptr[-1])
        self.idx = [torch.from_numpy(np.concatenate([m["idx"][l] + o for m, o in zip(mols, self.ptr)]).reshape(-1, ARITY[l])) for l in range(4)]
        self.mol_ptr = [torch.from_numpy(np.concatenate([[0], np.cumsum([m["idx"][l].shape[0] for m in mols])]).astype(np.int32)) for l in range(4)]
        self.ks = [torch.from_numpy(np.concatenate([m["ks"][l] for m in mols])) for l in range(4)]
        self.eqs = [torch.from_numpy(np.concatenate([m["eqs"][l] for m in mols])) for l in range(2)] + [None, None]
        self.params = [m["nb"] for m in mols]
        self.xyz = torch.from_numpy(np.concatenate([m["xyz"] for m in mols], axis=0))
        self.atom_mol = torch.repeat_interleave(torch.arange(self.B), torch.tensor(self.counts))
        self.n_per = N_PER

    @classmethod
    def from_tables(cls, counts, idx, mol_ptr, ks, eqs, n_per, params, xyz):
        """the same view made from a call's own tables (the fake backend of tests/test_host_relax.py)"""
        self = cls.__new__(cls)
        self.mols, self.B, self.counts = None, len(counts), [int(c) for c in counts]
        self.ptr = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.N = int(self.ptr[-1])
        self.idx, self.mol_ptr, self.ks, self.eqs, self.n_per, self.params, self.xyz = idx, mol_ptr, ks, eqs, list(n_per), params, xyz
        self.atom_mol = torch.repeat_interleave(torch.arange(self.B), torch.tensor(self.counts))
        return self

    def plan(self, device="cpu"):
        """the fields of a BatchPlan that the MM descriptor reads (BatchPlan itself refuses an atom without a bond: a single atom),
        with the atom -> (tuple, level, position) incidence built here"""
        atoms = np.concatenate([self.idx[l].numpy().T.reshape(-1) for l in range(4)])
        codes = np.concatenate([(np.tile(np.arange(self.idx[l].shape[0], dtype=np.int64), ARITY[l]) << 4) | (l << 2)
                                | np.repeat(np.arange(ARITY[l], dtype=np.int64), self.idx[l].shape[0]) for l in range(4)])
        order = np.argsort(atoms, kind="stable")
        inc_ptr = np.concatenate([[0], np.cumsum(np.bincount(atoms, minlength=self.N))]).astype(np.int32)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int32))).to(device)      # noqa: E731
        codes = codes[order] if len(codes) else np.zeros(1, np.int64)
        return SimpleNamespace(N=self.N, B=self.B, T={lv: int(self.idx[l].shape[0]) for l, lv in enumerate(LEVELS)},
                               idx32={lv: i32(self.idx[l].numpy() if self.idx[l].numel() else np.zeros(4)) for l, lv in enumerate(LEVELS)},
                               mol_ptr={lv: i32(self.mol_ptr[l].numpy()) for l, lv in enumerate(LEVELS)}, inc_ptr=i32(inc_ptr), inc_code=i32(codes),
                               atom_molptr=i32(self.ptr), indptr=i32(np.zeros(1)), device=torch.device(device))

    def nonbonded(self, zero=False):
        if zero:
            return NonbondedBatch([NonbondedParameters(np.zeros(p.n_atoms), p.sigma, np.zeros(p.n_atoms)) for p in self.params])
        return NonbondedBatch(self.params)

    def subset(self, which):
        return Batch([self.mols[k] for k in which])


def forces(batch: Batch, x: torch.Tensor, dtype=torch.float64, nonbonded=True):
    """x (N, C, 3) -> dict: E (B,C), terms (6,B,C), G (N,C,3), and the gate's scales abs_e (B,C), abs_terms (6,B,C), abs_f (N,C): the
    scales of the MM-energy GPU tests (the tensor's largest magnitude) and of the nonbonded ones (sum |e_ij|, sum_j |f_ij|), added"""
    C = x.shape[1]
    z = torch.zeros(batch.B, C), torch.zeros(batch.N, C, 3)
    if sum(int(i.shape[0]) for i in batch.idx):
        mm = kr.mm_ref64(batch.idx, batch.mol_ptr, batch.B, x, batch.ks, batch.eqs, batch.n_per, False, z[0], z[1], dtype=dtype)
    else:          # (single atoms only: nothing for autograd to differentiate)
        mm = dict(E=torch.zeros(batch.B, C, dtype=dtype), G=torch.zeros(batch.N, C, 3, dtype=dtype), terms=torch.zeros(4, batch.B, C, dtype=dtype))
    mx = lambda t: float(t.abs().max()) if t.numel() else 0.0      # noqa: E731
    E, G, terms = mm["E"], mm["G"], mm["terms"]
    abs_e, abs_f = torch.full((batch.B, C), mx(E), dtype=torch.float64), torch.full((batch.N, C), mx(G), dtype=torch.float64)
    abs_t = torch.stack([torch.full((batch.B, C), mx(terms[l]), dtype=torch.float64) for l in range(4)])
    if nonbonded:
        nb = nr.nb_ref(batch.params, x, dtype)
        E, G, terms = E + nb["energy"], G + nb["grad"], torch.cat([terms, nb["terms"]])
        abs_e, abs_f, abs_t = abs_e + nb["abs_e"].double(), abs_f + nb["abs_f"].double(), torch.cat([abs_t, nb["abs_terms"].double()])
    else:
        terms, abs_t = torch.cat([terms, torch.zeros(2, batch.B, C, dtype=dtype)]), torch.cat([abs_t, torch.zeros(2, batch.B, C, dtype=torch.float64)])
    return dict(E=E, terms=terms, G=G, abs_e=abs_e, abs_terms=abs_t, abs_f=abs_f)


def bond_rounding(batch: Batch, x: torch.Tensor):
    """(N, C) float64: sum over the atom's bonds of k r.  fp32 holds a bond length to u32 r whatever the size of r - eq (the square
    root and the sum under it round once each), so the bond's force k (r - eq) carries an absolute error of the order u32 k r on both
    of its atoms -- also at a minimum, where the force itself is almost zero."""
    x = x.detach().double()
    out = torch.zeros(x.shape[0], x.shape[1], dtype=torch.float64)
    ix = batch.idx[0].long()
    if ix.shape[0]:
        kr_ = batch.ks[0].double()[:, None] * (x[ix[:, 0]] - x[ix[:, 1]]).norm(dim=-1)
        out.index_add_(0, ix[:, 0], kr_)
        out.index_add_(0, ix[:, 1], kr_)
    return out


def _per_mol(batch, t, op):
    """t (N, C) -> (B, C): sum or max (NaN wins) over each molecule's atoms (a molecule without atoms gives 0)"""
    zero = torch.zeros(t.shape[1], dtype=t.dtype)
    red = (lambda u: u.sum(0)) if op == "sum" else (lambda u: u.max(0).values)
    return torch.stack([red(t[batch.ptr[b]:batch.ptr[b + 1]]) if batch.counts[b] else zero for b in range(batch.B)])


def fire_ref(batch: Batch, dtype=torch.float64, nonbonded=True, snapshots=(), **opts):
    """the loop of grappa_relax_fire_f32 for all (molecule, conformation) items at once.  -> dict: xyz (N,C,3), steps, status (B,C),
    gmax (B,C), snap {step: xyz after that many steps of every item still running}, margin: list over loop iterations of P / (Fn vn)
    (B,C) (nan where vn = 0 or the item has stopped), P: the same list of P"""
    o = {**RELAX_DEFAULTS, **opts}
    c = lambda v: torch.tensor(v, dtype=dtype)      # noqa: E731
    tol, dt_max, max_disp, f_inc, f_dec, a0, f_alpha = (c(o[k]) for k in ("tolerance", "dt_max", "max_disp", "f_inc", "f_dec", "alpha_start", "f_alpha"))
    x = batch.xyz.to(dtype).clone()
    B, C = batch.B, x.shape[1]
    v = torch.zeros_like(x)
    h, al = torch.full((B, C), o["dt_start"], dtype=dtype), torch.full((B, C), o["alpha_start"], dtype=dtype)
    npos, steps = torch.zeros(B, C, dtype=torch.long), torch.zeros(B, C, dtype=torch.long)
    status = torch.full((B, C), -1, dtype=torch.long)
    gmax_out = torch.zeros(B, C, dtype=dtype)
    empty = torch.tensor([n == 0 for n in batch.counts])[:, None].expand(B, C)
    snap, margins, Ps = {}, [], []
    am = batch.atom_mol
    it = 0
    while True:
        if it in snapshots:
            snap[it] = x.clone()
        g = forces(batch, x, dtype, nonbonded)["G"]
        run = status < 0
        gmax = _per_mol(batch, g.norm(dim=-1), "max")
        newly = lambda m, code: status.masked_fill_(run & m & (status < 0), code)      # noqa: E731
        gmax_out = torch.where(run, gmax, gmax_out)
        newly(~torch.isfinite(gmax), 2)
        newly(gmax <= tol, 1)
        newly(steps == o["max_steps"], 0)
        status.masked_fill_(empty, 0)
        run = status < 0
        if not bool(run.any()):
            break
        F = -g
        P = _per_mol(batch, (F * v).sum(-1), "sum")
        Fn = torch.sqrt(_per_mol(batch, (F * F).sum(-1), "sum"))
        vn = torch.sqrt(_per_mol(batch, (v * v).sum(-1), "sum"))
        nanv = torch.full_like(P, float("nan"))
        margins.append(torch.where(run & (vn > 0), P / (Fn * vn), nanv))
        Ps.append(torch.where(run, P, nanv))
        pos = P > 0
        mix = torch.where(pos, al * (vn / Fn), torch.zeros_like(al))
        keep = torch.where(pos, 1 - al, torch.zeros_like(al))
        grow = pos & (npos >= o["n_min"])
        h_new = torch.where(pos, torch.where(grow, torch.minimum(h * f_inc, dt_max), h), h * f_dec)
        al_new = torch.where(pos, torch.where(grow, al * f_alpha, al), a0.expand_as(al))
        npos_new = torch.where(pos, npos + 1, torch.zeros_like(npos))
        vv = keep[am][..., None] * v + mix[am][..., None] * F
        vv = vv + h_new[am][..., None] * F
        d = h_new[am][..., None] * vv
        dm = _per_mol(batch, d.norm(dim=-1), "max")
        s = torch.where(dm > 0, torch.minimum(torch.ones_like(dm), max_disp / dm), torch.ones_like(dm))
        ra = run[am][..., None]
        x = torch.where(ra, x + s[am][..., None] * d, x)
        v = torch.where(ra, s[am][..., None] * vv, v)
        h, al, npos = torch.where(run, h_new, h), torch.where(run, al_new, al), torch.where(run, npos_new, npos)
        steps = steps + run.long()
        it += 1
    return dict(xyz=x, steps=steps, status=status, gmax=gmax_out, snap=snap, margin=margins, P=Ps)


# ------------------------------------------------------------------------------------------------------------------------- cases
def max_atoms() -> int:
    """the kernel's size limit, from the library itself"""
    return _lib.relax_max_atoms()


def case_table():
    """name -> (molecule sizes, C).  "max": one molecule at the kernel's size limit, resolved when the case is built"""
    cases = {f"n{n}_C{C}": ((n,), C) for n in (1, 2, 3, 9, 33, 65) for C in (1, 3)}
    cases["mixed"] = ((1, 2, 17, 65, 5), 3)
    cases["max"] = (("max",), 1)
    return cases


SALT = {"mixed": 1}          # (seeds chosen so that every convergence case converges within the default max_steps in float64)
TRAJ_CASES = [k for k in case_table() if k != "max" and not k.startswith("n1_")]
CONV_CASES = [f"n{n}_C{C}" for n in (1, 2, 3, 9, 33) for C in (1, 3)] + ["mixed"]


@functools.lru_cache(maxsize=None)
def case(name) -> Batch:
    """computed once and shared: treat as read-only"""
    sizes, C = case_table()[name]
    sizes = tuple(max_atoms() if n == "max" else n for n in sizes)
    rng = np.random.default_rng(sum(map(ord, name)) * 7919 + C + 1000003 * SALT.get(name, 0))
    return Batch([gen_molecule(n, C, rng) for n in sizes])


@functools.lru_cache(maxsize=None)
def forces_of(name, dtype=torch.float64, nonbonded=True):
    b = case(name)
    return forces(b, b.xyz, dtype, nonbonded)


def trajectory(name, dtype=torch.float64, steps=max(TRAJ_STEPS)):
    """tolerance 0, `steps` steps, snapshots after TRAJ_STEPS"""
    return _trajectory(name, dtype, steps)


@functools.lru_cache(maxsize=None)
def _trajectory(name, dtype, steps):
    return fire_ref(case(name), dtype, True, snapshots=TRAJ_STEPS, tolerance=0.0, max_steps=steps)


@functools.lru_cache(maxsize=None)
def converged(name):
    """the float64 restatement with the default options"""
    return fire_ref(case(name), torch.float64, True)


def margin_ok(name, max_steps, steps=max(TRAJ_STEPS)):
    """(B, C) bool: |P| / (Fn vn) >= BRANCH_MARGIN in every compared loop iteration 1 .. max_steps - 1 of the float64 restatement"""
    m = trajectory(name, torch.float64, steps)["margin"][1:max_steps]
    b = case(name)
    ok = torch.ones(b.B, b.xyz.shape[1], dtype=torch.bool)
    for t in m:
        ok &= ~(t.abs() < BRANCH_MARGIN)          # (nan: the item has stopped, a single atom)
    return ok


def has_uphill_step(name, max_steps=max(TRAJ_STEPS)):
    return any(bool((p <= 0).any()) for p in trajectory(name)["P"][1:max_steps])


def gate_forces(got_e, got_terms, got_g, r64, r32, what):
    """energy, the six terms and every gradient row through the calibrated gate |gpu - f64| <= 2 |f32 - f64| + 64 u32 scale"""
    rows = nr.rows
    if got_e is not None:
        kr.assert_calibrated(rows(got_e, 1), rows(r32["E"], 1), rows(r64["E"], 1), C_GATE, r64["abs_e"].reshape(-1), f"{what}: energy")
    if got_terms is not None:
        for k, nm in enumerate(("bonds", "angles", "propers", "impropers", "LJ", "Coulomb")):
            kr.assert_calibrated(rows(got_terms[k], 1), rows(r32["terms"][k], 1), rows(r64["terms"][k], 1), C_GATE,
                                 r64["abs_terms"][k].reshape(-1), f"{what}: {nm} energy")
    if got_g is not None:
        kr.assert_calibrated(rows(got_g, 3), rows(r32["G"], 3), rows(r64["G"], 3), C_GATE, r64["abs_f"].reshape(-1), f"{what}: gradient")
