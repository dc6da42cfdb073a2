"""The restrained FIRE loop of include/grappa_hip.h (grappa_relax_fire_restr_f32) restated in torch, and the case tables of
tests/test_host_relax_restr.py (CPU) and tests/test_gpu_relax_restr.py.

Built on relax_refs: its molecules, its Batch and its forces.  The objective is E_ff + E_r with
E_r = sum_r k_r (1 - cos(phi_r - target_r,c)) + sum_i 0.5 pos_k_i |x_i - start_i|^2; the restraint gradient is torch autograd of E_r
(oracle.cpu_ref.dihedral: the library's convention), a frozen atom's gradient is replaced by 0.  float64 is the truth, float32 the
yardstick.  With no restraints fire_restr_ref returns exactly relax_refs.fire_ref's tensors (tests/test_host_relax_restr.py asserts it).

Restraints per case: dihedrals are propers of the molecule; a target lies 0.3 to 1.5 rad from the start dihedral of its conformation and
differs per conformation; k is 100 to 239 kcal/mol; frozen atoms and tethers (5 to 50 kcal/mol/A^2) where the table says so."""
import functools
import math

import numpy as np
import torch

import relax_refs as rr
from grappa_amd.nonbonded import NonbondedParameters
from grappa_amd.relax import RELAX_DEFAULTS
from grappa_amd.restraints import MAX_DIHEDRALS, RestraintBatch, Restraints

TRAJ_STEPS = rr.TRAJ_STEPS


# ------------------------------------------------------------------------------------------------------------------------- restraints
def dihedral_t(x, ix):
    """x (N, C, 3), ix (R, 4) long -> phi (R, C) in x's dtype"""
    from oracle.cpu_ref import dihedral
    return dihedral(*[x[ix[:, j]] for j in range(4)])


class Tables:
    """a RestraintBatch seen from the restatement: batch-global dihedral atoms and per-atom arrays that always exist"""

    def __init__(self, batch: rr.Batch, rb: RestraintBatch):
        self.rb, self.R = rb, rb.R
        off = np.repeat(batch.ptr[:-1], np.diff(rb.dih_molptr.numpy().astype(np.int64)))
        self.ix = rb.dih_atoms.long() + torch.from_numpy(off)[:, None]
        self.k, self.target = rb.dih_k.double(), rb.dih_target.double()
        self.row_mol = torch.from_numpy(np.repeat(np.arange(batch.B), np.diff(rb.dih_molptr.numpy().astype(np.int64))))
        self.frozen = torch.zeros(batch.N, dtype=torch.bool) if rb.frozen is None else rb.frozen != 0
        self.pos_k = torch.zeros(batch.N, dtype=torch.float64) if rb.pos_k is None else rb.pos_k.double()


def restraint_terms(batch: rr.Batch, tb: Tables, x, start, dtype=torch.float64):
    """x, start (N, C, 3) -> dict: E (B, C) = E_r, G (N, C, 3) = dE_r/dx by autograd, phi (R, C), abs_e (B, C) and abs_g (N, C): the
    sums of the absolute contributions (|k (1 - cos)| and 0.5 pos_k d^2 are non-negative, so abs_e = E; per atom the norms of
    k sin(phi - target) dphi/dx_atom over its rows plus pos_k |x - start|)"""
    C = x.shape[1]
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    s, k, tg, pk = start.detach().to(dtype), tb.k.to(dtype), tb.target.to(dtype), tb.pos_k.to(dtype)
    E = torch.zeros(batch.B, C, dtype=dtype)
    phi = torch.zeros(0, C, dtype=dtype)
    abs_g = torch.zeros(batch.N, C, dtype=torch.float64)
    if tb.R:
        phi = dihedral_t(xx, tb.ix)
        E = E.index_add(0, tb.row_mol, k[:, None] * (1 - torch.cos(phi - tg)))
        # the rows' own derivatives, for the scale: phi of detached copies of the four positions
        pos = [xx.detach()[tb.ix[:, j]].double().clone().requires_grad_(True) for j in range(4)]
        from oracle.cpu_ref import dihedral
        p64 = dihedral(*pos)
        dd = torch.autograd.grad(p64.sum(), pos)
        coef = (tb.k[:, None] * torch.sin(p64.detach() - tb.target)).abs()
        for j in range(4):
            abs_g.index_add_(0, tb.ix[:, j], coef * dd[j].norm(dim=-1))
    d = xx - s
    E = E + rr._per_mol(batch, 0.5 * pk[:, None] * (d * d).sum(-1), "sum")
    abs_g = abs_g + tb.pos_k[:, None] * d.detach().double().norm(dim=-1)
    G = torch.autograd.grad(E.sum(), xx)[0] if E.requires_grad else torch.zeros_like(xx)
    return dict(E=E.detach(), G=G.detach(), phi=phi.detach(), abs_e=E.detach().double().abs(), abs_g=abs_g)


def objective(batch: rr.Batch, tb, x, start, dtype=torch.float64, nonbonded=True):
    """relax_refs.forces plus the restraints: its dict (E, terms: the force field's) with G and abs_f those of the objective (a frozen
    atom's row 0), Er, phi, abs_er"""
    f = rr.forces(batch, x, dtype, nonbonded)
    if tb is None:
        return f
    r = restraint_terms(batch, tb, x, start, dtype)
    G = torch.where(tb.frozen[:, None, None], torch.zeros_like(f["G"]), f["G"] + r["G"])
    return {**f, "G": G, "abs_f": f["abs_f"] + r["abs_g"], "Er": r["E"], "phi": r["phi"], "abs_er": r["abs_e"]}


def fire_restr_ref(batch: rr.Batch, rb=None, dtype=torch.float64, nonbonded=True, snapshots=(), **opts):
    """relax_refs.fire_ref on the objective E_ff + E_r.  rb: a RestraintBatch, or None / an empty one: fire_ref's tensors exactly"""
    tb = None if rb is None or rb.empty else Tables(batch, rb)
    o = {**RELAX_DEFAULTS, **opts}
    c = lambda v: torch.tensor(v, dtype=dtype)      # noqa: E731
    tol, dt_max, max_disp, f_inc, f_dec, a0, f_alpha = (c(o[k]) for k in ("tolerance", "dt_max", "max_disp", "f_inc", "f_dec", "alpha_start", "f_alpha"))
    start = batch.xyz.to(dtype).clone()
    x = start.clone()
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
        g = objective(batch, tb, x, start, dtype, nonbonded)["G"]
        run = status < 0
        gmax = rr._per_mol(batch, g.norm(dim=-1), "max")
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
        P = rr._per_mol(batch, (F * v).sum(-1), "sum")
        Fn = torch.sqrt(rr._per_mol(batch, (F * F).sum(-1), "sum"))
        vn = torch.sqrt(rr._per_mol(batch, (v * v).sum(-1), "sum"))
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
        dm = rr._per_mol(batch, d.norm(dim=-1), "max")
        s = torch.where(dm > 0, torch.minimum(torch.ones_like(dm), max_disp / dm), torch.ones_like(dm))
        ra = run[am][..., None]
        if tb is not None:
            ra = ra & ~tb.frozen[:, None, None]          # a frozen atom's coordinates are never written (its v is 0 anyway)
        x = torch.where(ra, x + s[am][..., None] * d, x)
        v = torch.where(ra, s[am][..., None] * vv, v)
        h, al, npos = torch.where(run, h_new, h), torch.where(run, al_new, al), torch.where(run, npos_new, npos)
        steps = steps + run.long()
        it += 1
    return dict(xyz=x, steps=steps, status=status, gmax=gmax_out, snap=snap, margin=margins, P=Ps)


# ------------------------------------------------------------------------------------------------------------------------- cases
def gen_chain4(C, rng):
    """a plain 4-atom chain in relax_refs.gen_molecule's format: three bonds, two angles, one proper, no improper"""
    r0, th0 = 1.53, math.radians(111.0)
    pos = np.zeros((4, 3))
    pos[1] = [r0, 0.0, 0.0]
    pos[2] = pos[1] + r0 * np.array([-math.cos(th0), math.sin(th0), 0.0])
    pos[3] = rr._place(pos[0], pos[1], pos[2], r0, th0, math.radians(70.0))
    bonds = np.array([[0, 1], [1, 2], [2, 3]], dtype=np.int64)
    idx = [bonds, np.array([[0, 1, 2], [1, 2, 3]], dtype=np.int64), np.array([[0, 1, 2, 3]], dtype=np.int64), np.zeros((0, 4), np.int64)]
    f32 = lambda a: np.asarray(a, dtype=np.float32)      # noqa: E731
    ks = [f32(rng.uniform(400, 700, 3)), f32(rng.uniform(80, 140, 2)), f32(rng.uniform(-1, 1, (1, 3)) * np.array([1.0, 0.5, 0.3])), f32(np.zeros((0, 2)))]
    eqs = [f32(np.full(3, r0)), f32(np.full(2, th0)), None, None]
    nb = NonbondedParameters.from_bonds(bonds, np.zeros(4), rng.uniform(3.0, 3.5, 4), rng.uniform(0.05, 0.15, 4))
    xyz = pos[:, None, :] + rng.uniform(-0.15, 0.15, size=(4, C, 3))
    return dict(n=4, idx=idx, ks=ks, eqs=eqs, nb=nb, xyz=xyz.astype(np.float32))


def _restraints_of(mol, C, rng, n_dih, frozen_every=0, tether_every=0):
    """n_dih propers of the molecule (spread over its list) with targets 0.3 to 1.5 rad from each conformation's start"""
    props = mol["idx"][2]
    rows = props[np.linspace(0, len(props) - 1, n_dih).round().astype(int)] if n_dih else np.zeros((0, 4), np.int64)
    assert len({tuple(r) for r in rows.tolist()}) == n_dih
    x = torch.from_numpy(mol["xyz"]).double()
    phi0 = dihedral_t(x, torch.from_numpy(rows).long()).numpy() if n_dih else np.zeros((0, C))
    tg = phi0 + rng.choice([-1.0, 1.0], size=(n_dih, C)) * rng.uniform(0.3, 1.5, size=(n_dih, C))
    tg = np.mod(tg + np.pi, 2 * np.pi) - np.pi
    n = mol["n"]
    frozen = (np.arange(n) % frozen_every == 2) if frozen_every else None
    pk = np.where(np.arange(n) % tether_every == 1, rng.uniform(5, 50, n), 0.0) if tether_every else None
    return Restraints(frozen=frozen, position_k=pk, dihedrals=rows if n_dih else None, dihedral_k=rng.uniform(100, 239, n_dih) if n_dih else None,
                      dihedral_targets=tg if n_dih else None)


# name -> (sizes, C, per molecule (n_dih, frozen_every, tether_every) or None, nonbonded)
CASES = {
    "n4_C3": ((4,), 3, [(1, 0, 0)], False),
    "n9_C3": ((9,), 3, [(1, 0, 0)], True),
    "n33_C3": ((33,), 3, [(3, 0, 5)], True),
    "n65_C1": ((65,), 1, [(4, 7, 5)], True),
    "n257_C1": ((257,), 1, [(2, 0, 0)], True),
    "mixed": ((1, 2, 17, 65, 5), 3, [None, None, (MAX_DIHEDRALS, 0, 0), (0, 7, 5), None], True),
    "max": (("max",), 1, [(2, 11, 0)], True),
}
SALT = {"n65_C1": 2, "mixed": 2, "n33_C3": 1}      # (seeds with which every convergence case converges within max_steps in float64: tests/test_host_relax_restr.py)
TRAJ_CASES = [k for k in CASES if k != "max"]
TRAJ = [(n, s) for n in TRAJ_CASES for s in TRAJ_STEPS] + [("max", 1), ("max", 5)]
CONV_CASES = ["n4_C3", "n9_C3", "n33_C3", "n65_C1", "mixed"]
CONV_OPTS = {}          # the defaults: the CPU tests found nothing else necessary


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (Batch, RestraintBatch, nonbonded?): computed once and shared, treat as read-only"""
    sizes, C, spec, nb = CASES[name]
    sizes = tuple(rr.max_atoms() if n == "max" else n for n in sizes)
    rng = np.random.default_rng(sum(map(ord, name)) * 104729 + C + 1000003 * SALT.get(name, 0))
    mols = [gen_chain4(C, rng) if (name == "n4_C3") else rr.gen_molecule(n, C, rng) for n in sizes]
    items = [None if s is None else _restraints_of(m, C, rng, *s) for m, s in zip(mols, spec)]
    batch = rr.Batch(mols)
    return batch, RestraintBatch(items, C, atom_counts=batch.counts), nb


def subset(name, which):
    batch, rb, nb = case(name)
    sub = batch.subset(which)
    return sub, RestraintBatch([rb.items[k] for k in which], rb.C, atom_counts=sub.counts), nb


@functools.lru_cache(maxsize=None)
def objective_of(name, dtype=torch.float64):
    b, rb, nb = case(name)
    return objective(b, Tables(b, rb), b.xyz, b.xyz, dtype, nb)


@functools.lru_cache(maxsize=None)
def trajectory(name, dtype=torch.float64, steps=max(TRAJ_STEPS)):
    """tolerance 0, `steps` steps, snapshots after TRAJ_STEPS"""
    b, rb, nb = case(name)
    return fire_restr_ref(b, rb, dtype, nb, snapshots=TRAJ_STEPS, tolerance=0.0, max_steps=steps)


def total_steps(name):
    return 5 if name == "max" else max(TRAJ_STEPS)


@functools.lru_cache(maxsize=None)
def converged(name):
    """the float64 restatement with the options of the convergence test"""
    b, rb, nb = case(name)
    return fire_restr_ref(b, rb, torch.float64, nb, **CONV_OPTS)


def margin_ok(name, max_steps):
    """(B, C) bool: |P| / (Fn vn) >= relax_refs.BRANCH_MARGIN in every compared loop iteration 1 .. max_steps - 1 (float64)"""
    m = trajectory(name, torch.float64, total_steps(name))["margin"][1:max_steps]
    b = case(name)[0]
    ok = torch.ones(b.B, b.xyz.shape[1], dtype=torch.bool)
    for t in m:
        ok &= ~(t.abs() < rr.BRANCH_MARGIN)
    return ok


def series(ks, phi):
    """sum_n k_n cos(n phi) and its derivative, float64: the proper of n4_C3"""
    k = np.asarray(ks, dtype=np.float64).reshape(-1)
    n = np.arange(1, len(k) + 1)
    phi = np.asarray(phi, dtype=np.float64)
    return (k * np.cos(n * phi[..., None])).sum(-1), (-n * k * np.sin(n * phi[..., None])).sum(-1)
