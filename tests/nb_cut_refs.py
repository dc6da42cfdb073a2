"""Dense restatement of the nonbonded term under a cutoff (include/grappa_hip.h grappa_nb_cut, grappa_amd/nonbonded.py `Cutoff`), a host
restatement of the tile-skip rule, and the cases of tests/test_host_nb_cut.py (CPU) and tests/test_gpu_nb_cut.py.

nb_cut_ref is nonbonded_refs.nb_ref with the cutoff's formulas: the same (n, n) pair matrices per molecule made from the
NonbondedParameters lists themselves, in float64 (the truth) or float32 (what calibrates the gate).  A pair that is no exception
contributes below rc only, with the switch on Lennard-Jones and the reaction field on Coulomb; an exception is evaluated at any distance
with the plain formulas.  The constants (rc2, k_rf, c_rf, 1 / (rc - rs)) are rounded to float32 first, as the library rounds them.

Cutoff placement.  The float64 truth and the fp32 kernel must agree on which pairs are inside, so a case does not use its nominal
cutoff but `place_cutoff`'s: the midpoint of the largest gap between consecutive sorted non-exception pair distances, over all
conformations, within +-0.05 A of the nominal value (tests/test_host_nb_cut.py asserts a half gap of at least 1e-4 A for every case;
the fp32 error of r is about 1e-6 A).

expected_tiles restates the skip rule of the header on the host, in numpy float32, and returns what `tiles` must hold item for item."""
import functools

import numpy as np
import torch

import nonbonded_refs as nr
import relax_refs as rr
from grappa_amd.constants import COULOMB_CONSTANT
from grappa_amd.nonbonded import Cutoff, NonbondedBatch, NonbondedParameters

NT, CW = 256, 16          # threads per work item, conformations per work item at most (csrc/nb_plan.h)
MARGIN = 2.0 ** -18
WINDOW = 0.05


def constants(cut: Cutoff):
    """the constants as the library forms them: float64 arithmetic on the float32 options, each result rounded once to float32"""
    rc, rs, eps = (float(np.float32(v)) for v in (cut.distance, cut.switch_distance or 0.0, cut.rf_dielectric))
    f32 = lambda v: float(np.float32(v))      # noqa: E731
    rc2 = f32(rc * rc)
    return dict(rc=rc, rc2=rc2, rs=f32(rs) if rs > 0 else f32(rc), inv_w=f32(1.0 / (rc - rs)) if rs > 0 else 0.0,
                krf=f32((eps - 1.0) / ((2.0 * eps + 1.0) * rc ** 3)), crf=f32(3.0 * eps / ((2.0 * eps + 1.0) * rc)),
                thr=f32(rc2 * (1.0 + MARGIN)))


def _pair_tables(p, dtype):
    """(sij, e4, kqq, mask, exc) of one molecule, as nonbonded_refs.nb_ref makes them; exc marks the exception pairs"""
    t32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32).copy()).to(dtype)      # noqa: E731
    K = torch.tensor(COULOMB_CONSTANT, dtype=dtype)
    n = p.n_atoms
    q, sg, ep = t32(p.charge), t32(p.sigma), t32(p.epsilon)
    sij = 0.5 * (sg[:, None] + sg[None, :])
    e4 = 4 * torch.sqrt(ep[:, None] * ep[None, :])
    kqq = K * q[:, None] * q[None, :]
    mask = ~torch.eye(n, dtype=torch.bool)
    exc = torch.zeros(n, n, dtype=torch.bool)
    xq, xs, xe = t32(p.exception_chargeprod), t32(p.exception_sigma), t32(p.exception_epsilon)
    for own, par in ((p.exception_idx[:, 0], p.exception_idx[:, 1]), (p.exception_idx[:, 1], p.exception_idx[:, 0])):
        sij[own, par], e4[own, par], kqq[own, par] = xs, 4 * xe, K * xq
        mask[own, par] = ~((xe == 0) & (xq == 0))
        exc[own, par] = True
    return sij, e4, kqq, mask, exc


def nb_cut_ref(params, xyz: torch.Tensor, cut: Cutoff, dtype=torch.float64):
    """-> the dict of nonbonded_refs.nb_ref (energy, terms, grad, abs_e, abs_terms, abs_f) under `cut`; the scales are the sums of
    the magnitudes of every addend, the reaction-field ones included"""
    k = constants(cut)
    x = xyz.detach().cpu().to(dtype)
    N, C = x.shape[0], x.shape[1]
    ptr = np.concatenate([[0], np.cumsum([p.n_atoms for p in params])])
    assert ptr[-1] == N, (ptr[-1], N)
    B = len(params)
    c = lambda v: torch.tensor(v, dtype=torch.float64).to(dtype)      # noqa: E731
    rc2, rs, inv_w, krf, crf = (c(k[n]) for n in ("rc2", "rs", "inv_w", "krf", "crf"))
    out = {"energy": torch.zeros(B, C, dtype=dtype), "terms": torch.zeros(2, B, C, dtype=dtype), "grad": torch.zeros(N, C, 3, dtype=dtype),
           "abs_e": torch.zeros(B, C, dtype=dtype), "abs_terms": torch.zeros(2, B, C, dtype=dtype), "abs_f": torch.zeros(N, C, dtype=dtype)}
    zero, one = torch.zeros((), dtype=dtype), torch.ones((), dtype=dtype)
    for b in range(B):
        a0, a1 = int(ptr[b]), int(ptr[b + 1])
        if a1 == a0:
            continue
        sij, e4, kqq, mask, exc = _pair_tables(params[b], dtype)
        m, ex = mask[:, :, None], exc[:, :, None]
        d = x[a0:a1, None] - x[None, a0:a1]                           # (n, n, C, 3)
        r2raw = (d * d).sum(-1)
        m = m & (ex | (r2raw < rc2))                                  # an exception is not cut
        r2 = torch.where(m, r2raw, one)
        r = torch.sqrt(r2)
        inv = 1 / r
        sr6 = (sij[:, :, None] * inv) ** 6
        l6, l12 = e4[:, :, None] * sr6, e4[:, :, None] * sr6 * sr6
        lj, dlj = l12 - l6, (6 * l6 - 12 * l12) * inv                 # E_lj unswitched and its derivative in r
        u = torch.clamp((r - rs) * inv_w, min=0)
        S = torch.where(ex, one, 1 + u ** 3 * (-10 + u * (15 - 6 * u)))
        dS = torch.where(ex, zero, -30 * u * u * (1 - u) ** 2 * inv_w)
        kq = kqq[:, :, None]
        co = torch.where(ex, kq * inv, kq * (inv + krf * r2 - crf))
        dco = torch.where(ex, -kq * inv * inv, kq * (-inv * inv + 2 * krf * r))
        aco = torch.where(ex, (kq * inv).abs(), kq.abs() * (inv + krf * r2 + crf))
        adco = torch.where(ex, (kq * inv * inv).abs(), kq.abs() * (inv * inv + 2 * krf * r))
        elj, eco = torch.where(m, S * lj, zero), torch.where(m, co, zero)
        f = torch.where(m, (S * dlj + lj * dS + dco) * inv, zero)     # (dE/dr) / r
        af = torch.where(m, (S * dlj).abs() + (lj * dS).abs() + adco, zero)
        out["terms"][0, b], out["terms"][1, b] = 0.5 * elj.sum((0, 1)), 0.5 * eco.sum((0, 1))
        out["energy"][b] = 0.5 * (elj + eco).sum((0, 1))
        alj, aco = torch.where(m, (S * l12).abs() + (S * l6).abs(), zero), torch.where(m, aco, zero)
        out["abs_terms"][0, b], out["abs_terms"][1, b] = 0.5 * alj.sum((0, 1)), 0.5 * aco.sum((0, 1))
        out["abs_e"][b] = 0.5 * (alj + aco).sum((0, 1))
        out["grad"][a0:a1] = (f[..., None] * d).sum(1)
        out["abs_f"][a0:a1] = af.sum(1)
    return out


# ------------------------------------------------------------------------------------------------------------------------- placement
def pair_distances(params, xyz):
    """the float64 distances of all non-exception pairs of all molecules in all conformations, sorted (from the float32 coordinates)"""
    x = np.asarray(xyz, dtype=np.float64)
    ptr = np.concatenate([[0], np.cumsum([p.n_atoms for p in params])])
    out = []
    for b, p in enumerate(params):
        n = p.n_atoms
        if n < 2:
            continue
        xm = x[ptr[b]:ptr[b + 1]]
        keep = np.triu(np.ones((n, n), dtype=bool), 1)
        keep[np.minimum(p.exception_idx[:, 0], p.exception_idx[:, 1]), np.maximum(p.exception_idx[:, 0], p.exception_idx[:, 1])] = False
        i, j = np.nonzero(keep)
        out.append(np.sqrt(((xm[i] - xm[j]) ** 2).sum(-1)).reshape(-1))
    return np.sort(np.concatenate(out)) if out else np.zeros(0)


def place_cutoff(params, xyz, nominal):
    """-> (rc as a float32 value, half gap): the midpoint of the largest gap between consecutive pair distances inside
    [nominal - 0.05, nominal + 0.05] (the window's ends count as distances), and the distance from rc to the nearest pair"""
    d = pair_distances(params, xyz)
    lo, hi = nominal - WINDOW, nominal + WINDOW
    pts = np.concatenate([[lo], d[(d > lo) & (d < hi)], [hi]])
    k = int(np.argmax(np.diff(pts)))
    rc = float(np.float32(0.5 * (pts[k] + pts[k + 1])))
    return rc, (float(np.abs(d - rc).min()) if d.size else WINDOW)


# ------------------------------------------------------------------------------------------------------------------------- the skip rule
def items(counts, C, T):
    """the work items of grappa_nonbonded_plan in its order: (molecule, first atom within the batch, block, first conformation, ni, nc)"""
    out, blk, a0 = [], 0, 0
    for b, n in enumerate(counts):
        for i0 in range(0, n, T):
            ni = min(T, n - i0)
            cpw = min(NT // ni, CW)
            nch = -(-C // cpw)
            ncb = -(-C // nch)
            out += [(b, a0 + i0, blk, k * ncb, ni, min(ncb, C - k * ncb)) for k in range(nch)]
            blk += 1
        a0 += n
    return out


def expected_tiles(params, xyz, cut: Cutoff, T=None, prune=True):
    """-> (tiles per work item (int array), all tiles per work item, the smallest relative distance |d2 / thr - 1| of any tile's d2 to
    the threshold).  xyz (N, C, 3) float32; every operation of the rule in float32, in the header's order."""
    T = T or nr.iblock()
    x = np.asarray(xyz, dtype=np.float32)
    C = x.shape[1]
    counts = [p.n_atoms for p in params]
    ptr = np.concatenate([[0], np.cumsum(counts)])
    thr = np.float32(constants(cut)["thr"])
    got, full, closest = [], [], np.inf
    boxes = {}
    for b, n in enumerate(counts):
        nt = -(-n // T)
        xm = x[ptr[b]:ptr[b + 1]]
        lo = np.stack([xm[j * T:(j + 1) * T].min(0) for j in range(nt)]) if nt else np.zeros((0, C, 3), np.float32)      # (nt, C, 3)
        hi = np.stack([xm[j * T:(j + 1) * T].max(0) for j in range(nt)]) if nt else np.zeros((0, C, 3), np.float32)
        p = params[b]
        e_lo, e_hi = np.full(nt, np.iinfo(np.int32).max), np.full(nt, -1)
        for own, par in ((p.exception_idx[:, 0], p.exception_idx[:, 1]), (p.exception_idx[:, 1], p.exception_idx[:, 0])):
            for o, q in zip(own // T, par // T):
                e_lo[o], e_hi[o] = min(e_lo[o], q), max(e_hi[o], q)
        boxes[b] = (lo, hi, e_lo, e_hi, nt)
    for b, i0, _, c0, ni, nc in items(counts, C, T):
        lo, hi, e_lo, e_hi, nt = boxes[b]
        I = (i0 - int(ptr[b])) // T
        g = np.maximum(np.float32(0), np.maximum(lo[I][None] - hi, lo - hi[I][None]))[:, c0:c0 + nc]      # (nt, nc, 3) float32
        d2 = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
        near = ~(d2 > thr)
        closest = min(closest, float(np.abs(d2.astype(np.float64) / float(thr) - 1.0).min()))
        J = np.arange(nt)
        ev = near.any(1) | ((J >= e_lo[I]) & (J <= e_hi[I])) | (not prune)
        got.append(int(ev.sum()))
        full.append(nt)
    return np.array(got, dtype=np.int64), np.array(full, dtype=np.int64), closest


# ------------------------------------------------------------------------------------------------------------------------- cases
LATTICE = [k for k in nr.case_table() if k != "all_exceptions"]          # nonbonded_refs' cases: nominal cutoffs 2.5 and 4 A
# BIG: 257 j-tiles, so that a work item takes its verdicts in two batches (csrc/nb_cut.h nb_cut_decide is called again at tile 256).  Its
# tiles and the bits with and without pruning are tested, at BIG_CUTOFF as it stands: it has no dense reference, so it is in no entry of
# NOMINAL / CASES and its cutoff needs no placement.
BIG, BIG_CUTOFF = "c16448_C1", 9.0
CHAINS = {"c129_C3": ((129,), 3), "c513_C3": ((513,), 3), "chain_mixed": ((1, 2, 17, 130, 5, 64), 3), "c513_far_exception": ((513,), 3),
          BIG: ((16448,), 1)}
NOMINAL = {**{k: (2.5, 4.0) for k in LATTICE}, **{k: (6.0, 9.0) for k in CHAINS if k != BIG}}
VARIANTS = [(sw, eps) for sw in (False, True) for eps in (78.3, 1.0)]          # with and without a switch at 0.8 rc; eps = 1: no reaction field
CASES = [(name, nominal) for name in NOMINAL for nominal in NOMINAL[name]]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (list of NonbondedParameters, NonbondedBatch on the CPU, xyz (N, C, 3) float32 tensor); shared: treat as read-only"""
    if name in CHAINS:
        sizes, C = CHAINS[name]
        rng = np.random.default_rng(sum(map(ord, name)) * 7919 + C)
        mols = [rr.gen_molecule(n, C, rng) for n in sizes]
        params = [m["nb"] for m in mols]
        if name == "c513_far_exception":          # one 1-4 like exception between the chain's two ends, about 430 A apart
            p = params[0]
            params = [NonbondedParameters(p.charge, p.sigma, p.epsilon, np.concatenate([p.exception_idx, [[0, 512]]]),
                                          np.concatenate([p.exception_chargeprod, [0.04]]), np.concatenate([p.exception_sigma, [3.2]]),
                                          np.concatenate([p.exception_epsilon, [0.06]])).validate()]
        x = torch.from_numpy(np.concatenate([m["xyz"] for m in mols], axis=0))
        return params, NonbondedBatch(params), x
    params, nb, x, _, _ = nr.case(name)
    return params, nb, x


@functools.lru_cache(maxsize=None)
def placed(name, nominal):
    """-> (rc, half gap) of the case at its nominal cutoff"""
    params, _, x = inputs(name)
    return place_cutoff(params, x.numpy(), nominal)


def cutoff_of(name, nominal, switch, eps, prune=True) -> Cutoff:
    rc, _ = placed(name, nominal)
    return Cutoff(rc, 0.8 * rc if switch else None, eps, prune)


@functools.lru_cache(maxsize=None)
def refs(name, nominal, switch, eps):
    """-> (float64 reference, float32 restatement) of the case; computed once and shared: treat as read-only"""
    params, _, x = inputs(name)
    cut = cutoff_of(name, nominal, switch, eps)
    return nb_cut_ref(params, x, cut, torch.float64), nb_cut_ref(params, x, cut, torch.float32)
