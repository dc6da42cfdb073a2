"""Dense restatement of the nonbonded formulas (grappa_amd/nonbonded.py, include/grappa_hip.h grappa_nb_desc), the input generator and
the cases of tests/test_host_nonbonded.py (CPU) and tests/test_gpu_nonbonded.py.

nb_ref states the sums directly on (n, n) pair matrices per molecule, made from the NonbondedParameters lists themselves: a pair mask (no self pairs, no exclusions), exception overrides,
energies and the closed-form gradient, in float64 (the truth) or float32 (what calibrates the gate).  Masked pairs are given r = 1
before anything is divided, so two excluded atoms on one point stay finite.

The gate is the project's calibrated one (kernel_refs.assert_calibrated), per (molecule, conformation) and per (atom, conformation):
|gpu - f64| <= 2 |fp32 restatement - f64| + 64 u32 scale, scale = sum |e_ij| over the molecule's pairs for an energy, sum_j |f_ij| for
an atom's gradient (64: the constant of the MM-energy tests for sums over a molecule's terms)."""
import functools

import numpy as np
import torch

import kernel_refs as kr
from grappa_amd import _lib
from grappa_amd.constants import COULOMB_CONSTANT
from grappa_amd.nonbonded import NonbondedBatch, NonbondedParameters

C_GATE = 64


def nb_ref(params, xyz: torch.Tensor, dtype=torch.float64):
    """params: the list of NonbondedParameters, one per molecule -- the pair tables are made from THEIR lists, not from the CSR table
    the kernel reads (NonbondedBatch is code under test); values are rounded to float32 first, as the kernel's tables hold them.
    xyz (N, C, 3).  -> dict of energy (B,C), terms (2,B,C), grad (N,C,3), abs_e (B,C) = sum |e_ij|, abs_terms (2,B,C),
    abs_f (N,C) = sum_j |f_ij|"""
    x = xyz.detach().cpu().to(dtype)
    N, C = x.shape[0], x.shape[1]
    ptr = np.concatenate([[0], np.cumsum([p.n_atoms for p in params])])
    assert ptr[-1] == N, (ptr[-1], N)
    t32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32).copy()).to(dtype)      # noqa: E731
    K = torch.tensor(COULOMB_CONSTANT, dtype=dtype)
    B = len(params)
    out = {"energy": torch.zeros(B, C, dtype=dtype), "terms": torch.zeros(2, B, C, dtype=dtype), "grad": torch.zeros(N, C, 3, dtype=dtype),
           "abs_e": torch.zeros(B, C, dtype=dtype), "abs_terms": torch.zeros(2, B, C, dtype=dtype), "abs_f": torch.zeros(N, C, dtype=dtype)}
    for b in range(B):
        a0, a1 = int(ptr[b]), int(ptr[b + 1])
        n = a1 - a0
        if n == 0:
            continue
        p = params[b]
        q, sg, ep = t32(p.charge), t32(p.sigma), t32(p.epsilon)
        sij = 0.5 * (sg[:, None] + sg[None, :])
        e4 = 4 * torch.sqrt(ep[:, None] * ep[None, :])
        kqq = K * q[:, None] * q[None, :]
        mask = ~torch.eye(n, dtype=torch.bool)
        xq, xs, xe = t32(p.exception_chargeprod), t32(p.exception_sigma), t32(p.exception_epsilon)
        for own, par in ((p.exception_idx[:, 0], p.exception_idx[:, 1]), (p.exception_idx[:, 1], p.exception_idx[:, 0])):
            sij[own, par], e4[own, par], kqq[own, par] = xs, 4 * xe, K * xq
            mask[own, par] = ~((xe == 0) & (xq == 0))
        m = mask[:, :, None]
        d = x[a0:a1, None] - x[None, a0:a1]                           # (n, n, C, 3)
        r2 = torch.where(m, (d * d).sum(-1), torch.ones((), dtype=dtype))
        inv = 1 / torch.sqrt(r2)
        sr6 = (sij[:, :, None] * inv) ** 6
        l6, l12 = e4[:, :, None] * sr6, e4[:, :, None] * sr6 * sr6
        zero = torch.zeros((), dtype=dtype)
        lj, co = torch.where(m, l12 - l6, zero), torch.where(m, kqq[:, :, None] * inv, zero)
        f = torch.where(m, (6 * l6 - 12 * l12 - co) * inv * inv, zero)      # (dE/dr) / r
        out["terms"][0, b], out["terms"][1, b] = 0.5 * lj.sum((0, 1)), 0.5 * co.sum((0, 1))
        out["energy"][b] = 0.5 * (lj + co).sum((0, 1))
        out["abs_terms"][0, b], out["abs_terms"][1, b] = 0.5 * lj.abs().sum((0, 1)), 0.5 * co.abs().sum((0, 1))
        out["abs_e"][b] = 0.5 * (lj + co).abs().sum((0, 1))
        out["grad"][a0:a1] = (f[..., None] * d).sum(1)
        out["abs_f"][a0:a1] = (f.abs() * torch.sqrt(r2)).sum(1)
    return out


# ------------------------------------------------------------------------------------------------------------------------- inputs
def gen_molecule(n, C, rng, all_exceptions=False):
    """-> (NonbondedParameters, xyz (n, C, 3) float32).  Atoms on a cubic lattice of 1.5 A with a jitter of +-0.2 A per coordinate and
    conformation (closest approach 1.1 A: (3.5/1.1)^12 ~ 1e6 stays far from the fp32 range), sigma in [1, 3.5] A, epsilon in [0, 0.2]
    and q in [-0.8, 0.8], a sixth of each exactly 0; bonds: a chain, a ring closure every seventh atom, and one from the first to the
    last atom."""
    side = max(int(np.ceil(n ** (1 / 3))), 1)
    k = np.arange(n)
    site = np.stack([k % side, (k // side) % side, k // (side * side)], axis=1).astype(np.float64)
    xyz = 1.5 * site[:, None, :] + rng.uniform(-0.2, 0.2, size=(n, C, 3))
    sigma = rng.uniform(1.0, 3.5, n)
    eps = rng.uniform(0.0, 0.2, n) * (rng.random(n) > 1 / 6)
    q = rng.uniform(-0.8, 0.8, n) * (rng.random(n) > 1 / 6)
    if all_exceptions:
        i, j = np.triu_indices(n, 1)
        excl = rng.random(len(i)) < 0.3
        p = NonbondedParameters(q, sigma, eps, np.stack([i, j], 1), np.where(excl, 0, rng.uniform(-0.5, 0.5, len(i))),
                                rng.uniform(1.0, 3.5, len(i)), np.where(excl, 0, rng.uniform(0.0, 0.2, len(i))))
    else:
        bonds = {(a, a + 1) for a in range(n - 1)} | {(a, a + 4) for a in range(0, n - 4, 7)}
        if n >= 3:
            bonds.add((0, n - 1))
        p = NonbondedParameters.from_bonds(sorted(bonds), q, sigma, eps)
    return p.validate(), xyz.astype(np.float32)


def iblock() -> int:
    """the kernel's i-block size, from the library itself"""
    return _lib.nonbonded_iblock()


# molecule sizes are written in terms of T, the kernel's i-block, and resolved when a case is built: collecting the tests needs no library
_SIZES = {"1": lambda T: 1, "2": lambda T: 2, "Tm1": lambda T: T - 1, "T": lambda T: T, "Tp1": lambda T: T + 1, "2Tp1": lambda T: 2 * T + 1,
          "3Tp2": lambda T: 3 * T + 2}


def case_table():
    """name -> (molecule sizes as numbers or keys of _SIZES, C, options).  Sizes around T take the short-block, full-block and
    several-block paths; C = 1, 3, 33 the single-conformation path, an odd small count and more than one conformation chunk."""
    cases = {f"n{n}_C{C}": ((n,), C, {}) for n in ("1", "2", "Tm1", "T", "Tp1", "2Tp1") for C in (1, 3, 33)}
    cases["mixed"] = ((1, 2, 17, "Tp1", 5), 3, {})
    cases["ring_across_blocks"] = (("3Tp2",), 2, {})          # its (0, n-1) bond and the 1-3 / 1-4 pairs around it cross every block border
    cases["all_exceptions"] = ((7, 3), 3, {"all_exceptions": True})
    cases["coincident_excluded"] = ((6, 9), 2, {"coincide": True})
    return cases


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (list of NonbondedParameters, NonbondedBatch on the CPU, xyz (N, C, 3) float32 tensor, float64 reference, float32 restatement);
    computed once and shared: treat as read-only"""
    sizes, C, opt = case_table()[name]
    T = iblock()
    sizes = tuple(_SIZES[n](T) if isinstance(n, str) else n for n in sizes)
    rng = np.random.default_rng(sum(map(ord, name)) * 7919 + C)
    mols = [gen_molecule(n, C, rng, all_exceptions=opt.get("all_exceptions", False)) for n in sizes]
    xyz = np.concatenate([m[1] for m in mols], axis=0)
    if opt.get("coincide"):
        # bonded atoms 0 and 1 of every molecule (an exclusion) on one point, in every conformation
        o = 0
        for n in sizes:
            xyz[o + 1] = xyz[o]
            o += n
    params = [m[0] for m in mols]
    nb = NonbondedBatch(params)
    x = torch.from_numpy(xyz)
    return params, nb, x, nb_ref(params, x, torch.float64), nb_ref(params, x, torch.float32)


def rows(t, width):
    return t.reshape(-1, width)


def gate_all(got_e, got_terms, got_g, r64, r32, what):
    """every (molecule, conformation) energy, both terms and every (atom, conformation) gradient row through the calibrated gate"""
    if got_e is not None:
        kr.assert_calibrated(rows(got_e, 1), rows(r32["energy"], 1), rows(r64["energy"], 1), C_GATE, r64["abs_e"].reshape(-1), f"{what}: energy")
    if got_terms is not None:
        for k, nm in enumerate(("LJ", "Coulomb")):
            kr.assert_calibrated(rows(got_terms[k], 1), rows(r32["terms"][k], 1), rows(r64["terms"][k], 1), C_GATE,
                                 r64["abs_terms"][k].reshape(-1), f"{what}: {nm} energy")
    if got_g is not None:
        kr.assert_calibrated(rows(got_g, 3), rows(r32["grad"], 3), rows(r64["grad"], 3), C_GATE, r64["abs_f"].reshape(-1), f"{what}: gradient")
