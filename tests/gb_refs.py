"""Dense restatement of the GB/SA implicit solvent (grappa_amd/solvent.py, include/grappa_hip.h grappa_gb_desc), the input generator
and the cases of tests/test_host_gb.py (CPU) and tests/test_gpu_gb.py.

gb_ref states the energy directly on (C, n, n) pair matrices per molecule, made from the NonbondedParameters and GBParameters lists
themselves (not from the batch tables, which are code under test), in float64 (the truth) or float32 (what calibrates the gate); values
are rounded to float32 first, as the kernel's tables hold them.  The GRADIENT IS AUTOGRAD OF THE RESTATED ENERGY: the kernel's hand
derivative (three parts: fixed B, the chain through B_i, the chain through B_j) is checked against a derivative nobody wrote by hand.

The gate is the project's calibrated one (kernel_refs.assert_calibrated, C_GATE = 64):
    |gpu - f64| <= 2 |fp32 restatement - f64| + 64 u32 scale
with the scales below, all from the float64 run.  A scale is the first-order size of the result's error when every term it is made of
carries an independent relative rounding error of one u: independent errors add in QUADRATURE (rss = the root of the sum of squares),
and an error that enters many terms alike -- that of an atom's own Born radius -- acts on their SIGNED sum, taken from exact
derivatives (autograd), not from bounds on magnitudes.  (Absolute sums with worst-case sensitivities, as a first version had them,
compound to a floor of the size of the gradient itself on the saturated lattice: a gate nothing can fail.  tests/test_host_gb.py holds
the floors to a small fraction of |g_i|, |E| and B and to at most about a hundred times the fp32 restatement's own error.)
  I_i      sI_i = rss over j and over the five components of H (seven with the extra term): l, u, r (u^2 - l^2)/4, ln(u/l)/(2r),
           s_j^2 (l^2 - u^2)/(4r) [, 2/o_i, 2 l] -- H is a cancelling sum for far pairs, |H| would understate it.
  B_i      sB_i = rss(B, B^2/o, B^2 tanh/R, B^2 (1 - tanh^2)/R rss(alpha psi, beta psi^2, gamma psi^3), dB/dI sI_i): B = 1/(1/o - tanh/R), so
           the roundings of the two terms of its denominator and of the polynomial inside the tanh are amplified by B^2 (by B/o, about
           20, where the tanh saturates), and the error of I_i by dB/dI.
  energies rss over all e_ij, the self terms, all E_sa,i and all dE/dB_i sB_i; per term with that term's own parts.
  gradient of atom i, with e(r^2, P) the pair energy as a function of r^2 and P = B_i B_j, whose first and second derivatives e_P,
           e_r2, e_PP, e_r2P are exact (autograd, elementwise), and n_ij the unit vector along x_i - x_j:
             the part at fixed B, g_ij = 4 e_r2 r n_ij:   rss_j |g_ij|;  rss_j (4 |e_r2P| r B_i sB_j);  |sum_j 4 e_r2P r B_j n_ij| sB_i
             the chain parts, w_i dH_ij/dr n_ij + w_j dH_ji/dr n_ij:   W_i |sum_j dH_ij/dr n_ij|;  rss_j (W_j |dH_ji/dr|);
                 rss_j (|w_i| A_ij), rss_j (|w_j| A_ji), A = rss of the three components of dH/dr: (l^2 - u^2)/4, (l^2 - u^2) s^2/(4 r^2), ln(u/l)/(2 r^2)
           all seven in quadrature.  W_i is the error of w_i = dE/dB_i dB_i/dI_i over u:
             W_i = rss(dB/dI sdE_i,  dE/dB_i d2B/dI2 sI_i,  w_i,  w_i 2 tanh rss(alpha psi, beta psi^2, gamma psi^3))
             sdE_i = rss(rss_j t_ij, self', sa', rss_j (dt_ij/dB_j sB_j), (sum_j dt_ij/dB_i + dself'/dB_i + dsa'/dB_i) sB_i)
           with dE/dB_i = sum_j t_ij + self' + sa', t_ij = 2 e_P B_j, dt_ij/dB_i = 2 e_PP B_j^2, dt_ij/dB_j = 2 (e_PP B_i B_j + e_P),
           self' = K tau q_i^2/(2 B_i^2), sa' = -6 E_sa,i/B_i.  dE/dB_i is a sum over charges of both signs, so the roundings of its terms
           are counted by the terms' magnitudes; d2B/dI2 (autograd of the analytic dB/dI) carries the error of I_i into dB/dI, B^2 included."""
import functools
import math

import numpy as np
import torch

import kernel_refs as kr
import nonbonded_refs as nr
from grappa_amd.constants import COULOMB_CONSTANT
from grappa_amd.nonbonded import NonbondedBatch, NonbondedParameters
from grappa_amd.solvent import MODELS, GBBatch, GBParameters, as_implicit_solvent

C_GATE = 64
ELEMENTS = (1, 6, 7, 8, 16)


def _t32(a, dtype):
    return torch.from_numpy(np.asarray(a, dtype=np.float32).copy()).to(dtype)


def born_of(I, o, R, abc, want_d=False):
    """B(I) elementwise, the formula as stated; with want_d also (tanh, psi, the analytic dB/dI)"""
    al, be, ga = abc
    psi = 0.5 * o * I
    th = torch.tanh(psi * (al + psi * (-be + ga * psi)))
    B = 1 / (1 / o - th / R)
    if not want_d:
        return B
    dP = al + psi * (-2 * be + 3 * ga * psi)
    return B, th, psi, B * B * (1 - th * th) * dP * (0.5 * o) / R


def pair_geometry(o, s, r):
    """o, s (n,), r (C, n, n) -> the branch of every ordered pair (i row, j column) as booleans (swallowed, inside, far, overlap) and
    the distance of r from the nearest of the three borders r = o_i - s_j, r = s_j + o_i, r = s_j - o_i"""
    oi, sj = o[None, :, None], s[None, None, :]
    swallowed = oi >= r + sj
    inside = oi < sj - r
    far = ~swallowed & ~inside & ((r - sj).abs() > oi)
    overlap = ~swallowed & ~inside & ~far
    gap = torch.minimum(torch.minimum((r - (oi - sj)).abs(), (r - (sj + oi)).abs()), (r - (sj - oi)).abs())
    return swallowed, inside, far, overlap, gap


def h_parts(r, oi, sj):
    """-> (H, the root of the sum of its components' squares, dH/dr, the same root for dH/dr's three components), zero where j is swallowed"""
    rs = r + sj
    sw = oi >= rs
    L = torch.maximum(oi.expand_as(r), (r - sj).abs())
    l, u = 1 / L, 1 / rs
    lg = torch.log(u / l)
    comps = [l, -u, r * (u * u - l * l) / 4, lg / (2 * r), sj * sj * (l * l - u * u) / (4 * r)]
    inside = oi < sj - r
    zero = torch.zeros((), dtype=r.dtype)
    extra = [torch.where(inside, 2 / oi, zero), torch.where(inside, -2 * l, zero)]
    H = sum(comps + extra)
    dcomps = [-(l * l - u * u) / 4, -(l * l - u * u) * sj * sj / (4 * r * r), -lg / (2 * r * r)]
    Hrss, drss = sum(c * c for c in comps + extra).sqrt(), sum(c * c for c in dcomps).sqrt()
    return torch.where(sw, zero, H), torch.where(sw, zero, Hrss), torch.where(sw, zero, sum(dcomps)), torch.where(sw, zero, drss)


def gb_ref(nb_params, gb_params, xyz: torch.Tensor, solvent="obc2", dtype=torch.float64, scales=True):
    """-> dict of energy (B,C), terms (2,B,C: polar, SA), grad (N,C,3), born (N,C), I (N,C) and the scales of the docstring above:
    abs_e (B,C), abs_terms (2,B,C), abs_g (N,C), abs_born (N,C), abs_I (N,C); sat (N,C) = B_i over its saturation value.
    scales=False (the dynamics' restatements, which evaluate it every step): the scales of the gradient and of the energies are left
    at zero"""
    sv = as_implicit_solvent(solvent)
    abc = MODELS[sv.model]
    X = xyz.detach().cpu().to(dtype)
    N, C = X.shape[0], X.shape[1]
    ptr = np.concatenate([[0], np.cumsum([p.n_atoms for p in nb_params])])
    assert ptr[-1] == N and [g.n_atoms for g in gb_params] == [p.n_atoms for p in nb_params]
    Bm = len(nb_params)
    f32 = lambda v: torch.tensor(float(np.float32(v)), dtype=dtype)      # noqa: E731
    off, probe = f32(sv.offset), f32(sv.probe)
    kt = f32(COULOMB_CONSTANT * (1.0 / float(np.float32(sv.solute_dielectric)) - 1.0 / float(np.float32(sv.solvent_dielectric))))
    sa4 = f32(4.0 * math.pi * float(np.float32(sv.surface_tension)))
    z = lambda *s: torch.zeros(*s, dtype=dtype)      # noqa: E731
    out = {"energy": z(Bm, C), "terms": z(2, Bm, C), "grad": z(N, C, 3), "born": z(N, C), "I": z(N, C), "abs_e": z(Bm, C), "abs_terms": z(2, Bm, C),
           "abs_g": z(N, C), "abs_born": z(N, C), "abs_I": z(N, C), "sat": z(N, C)}
    zero, one = torch.zeros((), dtype=dtype), torch.ones((), dtype=dtype)
    for b in range(Bm):
        a0, a1 = int(ptr[b]), int(ptr[b + 1])
        n = a1 - a0
        if n == 0:
            continue
        q, R, S = _t32(nb_params[b].charge, dtype), _t32(gb_params[b].radius, dtype), _t32(gb_params[b].scale, dtype)
        o = R - off
        s = S * o
        x = X[a0:a1].permute(1, 0, 2).clone().requires_grad_(True)          # (C, n, 3)
        d = x[:, :, None] - x[:, None, :]
        m = ~torch.eye(n, dtype=torch.bool)[None]
        r2 = torch.where(m, (d * d).sum(-1), one)
        r = torch.sqrt(r2)
        oi, sj = o[None, :, None], s[None, None, :]
        H, Hrss, dHdr, drss = h_parts(r, oi, sj)
        I = torch.where(m, H, zero).sum(-1)                                 # (C, n)
        Bv, th, psi, dBdI = born_of(I, o[None], R[None], abc, want_d=True)
        P = Bv[:, :, None] * Bv[:, None, :]
        D = r2 / (4 * P)
        ex = torch.exp(-D)
        f = torch.sqrt(r2 + P * ex)
        qq = q[None, :, None] * q[None, None, :]
        e_pair = torch.where(m, -0.5 * kt * qq / f, zero)
        e_self = -0.5 * kt * q[None] * q[None] / Bv
        e_sa = sa4 * (R[None] + probe) ** 2 * (R[None] / Bv) ** 6
        Epol, Esa = e_pair.sum((1, 2)) + e_self.sum(1), e_sa.sum(1)
        gpol = torch.autograd.grad(Epol.sum(), [x, Bv], retain_graph=True, allow_unused=True)
        gsa = torch.autograd.grad(Esa.sum(), [x, Bv], allow_unused=True)
        gx = sum(g for g in (gpol[0], gsa[0]) if g is not None) + torch.zeros_like(x)
        dEdB_pol, dEdB_sa = gpol[1], gsa[1]
        if not scales:
            with torch.no_grad():
                out["energy"][b], out["terms"][0, b], out["terms"][1, b] = (Epol + Esa).detach(), Epol.detach(), Esa.detach()
                for k, v in (("grad", gx), ("born", Bv), ("I", I)):
                    out[k][a0:a1] = v.detach().transpose(0, 1)
            continue
        # ---- scales (plain numbers from here on; the derivation is the module's docstring)
        rss = lambda t, dim=-1: (t * t).sum(dim).sqrt()      # noqa: E731
        # the pair energy as a function of r^2 and P = B_i B_j alone, for its exact elementwise first and second derivatives
        Pl, r2l = P.detach().clone().requires_grad_(True), r2.detach().clone().requires_grad_(True)
        el = torch.where(m, -0.5 * kt * qq / torch.sqrt(r2l + Pl * torch.exp(-r2l / (4 * Pl))), zero)
        e_P, e_r2 = torch.autograd.grad(el.sum(), [Pl, r2l], create_graph=True)
        e_PP = torch.autograd.grad(e_P.sum(), Pl, retain_graph=True)[0].detach()
        e_r2P = torch.autograd.grad(e_r2.sum(), Pl)[0].detach()
        e_P, e_r2 = e_P.detach(), e_r2.detach()
        I2 = I.detach().clone().requires_grad_(True)
        d1 = born_of(I2, o[None], R[None], abc, want_d=True)[3]
        d2B = torch.autograd.grad(d1.sum(), I2)[0]
        with torch.no_grad():
            Bi, Bj = Bv[:, :, None], Bv[:, None, :]
            sI = rss(torch.where(m, Hrss, zero))
            al, be, ga = abc
            poly = ((al * psi) ** 2 + (be * psi * psi) ** 2 + (ga * psi ** 3) ** 2).sqrt()
            sB = (Bv ** 2 + Bv ** 4 * ((1 / o[None]) ** 2 + (th / R[None]) ** 2 + ((1 - th * th) / R[None] * poly) ** 2) + (dBdI * sI) ** 2).sqrt()
            sBi, sBj = sB[:, :, None], sB[:, None, :]
            # dE/dB_i = sum_j t_ij + self' + sa' (both orders of a pair: the factor 2)
            t_ij = 2 * e_P * Bj
            self_d, sa_d = 0.5 * kt * q[None] * q[None] / (Bv * Bv), -6 * e_sa / Bv
            dEdB = dEdB_pol + dEdB_sa
            assert torch.allclose(t_ij.sum(-1) + self_d + sa_d, dEdB, rtol=1e-6 if dtype == torch.float64 else 1e-2, atol=1e-9 if dtype == torch.float64 else 1e-2)
            own = (2 * e_PP * Bj * Bj).sum(-1) - 2 * self_d / Bv - 7 * sa_d / Bv          # d(dE/dB_i)/dB_i, signed
            sdE = (rss(t_ij) ** 2 + self_d ** 2 + sa_d ** 2 + rss(2 * (e_PP * Bi * Bj + e_P) * sBj) ** 2 + (own * sB) ** 2).sqrt()
            w = dEdB * dBdI
            W = ((dBdI * sdE) ** 2 + (dEdB * d2B * sI) ** 2 + w ** 2 * (1 + (2 * th * poly) ** 2)).sqrt()
            unit = d.detach() / r.detach()[..., None]
            dHv = torch.where(m, dHdr, zero)
            dA = torch.where(m, drss, zero)
            g_ij = 4 * e_r2 * r.detach()                                                   # the fixed-B gradient of the pair on atom i, along unit
            s_ij = 4 * e_r2P * r.detach()                                                  # ... and its derivative in P
            parts = [rss(g_ij), rss(s_ij * Bi * sBj), ((s_ij * Bj)[..., None] * unit).sum(2).norm(dim=-1) * sB,
                     W * (dHv[..., None] * unit).sum(2).norm(dim=-1), rss(W[:, None, :] * dHv.transpose(1, 2)),
                     rss(w[:, :, None] * dA), rss(w[:, None, :] * dA.transpose(1, 2))]
            sG = sum(p_ * p_ for p_ in parts).sqrt()
            abs_pol = (rss(e_pair.flatten(1)) ** 2 + rss(e_self) ** 2 + rss(dEdB_pol * sB) ** 2).sqrt()
            abs_sa = (rss(e_sa) ** 2 + rss(dEdB_sa * sB) ** 2).sqrt()
            out["energy"][b], out["terms"][0, b], out["terms"][1, b] = (Epol + Esa).detach(), Epol.detach(), Esa.detach()
            out["abs_terms"][0, b], out["abs_terms"][1, b], out["abs_e"][b] = abs_pol, abs_sa, (abs_pol ** 2 + abs_sa ** 2).sqrt()
            for k, v in (("grad", gx), ("born", Bv), ("I", I), ("abs_g", sG), ("abs_born", sB), ("abs_I", sI),
                         ("sat", Bv * (1 / o[None] - 1 / R[None]))):
                out[k][a0:a1] = v.detach().transpose(0, 1)
    return out


def border_report(gb_params, xyz, offset=0.09):
    """in both precisions' view (float32 arithmetic on the float32 inputs, and float64): the number of ordered pairs on each branch
    and the smallest distance of any pair from a branch border -> {"counts": {branch: n}, "gap": float, "worst": (atom, conformation) of
    the batch, "disagree": pairs the two views put on different branches}; such a pair counts as lying on a border (gap 0)"""
    X32 = xyz.detach().cpu().float()
    ptr = np.concatenate([[0], np.cumsum([g.n_atoms for g in gb_params])])
    names = ("swallowed", "inside", "far", "overlap")
    counts, gap, worst, disagree = dict.fromkeys(names, 0), math.inf, None, 0
    for b, g in enumerate(gb_params):
        a0, a1 = int(ptr[b]), int(ptr[b + 1])
        n = a1 - a0
        if n < 2:
            continue
        m = ~torch.eye(n, dtype=torch.bool)[None]
        views = []
        for dt in (torch.float32, torch.float64):
            x = X32[a0:a1].permute(1, 0, 2).to(dt)
            o = _t32(g.radius, dt) - torch.tensor(float(np.float32(offset)), dtype=dt)
            d = x[:, :, None] - x[:, None, :]
            views.append(pair_geometry(o, _t32(g.scale, dt) * o, torch.sqrt((d * d).sum(-1))))
        gp = torch.minimum(views[0][4].double(), views[1][4])
        for k in range(4):
            bad = (views[0][k] != views[1][k]) & m
            disagree += int(bad.sum())
            gp = torch.where(bad, torch.zeros((), dtype=torch.float64), gp)
            counts[names[k]] += int((views[1][k] & m).sum())
        gp = torch.where(m, gp, torch.full((), math.inf, dtype=torch.float64))
        v = float(gp.min())
        if v < gap:
            c, i, _ = np.unravel_index(int(gp.argmin()), gp.shape)
            gap, worst = v, (a0 + int(i), int(c))
    return {"counts": counts, "gap": gap, "worst": worst, "disagree": disagree // 2}


# ------------------------------------------------------------------------------------------------------------------------- inputs
GAP_BRANCHES, GAP_OTHER = 1e-3, 1e-5


def gb_of(n, bonds, rng):
    """GBParameters.from_elements on random elements of {H, C, N, O, S}"""
    return GBParameters.from_elements(rng.choice(ELEMENTS, size=n), np.asarray(sorted(bonds), dtype=np.int64).reshape(-1, 2))


def _bonds(n):
    """the bonds nonbonded_refs.gen_molecule makes"""
    bonds = {(a, a + 1) for a in range(n - 1)} | {(a, a + 4) for a in range(0, n - 4, 7)}
    if n >= 3:
        bonds.add((0, n - 1))
    return bonds


def clear_borders(gb_params, xyz, rng, gap=GAP_OTHER):
    """the atoms of pairs that lie within `gap` of a branch border are moved by up to 0.01 A per coordinate until none does: the branch a
    pair takes must not depend on the precision that judges it"""
    x = xyz.clone()
    for _ in range(200):
        rep = border_report(gb_params, x)
        if rep["gap"] >= gap:
            return x
        i, c = rep["worst"]
        x[i, c] += torch.from_numpy(rng.uniform(-0.01, 0.01, 3).astype(np.float32))
    raise AssertionError("could not move every pair away from the branch borders")


def branches_molecule():
    """four atoms with synthetic radii and scales (o = 3, 1, 3, 1.5 A; s = 0.3, 0.3, 3, 1.2 A), placed so that each of H's four
    branches occurs among the ordered pairs (i, j) -- e.g. (0, 1) swallowed: o_0 = 3 >= r + s_1 = 1.8; (1, 0) far: r = 1.5 > s_0 + o_1 =
    1.3; (1, 2) inside: o_1 = 1 < s_2 - r = 2; (0, 3) overlapping: |r - s_3| = 2.4 <= o_0 = 3 < r + s_3.  tests/test_host_gb.py counts
    them (6 swallowed, 2 inside, 6 far, 10 overlapping) and their distance from the borders.  Two conformations: the second moves every
    atom by a few hundredths of an Angstrom."""
    R = np.array([3.09, 1.09, 3.09, 1.59])
    S = np.array([0.1, 0.3, 1.0, 0.8])
    q = np.array([0.5, -0.4, 0.3, -0.6])
    x0 = np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [1.5, 1.0, 0.0], [3.6, 0.3, 0.2]])
    x1 = x0 + np.array([[0.02, -0.01, 0.03], [-0.03, 0.02, 0.01], [0.01, 0.03, -0.02], [0.02, 0.02, -0.03]])
    xyz = np.stack([x0, x1], axis=1).astype(np.float32)
    nbp = NonbondedParameters(q, np.full(4, 2.0), np.full(4, 0.1)).validate()
    return nbp, GBParameters(R, S).validate(), xyz


def case_table():
    """name -> (molecule sizes as numbers or keys of nonbonded_refs._SIZES, C).  Sizes around T take the short-block, full-block and
    several-block paths; C = 1, 3, 33 the single-conformation path, an odd small count and more than one conformation chunk; `mixed` has
    an empty molecule among the others; n257 is five j-tiles, the last one short"""
    cases = {f"n{n}_C{C}": ((n,), C) for n in ("1", "2", "Tm1", "T", "Tp1", "2Tp1") for C in (1, 3, 33)}
    cases["mixed"] = ((1, 2, 0, 17, "Tp1", 5), 3)
    cases["n257"] = ((257,), 2)
    return cases


CASES = list(case_table()) + ["chain513", "branches"]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (list of NonbondedParameters, list of GBParameters, xyz (N, C, 3) float32 tensor); shared: treat as read-only"""
    if name == "branches":
        nbp, gbp, xyz = branches_molecule()
        return [nbp], [gbp], torch.from_numpy(xyz)
    rng = np.random.default_rng(sum(map(ord, name)) * 7919 + 17)
    if name == "chain513":
        import nb_cut_refs as nc
        params, _, x = nc.inputs("c513_C3")
        n = params[0].n_atoms
        gbs = [gb_of(n, {(a, a + 1) for a in range(n - 1)}, rng)]
        return list(params), gbs, clear_borders(gbs, x, rng)
    sizes, C = case_table()[name]
    T = nr.iblock()
    sizes = tuple(nr._SIZES[n](T) if isinstance(n, str) else n for n in sizes)
    mols = [nr.gen_molecule(n, C, rng) for n in sizes]
    gbs = [gb_of(n, _bonds(n), rng) for n in sizes]
    x = torch.from_numpy(np.concatenate([m[1] for m in mols], axis=0))
    return [m[0] for m in mols], gbs, clear_borders(gbs, x, rng)


@functools.lru_cache(maxsize=None)
def refs(name, solvent="obc2"):
    """-> (float64 reference, float32 restatement) of the case; computed once and shared: treat as read-only"""
    nbp, gbp, x = inputs(name)
    return gb_ref(nbp, gbp, x, solvent, torch.float64), gb_ref(nbp, gbp, x, solvent, torch.float32)


def batches(name, device="cpu"):
    nbp, gbp, _ = inputs(name)
    return NonbondedBatch(nbp).to(device), GBBatch(gbp).to(device)


def rows(t, width):
    return t.reshape(-1, width)


def gate_all(got, r64, r32, what):
    """energy, both terms, every gradient row and every Born radius that `got` holds through the calibrated gate"""
    if got.get("energy") is not None:
        kr.assert_calibrated(rows(got["energy"], 1), rows(r32["energy"], 1), rows(r64["energy"], 1), C_GATE, r64["abs_e"].reshape(-1), f"{what}: energy")
    if got.get("terms") is not None:
        for k, nm in enumerate(("polar", "surface-area")):
            kr.assert_calibrated(rows(got["terms"][k], 1), rows(r32["terms"][k], 1), rows(r64["terms"][k], 1), C_GATE,
                                 r64["abs_terms"][k].reshape(-1), f"{what}: {nm} energy")
    if got.get("grad") is not None:
        kr.assert_calibrated(rows(got["grad"], 3), rows(r32["grad"], 3), rows(r64["grad"], 3), C_GATE, r64["abs_g"].reshape(-1), f"{what}: gradient")
    if got.get("born") is not None:
        kr.assert_calibrated(rows(got["born"], 1), rows(r32["born"], 1), rows(r64["born"], 1), C_GATE, r64["abs_born"].reshape(-1), f"{what}: Born radii")
