"""Float64 references of the kernels and the elementwise gates the domain tests assert with (tests/test_gpu_kernel_domains.py,
tests/test_gpu_mm_float64.py, tests/test_gpu_gemm_routes.py; checked against oracle/ops_ref.RefBackend and cpu_ref.RefMolwiseLoss on the
CPU by tests/test_kernel_domain_refs.py).

The references are independent of the kernels' closed forms: they state each operation directly in float64 and take gradients with
torch.autograd (the GAT from cpu_ref.dot_gat, the MM terms from cpu_ref.bond_length / bond_angle / dihedral)."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24          # unit roundoff of float32
BF = torch.bfloat16


# ----------------------------------------------------------------------------------------------------------------------------- gates
def rowmax(t: torch.Tensor) -> torch.Tensor:
    """the largest magnitude of each row (first axis), shaped to broadcast against t"""
    t = t.detach().double()
    if t.shape[0] == 0:
        return t.abs()
    return t.abs().reshape(t.shape[0], -1).amax(1).reshape(-1, *([1] * (t.dim() - 1)))


def assert_el(got, want64, c, scale, what):
    """fp32 kernels, elementwise: |got - f64| <= c * u32 * (|f64| + scale)  (scale: the row's or head's largest magnitude)"""
    got = got.detach().cpu().double()
    want64 = want64.detach().cpu().double()
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    bound = c * U32 * (want64.abs() + torch.as_tensor(scale, dtype=torch.float64))
    d = (got - want64).abs()
    bad = d > bound
    if bool(bad.any()):
        i = int(torch.argmax((d / bound.clamp_min(1e-300)).reshape(-1)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside c={c} u32 (|f64| + scale); worst at flat index {i}: "
                             f"got {float(got.reshape(-1)[i]):.9g} f64 {float(want64.reshape(-1)[i]):.9g} ({float(d.reshape(-1)[i] / bound.reshape(-1)[i]):.3g}x the bound)")


def assert_calibrated(got, ref32, want64, c, scale, what, period=None, ref32b=None):
    """the self-calibrating gate, row by row: max|gpu - f64| <= 2 * max|fp32 RefBackend - f64| + c * u32 * scale.
    period: compare modulo period (angles: +pi and -pi are the same torsion).  ref32b: a second fp32 implementation (another summation
    order); the farther of the two calibrates the gate."""
    got, ref32, want64 = (t.detach().cpu().double() for t in (got, ref32, want64))
    assert got.shape == want64.shape == ref32.shape, what
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"

    def dist(a):
        d = a - want64
        if period is not None:
            d = torch.remainder(d + period / 2, period) - period / 2
        return d.abs().reshape(max(d.shape[0], 1) if d.numel() else 0, -1).amax(1) if d.numel() else d.reshape(0)

    dg, dr = dist(got), dist(ref32)
    if ref32b is not None:
        dr = torch.maximum(dr, dist(ref32b.detach().cpu().double()))
    floor = c * U32 * torch.as_tensor(scale, dtype=torch.float64).reshape(-1).expand(dg.shape[0]) if dg.numel() else dg
    bad = dg > 2.0 * dr + floor
    if bool(bad.any()):
        i = int(torch.argmax(dg - 2.0 * dr - floor))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} rows fail; row {i}: gpu {float(dg[i]):.3e} vs 2 x fp32 ref "
                             f"{float(dr[i]):.3e} + floor {float(floor[i]):.3e}")


def close_bf16(got16, want64, what, frac=0.97, steps=2.0):
    """bf16 kernels (tests/test_gpu_writer_layer.py's _close_bf16 on a float64 reference of the bf16-rounded inputs): most elements are
    the bf16 rounding of the float64 value, none is more than `steps` bf16 steps (2^-7 relative) away -- of the value or of the tensor's
    RMS where a sum cancels"""
    got = got16.detach().cpu().double()
    want = want64.detach().cpu().double()
    assert got.shape == want.shape, what
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    if got.numel() == 0:
        return
    want16 = want.to(BF).double()
    same = float((got == want16).double().mean())
    d = (got - want).abs()
    bound = steps * 2.0 ** -7 * (want.abs() + want.pow(2).mean().sqrt())
    bad = int((d > bound).sum())
    assert same >= frac and bad == 0, f"{what}: equal {same:.4f}, outside {steps} steps: {bad}, worst {float((d / bound.clamp_min(1e-300)).max()):.2f}"


# ----------------------------------------------------------------------------------------------------------------------------- graph
class CsrPlan:
    """the fields HipBackend's graph entry points read (_csr_check: N, E, indptr, indices, rev), built from a symmetric edge list the
    way batch._plan_arrays_numpy does: CSR by destination, sources ascending, rev = the slot of the reverse edge"""

    def __init__(self, N, src, dst, device="cpu"):
        src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
        order = np.lexsort((src, dst))
        s, d = src[order], dst[order]
        indptr = np.zeros(N + 1, dtype=np.int64)
        np.add.at(indptr, d + 1, 1)
        indptr = np.cumsum(indptr)
        key, rkey = d * max(N, 1) + s, s * max(N, 1) + d
        rev = np.searchsorted(key, rkey)
        assert len(s) == 0 or (np.all(rev < len(s)) and np.all(key[np.minimum(rev, len(s) - 1)] == rkey)), "edge list must be symmetric"
        self.N, self.E = N, len(s)
        self.src, self.dst = torch.from_numpy(s), torch.from_numpy(d)          # (CPU, int64, CSR order: edge e = src[e] -> dst[e])
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)      # noqa: E731
        self.indptr, self.indices, self.rev = i32(indptr), i32(s), i32(rev)
        self.device = torch.device(device)

    def to(self, device):
        p = CsrPlan.__new__(CsrPlan)
        p.__dict__.update(self.__dict__)
        p.indptr, p.indices, p.rev = self.indptr.to(device), self.indices.to(device), self.rev.to(device)
        p.device = torch.device(device)
        return p

    @property
    def degree(self):
        return (self.indptr[1:] - self.indptr[:-1]).long().cpu()


def domain_graph(real_src=None, real_dst=None, n_real=0, hub_leaves=120):
    """a real batch's bonds (optional), then a star whose hub has `hub_leaves` neighbours, a single atom (degree 0), and a 2-atom molecule
    behind it -> (N, src, dst, hub index, isolated atom index)"""
    src = list(real_src) if real_src is not None else []
    dst = list(real_dst) if real_dst is not None else []
    hub = n_real
    for j in range(1, hub_leaves + 1):
        src += [hub, hub + j]
        dst += [hub + j, hub]
    iso = hub + hub_leaves + 1
    a, b = iso + 1, iso + 2
    src += [a, b]
    dst += [b, a]
    return b + 1, np.array(src), np.array(dst), hub, iso


def gat_ref64(ft, plan, H, D, dout):
    """-> out, alpha (E,H) in CSR order, dft: cpu_ref.dot_gat in float64, alpha by a dense masked softmax, dft by autograd"""
    from oracle.cpu_ref import dot_gat
    N = ft.shape[0]
    f = ft.detach().double().clone().requires_grad_(True)
    out = dot_gat(f.view(N, H, D), plan.src, plan.dst).reshape(N, H * D)
    dft, = torch.autograd.grad(out, f, dout.double())
    with torch.no_grad():
        fv = f.view(N, H, D)
        sc = torch.full((N, N, H), float("-inf"), dtype=torch.float64)        # [destination, source, head]
        sc[plan.dst, plan.src] = (fv[plan.src] * fv[plan.dst]).sum(-1) / math.sqrt(D)
        has = plan.degree > 0
        p = torch.zeros_like(sc)
        p[has] = torch.softmax(sc[has], dim=1)
        alpha = p[plan.dst, plan.src]
    return out.detach(), alpha, dft


def neighbor_mean_ref64(x, plan, scale_by_neighbor):
    """out_v = sum over in-neighbours u of x_u / deg(u) (scale_by_neighbor) or / deg(v); 0 for an atom without neighbours"""
    x = x.double()
    deg = plan.degree.double()
    w = 1.0 / (deg[plan.src] if scale_by_neighbor else deg[plan.dst])
    return torch.zeros_like(x).index_add(0, plan.dst, x[plan.src] * w[:, None])


def neighbour_abs_max(x, plan):
    """per destination: the largest |x| over its in-neighbours' rows (0 without neighbours) -- the scale of a convex combination"""
    m = x.detach().double().abs().amax(1)
    return torch.zeros(plan.N, dtype=torch.float64).index_reduce(0, plan.dst, m[plan.src], "amax", include_self=True)[:, None]


# ----------------------------------------------------------------------------------------------------------------------------- row-wise
def layernorm_ref64(x, gamma, beta, dy):
    """-> y, mean, rstd, dx, dgamma, dbeta in float64 (F.layer_norm + autograd), eps = 1e-5 as the kernels"""
    xd = x.detach().double().clone().requires_grad_(True)
    gd = gamma.detach().double().clone().requires_grad_(True)
    bd = beta.detach().double().clone().requires_grad_(True)
    W = x.shape[1]
    y = F.layer_norm(xd, (W,), gd, bd, 1e-5)
    dx, dg, db = torch.autograd.grad(y, (xd, gd, bd), dy.double())
    with torch.no_grad():
        mean = xd.mean(1)
        rstd = 1.0 / torch.sqrt(xd.var(1, unbiased=False) + 1e-5)
    return y.detach(), mean, rstd, dx, dg, db


def act_dropout_ref64(dy, y, p, seed):
    """dz = dy * keep / (1 - p) * ELU'(y), keep = the documented counter hash of the element index row * N + col"""
    from oracle.ops_ref import dropout_keep
    M, N = dy.shape
    v = dy.double()
    keep = None
    if p > 0:
        keep = dropout_keep(seed, torch.arange(M * N).view(M, N), p)
        v = torch.where(keep, v / (1.0 - p), torch.zeros_like(v))
    if y is not None:
        yd = y.double()
        v = v * torch.where(yd > 0, torch.ones_like(yd), yd + 1.0)
    return v, keep


# ----------------------------------------------------------------------------------------------------------------------------- tuples
def seqattn_ref64(qkv, dout, s, T, nheads):
    """softmax attention over each tuple's s tokens (rows pos * T + t), per head, scale 1/sqrt(dh); -> out, dqkv (autograd)"""
    Fd = qkv.shape[1] // 3
    dh = Fd // nheads
    x = qkv.detach().double().clone().requires_grad_(True)
    q, k, v = (t.reshape(s, T, nheads, dh) for t in x.split(Fd, dim=1))
    sc = torch.einsum("ithd,jthd->thij", q, k) / math.sqrt(dh)
    out = torch.einsum("thij,jthd->ithd", torch.softmax(sc, dim=-1), v).reshape(s * T, Fd)
    dqkv = torch.autograd.grad(out, x, dout.double())[0] if dout is not None else None
    return out.detach(), dqkv


def perm_concat_ref64(x, s, T, perms, dz):
    """z[p*T + t] = concat_j x[perms[p][j] * T + t]; dx = the sum of the slots each row went to"""
    xd = x.detach().double().clone().requires_grad_(True)
    xv = xd.view(s, T, -1)
    z = torch.cat([torch.cat([xv[i] for i in p], dim=1) for p in perms], dim=0)
    dx, = torch.autograd.grad(z, xd, dz.double())
    return z.detach(), dx


# ----------------------------------------------------------------------------------------------------------------------------- MM
def mm_ref64(idx, mol_ptr, B, xyz, ks, eqs, n_per, offset_torsion, gE, gG, dtype=torch.float64):
    """the MM energy of a batch in float64 from cpu_ref.bond_length / bond_angle / dihedral:
    E (B,C), term energies (4,B,C), tuple energies and internal coordinates per level, G = dE/dx (N,C,3, create_graph), and
    gk, geq = d/d(k, eq) of <gE, E> + <gG, G> (what csrc/mm_energy.hip's double backward stands for).
    idx: 4 (T,s) int64 tensors; mol_ptr: 4 (B+1,) tensors; ks: [(T,), (T,), (T,n2), (T,n3)]; eqs: [(T,), (T,), None, None].
    dtype=float32: the same formulas in fp32 (a second fp32 implementation for the self-calibrating gate)."""
    from oracle.cpu_ref import bond_angle, bond_length, dihedral
    x = xyz.detach().to(dtype).clone().requires_grad_(True)
    kk = [k.detach().to(dtype).clone().requires_grad_(True) for k in ks]
    ee = [None if q is None else q.detach().to(dtype).clone().requires_grad_(True) for q in eqs]
    C = xyz.shape[1]
    E = torch.zeros(B, C, dtype=dtype)
    terms, tes, txs = [], [], []
    for l in range(4):
        ix = idx[l].long()
        T = ix.shape[0]
        if T == 0:
            te = tx = torch.zeros(0, C, dtype=dtype)
        else:
            pos = [x[ix[:, j]] for j in range(ix.shape[1])]
            if l == 0:
                tx = bond_length(*pos)
            elif l == 1:
                tx = bond_angle(*pos)
            else:
                tx = dihedral(*pos)
            if l < 2:
                te = 0.5 * kk[l][:, None] * (tx - ee[l][:, None]) ** 2
            else:
                k = kk[l].view(T, n_per[l])
                n = torch.arange(1, n_per[l] + 1, dtype=dtype).view(1, -1, 1)
                te = (k[:, :, None] * torch.cos(n * tx[:, None, :])).sum(1)
                if offset_torsion:
                    te = te + k.abs().sum(1, keepdim=True)
        ptr = mol_ptr[l].long()
        seg = torch.repeat_interleave(torch.arange(B), ptr[1:] - ptr[:-1])
        contrib = torch.zeros(B, C, dtype=dtype).index_add(0, seg, te)
        terms.append(contrib)
        tes.append(te)
        txs.append(tx)
        E = E + contrib
    G, = torch.autograd.grad(E.sum(), x, create_graph=True)
    L = (gE.to(dtype) * E).sum() + (gG.to(dtype) * G).sum()
    wrt = [kk[0], kk[1], kk[2], kk[3], ee[0], ee[1]]
    g = torch.autograd.grad(L, wrt, allow_unused=True)
    g = [torch.zeros_like(w) if gi is None else gi for gi, w in zip(g, wrt)]
    det = lambda t: t.detach()          # noqa: E731
    return dict(E=det(E), terms=det(torch.stack(terms)), te=[det(t) for t in tes], tx=[det(t) for t in txs], G=det(G),
                gk=[det(t) for t in g[:4]], geq=[det(g[4]), det(g[5])])


# ----------------------------------------------------------------------------------------------------------------------------- loss
def loss_ef_ref64(atom_counts, energy, energy_ref, is_dummy, grad, grad_ref, wE, wG, inv_B):
    """the molecule-wise energy + force loss, everything in float64: per molecule, the real conformations' energies centred on their
    mean (wE * mean squared difference) and the forces' mean squared difference over atoms x real conformations x 3 (wG); the
    gradients of inv_B * sum(loss) by autograd.  -> loss per molecule (B,), d/d energy (B,C), d/d grad (N,C,3), eval_se (B,4) =
    {sum of squared centred energy differences, real conformations, sum of squared force differences, atoms x real conformations}"""
    cnt = torch.as_tensor(atom_counts, dtype=torch.int64)
    B, C = energy.shape
    e = energy.detach().double().clone().requires_grad_(True)
    g = grad.detach().double().clone().requires_grad_(True)
    m = torch.ones(B, C, dtype=torch.float64) if is_dummy is None else (is_dummy == 0).double()
    nreal = m.sum(1)
    er = energy_ref.double()
    d = (e - (m * e).sum(1, keepdim=True) / nreal[:, None]) - (er - (m * er).sum(1, keepdim=True) / nreal[:, None])
    se_e = (m * d * d).sum(1)
    seg = torch.repeat_interleave(torch.arange(B), cnt)
    sq = (m[seg] * ((g - grad_ref.double()) ** 2).sum(-1)).sum(1)
    se_g = torch.zeros(B, dtype=torch.float64).index_add(0, seg, sq)
    n_g = cnt.double() * nreal
    loss = wE * se_e / nreal + wG * se_g / (n_g * 3.0)
    gE, gG = torch.autograd.grad(inv_B * loss.sum(), (e, g))
    se = torch.stack([se_e, nreal, se_g, n_g], 1).detach()
    return loss.detach(), gE, gG, se


def loss_param_ref64(mol_ptrs, params, refs, fac, reg, pw, inv_B):
    """the parameter MSE + torsion regularisers of one batch, per molecule, in float64 (training/loss.py:80-132 as grappa_amd.loss hands
    it to the kernel: six levels n2_k, n2_eq, n3_k, n3_eq, n4_k, n4_improper_k; fac and reg per level, pw per molecule or None):
        den_b  = sum over the levels with a table and a reference of tuples_b * width          (NaN references still count)
        mse_b  = pw_b * sum_l fac_l^2 sum (p - ref)^2 over the non-NaN references / den_b      (ref zero-padded / cut to p's width;
                 0 where pw_b == 0 or den_b == 0 -- the documented deviation: the reference loop gives NaN for den_b == 0)
        reg_b  = sum_l reg_l * mean over the molecule's elements of p^2                        (0 for a molecule without tuples on l)
    -> (mse + reg per molecule (B,), [d(inv_B * sum_b loss_b)/d params[l] by autograd, None where params[l] is None])"""
    B = int(mol_ptrs[0].numel()) - 1
    ps = [None if p is None else p.detach().cpu().double().clone().requires_grad_(True) for p in params]
    cnts = [mp.detach().cpu().long()[1:] - mp.detach().cpu().long()[:-1] for mp in mol_ptrs]
    tables = []
    for l in range(6):
        if ps[l] is None:
            tables.append(None)
            continue
        T = int(cnts[l].sum())
        tables.append(ps[l].reshape(T, -1) if T else ps[l].reshape(0, ps[l].shape[1] if ps[l].dim() == 2 else 1))
    den = torch.zeros(B, dtype=torch.float64)
    for l in range(6):
        if tables[l] is not None and refs[l] is not None:
            den = den + cnts[l].double() * tables[l].shape[1]
    pwv = torch.zeros(B, dtype=torch.float64) if pw is None else pw.detach().cpu().double()
    num, regsum = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    for l in range(6):
        pv = tables[l]
        if pv is None or pv.shape[0] == 0:
            continue
        T, w = pv.shape
        seg = torch.repeat_interleave(torch.arange(B), cnts[l])
        if refs[l] is not None:
            r = _ref_table64(refs[l], T, w)
            ok = ~torch.isnan(r)
            diff = torch.where(ok, pv - torch.where(ok, r, torch.zeros_like(r)), torch.zeros_like(pv))
            num = num + torch.zeros(B, dtype=torch.float64).index_add(0, seg, float(fac[l]) ** 2 * (diff * diff).sum(1))
        if reg[l] > 0:
            n_el = cnts[l].double() * w
            sq = torch.zeros(B, dtype=torch.float64).index_add(0, seg, (pv * pv).sum(1))
            regsum = regsum + torch.where(n_el > 0, float(reg[l]) * sq / n_el.clamp(min=1), torch.zeros_like(sq))
    loss = regsum + torch.where((pwv != 0) & (den > 0), pwv * num / den.clamp(min=1), torch.zeros_like(num))
    live = [p for p in ps if p is not None]
    if loss.requires_grad:
        g = list(torch.autograd.grad(inv_B * loss.sum(), live, allow_unused=True))
    else:
        g = [None] * len(live)
    g = [torch.zeros_like(p) if gi is None else gi for gi, p in zip(g, live)]
    it = iter(g)
    return loss.detach(), [None if p is None else next(it).reshape(p.shape) for p in ps]


def _ref_table64(ref, T, w):
    """a reference table (T, rw) as float64 (T, w): zero-padded where narrower than the parameters, cut where wider"""
    r = ref.detach().cpu().double().reshape(T, -1)
    if r.shape[1] < w:
        r = torch.cat([r, torch.zeros(T, w - r.shape[1], dtype=torch.float64)], 1)
    return r[:, :w]


def loss_param_grad_scales(mol_ptrs, params, refs, fac, reg, pw, inv_B):
    """per element of params[l], the magnitude its gradient's gate is relative to (float64):
    inv_B * (pw * fac^2 * 2 * (|p| + |ref|) / den  [where the element has an MSE term]  +  reg / n_el * 2 * |p|  [a regulariser term]);
    0 for an element with neither: its gradient must be exactly 0.  -> list of tensors shaped like params[l] (None where that is None)"""
    B = int(mol_ptrs[0].numel()) - 1
    cnts = [mp.detach().cpu().long()[1:] - mp.detach().cpu().long()[:-1] for mp in mol_ptrs]
    widths = [None if p is None else (p.numel() // int(c.sum()) if int(c.sum()) else 1) for p, c in zip(params, cnts)]
    den = torch.zeros(B, dtype=torch.float64)
    for l in range(6):
        if params[l] is not None and refs[l] is not None:
            den = den + cnts[l].double() * widths[l]
    pwv = torch.zeros(B, dtype=torch.float64) if pw is None else pw.detach().cpu().double()
    out = []
    for l in range(6):
        if params[l] is None:
            out.append(None)
            continue
        T, w = int(cnts[l].sum()), widths[l]
        pv = params[l].detach().cpu().double().reshape(T, w).abs()
        seg = torch.repeat_interleave(torch.arange(B), cnts[l])
        s = torch.zeros_like(pv)
        if refs[l] is not None and T:
            r = _ref_table64(refs[l], T, w)
            term = (~torch.isnan(r)) & (pwv != 0)[seg][:, None]
            mse = (pwv * float(fac[l]) ** 2 * 2.0 / den.clamp(min=1))[seg][:, None] * (pv + torch.nan_to_num(r, nan=0.0).abs())
            s = s + torch.where(term, mse, torch.zeros_like(mse))
        if reg[l] > 0 and T:
            s = s + (float(reg[l]) / (cnts[l].double() * w).clamp(min=1))[seg][:, None] * 2.0 * pv
        out.append((inv_B * s).reshape(params[l].shape))
    return out


# ----------------------------------------------------------------------------------------------------------------------------- output maps
OUT_BOND, OUT_ANGLE, OUT_TORSION = 0, 1, 2
BOND_CONSTS = [6.3, 0.1953, 0.0, 4.7, 161.2, 0.0]             # [mos_eq, std_eq, min_eq, mos_k, std_k, min_k]: production-like statistics
ANGLE_CONSTS = [0.0292, math.pi, 0.0, 3.97, 26.6, 0.0]        # [std_over_max, max, -, mos_k, std_k, min_k]
Z_POINTS = [0.0, 2.0 ** -20, -2.0 ** -20, -1.0, -20.0, -104.0, -200.0, 50.0]      # the ELU argument z = mos + c - 1: the kink, expm1f / expf underflow
X_POINTS = [0.0, 1.0, -1.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 1000.0, -1000.0]   # the angle sigmoid's argument s * c0: expf overflow, sg (1 - sg) = 0


def _to_positive64(c, mos, std, mn):
    """models/final_layer.py ToPositive: std * (elu(mean_over_std + x - 1) + 1) + min"""
    return std * (F.elu(mos + c - 1.0) + 1.0) + mn


def param_out_forward64(kind, c, cst, n_per, gated, cutoff):
    """the output maps on the per-tuple sums c (T, nout) and the statistics cst, in the dtype of c -> (k, eq or None):
    bond k, eq = ToPositive; angle k = ToPositive, eq = ToRange: max * sigmoid(std_over_max * x); torsion k = x k_std + k_mean or, gated,
    x sigmoid(gate) k_std, with the hard cutoff k = 0 unless |k| > cutoff"""
    if kind == OUT_TORSION:
        if gated:
            v = c[:, :n_per] * torch.sigmoid(c[:, n_per:2 * n_per]) * cst[:n_per]
        else:
            v = c[:, :n_per] * cst[:n_per] + cst[n_per:2 * n_per]
        if cutoff > 0:
            v = torch.where(v.abs() > float(np.float32(cutoff)), v, torch.zeros_like(v))
        return v, None
    eq = _to_positive64(c[:, 0], cst[0], cst[1], cst[2]) if kind == OUT_BOND else cst[1] * torch.sigmoid(cst[0] * c[:, 0])
    return _to_positive64(c[:, 1], cst[3], cst[4], cst[5]), eq


def param_out_ref64(kind, o, T, P, n_per, gated, cutoff, consts, dk, deq):
    """-> (k, eq, d_o, d_consts) in float64: the forward stated directly, d_o and d_consts = the gradients of <dk, k> + <deq, eq> by
    torch.autograd (dk / deq = None: no upstream gradient on that output).  eq is None for torsions.  T = 0: zeros."""
    nout, ncst = o.shape[1], consts.numel()
    if T == 0:
        k = torch.zeros((0, n_per) if kind == OUT_TORSION else (0,), dtype=torch.float64)
        return k, (None if kind == OUT_TORSION else torch.zeros(0, dtype=torch.float64)), torch.zeros(0, nout, dtype=torch.float64), \
            torch.zeros(ncst, dtype=torch.float64)
    od = o.detach().cpu().double().clone().requires_grad_(True)
    cst = consts.detach().cpu().double().clone().requires_grad_(True)
    k, eq = param_out_forward64(kind, od.view(P, T, nout).sum(0), cst, n_per, gated, cutoff)
    loss = (od * 0.0).sum() + (cst * 0.0).sum()
    if dk is not None:
        loss = loss + (k * dk.detach().cpu().double().reshape(k.shape)).sum()
    if deq is not None and eq is not None:
        loss = loss + (eq * deq.detach().cpu().double()).sum()
    d_o, d_c = torch.autograd.grad(loss, (od, cst))
    return k.detach(), (None if eq is None else eq.detach()), d_o, d_c


def param_out_scales(kind, o, T, P, consts):
    """bond / angle: per tuple, the magnitude the outputs' gates are relative to -> (k scale, eq scale), float64 (T,):
    ToPositive  std * (|mos| + sum_p |o_p| + 1) + |min|;   angle eq  max * (1 + |s| * sum_p |o_p|)"""
    a = o.detach().cpu().double().abs().view(P, T, -1).sum(0)
    c = [abs(float(v)) for v in consts.detach().cpu().double()]
    sk = c[4] * (c[3] + a[:, 1] + 1.0) + c[5]
    seq = c[1] * (c[0] + a[:, 0] + 1.0) + c[2] if kind == OUT_BOND else c[1] * (1.0 + c[0] * a[:, 0])
    return sk, seq


def param_out_grad_scale(kind, o, T, P, consts, dk, deq):
    """the scale of d_o (P*T, nout): column 0 |deq| x the eq scale, column 1 |dk| x the k scale (0 without that upstream gradient),
    further columns 0 (they must come back exactly 0)"""
    sk, seq = param_out_scales(kind, o, T, P, consts)
    s = torch.zeros(T, o.shape[1], dtype=torch.float64)
    if deq is not None:
        s[:, 0] = deq.detach().cpu().double().abs() * seq
    if dk is not None:
        s[:, 1] = dk.detach().cpu().double().abs() * sk
    return s.repeat(P, 1)


def param_out_stat_terms64(kind, o, T, P, n_per, gated, cutoff, consts, dk, deq):
    """(T, ncst) float64: tuple t's term of d_consts[i] (its closed form; the rows' sum is param_out_ref64's d_consts, which
    tests/test_kernel_domain_refs.py checks) -- sum_t |term| is the magnitude the statistics gradients' gate is relative to"""
    ncst = consts.numel()
    terms = torch.zeros(T, ncst, dtype=torch.float64)
    if T == 0:
        return terms
    c = o.detach().cpu().double().view(P, T, -1).sum(0)
    cst = consts.detach().cpu().double()
    d = lambda t, shape: torch.zeros(shape, dtype=torch.float64) if t is None else t.detach().cpu().double().reshape(shape)      # noqa: E731
    if kind == OUT_TORSION:
        up = d(dk, (T, n_per))
        v, _ = param_out_forward64(kind, c, cst, n_per, gated, cutoff)
        if cutoff > 0:
            up = torch.where(v != 0, up, torch.zeros_like(up))
        if gated:
            terms[:, :n_per] = up * c[:, :n_per] * torch.sigmoid(c[:, n_per:2 * n_per])
        else:
            terms[:, :n_per] = up * c[:, :n_per]
            terms[:, n_per:] = up
        return terms

    def pos(x, mos, std, u):          # d/d mos, d/d std, d/d min of u * ToPositive
        z = mos + x - 1.0
        return u * std * torch.where(z > 0, torch.ones_like(z), torch.exp(z)), u * (F.elu(z) + 1.0), u
    ueq, uk = d(deq, (T,)), d(dk, (T,))
    if kind == OUT_BOND:
        terms[:, 0], terms[:, 1], terms[:, 2] = pos(c[:, 0], cst[0], cst[1], ueq)
    else:
        sg = torch.sigmoid(cst[0] * c[:, 0])
        terms[:, 0] = ueq * cst[1] * sg * (1.0 - sg) * c[:, 0]
        terms[:, 1] = ueq * sg
    terms[:, 3], terms[:, 4], terms[:, 5] = pos(c[:, 1], cst[3], cst[4], uk)
    return terms


def param_out_stats_c(T):
    """the constant of the statistics gradients' gate |gpu - f64| <= c u32 sum_t |term_t|: the longest chain of fp32 additions an element
    goes through in param_out_stats_kernel + param_out_stats_final_kernel (csrc/tuples.hip) -- a thread's serial sum over its
    ceil(T / 65536) tuples (256 blocks x 256 threads at the most), the final serial sum over the min(256, ceil(T / 256)) blocks, the
    six butterfly steps of a wave plus the two additions of the four waves (8) -- and 16 for each term's own arithmetic"""
    return -(-T // 65536) + min(256, -(-T // 256)) + 8 + 16


def param_out_case(kind, T, P, nout, consts, seed, n_per=0, gated=False):
    """inputs of one output-map case (fp32, CPU): o (P*T, nout) randn, dk, deq.  Bond / angle: the leading tuples (as many as T holds)
    sit on the named points -- tuple t has z = mos + c - 1 = Z_POINTS[(t + P) % 8] in BOTH ToPositive columns (bond) and the angle
    sigmoid's argument s * c0 = X_POINTS[(t + P) % 11]; the sum over the P rows is exact (row 0 carries c - (P - 1) / 2, the others 1/2).
    Torsion: randn, with the gate columns of the leading tuples at +-20, +-88, +-100 (sigmoid saturated both ways)."""
    gen = torch.Generator().manual_seed(seed)
    o = torch.randn(P * T, nout, generator=gen)
    cst = [float(np.float32(v)) for v in consts]

    def put(t, col, c):
        o[t, col] = c - 0.5 * (P - 1)
        for p in range(1, P):
            o[p * T + t, col] = 0.5
    if kind == OUT_TORSION:
        if gated:
            for t in range(min(T, 12)):
                g = [20.0, -20.0, 88.0, -88.0, 100.0, -100.0][t % 6]
                for n in range(n_per):
                    put(t, n_per + n, g)
        dk, deq = torch.randn(T, n_per, generator=gen), None
    else:
        for t in range(min(T, 3 * len(X_POINTS))):
            put(t, 1, 1.0 - cst[3] + Z_POINTS[(t + P) % len(Z_POINTS)])
            if kind == OUT_BOND:
                put(t, 0, 1.0 - cst[0] + Z_POINTS[(t + P + t // len(Z_POINTS)) % len(Z_POINTS)])
            else:
                put(t, 0, X_POINTS[(t + P) % len(X_POINTS)] / cst[0])
        dk, deq = torch.randn(T, generator=gen), torch.randn(T, generator=gen)
    return o, dk, deq


# ----------------------------------------------------------------------------------------------------------------------------- column sums, charges
def colsum_chain(M):
    """grappa_colsum_f32 (csrc/rowwise.hip) -> (rows per block, additions of the partials' reduction, blocks used).
    colsum_partial_kernel: min(512, ceil(M / 64)) blocks, each a serial sum over rows_per_block = ceil(M / blocks) rows.  reduce_rows:
    up to 64 partials in one stage, more in two (32 groups of rpg = ceil(blocks / 32), then the groups); a stage over n values keeps four
    interleaved accumulators of n // 4 additions, adds the n % 4 left-over values to the first and combines the four pairwise (2):
    n // 4 + n % 4 + 2 additions on the longest path.  (The last stage's `out + s` and slack are the gate's + 8.)"""
    blocks = min(512, max(1, -(-M // 64)))
    rpb = -(-M // blocks)
    used = -(-M // rpb)
    stage = lambda n: n // 4 + n % 4 + 2          # noqa: E731
    if used <= 64:
        return rpb, stage(used), used
    rpg = -(-used // 32)
    return rpb, stage(rpg) + stage(-(-used // rpg)), used


def charge_encoding_ref64(q, dim, lo, hi):
    """the reference encoder (models/graph_attention.py via oracle/cpu_ref.charge_encoding) in float64, its scaling quirk included:
    v = clamp(q, lo, hi); s = (v + hi) / (hi - lo)  [not (v - lo)]; out[:, 2j] = sin(s f_j), out[:, 2j+1] = cos(s f_j), f_j = 10000^(-j / (dim/2))"""
    v = torch.clamp(q.detach().cpu().double(), lo, hi)
    s = (v + hi) / (hi - lo)
    half = dim // 2
    f = torch.exp(torch.arange(half, dtype=torch.float64) * (-math.log(10000.0) / half))
    out = torch.zeros(q.numel(), dim, dtype=torch.float64)
    out[:, 0::2] = torch.sin(s[:, None] * f)
    out[:, 1::2] = torch.cos(s[:, None] * f)
    return out


def assert_sum(got, want64, c, abs_sum, what):
    """a sum of terms, per element: |got - f64| <= c * u32 * sum |term|  (abs_sum, float64) -> the largest error / bound"""
    got, want64 = got.detach().cpu().double(), want64.detach().cpu().double()
    abs_sum = torch.as_tensor(abs_sum, dtype=torch.float64).expand(want64.shape)
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    d, bound = (got - want64).abs(), c * U32 * abs_sum
    bad = d > bound
    if bool(bad.any()):
        i = int(torch.argmax((d / bound.clamp_min(1e-300)).reshape(-1)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} sums outside c={c} u32 sum|term|; worst at flat index {i}: got "
                             f"{float(got.reshape(-1)[i]):.9g} f64 {float(want64.reshape(-1)[i]):.9g} ({float(d.reshape(-1)[i] / bound.reshape(-1)[i]):.3g}x the bound)")
    ok = bound > 0
    return float((d[ok] / bound[ok]).max()) if bool(ok.any()) else 0.0


def el_ratio(got, want64, c, scale):
    """the largest |got - f64| / (c u32 (|f64| + scale)) of assert_el (the figure the test files' docstrings record)"""
    got, want64 = got.detach().cpu().double(), want64.detach().cpu().double()
    bound = c * U32 * (want64.abs() + torch.as_tensor(scale, dtype=torch.float64))
    ok = bound > 0
    return float(((got - want64).abs() / bound.clamp_min(1e-300))[ok].max()) if bool(ok.any()) else 0.0


# ----------------------------------------------------------------------------------------------------------------------------- dense products
GOLDEN64 = 0x9E3779B97F4A7C15      # include/grappa_hip.h, drop_salt: seed + word * 0x9E3779B97F4A7C15 (mod 2^64)
FP32_GRADE = ("f32", "f32_bf16x9", "f32_bf16x6", "f32_f16x3")


def bf16_round(t):
    """round to nearest even bf16, back in float64: what a bf16 tensor (`*_nplanes = 1`, C1p, Cp) holds"""
    return t.float().to(BF).double()


@functools.lru_cache(maxsize=2)
def gemm_keep_mask(drop_seed, drop_salt, M, N, drop_p):
    """the documented keep mask of an [M, N] output: oracle.ops_ref.dropout_keep(seed + salt * 0x9E3779B97F4A7C15, m * N + n, p), p as the fp32
    value the descriptor carries"""
    from oracle.ops_ref import dropout_keep
    seed = (int(drop_seed) + int(drop_salt) * GOLDEN64) & ((1 << 64) - 1)
    return dropout_keep(seed, torch.arange(M * N).view(M, N), float(np.float32(drop_p)))


def gemm_operands64(A, B, layout):
    """the operands as the header's A(m, k) and B(n, k), float64: "fwd" A[M,K] B[N,K]; "dgrad" A[M,K] B[K,N]; "wgrad" A[K,M] B[K,N]"""
    A, B = A.detach().cpu().double(), B.detach().cpu().double()
    if layout == "fwd":
        return A, B
    if layout == "dgrad":
        return A, B.t()
    assert layout == "wgrad", layout
    return A.t(), B.t()


def gemm_ref64(A, B, layout, *, pre=None, bias=None, act=0, aux=None, drop_p=0.0, drop_seed=0, drop_salt=0, res=None, res_ln=None,
               old=None, two_outputs=False, a_colsum_old=None):
    """The dense product as include/grappa_hip.h documents it (the comment above GRAPPA_ACT_NONE; res_ln_*: ABI 7; a_colsum), in float64 on
    what the kernel is given (a bf16 tensor is passed in already rounded: bf16_round).  -> (C, OUT, colsum):
        v = sum_k A(m,k) B(n,k);  v += pre;  v += bias[n];  v = elu(v) (act == 1);  v *= (aux > 0 ? 1 : aux + 1);
        C = v (two_outputs: the copy before dropout, else None);
        v = keep(seed + salt * 0x9E3779B97F4A7C15, m * N + n) ? v / (1 - p) : 0;
        v += res, or with res_ln = (mean, rstd, gamma, beta): v += (res - mean[m]) * rstd[m] * gamma[n] + beta[n];
        v += old (accumulate);  OUT = v;   colsum[m] = a_colsum_old[m] + sum_k A(m, k).
    C1p / Cp are bf16_round(C) / bf16_round(OUT).  The keep mask is oracle.ops_ref.dropout_keep (tests/test_capi_symbols.py ties it to the
    library's host function)."""
    a, b = gemm_operands64(A, B, layout)
    d = lambda t: None if t is None else t.detach().cpu().double()          # noqa: E731
    v = a @ b.t()
    M, N = v.shape
    if pre is not None:
        v = v + d(pre)
    if bias is not None:
        v = v + d(bias)[None, :]
    if act == 1:
        v = torch.where(v > 0, v, torch.expm1(v))
    if aux is not None:
        x = d(aux)
        v = v * torch.where(x > 0, torch.ones_like(x), x + 1.0)
    C = v.clone() if two_outputs else None
    if drop_p > 0:
        keep = gemm_keep_mask(int(drop_seed), int(drop_salt), M, N, float(drop_p))
        v = torch.where(keep, v / (1.0 - float(np.float32(drop_p))), torch.zeros_like(v))
    if res is not None:
        r = d(res)
        if res_ln is not None:
            mean, rstd, gamma, beta = (d(t) for t in res_ln)
            r = (r - mean[:, None]) * rstd[:, None] * gamma[None, :] + beta[None, :]
        v = v + r
    if old is not None:
        v = v + d(old)
    colsum = None if a_colsum_old is None else d(a_colsum_old) + a.sum(1)
    return C, v, colsum


def gemm_terms(A, B, layout, *, pre=None, bias=None, drop_p=0.0, drop_seed=0, drop_salt=0, res=None, res_ln=None, old=None, amax_bcast=0):
    """what assert_gemm's bound is made of, all float64 (M, N): S = sum_k |a_mk| |b_nk| + |pre| + |bias|; gain = 1 / (1 - p) where the
    dropout keeps the element (1 elsewhere and without dropout); |res| (the LayerNorm rows with res_ln), |old|; h = the absolute term
    of F32_F16X3, amax_A[m] ||b_n||_1 + amax_B[n] ||a_m||_1 (amax_bcast bit 0 / 1: the whole operand's maximum instead of the row's)"""
    a, b = gemm_operands64(A, B, layout)
    a, b = a.abs(), b.abs()
    S = a @ b.t()
    M, N = S.shape
    d = lambda t: t.detach().cpu().double()          # noqa: E731
    if pre is not None:
        S = S + d(pre).abs()
    if bias is not None:
        S = S + d(bias).abs()[None, :]
    gain = torch.ones_like(S)
    if drop_p > 0:
        keep = gemm_keep_mask(int(drop_seed), int(drop_salt), M, N, float(drop_p))
        gain = torch.where(keep, gain / (1.0 - float(np.float32(drop_p))), gain)
    zero = torch.zeros_like(S)
    r = zero
    if res is not None:
        r = d(res)
        if res_ln is not None:
            mean, rstd, gamma, beta = (d(t) for t in res_ln)
            r = ((r - mean[:, None]) * rstd[:, None] * gamma[None, :]).abs() + beta.abs()[None, :]
        r = r.abs()
    am_a = a.amax(1) if not (amax_bcast & 1) else a.amax().expand(M)
    am_b = b.amax(1) if not (amax_bcast & 2) else b.amax().expand(N)
    h = am_a[:, None] * b.sum(1)[None, :] + am_b[None, :] * a.sum(1)[:, None]
    return dict(S=S, gain=gain, res=r, old=zero if old is None else d(old).abs(), h=h)


def gemm_rep(arithmetic, terms):
    """the representation error include/grappa_hip.h states for each GRAPPA_GEMM_* arithmetic, as an absolute bound per element:
      f32, f32_bf16x9  0: "every partial product is exact, the result differs from an fp32 FMA chain only by accumulation order";
      f32_bf16x6       3 u32 S: "drops terms <= 2^-24 |a||b|": the three dropped piece products, each at most 2^-24 |a||b|;
      f32_f16x3        3 u32 S + 2^-39 h: "a - hi - lo <= 2^-24 |a|" for each operand and "the dropped lo*lo is <= 2^-24 |a||b|" (three
                       terms of u32 S), and "elements more than 2^16 below their row's maximum lose relative (never absolute: <= 2^-39 of
                       the maximum) precision": |da| <= 2^-39 amax_A[m] against |b|, |db| <= 2^-39 amax_B[n] against |a| (h of gemm_terms);
      bf16x3           4 * 2^-16 S: "2 pieces / 3 products (~2^-16 relative)" -- the header's figure once for each operand's two-piece
                       representation, once for the dropped lo*lo product, rounded up to a power of two;
      bf16             (2 + 2^-8) 2^-8 S: "operands rounded to bf16", unit roundoff 2^-8 each: (1 + 2^-8)^2 - 1; 0 ("bf16_given") where both
                       operands are handed over as bf16 tensors and the reference is taken on those: the kernel rounds nothing."""
    S = terms["S"]
    if arithmetic in ("f32", "f32_bf16x9", "bf16_given"):       # bf16_given: BF16 on operands handed over as bf16 (both in one plane) -- exact products
        return torch.zeros_like(S)
    if arithmetic == "f32_bf16x6":
        return 3.0 * U32 * S
    if arithmetic == "f32_f16x3":
        return 3.0 * U32 * S + 2.0 ** -39 * terms["h"]
    if arithmetic == "bf16x3":
        return 4.0 * 2.0 ** -16 * S
    assert arithmetic == "bf16", arithmetic
    return (2.0 + 2.0 ** -8) * 2.0 ** -8 * S


def gemm_bound(want64, terms, arithmetic, c_acc, bf16_out=False):
    """gain * (c_acc * u32 * S + rep) + 4 * u32 * (|f64| + |res| + |old|)  [+ 2^-8 |f64| for a bf16 output]: the accumulation of K products
    in fp32 in some order (c_acc, calibrated on two fp32 CPU references: tests/gemm_routes.py), the arithmetic's representation error, and
    four roundings of the epilogue's additions (bias / activation, dropout scale, residual, accumulate).  ELU and ELU' do not amplify
    (slopes <= 1)."""
    w = want64.abs()
    bound = terms["gain"] * (c_acc * U32 * terms["S"] + gemm_rep(arithmetic, terms)) + 4.0 * U32 * (w + terms["res"] + terms["old"])
    if bf16_out:
        bound = bound + 2.0 ** -8 * w
    return bound


def gemm_ratio(got, want64, terms):
    """max |got - f64| / (u32 * gain * S): the figure c_acc is compared with (the report of the GPU sweep)"""
    d = (got.detach().cpu().double() - want64).abs() / (U32 * terms["gain"] * terms["S"]).clamp_min(1e-300)
    return float(d.max()) if d.numel() else 0.0


def gemm_c_acc_used(got, want64, terms, arithmetic, bf16_out=False):
    """the smallest c_acc under which `got` passes assert_gemm: max over the elements of the error left after the arithmetic's
    representation term and the epilogue's roundings, in units of u32 gain S (0 where those alone cover the error)"""
    d = (got.detach().cpu().double() - want64).abs() - gemm_bound(want64, terms, arithmetic, 0.0, bf16_out)
    d = d / (U32 * terms["gain"] * terms["S"]).clamp_min(1e-300)
    return max(float(d.max()), 0.0) if d.numel() else 0.0


def assert_gemm(got, want64, terms, arithmetic, what, c_acc, bf16_out=False):
    """the elementwise gate of the dense products (gemm_bound)"""
    got = got.detach().cpu().double()
    want64 = want64.detach().cpu().double()
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    if not bool(torch.isfinite(got).all()):
        i = int(torch.argmax((~torch.isfinite(got)).reshape(-1).int()))
        raise AssertionError(f"{what}: {int((~torch.isfinite(got)).sum())} non-finite values (unwritten?), first at (m, n) = {divmod(i, got.shape[1])}")
    bound = gemm_bound(want64, terms, arithmetic, c_acc, bf16_out)
    d = (got - want64).abs()
    bad = d > bound
    if bool(bad.any()):
        i = int(torch.argmax((d / bound.clamp_min(1e-300)).reshape(-1)))
        m, n = divmod(i, got.shape[1])
        rows, cols = torch.nonzero(bad.any(1)).reshape(-1), torch.nonzero(bad.any(0)).reshape(-1)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the {arithmetic} gate (c_acc {c_acc}); worst at (m, n) = ({m}, {n}): "
                             f"got {float(got[m, n]):.9g} f64 {float(want64[m, n]):.9g} ({float(d[m, n] / bound[m, n]):.3g}x the bound); "
                             f"rows {int(rows[0])}..{int(rows[-1])}, columns {int(cols[0])}..{int(cols[-1])}")


def matmul_chain32(a, b, block=8):
    """a second fp32 summation order of a(M,K) b(N,K)^T: a sequential fp32 chain over blocks of `block` columns of K, each block summed
    exactly (float64, rounded once)"""
    a64, b64 = a.double(), b.double()
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float32)
    for k0 in range(0, a.shape[1], block):
        acc = acc + (a64[:, k0:k0 + block] @ b64[:, k0:k0 + block].t()).float()
    return acc
