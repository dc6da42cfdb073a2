"""References and gates of the fused writer-head layer (csrc/writer_layer.hip, C ABI 11), no GPU needed: tests/test_gpu_writer_layer_rows.py
asserts with them, tests/test_writer_layer_refs.py checks them on the CPU.

  * truth: the forward as include/grappa_hip.h states it, in float64 with no storage rounding (`layer_fwd`), its gradients by torch.autograd
    (`autograd64`), and the header's backward chain written out (`layer_bwd`), which also yields the by-products and the per-row LayerNorm
    contributions the per-tile partial sums are made of;
  * two fp32 restatements of each that round to bf16 where the kernels store -- a: oracle.ops_ref.RefBackend.writer_layer for the forward and
    `layer_bwd` in fp32 for the backward, b: the same formulas with kernel_refs.matmul_chain32 for the products (another summation order) and
    the LayerNorm sums taken exactly and rounded once;
  * the row gates (`check_fwd`, `check_bwd`): kernel_refs.assert_calibrated row by row, max|gpu - f64| <= 2 max(|a - f64|, |b - f64|) + floor;
  * faulty copies of the restatements (`mutant_*`) that the gates must reject.

Token rows as everywhere: row = pos * T + t.  A tile holds the s tokens of TT = 64 // s consecutive tuples; tile row r = pos * TT + j."""
import functools
import math

import numpy as np
import torch

import kernel_refs as kr

F = 512
NHEADS = 8
BF = torch.bfloat16
D64 = torch.float64
ORDER = ("n1_w", "n1_b", "w_in", "b_in", "w_o", "b_o", "nf_w", "nf_b", "w1", "b1", "w2", "b2")
FWD_BF16 = ("x1", "qkv", "att", "x2", "x3", "u", "out")
FWD_STATS = ("mean1", "rstd1", "meanf", "rstdf")
BWD_BF16 = ("dz2", "dz1", "dzo", "dqkv", "dx")
SEED1, SEED2 = 1234567, 7654321

# floors of the gates, in units of u32 (kernel_refs.assert_calibrated's c):
C_BF16 = 2.0 ** 15        # 2^-9 of the row's largest |f64|: the rounding of the stored bf16 value itself (half a step)
# fp32 tensors: the constants of tests/test_gpu_kernel_domains.py test_layernorm_branches_against_float64 for sums of this length --
# mean: 64 u32 of the row's largest |x|; rstd: 64 u32 rstd max(x - mean)^2 / var; dgamma: 256 u32, dbeta: 64 u32 of the sum of |terms|
C_MEAN, C_RSTD, C_DGAMMA, C_DBETA = 64.0, 64.0, 256.0, 64.0


def bf(t):
    """round to nearest even bf16, the dtype kept"""
    return t.to(BF).to(t.dtype)


def tiles(s, T):
    TT = 64 // s
    return (T + TT - 1) // TT


def tile_rows(s, T, b):
    """the token rows of tile b, in tile order (pos-major)"""
    TT = 64 // s
    t = torch.arange(b * TT, min(T, (b + 1) * TT))
    return (torch.arange(s)[:, None] * T + t[None, :]).reshape(-1)


def tuple_rows(s, T, t):
    return torch.arange(s) * T + t


# ----------------------------------------------------------------------------------------------------------------------------- inputs
T_OF = {s: tuple(sorted({1, 64 // s - 1, 64 // s, 64 // s + 1, 2 * (64 // s), 3 * (64 // s) + 1})) for s in (2, 3, 4)}
CASES = [(s, T) for s in (2, 3, 4) for T in T_OF[s]]


@functools.lru_cache(maxsize=None)
def params(seed=0):
    """the twelve parameters (fp32, CPU); the four weights already rounded to bf16, which is what the kernel is given"""
    gen = torch.Generator().manual_seed(1000 + seed)
    rn = lambda *sh: torch.randn(sh, generator=gen)      # noqa: E731
    k = 1.0 / F ** 0.5
    P = dict(n1_w=1 + 0.1 * rn(F), n1_b=0.1 * rn(F), w_in=rn(3 * F, F) * k, b_in=0.1 * rn(3 * F), w_o=rn(F, F) * k, b_o=0.1 * rn(F),
             nf_w=1 + 0.1 * rn(F), nf_b=0.1 * rn(F), w1=rn(F, F) * k, b1=0.1 * rn(F), w2=rn(F, F) * k, b2=0.1 * rn(F))
    return {n: (bf(v) if n.startswith("w") else v).contiguous() for n, v in P.items()}


@functools.lru_cache(maxsize=None)
def inputs(s, T, degenerate=False):
    """-> x, dout (s*T, F): fp32 tensors of bf16-exact values.  degenerate (T >= 4): tuple 0's first token is a constant row (variance 0 in the
    first LayerNorm), tuple 1's tokens are all equal (uniform softmax), tuple 2's last token is scaled by 2^12"""
    gen = torch.Generator().manual_seed(100 * s + T + (7 if degenerate else 0))
    x = bf(torch.randn(s * T, F, generator=gen) * 1.5 + 0.2)
    dout = bf(torch.randn(s * T, F, generator=gen))
    if degenerate:
        assert T >= 4
        x[0 * T + 0] = 0.75
        x[tuple_rows(s, T, 1)] = x[1].clone()
        x[(s - 1) * T + 2] *= 4096.0
    return x, dout


@functools.lru_cache(maxsize=None)
def gather_case(s, T):
    """GATHER mode with repeats: -> idx (T, s) int64 into a table of N = T - 3 rows, x1_tab (N, F), qkv_tab (N, 3F) (bf16-exact fp32: the
    first LayerNorm and q | k | v of N input rows, as the table-level kernels would leave them)"""
    N = max(T - 3, 2)
    x, _ = inputs(s, T)
    f = fwd32a(x[:N], params(), 1, N, 0.0)
    idx = torch.randint(0, N, (T, s), generator=torch.Generator().manual_seed(s * T))
    return idx, f["x1"].contiguous(), f["qkv"].contiguous()


def keep_masks(s, T, p, seed1=SEED1, seed2=SEED2, salt=0):
    """the two dropout masks (row * 512 + column, kernel_refs.gemm_keep_mask = oracle.ops_ref.dropout_keep on the salted seed), or None"""
    if p <= 0:
        return None, None
    return kr.gemm_keep_mask(seed1, salt, s * T, F, p), kr.gemm_keep_mask(seed2, salt, s * T, F, p)


def salted(seed, salt):
    return (int(seed) + int(salt) * kr.GOLDEN64) & ((1 << 64) - 1)


# ----------------------------------------------------------------------------------------------------------------------------- the layer
def _mm(a, w):
    return a @ w.t()


def _stats(x, exact=False):
    if exact:          # the sums taken in float64 and rounded once: another fp32 implementation
        xd = x.double()
        mu = xd.mean(1)
        return mu.to(x.dtype), (1.0 / torch.sqrt(((xd - mu[:, None]) ** 2).mean(1) + 1e-5)).to(x.dtype)
    mu = x.mean(1)
    return mu, 1.0 / torch.sqrt(((x - mu[:, None]) ** 2).mean(1) + 1e-5)


def _drop(v, keep, p):
    if keep is None:
        return v
    return torch.where(keep, v * (1.0 / (1.0 - float(np.float32(p)))), torch.zeros_like(v))


def attention(qkv, s, T):
    """softmax(q k^T / sqrt(64)) v over the s tokens of each tuple, per head"""
    dh = F // NHEADS
    q, k, v = (t.reshape(s, T, NHEADS, dh) for t in qkv.split(F, dim=1))
    sc = torch.einsum("ithd,jthd->thij", q, k) / math.sqrt(dh)
    return torch.einsum("thij,jthd->ithd", torch.softmax(sc, dim=-1), v).reshape(s * T, F)


def attention_bwd(qkv, datt, s, T):
    dh = F // NHEADS
    q, k, v = (t.reshape(s, T, NHEADS, dh) for t in qkv.split(F, dim=1))
    go = datt.reshape(s, T, NHEADS, dh)
    scale = 1.0 / math.sqrt(dh)
    pr = torch.softmax(torch.einsum("ithd,jthd->thij", q, k) * scale, dim=-1)
    dp = torch.einsum("ithd,jthd->thij", go, v)
    ds = pr * (dp - (pr * dp).sum(-1, keepdim=True)) * scale
    dq = torch.einsum("thij,jthd->ithd", ds, k)
    dk = torch.einsum("thij,ithd->jthd", ds, q)
    dv = torch.einsum("thij,ithd->jthd", pr, go)
    return torch.cat([t.reshape(s * T, F) for t in (dq, dk, dv)], dim=1)


def layer_fwd(x, P, s, T, p=0.0, keep1=None, keep2=None, dtype=D64, rnd=None, mm=_mm, exact_stats=False, gathered=None, hook=None):
    """the forward of include/grappa_hip.h (ABI 11) -> dict(mean1, rstd1, x1, qkv, att, x2, meanf, rstdf, x3, u, out).
    float64, rnd None: the truth.  dtype fp32 with rnd = bf: a restatement that rounds every stored tensor.  gathered = (x1, qkv) token rows:
    GATHER mode, the layer behind them.  hook(name, tensor) -> tensor: a fault injected behind a stage (the mutants)."""
    rnd = rnd or (lambda t: t)
    hook = hook or (lambda name, t: t)
    Q = {n: v.to(dtype) for n, v in P.items()}
    r = {}
    if gathered is None:
        x = x.to(dtype)
        r["mean1"], r["rstd1"] = _stats(x, exact_stats)
        r["x1"] = rnd((x - r["mean1"][:, None]) * r["rstd1"][:, None] * Q["n1_w"] + Q["n1_b"])
        r["qkv"] = rnd(mm(r["x1"], Q["w_in"]) + Q["b_in"])
    else:
        r["x1"], r["qkv"] = gathered[0].to(dtype), gathered[1].to(dtype)
    r["att"] = hook("att", rnd(attention(r["qkv"], s, T)))
    zo = hook("zo", mm(r["att"], Q["w_o"]) + Q["b_o"])
    r["x2"] = rnd(_drop(zo, keep1, p) + r["x1"])
    r["meanf"], r["rstdf"] = _stats(r["x2"], exact_stats)
    r["x3"] = rnd((r["x2"] - r["meanf"][:, None]) * r["rstdf"][:, None] * Q["nf_w"] + Q["nf_b"])
    z1 = mm(r["x3"], Q["w1"]) + Q["b1"]
    r["u"] = rnd(torch.where(z1 > 0, z1, torch.expm1(z1)))
    r["out"] = rnd(_drop(mm(r["u"], Q["w2"]) + Q["b2"], keep2, p) + r["x3"])
    return r


def fwd64(x, P, s, T, p, k1, k2, gathered=None):
    return layer_fwd(x, P, s, T, p, k1, k2, gathered=gathered)


def fwd32a(x, P, s, T, p, seed1=SEED1, seed2=SEED2, salt=0):
    """restatement a of the forward: oracle.ops_ref.RefBackend.writer_layer in fp32, rounding to bf16 where the storage configuration rounds"""
    from oracle.ops_ref import RefBackend
    return RefBackend().writer_layer(x.float(), s, T, NHEADS, float(np.float32(p)), salted(seed1, salt), salted(seed2, salt),
                                     *[P[n] for n in ORDER], rnd=bf)


def fwd32a_gathered(P, s, T, p, k1, k2, gathered):
    """restatement a behind gathered x1, q | k | v (RefBackend.writer_layer has no gather mode): the same formulas in fp32, torch's products"""
    return layer_fwd(None, P, s, T, p, k1, k2, dtype=torch.float32, rnd=bf, gathered=gathered)


def fwd32b(x, P, s, T, p, k1, k2, gathered=None, hook=None):
    """restatement b: the products as sequential fp32 chains over blocks of 8 (kernel_refs.matmul_chain32), the LayerNorm sums exact"""
    return layer_fwd(x, P, s, T, p, k1, k2, dtype=torch.float32, rnd=bf, mm=kr.matmul_chain32, exact_stats=True, gathered=gathered, hook=hook)


def autograd64(x, P, dout, s, T, p=0.0, k1=None, k2=None):
    """-> out, dx, {name: gradient} of <dout, out> through the float64 forward (the same masks with p > 0)"""
    xd = x.double().clone().requires_grad_(True)
    Q = {n: v.double().clone().requires_grad_(True) for n, v in P.items()}
    out = layer_fwd(xd, Q, s, T, p, k1, k2)["out"]
    g = torch.autograd.grad(out, [xd] + [Q[n] for n in ORDER], dout.double())
    return out.detach(), g[0], dict(zip(ORDER, g[1:]))


def _ln_bwd(dy, x, mean, rstd, gamma):
    """-> dx, the rows' contributions to dgamma, to dbeta"""
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    m1, m2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    return rstd[:, None] * (g - m1 - xh * m2), dy * xh, dy


def layer_bwd(dout, sv, P, s, T, p=0.0, keep1=None, keep2=None, dtype=D64, rnd=None, mm=_mm, gather=False):
    """the backward chain of include/grappa_hip.h on the saved tensors sv = dict(x, qkv, x2, u, mean1, rstd1, meanf, rstdf):
        dz2 = mask2(dout); dz1 = (dz2 W_2) ELU'(u); dx3 = dz1 W_1 + dout; dx2 = LN'(dx3; x2, nf); dzo = mask1(dx2); datt = dzo W_o;
        dqkv = attention'(qkv, datt); dx1 = dqkv W_in + dx2; dx = LN'(dx1; x, n1)
    -> dict of all nine, lnf_rows / ln1_rows = (rows' dgamma contributions, rows' dbeta contributions).  rnd: the rounding of every tensor
    the unfused kernels store, which the fused kernel repeats: the five by-products AND dx3, dx2, datt, dx1 (csrc/writer_layer.hip "as the
    unfused product stores it").  gather: the chain ends behind the attention, dx = dx2 (qkv = the gathered token rows)."""
    rnd = rnd or (lambda t: t)
    c = lambda t: t.to(dtype)      # noqa: E731
    Q = {n: c(v) for n, v in P.items()}
    dout, u, x2, qkv = c(dout), c(sv["u"]), c(sv["x2"]), c(sv["qkv"])
    r = {}
    r["dz2"] = rnd(_drop(dout, keep2, p))
    r["dz1"] = rnd(mm(r["dz2"], Q["w2"].t()) * torch.where(u > 0, torch.ones_like(u), u + 1.0))
    r["dx3"] = rnd(mm(r["dz1"], Q["w1"].t()) + dout)
    dx2, dg, db = _ln_bwd(r["dx3"], x2, c(sv["meanf"]), c(sv["rstdf"]), Q["nf_w"])
    r["dx2"], r["lnf_rows"] = rnd(dx2), (dg, db)
    r["dzo"] = rnd(_drop(r["dx2"], keep1, p))
    r["datt"] = rnd(mm(r["dzo"], Q["w_o"].t()))
    r["dqkv"] = rnd(attention_bwd(qkv, r["datt"], s, T))
    if gather:
        r["dx"] = r["dx2"]
        return r
    r["dx1"] = rnd(mm(r["dqkv"], Q["w_in"].t()) + r["dx2"])
    dx, dg, db = _ln_bwd(r["dx1"], c(sv["x"]), c(sv["mean1"]), c(sv["rstd1"]), Q["n1_w"])
    r["dx"], r["ln1_rows"] = rnd(dx), (dg, db)
    return r


def bwd64(dout, sv, P, s, T, p, k1, k2, gather=False):
    return layer_bwd(dout, sv, P, s, T, p, k1, k2, gather=gather)


def bwd32a(dout, sv, P, s, T, p, k1, k2, gather=False):
    return layer_bwd(dout, sv, P, s, T, p, k1, k2, dtype=torch.float32, rnd=bf, gather=gather)


def bwd32b(dout, sv, P, s, T, p, k1, k2, gather=False):
    return layer_bwd(dout, sv, P, s, T, p, k1, k2, dtype=torch.float32, rnd=bf, mm=kr.matmul_chain32, gather=gather)


def partials(rows, s, T, reverse=False):
    """per-tile partial sums [tile][dgamma | dbeta][F] of the rows' contributions, summed in the contributions' dtype (reverse: the rows
    taken in the opposite order, another summation order) -> float64"""
    dg, db = rows
    out = torch.zeros(tiles(s, T), 2, F, dtype=D64)
    for b in range(tiles(s, T)):
        idx = tile_rows(s, T, b)
        if reverse:
            idx = idx.flip(0)
        for j, t in enumerate((dg, db)):
            acc = torch.zeros(F, dtype=t.dtype)
            for i in idx.tolist():
                acc = acc + t[i]
            out[b, j] = acc.double()
    return out


def partial_scale(rows64, s, T):
    """per (tile, dgamma | dbeta): the sum over the tile's rows of |contribution|, largest column"""
    dg, db = rows64
    return torch.stack([torch.stack([t[tile_rows(s, T, b)].abs().sum(0).amax() for t in (dg, db)]) for b in range(tiles(s, T))])


def with_partials(r, s, T, reverse=False):
    """a layer_bwd result with lnf_part / ln1_part in place of the rows' contributions"""
    r = dict(r)
    for n in ("lnf", "ln1"):
        if n + "_rows" in r:
            r[n + "_part"] = partials(r[n + "_rows"], s, T, reverse)
    return r


# ----------------------------------------------------------------------------------------------------------------------------- gates
def ratio_calibrated(got, ra, rb, want, c, scale):
    """the worst row's |got - f64| / (2 max(|a - f64|, |b - f64|) + c u32 scale): what kernel_refs.assert_calibrated compares with 1
    (0 / 0 = 0); rb None: calibrated by a alone"""
    got, ra, want = (t.detach().cpu().double().reshape(max(t.shape[0], 1), -1) for t in (got, ra, want))
    dist = lambda a: (a - want).abs().amax(1)      # noqa: E731
    dr = dist(ra) if rb is None else torch.maximum(dist(ra), dist(rb.detach().cpu().double().reshape(want.shape)))
    bound = 2.0 * dr + c * kr.U32 * torch.as_tensor(scale, dtype=D64).reshape(-1).expand(want.shape[0])
    dg = dist(got)
    return float(torch.where(dg > 0, dg / bound.clamp_min(1e-300), torch.zeros_like(dg)).max())


def gate(ratios, name, got, ra, rb, want, c, scale, what, rows=None):
    got, ra, want = got.detach().cpu(), ra.detach().cpu(), want.detach().cpu()
    rb = None if rb is None else rb.detach().cpu()
    scale = torch.as_tensor(scale, dtype=D64).reshape(-1)
    if rows is not None:
        got, ra, want, scale = got[rows], ra[rows], want[rows], scale[rows]
        rb = None if rb is None else rb[rows]
    ratios[name] = max(ratios.get(name, 0.0), ratio_calibrated(got, ra, rb, want, c, scale))
    kr.assert_calibrated(got, ra, want, c, scale, f"{what} {name}", ref32b=rb)


def stat_scales(x64):
    """the scales of the LayerNorm statistics' floors (tests/test_gpu_kernel_domains.py): the row's largest |x| for the mean,
    rstd max(x - mean)^2 / (var + eps) for rstd -- and rstd itself where that ratio is below 1 (a constant row: var << eps), the relative
    gate the domain test holds constant rows to"""
    mu = x64.mean(1)
    xc = x64 - mu[:, None]
    var = (xc * xc).mean(1)
    return x64.abs().amax(1), ((xc * xc).amax(1) / (var + 1e-5)).clamp_min(1.0) / torch.sqrt(var + 1e-5)


def check_fwd(got, ra, rb, want, x64, what, names=None, rows=None, ratios=None):
    """the row gates of the forward: got / ra / rb / want = dicts of the kernel's tensors, the two restatements and the float64 truth.
    x64: the layer's input (None in GATHER mode, where the first LayerNorm is not part of the launch).  -> {tensor: worst ratio}"""
    ratios = {} if ratios is None else ratios
    for n in names or (FWD_STATS + FWD_BF16):
        if n not in got:
            continue
        b = None if rb is None else rb[n]
        if n in FWD_BF16:
            gate(ratios, n, got[n], ra[n], b, want[n], C_BF16, kr.rowmax(want[n]).reshape(-1), what, rows)
        elif n.endswith("1"):
            sm, sr = stat_scales(x64)
            gate(ratios, n, got[n], ra[n], b, want[n], C_MEAN if n.startswith("mean") else C_RSTD, sm if n.startswith("mean") else sr, what, rows)
        else:
            # the second LayerNorm's statistics are taken of the STORED x2 (csrc/writer_layer.hip phase 2 sums the rounded values), and a "row"
            # of theirs is one number: against the unrounded truth it carries x2's bf16 noise, which a single number of a restatement cannot
            # calibrate (it may sit on the truth by chance).  So, like the backward chain, they are gated on the tensor they were computed from:
            # truth = the float64 statistic of got's own x2, restatements = the fp32 statistics of that x2 (x2 itself is gated above)
            x2 = got["x2"].detach().cpu()
            i = 0 if n.startswith("mean") else 1
            sc = stat_scales(x2.double())[i]
            gate(ratios, n, got[n], _stats(x2.float())[i], None if rb is None else _stats(x2.float(), exact=True)[i], _stats(x2.double())[i],
                  C_MEAN if i == 0 else C_RSTD, sc, what, rows)
    return ratios


def check_bwd(got, ra, rb, want, s, T, what, names=None, rows=None, tile_sel=None, ratios=None):
    """the row gates of the backward; ra / rb / want: with_partials(layer_bwd(...)).  The partial tensors are gated per (tile, dgamma | dbeta)
    row with scale = the sum over the tile's rows of |contribution| (tile_sel: only these tiles)"""
    ratios = {} if ratios is None else ratios
    for n in names or (BWD_BF16 + ("lnf_part", "ln1_part")):
        if n not in got or n not in want:
            continue
        b = None if rb is None else rb[n]
        if n in BWD_BF16:
            gate(ratios, n, got[n], ra[n], b, want[n], C_BF16, kr.rowmax(want[n]).reshape(-1), what, rows)
            continue
        sc = partial_scale(want[n[:3] + "_rows"], s, T)
        for j, (kind, c) in enumerate((("dgamma", C_DGAMMA), ("dbeta", C_DBETA))):
            gate(ratios, f"{n}.{kind}", got[n][:, j], ra[n][:, j], None if b is None else b[:, j], want[n][:, j], c, sc[:, j], what, tile_sel)
    return ratios


def param_grads(bw, sv, part=True):
    """the twelve parameter gradients the caller forms from the backward kernel's by-products and the forward's saves, in float64:
    dW_2 = dz2^T u, dW_1 = dz1^T x3, dW_o = dzo^T att, dW_in = dqkv^T x1, the biases = column sums, the LayerNorms' = the partials summed"""
    d = lambda t: t.detach().cpu().double()      # noqa: E731
    g = {"w2": d(bw["dz2"]).t() @ d(sv["u"]), "b2": d(bw["dz2"]).sum(0), "w1": d(bw["dz1"]).t() @ d(sv["x3"]), "b1": d(bw["dz1"]).sum(0),
         "w_o": d(bw["dzo"]).t() @ d(sv["att"]), "b_o": d(bw["dzo"]).sum(0), "w_in": d(bw["dqkv"]).t() @ d(sv["x1"]), "b_in": d(bw["dqkv"]).sum(0)}
    if part:
        g["nf_w"], g["nf_b"] = d(bw["lnf_part"])[:, 0].sum(0), d(bw["lnf_part"])[:, 1].sum(0)
        g["n1_w"], g["n1_b"] = d(bw["ln1_part"])[:, 0].sum(0), d(bw["ln1_part"])[:, 1].sum(0)
    return g


# ----------------------------------------------------------------------------------------------------------------------------- mutants
# Faulty copies of a restatement, each the image of a fault a tiled kernel can have.  The forward ones are hooks of layer_fwd (the fault sits
# behind one stage, everything downstream is computed from it, as in a kernel); the backward ones damage the outputs.
def mutant_i(bw, s, T):
    """the last tile's LayerNorm partials are dropped"""
    r = {n: v.clone() if torch.is_tensor(v) else v for n, v in bw.items()}
    r["lnf_part"][-1] = 0
    r["ln1_part"][-1] = 0
    return r


def mutant_ii_hook(s, T):
    """two heads' attention outputs swapped in one tuple of the last tile"""
    rows = tuple_rows(s, T, T - 1)

    def hook(name, t):
        if name == "att":
            t = t.clone()
            a, b = t[rows, 64:128].clone(), t[rows, 320:384].clone()
            t[rows, 64:128], t[rows, 320:384] = b, a
        return t
    return hook


def mutant_iii_hook(s, T, P, tile):
    """b_o missing in the rows of one tile"""
    rows = tile_rows(s, T, tile)

    def hook(name, t):
        if name == "zo":
            t = t.clone()
            t[rows] -= P["b_o"].to(t.dtype)
        return t
    return hook


def mutant_iv(bw, s, T, tile):
    """row 63 of a tile added into that tile's dbeta partials.  s = 4: tuple 15's last token, counted twice.  s = 3: row 63 is padding and
    holds nothing of its own; what leaks is taken to be the row in front of it (tile row 62, the tile's last real row).  s = 2: as s = 4."""
    r = {n: v.clone() if torch.is_tensor(v) else v for n, v in bw.items()}
    row = int(tile_rows(s, T, tile)[-1])
    for n in ("lnf", "ln1"):
        r[n + "_part"][tile, 1] += r[n + "_rows"][1][row].double()
    return r


def mutant_v_masks(s, T, p, tile, seed1=SEED1, seed2=SEED2):
    """the dropout masks of one tile taken at the column index only"""
    from oracle.ops_ref import dropout_keep
    k1, k2 = (k.clone() for k in keep_masks(s, T, p, seed1, seed2))
    rows = tile_rows(s, T, tile)
    k1[rows] = dropout_keep(seed1, torch.arange(F), float(np.float32(p)))[None, :]
    k2[rows] = dropout_keep(seed2, torch.arange(F), float(np.float32(p)))[None, :]
    return k1, k2


def mutant_vi(bw, row):
    """dz1 of one row replaced by its neighbour's"""
    r = {n: v.clone() if torch.is_tensor(v) else v for n, v in bw.items()}
    r["dz1"][row] = r["dz1"][row + 1 if row + 1 < r["dz1"].shape[0] else row - 1]
    return r
