"""GPU (-m gpu): the fused writer-head layer (C ABI 11, csrc/writer_layer.hip) per row, per tile and per tuple.

tests/test_gpu_writer_layer.py holds the layer to tensor-wide bounds (a few bf16 steps of value + RMS, 2e-2 of the largest gradient).  Here every
launch goes through the C ABI directly with buffers the test owns, every output lies between sentinels, and every tensor the kernels write is
gated row by row against float64 (tests/writer_layer_refs.py: max|gpu - f64| <= 2 max(|r32a - f64|, |r32b - f64|) + floor, admissible because
tests/test_writer_layer_refs.py shows either restatement passing it calibrated by the other alone).  On top of that the exact properties of a
per-tuple function: a tuple's rows do not depend on where the tuple sits, a localised cotangent leaves every other row and tile exactly zero,
and the dropout masks sit where the documented hash puts them.

The cases are one to four tiles of each tuple length: T in {1, TT - 1, TT, TT + 1, 2 TT, 3 TT + 1}, TT = 64 // s (writer_layer_refs.CASES).
`be._packed_weight` is a private helper of the backend (the weights in MFMA fragment order); the tests use it to hand the kernel its weights."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

import kernel_refs as kr
import writer_layer_refs as wl

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F = wl.F
FILL = 1024.0          # exact in bf16 and fp32
ERR_ARG = -1
STATS = ("mean1", "rstd1", "meanf", "rstdf")
SAVES = ("x1", "qkv", "att", "x2", "x3", "u")
BWD_OUT = ("dx", "dz2", "dz1", "dzo", "dqkv")
RATIOS = {}            # tensor -> worst gpu distance / bound over the module's cases


@pytest.fixture(scope="module", autouse=True)
def _report():
    """the worst ratio per tensor (profiles/writer_layer_gates.txt is this table): printed, and written where GRAPPA_WRITER_GATES_REPORT says"""
    yield
    lines = [f"{n:18s} {r:.3f}" for n, r in sorted(RATIOS.items())]
    print("\nwriter layer row gates, worst gpu distance / bound:\n" + "\n".join(lines))
    path = os.environ.get("GRAPPA_WRITER_GATES_REPORT")
    if path:
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


@pytest.fixture(scope="module")
def be():
    from grappa_amd.backend import get_backend
    return get_backend()


class Guarded:
    """a tensor between two sentinel blocks of its own dtype, each at least a whole tile of its rows long"""

    def __init__(self, shape, dtype=BF):
        self.n = int(np.prod(shape))
        self.g = max(4096, 64 * int(shape[-1]))
        self.flat = torch.full((self.n + 2 * self.g,), FILL, dtype=dtype, device="cuda")
        self.t = self.flat[self.g:self.g + self.n].view(shape)

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what, written=True):
        assert bool((self.flat[:self.g] == FILL).all()), f"{what}: written in front of the tensor"
        assert bool((self.flat[self.g + self.n:] == FILL).all()), f"{what}: written behind the tensor"
        if written:          # (whole rows: a single element may be 1024 by right -- dx of a constant input row is rstd = 316 times O(1); the row gates see the rest)
            left = int((self.t.reshape(self.t.shape[0], -1) == FILL).all(1).sum())
            assert left == 0, f"{what}: {left} rows still hold the fill"

    def untouched(self):
        return bool((self.flat == FILL).all())


@functools.lru_cache(maxsize=None)
def _dev_params():
    return {n: v.cuda().contiguous() for n, v in wl.params().items()}


def _salt(be):
    return int(be._salt.item()) if getattr(be, "_salt_ptr", None) else 0


@functools.lru_cache(maxsize=8)
def _ref(s, T, p, salt=0, degenerate=False):
    """inputs, masks, the float64 forward and its two restatements (CPU, shared by the tests of a case, never modified)"""
    x, dout = wl.inputs(s, T, degenerate)
    P = wl.params()
    k1, k2 = wl.keep_masks(s, T, p, salt=salt)
    return dict(x=x, dout=dout, P=P, k1=k1, k2=k2, f64=wl.fwd64(x, P, s, T, p, k1, k2), fa=wl.fwd32a(x, P, s, T, p, salt=salt),
                fb=wl.fwd32b(x, P, s, T, p, k1, k2))


def _fwd(be, s, T, p, x=None, *, save=True, tiled=False, gather=None, expect=0, extra=None):
    """grappa_writer_head_fwd on guarded buffers -> {name: Guarded}.  x: (s*T, F) bf16 on the device; gather = (idx (T, s) int32, x1_tab, qkv_tab);
    extra: descriptor fields set last (the refusal cases).  Guards checked behind the launch."""
    from grappa_amd import _lib
    P, M = _dev_params(), s * T
    d = _lib.WriterLayerDesc()
    d.s, d.T, d.F, d.nheads, d.dtype = s, T, F, wl.NHEADS, _lib.WRITER_BF16
    B = {"out": Guarded((M, F))}
    d.out = B["out"].ptr()
    if gather is None:
        d.x, d.w_in_pk = x.data_ptr(), be._packed_weight(P["w_in"]).data_ptr()
        d.n1_gamma, d.n1_beta = P["n1_w"].data_ptr(), P["n1_b"].data_ptr()
    else:
        d.gather_idx, d.x1_tab, d.qkv_tab = (t.data_ptr() for t in gather)
    d.w_o_pk, d.w1_pk, d.w2_pk = (be._packed_weight(P[n]).data_ptr() for n in ("w_o", "w1", "w2"))
    d.b_in, d.b_o, d.b1, d.b2 = (P[n].data_ptr() for n in ("b_in", "b_o", "b1", "b2"))
    d.nf_gamma, d.nf_beta = P["nf_w"].data_ptr(), P["nf_b"].data_ptr()
    d.drop_p, d.seed1, d.seed2, d.drop_salt = float(p), wl.SEED1, wl.SEED2, be._salt_ptr
    if save:
        tl = be.lib.grappa_writer_head_tiles(s, T)
        for n in STATS + SAVES:
            if gather is not None and n in ("mean1", "rstd1", "x1", "qkv"):
                continue
            shape = (M,) if n in STATS else ((tl * 64, F) if (n == "x2" and tiled) else (M, 3 * F if n == "qkv" else F))
            B[n] = Guarded(shape, torch.float32 if n in STATS else BF)
            setattr(d, "save_" + n, B[n].ptr())
        d.x2_tiled = int(tiled)
    for k, v in (extra or {}).items():
        if isinstance(v, Guarded):
            B["extra_" + k] = v
            v = v.ptr()
        setattr(d, k, v)
    rc = be.lib.grappa_writer_head_fwd(be._stream(), C.byref(d))
    torch.cuda.synchronize()
    assert rc == expect, rc
    what = f"fwd s={s} T={T} p={p} tiled={tiled} gather={gather is not None}"
    if expect != 0:
        assert all(b.untouched() for b in B.values()), what + ": a refused call wrote something"
        return B
    for n, b in B.items():
        b.check(f"{what} {n}", written=not (n == "x2" and tiled))      # (tile order: the padding rows may hold anything)
    return B


def _bwd(be, s, T, p, dout, x, sv, *, tiled=False, gather=None):
    """grappa_writer_head_bwd on guarded outputs; sv: {name: Guarded} of a forward call (x2 in the layout `tiled` says);
    gather = (idx (T, s) int32, qkv_tab)"""
    from grappa_amd import _lib
    P, M = _dev_params(), s * T
    tl = be.lib.grappa_writer_head_tiles(s, T)
    assert tl == wl.tiles(s, T)
    d = _lib.WriterLayerBwdDesc()
    d.s, d.T, d.F, d.nheads, d.dtype = s, T, F, wl.NHEADS, _lib.WRITER_BF16
    d.dout, d.x2, d.u, d.meanf, d.rstdf = dout.data_ptr(), sv["x2"].ptr(), sv["u"].ptr(), sv["meanf"].ptr(), sv["rstdf"].ptr()
    d.nf_gamma = P["nf_w"].data_ptr()
    d.w_o_tpk, d.w1_tpk, d.w2_tpk = (be._packed_weight(P[n], transposed=True).data_ptr() for n in ("w_o", "w1", "w2"))
    if gather is None:
        d.x, d.qkv, d.mean1, d.rstd1 = x.data_ptr(), sv["qkv"].ptr(), sv["mean1"].ptr(), sv["rstd1"].ptr()
        d.n1_gamma, d.w_in_tpk = P["n1_w"].data_ptr(), be._packed_weight(P["w_in"], transposed=True).data_ptr()
    else:
        d.gather_idx, d.qkv = gather[0].data_ptr(), gather[1].data_ptr()
    d.drop_p, d.seed1, d.seed2, d.drop_salt = float(p), wl.SEED1, wl.SEED2, be._salt_ptr
    d.x2_tiled = int(tiled)
    B = {n: Guarded((M, 3 * F if n == "dqkv" else F)) for n in BWD_OUT}
    B["ln1_part"], B["lnf_part"] = Guarded((tl, 2, F), torch.float32), Guarded((tl, 2, F), torch.float32)
    for n, b in B.items():
        setattr(d, n, b.ptr())
    rc = be.lib.grappa_writer_head_bwd(be._stream(), C.byref(d))
    torch.cuda.synchronize()
    assert rc == 0, rc
    what = f"bwd s={s} T={T} p={p} tiled={tiled} gather={gather is not None}"
    for n, b in B.items():
        if gather is not None and n == "ln1_part":
            assert b.untouched(), what + ": ln1_part is not an output in gather mode"
        else:
            b.check(f"{what} {n}")
    return B


def _cpu(B, names=None):
    return {n: b.t.detach().cpu().clone() for n, b in B.items() if names is None or n in names}


def _same_bits(a, b, names, what):
    for n in names:
        ta, tb = a[n], b[n]
        eq = ta.view(torch.int16 if ta.dtype == BF else torch.int32) == tb.view(torch.int16 if tb.dtype == BF else torch.int32)
        if not bool(eq.all()):
            rows = torch.nonzero(~eq.reshape(eq.shape[0], -1).all(1)).reshape(-1)
            raise AssertionError(f"{what} {n}: {int((~eq).sum())} elements differ, rows {rows[:8].tolist()} ({rows.numel()} rows)")


def _chain_refs(c, sv, s, T, p, dout=None, gather=False, qkv_rows=None):
    """the backward chain in float64 and its two restatements on the KERNEL's saves (upcast), so that the gate does not inherit the forward's
    flipped roundings"""
    dout = c["dout"] if dout is None else dout
    sv = dict(sv, x=c["x"])
    if qkv_rows is not None:
        sv["qkv"] = qkv_rows
    args = (dout, sv, c["P"], s, T, p, c["k1"], c["k2"])
    return (wl.with_partials(wl.bwd64(*args, gather=gather), s, T), wl.with_partials(wl.bwd32a(*args, gather=gather), s, T),
            wl.with_partials(wl.bwd32b(*args, gather=gather), s, T, reverse=True))


class _Tagged(dict):
    """a ratios dict that folds into RATIOS under `tag.name` when updated"""

    def __init__(self, tag):
        super().__init__()
        self.tag = tag

    def __setitem__(self, k, v):
        super().__setitem__(k, v)
        key = f"{self.tag}.{k}"
        RATIOS[key] = max(RATIOS.get(key, 0.0), v)


def _ratios(tag):
    return _Tagged(tag)


# ----------------------------------------------------------------------------------------------------------------------------- a, b: forward
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("s,T", wl.CASES)
def test_forward_rows_against_float64(be, s, T, p):
    c = _ref(s, T, p, _salt(be))
    x = c["x"].to(BF).cuda()
    B = _fwd(be, s, T, p, x)
    got = _cpu(B)
    wl.check_fwd(got, c["fa"], c["fb"], c["f64"], c["x"].double(), f"s={s} T={T} p={p}", ratios=_ratios("fwd"))
    # inference (no by-products): the same bits
    _same_bits(_cpu(_fwd(be, s, T, p, x, save=False)), got, ("out",), "inference")
    # save_x2 in tile order: every other tensor the same bits (the tiled x2 itself: test_backward_rows_against_float64)
    Bt = _fwd(be, s, T, p, x, tiled=True)
    assert Bt["x2"].t.shape == (wl.tiles(s, T) * 64, F)
    _same_bits(_cpu(Bt), got, ("out",) + STATS + tuple(n for n in SAVES if n != "x2"), "x2_tiled")


# ----------------------------------------------------------------------------------------------------------------------------- c: backward
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("s,T", wl.CASES)
def test_backward_rows_against_float64(be, s, T, p):
    c = _ref(s, T, p, _salt(be))
    x, dout = c["x"].to(BF).cuda(), c["dout"].to(BF).cuda()
    sv = _fwd(be, s, T, p, x)
    B = _bwd(be, s, T, p, dout, x, sv)
    got = _cpu(B)
    b64, ba, bb = _chain_refs(c, _cpu(sv), s, T, p)
    wl.check_bwd(got, ba, bb, b64, s, T, f"s={s} T={T} p={p}", ratios=_ratios("bwd"))
    # the tiled save_x2 of another forward call, read back by the backward kernel: the same bits in every output
    svt = _fwd(be, s, T, p, x, tiled=True)
    _same_bits(_cpu(_bwd(be, s, T, p, dout, x, svt, tiled=True)), got, BWD_OUT + ("ln1_part", "lnf_part"), "backward from the tiled x2")


@pytest.mark.parametrize("s", [2, 3, 4])
def test_gradients_end_to_end_against_float64_autograd(be, s):
    """dx and the twelve parameter gradients of one ragged case against autograd through the float64 forward.  The four weight gradients are
    formed here, as float64 products of the kernel's by-products with its saves (the caller's grouped products have their own gates,
    tests/test_gpu_gemm_routes.py); the restatements go the same way, each from its own forward.  Rows of a weight gradient = its columns
    (one input feature, all output features); a bias or LayerNorm gradient is one row."""
    T, p = 64 // s + 1, 0.0
    c = _ref(s, T, p, _salt(be))
    x, dout = c["x"].to(BF).cuda(), c["dout"].to(BF).cuda()
    sv = _fwd(be, s, T, p, x)
    got_sv = _cpu(sv)
    got_bw = _cpu(_bwd(be, s, T, p, dout, x, sv))
    _, dx64, g64 = wl.autograd64(c["x"], c["P"], c["dout"], s, T)
    res = []
    for fw, bwd, rev in ((c["fa"], wl.bwd32a, False), (c["fb"], wl.bwd32b, True)):
        bw = wl.with_partials(bwd(c["dout"], dict(fw, x=c["x"]), c["P"], s, T, p, None, None), s, T, reverse=rev)
        res.append((bw["dx"], wl.param_grads(bw, fw)))
    (dxa, ga), (dxb, gb) = res
    gg = wl.param_grads(got_bw, got_sv)
    rt = _ratios("e2e")
    wl.gate(rt, "dx", got_bw["dx"], dxa, dxb, dx64, wl.C_BF16, kr.rowmax(dx64).reshape(-1), f"s={s}")
    for n in wl.ORDER:
        rows = (lambda t: t.t()) if n.startswith("w") else (lambda t: t.reshape(1, -1))
        w = rows(g64[n])
        wl.gate(rt, n, rows(gg[n]), rows(ga[n]), rows(gb[n]), w, wl.C_BF16, kr.rowmax(w).reshape(-1), f"s={s}")


# ----------------------------------------------------------------------------------------------------------------------------- d: placement
@pytest.mark.parametrize("s", [2, 3, 4])
def test_a_tuple_does_not_depend_on_where_it_sits(be, s):
    """p = 0: the tuples in reversed order, and the last tuple alone -- every row of every tensor of a tuple has the same bits (each token is
    one column of the B operand; its sums run over k and over registers in an order that does not depend on the row)"""
    T, p = 3 * (64 // s) + 1, 0.0
    c = _ref(s, T, p, _salt(be))
    names_f, names_b = ("out",) + STATS + SAVES, BWD_OUT

    def run(x, dout, T_):
        xd, dd = x.to(BF).cuda(), dout.to(BF).cuda()
        sv = _fwd(be, s, T_, p, xd)
        return dict(_cpu(sv), **_cpu(_bwd(be, s, T_, p, dd, xd, sv), names_b))
    base = run(c["x"], c["dout"], T)
    rev = (torch.arange(s)[:, None] * T + torch.arange(T - 1, -1, -1)[None, :]).reshape(-1)      # row pos * T + t <- pos * T + (T - 1 - t)
    other = run(c["x"][rev], c["dout"][rev], T)
    _same_bits({n: other[n][rev] for n in names_f + names_b}, base, names_f + names_b, "tuples reversed")
    last = wl.tuple_rows(s, T, T - 1)
    alone = run(c["x"][last], c["dout"][last], 1)
    _same_bits(alone, {n: base[n][last] for n in names_f + names_b}, names_f + names_b, "the last tuple alone")


# ----------------------------------------------------------------------------------------------------------------------------- e: localised cotangent
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("where", ["last tile", "one tuple of the middle tile"])
@pytest.mark.parametrize("s,T", [(s, T) for s in (2, 3, 4) for T in (3 * (64 // s) + 1, 2 * (64 // s))])
def test_localised_cotangent_stays_where_it_is(be, s, T, where, p):
    """dout zero except on one tile's tokens, or one tuple's: every other row of dx and of the four by-products, and every other tile's
    partials, are exactly zero; the supported rows and tile pass the row gates.  What a dropped or misplaced tile cannot pass."""
    c = _ref(s, T, p, _salt(be))
    tl, TT = wl.tiles(s, T), 64 // s
    tile = tl - 1 if where == "last tile" else tl // 2
    rows = wl.tile_rows(s, T, tile) if where == "last tile" else wl.tuple_rows(s, T, tile * TT + min(5, T - tile * TT - 1))
    dout = torch.zeros_like(c["dout"])
    dout[rows] = c["dout"][rows]
    x = c["x"].to(BF).cuda()
    sv = _fwd(be, s, T, p, x)
    got = _cpu(_bwd(be, s, T, p, dout.to(BF).cuda(), x, sv))
    off = torch.ones(s * T, dtype=torch.bool)
    off[rows] = False
    for n in BWD_OUT:
        bad = torch.nonzero((got[n][off] != 0).any(1)).reshape(-1)
        assert bad.numel() == 0, f"{n}: {bad.numel()} rows outside the support are not zero, first {torch.nonzero(off).reshape(-1)[bad[:8]].tolist()}"
    others = [b for b in range(tl) if b != tile]
    for n in ("ln1_part", "lnf_part"):
        assert not bool((got[n][others] != 0).any()), f"{n}: tiles {[b for b in others if bool((got[n][b] != 0).any())]} are not zero"
    b64, ba, bb = _chain_refs(c, _cpu(sv), s, T, p, dout=dout)
    wl.check_bwd(got, ba, bb, b64, s, T, f"s={s} T={T} p={p} {where}", rows=rows, tile_sel=[tile], ratios=_ratios("bwd"))


# ----------------------------------------------------------------------------------------------------------------------------- f: mask positions
@pytest.mark.parametrize("s", [2, 3, 4])
def test_dropout_masks_sit_where_the_hash_puts_them(be, s):
    T, p = 3 * (64 // s) + 1, 0.3
    c = _ref(s, T, p, _salt(be))
    k1, k2 = c["k1"], c["k2"]
    for b in range(wl.tiles(s, T)):
        r = wl.tile_rows(s, T, b)
        for k in (k1, k2):
            assert bool(k[r].any()) and bool((~k[r]).any()), "every tile needs dropped and kept elements"
            assert bool((k[r] != k[r][:1]).any()), "... and rows that differ"
    x, dout = c["x"].to(BF).cuda(), c["dout"].to(BF).cuda()
    sv = _fwd(be, s, T, p, x)
    f, g = _cpu(sv), _cpu(_bwd(be, s, T, p, dout, x, sv))
    assert torch.equal(f["out"][~k2], f["x3"][~k2]), "out != x3 where mask 2 drops"
    assert torch.equal(f["x2"][~k1], f["x1"][~k1]), "x2 != x1 where mask 1 drops"
    assert not bool((g["dz2"][~k2] != 0).any()) and not bool((g["dzo"][~k1] != 0).any())
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    kept = (c["dout"] * torch.tensor(scale, dtype=torch.float32)).to(BF)
    assert torch.equal(g["dz2"][k2], kept[k2]), "dz2 != bf16(dout / (1 - p)) where mask 2 keeps"
    # where kept, the dropout is not the identity: a mask shifted onto kept elements would show
    assert float((f["out"][k2].float() - f["x3"][k2].float()).abs().mean()) > 0.1


# ----------------------------------------------------------------------------------------------------------------------------- g: gather mode
def _idx_dev(idx):
    return idx.to(torch.int32).contiguous().cuda()


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("s,T", [(s, T) for s in (3, 4) for T in (64 // s + 1, 3 * (64 // s) + 1)])
def test_gather_mode_through_the_identity_index_equals_the_plain_layer(be, s, T, p):
    """x1_tab / qkv_tab = what a plain run saved, gather_idx[t * s + pos] = pos * T + t: out, att, x2, x3, u, the second LayerNorm's statistics
    and the backward's dqkv have the plain run's bits; dx (= dx2) and lnf_part pass the row gates"""
    c = _ref(s, T, p, _salt(be))
    x, dout = c["x"].to(BF).cuda(), c["dout"].to(BF).cuda()
    sv = _fwd(be, s, T, p, x)
    plain = dict(_cpu(sv), **_cpu(_bwd(be, s, T, p, dout, x, sv)))
    idx = _idx_dev(torch.arange(s)[None, :] * T + torch.arange(T)[:, None])
    svg = _fwd(be, s, T, p, gather=(idx, sv["x1"].t, sv["qkv"].t))
    Bg = _bwd(be, s, T, p, dout, None, svg, gather=(idx, sv["qkv"].t))
    got = dict(_cpu(svg), **_cpu(Bg))
    _same_bits(got, plain, ("out", "att", "x2", "x3", "u", "meanf", "rstdf", "dqkv", "dz2", "dz1", "dzo", "lnf_part"), "gather, identity index")
    b64, ba, bb = _chain_refs(c, dict(_cpu(svg), qkv=plain["qkv"]), s, T, p, gather=True)
    wl.check_bwd(got, ba, bb, b64, s, T, f"gather s={s} T={T} p={p}", names=("dqkv", "dx", "lnf_part"), ratios=_ratios("gather_bwd"))


@pytest.mark.parametrize("s,T", [(s, T) for s in (3, 4) for T in (64 // s + 1, 3 * (64 // s) + 1)])
def test_gather_mode_with_repeated_table_rows_against_float64(be, s, T):
    """a table of N < T rows and a random index with repeats: every row against the float64 layer evaluated behind the gathered x1, q | k | v"""
    p = 0.3
    c = _ref(s, T, p, _salt(be))
    idx, x1_tab, qkv_tab = wl.gather_case(s, T)
    assert idx.unique().numel() < idx.numel() and int(idx.max()) < x1_tab.shape[0] < T
    rows = idx.t().reshape(-1)
    tabs = (x1_tab[rows], qkv_tab[rows])
    x1d, qkvd, idxd = x1_tab.to(BF).cuda(), qkv_tab.to(BF).cuda(), _idx_dev(idx)
    svg = _fwd(be, s, T, p, gather=(idxd, x1d, qkvd))
    got = _cpu(svg)
    g64 = wl.fwd64(None, c["P"], s, T, p, c["k1"], c["k2"], gathered=tabs)
    ga, gb = wl.fwd32a_gathered(c["P"], s, T, p, c["k1"], c["k2"], tabs), wl.fwd32b(None, c["P"], s, T, p, c["k1"], c["k2"], gathered=tabs)
    wl.check_fwd(got, ga, gb, g64, None, f"gather s={s} T={T}", names=("att", "x2", "meanf", "rstdf", "x3", "u", "out"), ratios=_ratios("gather_fwd"))
    _same_bits(_cpu(_fwd(be, s, T, p, gather=(idxd, x1d, qkvd), save=False)), got, ("out",), "gather inference")
    dout = c["dout"].to(BF).cuda()
    gotb = _cpu(_bwd(be, s, T, p, dout, None, svg, gather=(idxd, qkvd)))
    b64, ba, bb = _chain_refs(c, got, s, T, p, gather=True, qkv_rows=tabs[1])
    wl.check_bwd(gotb, ba, bb, b64, s, T, f"gather s={s} T={T}", names=("dz2", "dz1", "dzo", "dqkv", "dx", "lnf_part"), ratios=_ratios("gather_bwd"))


def test_gather_mode_refuses_a_first_layernorm_save_and_a_misaligned_table(be):
    s, T = 3, 22
    idx, x1_tab, qkv_tab = wl.gather_case(s, T)
    x1d, qkvd, idxd = x1_tab.to(BF).cuda(), qkv_tab.to(BF).cuda(), _idx_dev(idx)
    _fwd(be, s, T, 0.0, gather=(idxd, x1d, qkvd), expect=ERR_ARG, extra={"save_x1": Guarded((s * T, F))})
    odd = torch.zeros(x1d.numel() + 8, dtype=BF, device="cuda")[1:1 + x1d.numel()].view_as(x1d)      # 2 bytes off a 16-byte boundary
    assert odd.data_ptr() % 16 == 2
    _fwd(be, s, T, 0.0, gather=(idxd, odd, qkvd), expect=ERR_ARG)
    _fwd(be, s, T, 0.0, gather=(idxd, x1d, qkvd))          # (the same call with valid arguments runs)


# ----------------------------------------------------------------------------------------------------------------------------- h: degenerate values
@pytest.mark.parametrize("s", [2, 3, 4])
def test_degenerate_rows(be, s):
    """a constant input row (variance 0 in the first LayerNorm), a tuple of equal tokens (uniform softmax), a row scaled by 2^12: finite, and
    inside the row gates; the constant row as the reference's eps makes it: mean = the constant, rstd = 1 / sqrt(eps), x1 = beta"""
    T, p = 64 // s + 1, 0.0
    c = _ref(s, T, p, _salt(be), True)
    x, dout = c["x"].to(BF).cuda(), c["dout"].to(BF).cuda()
    sv = _fwd(be, s, T, p, x)
    got = _cpu(sv)
    B = _bwd(be, s, T, p, dout, x, sv)
    gotb = _cpu(B)
    assert all(bool(torch.isfinite(t).all()) for t in list(got.values()) + list(gotb.values()))
    wl.check_fwd(got, c["fa"], c["fb"], c["f64"], c["x"].double(), f"degenerate s={s}", ratios=_ratios("degenerate"))
    b64, ba, bb = _chain_refs(c, got, s, T, p)
    wl.check_bwd(gotb, ba, bb, b64, s, T, f"degenerate s={s}", ratios=_ratios("degenerate"))
    assert float(got["mean1"][0]) == 0.75
    kr.assert_el(got["rstd1"][:1], torch.full((1,), 1.0 / math.sqrt(1e-5), dtype=torch.float64), 4, 0.0, "constant row: rstd")      # (test_gpu_kernel_domains.py)
    assert torch.equal(got["x1"][0], c["P"]["n1_b"].to(BF)), "constant row: x1 = beta"
    # uniform softmax: the attention output of tuple 1's tokens is their common v (one bf16 rounding of an average of equal numbers)
    r1 = wl.tuple_rows(s, T, 1)
    assert torch.equal(got["att"][r1[0]], got["att"][r1[-1]])
    assert float((got["att"][r1[0]].double() - got["qkv"][r1[0], 2 * F:].double()).abs().max()) <= 2.0 ** -8 * float(got["qkv"][r1[0], 2 * F:].abs().max())
