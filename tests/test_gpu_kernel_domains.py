"""GPU (-m gpu): every dispatch branch of the non-GEMM kernels (graph attention and neighbour mean, LayerNorm, ELU' / dropout backward,
Adam, the tuple kernels, the batched row-wise launches, the loss) run at least once at the edges of its domain and compared with
float64 elementwise (tests/kernel_refs.py: the gates and the references).  Parameter ids name the branch a case is for."""
import itertools
import math

import numpy as np
import pytest
import torch

import kernel_refs as kr
from kernel_refs import BF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from grappa_amd.backend import HipBackend
    return HipBackend()


@pytest.fixture(scope="module")
def ref():
    from oracle.ops_ref import RefBackend
    return RefBackend()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _err():
    from grappa_amd.backend import GrappaHipError
    return GrappaHipError


FILL = 1024.0       # sentinel behind every output buffer (exact in fp32 and bf16): a kernel writing out of range changes it


def _guarded(n, dtype, offset=0, guard=64):
    """-> (flat buffer, view of n elements at `offset`) with FILL before and after the view"""
    buf = torch.full((offset + n + guard,), FILL, dtype=dtype, device="cuda")
    return buf, buf[offset:offset + n]


def _guard_ok(buf, offset, n):
    return bool((buf[:offset] == FILL).all()) and bool((buf[offset + n:] == FILL).all())


# =============================================================================================================== A. graph kernels
@pytest.fixture(scope="module")
def graph():
    """a real batch, a star whose hub has 120 neighbours (symmetric, so the reverse-edge backward holds), a single atom (degree 0) and a
    2-atom molecule behind it"""
    from grappa_amd.datasets import build_batch_from_pool
    p = build_batch_from_pool(list(range(300, 304)), n_confs=1, seed=0).plan()
    deg = (p.indptr[1:] - p.indptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(p.N), deg).numpy()
    N, s, d, hub, iso = kr.domain_graph(p.indices.long().numpy(), dst, p.N, hub_leaves=120)
    pc = kr.CsrPlan(N, s, d)
    assert int(pc.degree[hub]) == 120 and int(pc.degree[iso]) == 0
    return pc, pc.to("cuda"), hub, iso


def _nc(F):
    nc = (F // 4 + 63) // 64
    return 1 if nc <= 1 else 2 if nc <= 2 else 4 if nc <= 4 else 8


def _nc8(F):
    nc = (F // 8 + 63) // 64
    return 1 if nc <= 1 else 2 if nc <= 2 else 4


# (H, D): NC = chunks_for(H*D) float4 chunks per lane, lph = D/4 lanes per head (graph.hip)
GAT_F32 = [(1, 4), (5, 4), (32, 8), (24, 16), (16, 32), (3, 64), (16, 64), (8, 128), (4, 256), (9, 128), (64, 32), (8, 256)]
# bf16: the wide kernel (8 bf16 per lane, nc8 = chunks_for8) and the narrow fallback (D = 4, or rows 8- but not 16-byte aligned)
GAT_BF16 = [("wide", 16, 32, 0), ("wide", 6, 128, 0), ("wide", 8, 128, 0), ("wide", 9, 128, 0), ("wide", 8, 256, 0),
            ("narrow", 4, 4, 0), ("narrow", 128, 4, 0), ("narrow", 16, 32, 4), ("narrow", 8, 256, 4)]
GAT_CASES = [pytest.param(torch.float32, H, D, 0, id=f"gat-f32-NC{_nc(H * D)}-lph{D // 4}-H{H}") for H, D in GAT_F32] + \
            [pytest.param(BF, H, D, off, id=(f"gat-bf16-wide-nc8-{_nc8(H * D)}-lph{D // 8}-H{H}" if k == "wide" else
                                             f"gat-bf16-narrow-NC{_nc(H * D)}-D{D}" + ("-align8" if off else "")))
             for k, H, D, off in GAT_BF16]


@pytest.mark.parametrize("dtype,H,D,offset", GAT_CASES)
def test_gat_branches_against_float64(hip, ref, graph, dtype, H, D, offset):
    pc, pg, hub, iso = graph
    N, F, E = pc.N, H * D, pc.E
    gen = _gen(H * 1000 + D)
    ft, dout = torch.randn(N, F, generator=gen), torch.randn(N, F, generator=gen)
    if dtype == BF:
        ft, dout = ft.to(BF).float(), dout.to(BF).float()
    out64, alpha64, dft64 = kr.gat_ref64(ft, pc, H, D, dout)
    fb, ft_d = _guarded(N * F, dtype, offset)
    db, dout_d = _guarded(N * F, dtype, offset)
    ob, out_d = _guarded(N * F, dtype, offset)
    ab, alpha_d = _guarded(E * H, torch.float32)
    gb, dft_d = _guarded(N * F, dtype, offset)
    ft_d, dout_d, out_d, alpha_d, dft_d = ft_d.view(N, F), dout_d.view(N, F), out_d.view(N, F), alpha_d.view(E, H), dft_d.view(N, F)
    ft_d.copy_(ft.to(dtype)), dout_d.copy_(dout.to(dtype))
    hip.gat_fwd(pg, ft_d, H, D, out_d, alpha_d)
    hip.gat_bwd(pg, ft_d, out_d, alpha_d, dout_d, H, D, dft_d)
    torch.cuda.synchronize()
    for b, n, what in ((ob, N * F, "out"), (ab, E * H, "alpha"), (gb, N * F, "dft")):
        assert _guard_ok(b, offset if b is not ab else 0, n), f"{what}: written outside its rows"
    # degree 0: exactly zero output and gradient
    assert bool((out_d[iso] == 0).all()) and bool((dft_d[iso] == 0).all())
    # alpha: scores are dot products of <= 256 terms (<= 16 u of relative noise each through exp), x4; scale = the destination's largest alpha
    amax = torch.zeros(N, H, dtype=torch.float64).index_reduce(0, pc.dst, alpha64, "amax", include_self=True)[pc.dst]
    kr.assert_el(alpha_d, alpha64, 64, amax, "gat alpha")
    if dtype == torch.float32:
        # out: a convex combination of the neighbours' rows: the alpha noise above times the largest neighbour value
        kr.assert_el(out_d, out64, 64, kr.neighbour_abs_max(ft, pc), "gat out")
        o32, a32, d32 = torch.empty(N, F), torch.empty(E, H), torch.empty(N, F)
        ref.gat_fwd(pc, ft, H, D, o32, a32)
        ref.gat_bwd(pc, ft, o32, a32, dout, H, D, d32)
        # dft sums over up to 120 edges (the hub): summation order dominates -> the self-calibrating gate, floor 64 u of the row's largest value
        kr.assert_calibrated(dft_d, d32, dft64, 64, kr.rowmax(dft64), "gat dft")
    else:
        kr.close_bf16(out_d, out64, "gat out (bf16)")
        # the backward reads the STORED output (bf16): the float64 reference of the kernel's inputs uses the same rounded rows
        d64 = torch.empty(N, F, dtype=torch.float64)
        ref.gat_bwd(pc, ft.double(), out_d.float().cpu().double(), alpha64, dout.double(), H, D, d64)
        kr.close_bf16(dft_d, d64, "gat dft (bf16)", frac=0.95)


# F = H*D; NC = chunks_for(F)
NM_F = [4, 256, 260, 512, 1024, 1028, 2048]
NM_CASES = [pytest.param(dt, of, F, id=f"nmean-{name}-NC{_nc(F)}-F{F}") for F in NM_F
            for dt, of, name in ((torch.float32, False, "f32"), (BF, False, "bf16"), (BF, True, "bf16-outf32"))]


@pytest.mark.parametrize("dtype,out_f32,F", NM_CASES)
def test_neighbor_mean_branches_against_float64(hip, graph, dtype, out_f32, F):
    pc, pg, hub, iso = graph
    N = pc.N
    x = torch.randn(N, F, generator=_gen(F))
    if dtype == BF:
        x = x.to(BF).float()
    odt = torch.float32 if (dtype == torch.float32 or out_f32) else BF
    xd = x.to(dtype).cuda()
    for flag in (False, True):
        want = kr.neighbor_mean_ref64(x, pc, flag)
        ob, out = _guarded(N * F, odt)
        out = out.view(N, F)
        hip.neighbor_mean(pg, xd, out, flag)
        torch.cuda.synchronize()
        assert _guard_ok(ob, 0, N * F) and bool((out[iso] == 0).all())
        if odt == torch.float32:
            # the hub's mean adds 120 weighted rows in sequence: <= 2 roundings per edge of the largest neighbour value
            kr.assert_el(out, want, 256, kr.neighbour_abs_max(x, pc), f"neighbor_mean F={F} scale_by_neighbor={flag}")
        else:
            kr.close_bf16(out, want, f"neighbor_mean bf16 F={F} scale_by_neighbor={flag}")


def test_graph_refusals(hip, graph):
    """the first shapes outside the validated domains return an error before anything is launched"""
    pc, pg, hub, iso = graph
    N, E = pc.N, pc.E
    for H, D in ((1, 512), (1, 12), (513, 4)):          # lph = 128 > 64; lph = 3 not a power of two; H*D = 2052 > 2048
        ft = torch.zeros(N, H * D, device="cuda")
        with pytest.raises(_err()):
            hip.gat_fwd(pg, ft, H, D, torch.empty_like(ft), torch.empty(E, H, device="cuda"))
        with pytest.raises(_err()):
            hip.gat_bwd(pg, ft, ft, torch.zeros(E, H, device="cuda"), ft, H, D, torch.empty_like(ft))
    x = torch.zeros(N, 2052, device="cuda")
    with pytest.raises(_err()):
        hip.neighbor_mean(pg, x, torch.empty_like(x), False)


# =============================================================================================================== B. row-wise kernels
def _nch(W):
    return 1 if W <= 256 else 2 if W <= 512 else 4 if W <= 1024 else 8


LN_W = [4, 256, 260, 512, 516, 1024, 1028, 2048]
# (M, W, ld pad): 37 rows at every width; M = 1; ld > W; more rows than one grid-stride round (fwd: 8192 rows for W <= 1024, 4096 above;
# bwd: 4096)
LN_SHAPES = [(37, W, 0) for W in LN_W] + [(1, 516, 0), (37, 260, 12), (5, 2048, 4), (8197, 256, 0), (8197, 1028, 8)]
LN_CASES = [pytest.param(dt, M, W, pad, id=f"ln-{n}-NCH{_nch(W)}-W{W}-M{M}" + (f"-ld{W + pad}" if pad else ""))
            for M, W, pad in LN_SHAPES for dt, n in ((torch.float32, "f32"), (BF, "bf16"))]


def _rows(t, pad, dtype):
    """t on the GPU as a (M, W) view with leading dimension W + pad"""
    M, W = t.shape
    buf = torch.zeros(M, W + pad, dtype=dtype, device="cuda")
    buf[:, :W] = t.to(dtype)
    return buf[:, :W]


@pytest.mark.parametrize("dtype,M,W,pad", LN_CASES)
def test_layernorm_branches_against_float64(hip, dtype, M, W, pad):
    gen = _gen(M * 7 + W)
    x = torch.randn(M, W, generator=gen) * 2 + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(W, generator=gen), 0.1 * torch.randn(W, generator=gen)
    dy = torch.randn(M, W, generator=gen)
    if dtype == BF:
        x, dy = x.to(BF).float(), dy.to(BF).float()
    y64, mean64, rstd64, dx64, dg64, db64 = kr.layernorm_ref64(x, gamma, beta, dy)
    xd, dyd, g, b = _rows(x, pad, dtype), _rows(dy, pad, dtype), gamma.cuda(), beta.cuda()
    xc = x.double() - mean64[:, None]
    xh = xc * rstd64[:, None]
    cond = (xc * xc).amax(1, keepdim=True) / (xc * xc).mean(1, keepdim=True).add(1e-5)
    for amax in ((False, True) if dtype == torch.float32 else (False,)):         # the plain kernels and the ones that write row maxima
        y, mean, rstd = _rows(torch.zeros(M, W), pad, dtype), torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
        hip.layernorm_fwd(xd, g, b, y, mean, rstd, amax=amax)
        dx, dg, db = _rows(torch.zeros(M, W), pad, dtype), torch.zeros(W, device="cuda"), torch.zeros(W, device="cuda")
        hip.layernorm_bwd(dyd, xd, mean, rstd, g, dx, dg, db, accumulate=True, amax=amax)
        torch.cuda.synchronize()
        what = f"layernorm {dtype} M={M} W={W} ld={W + pad} amax={amax}"
        # mean: a sum of <= 2048 terms in per-lane chains of <= 32 and a 64-lane tree (<= 38 roundings of the largest term)
        kr.assert_el(mean, mean64, 64, kr.rowmax(x).reshape(-1), what + " mean")
        # rstd: the variance is such a sum of squares; its relative error is that times max(x - mean)^2 / var
        kr.assert_el(rstd, rstd64, 64, rstd64 * cond.reshape(-1), what + " rstd")
        # dgamma / dbeta: column sums over M rows (per-block partials, then a tree): <= 64 roundings of the sum of |terms|, x4 for xhat's noise
        kr.assert_el(dg, dg64, 256, (dy.double().abs() * (xh.abs() + kr.rowmax(xh))).sum(0), what + " dgamma")
        kr.assert_el(db, db64, 64, dy.double().abs().sum(0), what + " dbeta")
        if dtype == torch.float32:
            # y: the mean's and rstd's roundings carried into every element (scale: the row's largest |x| in units of y), x4
            kr.assert_el(y, y64, 256, kr.rowmax(x) * rstd64[:, None] * gamma.abs().max() + beta.abs().max(), what + " y")
            # dx = rstd (g - mean(g) - xhat mean(g xhat)), g = gamma dy: the three terms' scale, 256 roundings
            sg = kr.rowmax(dy.double() * gamma.double())
            kr.assert_el(dx, dx64, 256, rstd64[:, None] * sg * (1 + kr.rowmax(xh)), what + " dx")
        else:
            kr.close_bf16(y.cpu(), y64, what + " y")
            kr.close_bf16(dx.cpu(), dx64, what + " dx", frac=0.95)


@pytest.mark.parametrize("W", [512, 2048], ids=lambda w: f"ln-f32-offset-and-constant-rows-W{w}")
def test_layernorm_offset_and_constant_rows(hip, W):
    """rows with a large common offset (mean 1e4, spread 1e-2) and constant rows (variance 0): fp32 cannot hold the mean to better than
    a few roundings of 1e4, so given the kernel's mean, rstd and y are checked against float64; the mean against float64 directly"""
    gen = _gen(W)
    M = 40
    x = 1e4 + (torch.rand(M, W, generator=gen) * 2 - 1) * 1e-2
    x[30:35] = -0.75                       # constant rows with an exact mean (W is a power of two)
    x[35:] = 1e4
    gamma, beta = 1 + 0.1 * torch.randn(W, generator=gen), 0.1 * torch.randn(W, generator=gen)
    y, mean, rstd = torch.empty(M, W, device="cuda"), torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    hip.layernorm_fwd(x.cuda(), gamma.cuda(), beta.cuda(), y, mean, rstd, amax=False)
    torch.cuda.synchronize()
    xd = x.double()
    kr.assert_el(mean, xd.mean(1), 64, kr.rowmax(x).reshape(-1), "offset rows: mean")
    mk = mean.cpu().double()
    xc = xd - mk[:, None]                                  # exact in fp32 too: x and the mean are within a factor 2 (Sterbenz)
    var_k = (xc * xc).mean(1)
    rstd_k = 1.0 / torch.sqrt(var_k + 1e-5)
    # a sum of squares (<= 38 roundings) and one square root; 1e-5 itself is rounded to fp32 (u/2)
    kr.assert_el(rstd, rstd_k, 64, 0.0, "offset rows: rstd given the kernel's mean")
    y_k = xc * rstd.cpu().double()[:, None] * gamma.double() + beta.double()
    # (x - mean) * rstd * gamma + beta: four roundings of the row's largest term
    kr.assert_el(y, y_k, 8, kr.rowmax(xc) * rstd.cpu().double()[:, None] * gamma.abs().max() + beta.abs().max(), "offset rows: y")
    # constant rows: variance 0 -> rstd = 1/sqrt(1e-5), y = beta
    kr.assert_el(rstd[30:], torch.full((10,), 1.0 / math.sqrt(1e-5), dtype=torch.float64), 4, 0.0, "constant rows: rstd")
    assert torch.equal(y[30:35].cpu(), beta.expand(5, W)), "constant rows: y == beta"


AD_N = [4, 256, 260, 512, 516, 1024, 1028, 2048, 130]
AD_CASES = []
for N_ in AD_N:
    for dt, n in ((torch.float32, "f32"), (BF, "bf16")):
        kern = "scalar" if N_ % 4 else "vec"
        AD_CASES.append(pytest.param(dt, N_, False, id=f"actdrop-{n}-{kern}-N{N_}"))
        if dt == torch.float32 and N_ % 4 == 0:
            AD_CASES.append(pytest.param(dt, N_, True, id=f"actdrop-f32-rows-NCH{_nch(N_)}-N{N_}"))


@pytest.mark.parametrize("dtype,N,rows", AD_CASES)
def test_act_dropout_bwd_branches_against_float64(hip, dtype, N, rows):
    """with ELU' and without, with dropout and without; the mask bit-identical to ops_ref.dropout_keep (index row * N + col, also when
    the rows are padded)"""
    M = 67
    gen = _gen(N + 3)
    dy = torch.randn(M, N, generator=gen)
    y = torch.nn.functional.elu(torch.randn(M, N, generator=gen))
    if dtype == BF:
        dy, y = dy.to(BF).float(), y.to(BF).float()
    for p, with_y, pad in ((0.3, True, 0), (0.3, False, 4), (0.0, True, 8)):
        want, keep = kr.act_dropout_ref64(dy, y if with_y else None, p, 4242)
        dz = _rows(torch.zeros(M, N), pad, dtype)
        rec = hip.act_dropout_bwd(_rows(dy, pad, dtype), _rows(y, pad, dtype) if with_y else None, p, 4242, dz, amax=rows)
        torch.cuda.synchronize()
        assert (rec is not None) == rows
        what = f"act_dropout_bwd {dtype} N={N} p={p} elu={with_y} ld={N + pad}"
        got = dz.cpu()
        if keep is not None:
            assert torch.equal(got != 0, keep), what + ": mask"
        if dtype == torch.float32:
            kr.assert_el(got, want, 4, 0.0, what)            # dy * (1 / (1 - p)) * (y + 1): three roundings
        else:
            kr.close_bf16(got, want, what)


def test_rowwise_refusals(hip):
    x = torch.zeros(4, 2052, device="cuda")
    g = torch.ones(2052, device="cuda")
    with pytest.raises(_err()):
        hip.layernorm_fwd(x, g, g, torch.empty_like(x), torch.empty(4, device="cuda"), torch.empty(4, device="cuda"), amax=False)
    with pytest.raises(_err()):
        hip.layernorm_bwd(x, x, torch.zeros(4, device="cuda"), torch.ones(4, device="cuda"), g, torch.empty_like(x), torch.zeros_like(g),
                          torch.zeros_like(g), accumulate=True, amax=False)


# =============================================================================================================== C. tuple kernels
SA_CASES = [pytest.param(torch.float32, s, dh, 2, 37, 0, id=f"seqattn-f32-s{s}-dh{dh}") for s in (1, 2, 3, 4) for dh in (4, 8, 16, 32, 64, 128, 256)]
SA_CASES += [pytest.param(torch.float32, 4, 256, 4, 37, 0, id="seqattn-f32-s4-F1024-dh256"),
             pytest.param(torch.float32, 3, 4, 256, 37, 0, id="seqattn-f32-s3-F1024-dh4"),
             pytest.param(torch.float32, 2, 64, 16, 1, 0, id="seqattn-f32-s2-F1024-T1"),
             pytest.param(torch.float32, 1, 16, 8, 1, 0, id="seqattn-f32-s1-T1")]
SA_CASES += [pytest.param(BF, s, dh, nh, 37, 0, id=f"seqattn-bf16-wide-s{s}-dh{dh}") for s, dh, nh in ((1, 8, 4), (2, 16, 8), (3, 64, 8), (4, 128, 8), (4, 256, 4))]
SA_CASES += [pytest.param(BF, s, 4, 16, 37, 0, id=f"seqattn-bf16-narrow-s{s}-dh4") for s in (1, 4)]
SA_CASES += [pytest.param(BF, 3, 64, 8, 37, 4, id="seqattn-bf16-narrow-s3-dh64-align8")]


@pytest.mark.parametrize("dtype,s,dh,nh,T,offset", SA_CASES)
def test_seqattn_branches_against_float64(hip, ref, dtype, s, dh, nh, T, offset):
    Fd = nh * dh
    gen = _gen(s * 1000 + dh + nh)
    qkv, dout = torch.randn(s * T, 3 * Fd, generator=gen), torch.randn(s * T, Fd, generator=gen)
    if dtype == BF:
        qkv, dout = qkv.to(BF).float(), dout.to(BF).float()
    out64, d64 = kr.seqattn_ref64(qkv, dout, s, T, nh)
    qb, qd = _guarded(s * T * 3 * Fd, dtype, offset)
    gb, gd = _guarded(s * T * Fd, dtype, offset)
    ob, od = _guarded(s * T * Fd, dtype, offset)
    db, dd = _guarded(s * T * 3 * Fd, dtype, offset)
    qd, gd, od, dd = qd.view(s * T, 3 * Fd), gd.view(s * T, Fd), od.view(s * T, Fd), dd.view(s * T, 3 * Fd)
    qd.copy_(qkv.to(dtype)), gd.copy_(dout.to(dtype))
    hip.seqattn_fwd(qd, s, T, nh, od, amax=False)
    hip.seqattn_bwd(qd, gd, s, T, nh, dd, amax=False)
    torch.cuda.synchronize()
    assert _guard_ok(ob, offset, s * T * Fd) and _guard_ok(db, offset, s * T * 3 * Fd), "written outside the output rows"
    what = f"seqattn {dtype} s={s} dh={dh} nheads={nh} T={T}"
    if dtype == torch.float32:
        # the output is a convex combination of the tuple's v rows: scores carry <= 16 u (dh <= 256 terms) through exp, x4
        vmax = qkv[:, 2 * Fd:].double().abs().view(s, T, Fd).amax((0, 2)).repeat(s)[:, None]
        kr.assert_el(od, out64, 64, vmax, what + " out")
        d32 = torch.empty(s * T, 3 * Fd)
        ref.seqattn_bwd(qkv, dout, s, T, nh, d32)
        # the backward sums over the s tokens in the kernel's order: self-calibrating gate, floor 64 u of the row's largest value
        kr.assert_calibrated(dd, d32, d64, 64, kr.rowmax(d64), what + " dqkv")
    else:
        kr.close_bf16(od, out64, what + " out")
        kr.close_bf16(dd, d64, what + " dqkv", frac=0.95)


PERMS = {1: [[0]], 2: [[0, 1], [1, 0]], 3: [list(p) for p in itertools.permutations(range(3))],
         4: [[0, 1, 2, 3], [3, 1, 2, 0], [1, 3, 2, 0], [0, 3, 2, 1], [3, 0, 2, 1], [1, 0, 2, 3]]}


@pytest.mark.parametrize("s", [1, 2, 3, 4], ids=lambda s: f"perm-concat-s{s}-P{len(PERMS[s])}")
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_perm_concat_edges(hip, s, dtype):
    perms, T, Fd = PERMS[s], 37, 68
    P = len(perms)
    gen = _gen(s * 10 + P)
    x, dz = torch.randn(s * T, Fd, generator=gen).to(dtype).float(), torch.randn(P * T, s * Fd, generator=gen).to(dtype).float()
    z64, dx64 = kr.perm_concat_ref64(x, s, T, perms, dz)
    z = torch.empty(P * T, s * Fd, dtype=dtype, device="cuda")
    hip.perm_concat_fwd(x.to(dtype).cuda(), s, T, perms, z)
    dx = torch.empty(s * T, Fd, dtype=dtype, device="cuda")
    hip.perm_concat_bwd(dz.to(dtype).cuda(), s, T, perms, dx)
    torch.cuda.synchronize()
    assert torch.equal(z.cpu().double(), z64), "perm_concat_fwd: a copy, bit exact"
    if dtype == torch.float32:
        # each row of dx is a sum of P slots: <= P - 1 roundings of the sum of |terms|
        kr.assert_el(dx, dx64, 8, kr.perm_concat_ref64(x, s, T, perms, dz.abs())[1], f"perm_concat_bwd s={s} P={P}")
    else:
        kr.close_bf16(dx.cpu(), dx64, f"perm_concat_bwd bf16 s={s} P={P}")


@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
@pytest.mark.parametrize("n_per", [1, 2, 3, 6, 8], ids=lambda n: f"param-out-torsion-nper{n}")
def test_param_out_torsion_n_per(hip, ref, n_per, gated):
    T, P = 101, 2
    nout = (2 if gated else 1) * n_per
    gen = _gen(n_per * 2 + int(gated))
    o = torch.randn(P * T, nout, generator=gen)
    o = torch.sign(o) * (o.abs() + 1e-2)        # away from the hard cutoff, where fp32 and float64 may take different sides
    o[:20] *= 1e-6                              # ... except these rows, which take the cutoff branch on both
    consts = torch.cat([0.1 + torch.rand(n_per, generator=gen), torch.randn(n_per, generator=gen)])
    dk = torch.randn(T, n_per, generator=gen)
    k64, d64 = torch.empty(T, n_per, dtype=torch.float64), torch.empty(P * T, nout, dtype=torch.float64)
    ref.param_out_fwd(2, o.double(), T, P, n_per, gated, 1e-4, consts.double(), k64, None)
    ref.param_out_bwd(2, o.double(), T, P, n_per, gated, 1e-4, consts.double(), dk.double(), None, d64)
    k, d = torch.empty(T, n_per, device="cuda"), torch.empty(P * T, nout, device="cuda")
    hip.param_out_fwd(2, o.cuda(), T, P, n_per, gated, 1e-4, consts.cuda(), k, None)
    hip.param_out_bwd(2, o.cuda(), T, P, n_per, gated, 1e-4, consts.cuda(), dk.cuda(), None, d)
    torch.cuda.synchronize()
    # a mean over P permutations, a sigmoid and a product: a few roundings of the row's largest value, x8
    kr.assert_el(k, k64, 32, kr.rowmax(k64), f"param_out k n_per={n_per} gated={gated}")
    kr.assert_el(d, d64, 32, kr.rowmax(d64), f"param_out_bwd n_per={n_per} gated={gated}")


def test_tuple_gather_empty_and_odd_width(hip):
    """T = 0 (no tuples: nothing written, the backward zeroes or keeps), and W = 68 (not a multiple of 64) against float64"""
    N, W, s = 50, 68, 3
    gen = _gen(68)
    a = torch.randn(N, W, generator=gen)
    x0 = torch.empty(0, W, device="cuda")
    hip.tuple_gather_fwd(a.cuda(), torch.zeros(0, s, dtype=torch.int32, device="cuda"), s, None, x0)
    ptr0, rows0 = torch.zeros(N + 1, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda")
    for acc in (False, True):
        da = torch.full((N, W), 5.0, device="cuda")
        hip.tuple_gather_bwd(ptr0, rows0, x0, da, False, accumulate=acc)
        torch.cuda.synchronize()
        assert bool((da == (5.0 if acc else 0.0)).all()), f"T = 0, accumulate={acc}"
    T = 37
    idx = torch.randint(0, N, (T, s), generator=gen, dtype=torch.int64)
    atoms = idx.t().reshape(-1).numpy()
    rows = np.argsort(atoms, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(atoms, minlength=N))])
    x = torch.empty(s * T, W, device="cuda")
    hip.tuple_gather_fwd(a.cuda(), idx.to(torch.int32).cuda(), s, None, x)
    dx = torch.randn(s * T, W, generator=gen)
    da = torch.empty(N, W, device="cuda")
    hip.tuple_gather_bwd(torch.from_numpy(ptr.astype(np.int32)).cuda(), torch.from_numpy(rows.astype(np.int32)).cuda(), dx.cuda(), da, False)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), a[idx.t().reshape(-1)]), "tuple_gather_fwd: a copy, bit exact"
    at = torch.from_numpy(atoms)
    want = torch.zeros(N, W, dtype=torch.float64).index_add(0, at, dx.double())
    scale = torch.zeros(N, W, dtype=torch.float64).index_add(0, at, dx.double().abs())
    assert int(np.bincount(atoms).max()) <= 16
    kr.assert_el(da, want, 16, scale, "tuple_gather_bwd W=68")       # <= 15 roundings of the sum of |terms| (<= 16 rows per atom)


def test_tuple_refusals(hip):
    for s, nh, dh in ((2, 1, 512), (2, 257, 4), (5, 2, 16), (2, 1, 12)):      # dh/4 = 128 > 64; nheads*dh = 1028; s = 5; dh/4 = 3
        F = nh * dh
        qkv = torch.zeros(s * 3, 3 * F, device="cuda")
        with pytest.raises(_err()):
            hip.seqattn_fwd(qkv, s, 3, nh, torch.empty(s * 3, F, device="cuda"), amax=False)
        with pytest.raises(_err()):
            hip.seqattn_bwd(qkv, torch.zeros(s * 3, F, device="cuda"), s, 3, nh, torch.empty_like(qkv), amax=False)
    perms7 = [list(p) for p in itertools.permutations(range(4))][:7]          # P = 7 > 6
    with pytest.raises((_err(), ValueError)):
        hip.perm_concat_fwd(torch.zeros(8, 16, device="cuda"), 4, 2, perms7, torch.empty(14, 64, device="cuda"))


# =============================================================================================================== D. batched launches
def _i(t):
    return t.data_ptr() if t is not None and t.numel() else None


LN_BATCHES = {2: [(300, 512), (0, 256)], 3: [(37, 4), (1000, 1028), (5, 260)], 4: [(0, 2048), (77, 2048), (513, 516), (4100, 256)]}


@pytest.mark.parametrize("n", [2, 3, 4], ids=lambda n: f"ln-batched-{n}items")
def test_layernorm_batched_equals_single_launches(hip, n):
    """grappa_layernorm_{fwd,bwd}_batched_f32 over heterogeneous items (one empty) = the single-tensor launches bit for bit, row maxima and
    the backward's parameter-gradient partials included (include/grappa_hip.h: same arithmetic per tensor)"""
    from grappa_amd import _lib
    lib, st = hip.lib, _st()
    gen = _gen(n)
    items = []
    for M, W in LN_BATCHES[n]:
        x, dy = (torch.randn(M, W, generator=gen) * 2 + 0.5).cuda(), torch.randn(M, W, generator=gen).cuda()
        g, b = (1 + 0.1 * torch.randn(W, generator=gen)).cuda(), (0.1 * torch.randn(W, generator=gen)).cuda()
        items.append((M, W, x, dy, g, b))

    def outs(M, W):
        return (torch.empty(M, W, device="cuda"), torch.empty(M, device="cuda"), torch.empty(M, device="cuda"), torch.empty(M, dtype=torch.int32, device="cuda"))

    single, batched = [outs(M, W) for M, W, *_ in items], [outs(M, W) for M, W, *_ in items]
    arr = (_lib.LnFwdItem * n)()
    for a, (M, W, x, dy, g, b), (y, mean, rstd, row), (y1, mean1, rstd1, row1) in zip(arr, items, batched, single):
        a.M, a.W, a.x, a.ldx, a.gamma, a.beta, a.y, a.ldy = M, W, _i(x), W, g.data_ptr(), b.data_ptr(), _i(y), W
        a.mean, a.rstd, a.y_amax = _i(mean), _i(rstd), _i(row)
        assert lib.grappa_layernorm_fwd_amax_f32(st, M, W, _i(x), W, g.data_ptr(), b.data_ptr(), _i(y1), W, _i(mean1), _i(rstd1), _i(row1)) == 0
    assert lib.grappa_layernorm_fwd_batched_f32(st, arr, n) == 0
    torch.cuda.synchronize()
    for (M, W, *_), bt, sg in zip(items, batched, single):
        for u, v, nm in zip(bt, sg, ("y", "mean", "rstd", "row maxima")):
            assert torch.equal(u, v), f"layernorm_fwd_batched item M={M} W={W}: {nm}"
    # backward, accumulate = 2 (the partials stay in the workspace)
    arr = (_lib.LnBwdItem * n)()
    res = []
    for a, (M, W, x, dy, g, b), (y, mean, rstd, row) in zip(arr, items, batched):
        wsb = lib.grappa_layernorm_bwd_workspace_bytes(M, W)
        ws, ws1 = torch.zeros(wsb // 4 + 1, device="cuda"), torch.zeros(wsb // 4 + 1, device="cuda")
        dx, dx1 = torch.empty(M, W, device="cuda"), torch.empty(M, W, device="cuda")
        r, r1 = torch.empty(M, dtype=torch.int32, device="cuda"), torch.empty(M, dtype=torch.int32, device="cuda")
        a.M, a.W, a.dy, a.lddy, a.x, a.ldx = M, W, _i(dy), W, _i(x), W
        a.mean, a.rstd, a.gamma, a.dx, a.lddx, a.part, a.dx_amax = _i(mean), _i(rstd), g.data_ptr(), _i(dx), W, ws.data_ptr(), _i(r)
        assert lib.grappa_layernorm_bwd_amax_f32(st, M, W, _i(dy), W, _i(x), W, _i(mean), _i(rstd), g.data_ptr(), _i(dx1), W, None, None, 2,
                                                 ws1.data_ptr(), wsb, _i(r1)) == 0
        res.append((M, W, dx, dx1, r, r1, ws, ws1, lib.grappa_layernorm_bwd_partial_rows(M) * 2 * W))
    assert lib.grappa_layernorm_bwd_batched_f32(st, arr, n) == 0
    torch.cuda.synchronize()
    for M, W, dx, dx1, r, r1, ws, ws1, npart in res:
        assert torch.equal(dx, dx1) and torch.equal(r, r1), f"layernorm_bwd_batched item M={M} W={W}: dx / row maxima"
        assert torch.equal(ws[:npart], ws1[:npart]), f"layernorm_bwd_batched item M={M} W={W}: parameter-gradient partials"


AD_BATCHES = {2: [(300, 512, True, 0.3), (0, 256, False, 0.5)], 3: [(37, 4, True, 0.0), (1000, 1028, False, 0.2), (5, 260, True, 0.3)],
              4: [(77, 2048, True, 0.3), (0, 2048, True, 0.3), (513, 516, False, 0.1), (4100, 256, True, 0.4)]}


@pytest.mark.parametrize("n", [2, 3, 4], ids=lambda n: f"actdrop-batched-{n}items")
def test_act_dropout_bwd_batched_equals_single_launches(hip, n):
    from grappa_amd import _lib
    lib, st = hip.lib, _st()
    gen = _gen(10 + n)
    arr = (_lib.ActDropoutItem * n)()
    res = []
    for a, (M, N, with_y, p) in zip(arr, AD_BATCHES[n]):
        dy = torch.randn(M, N, generator=gen).cuda()
        y = torch.nn.functional.elu(torch.randn(M, N, generator=gen)).cuda() if with_y else None
        dz, dz1 = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
        r, r1 = torch.empty(M, dtype=torch.int32, device="cuda"), torch.empty(M, dtype=torch.int32, device="cuda")
        seed = 1000 + M
        a.M, a.N, a.dy, a.lddy, a.y, a.ldy = M, N, _i(dy), N, _i(y), N if with_y else 0
        a.drop_p, a.drop_seed, a.dz, a.lddz, a.dz_amax, a.drop_salt = p, seed, _i(dz), N, _i(r), None
        assert lib.grappa_act_dropout_bwd_amax_f32(st, M, N, _i(dy), N, _i(y), N if with_y else 0, p, seed, _i(dz1), N, _i(r1), None) == 0
        res.append((M, N, dz, dz1, r, r1, (dy, y)))          # (the inputs stay alive until the batched launch ran)
    assert lib.grappa_act_dropout_bwd_batched_f32(st, arr, n) == 0
    torch.cuda.synchronize()
    for M, N, dz, dz1, r, r1, _ in res:
        assert torch.equal(dz, dz1) and torch.equal(r, r1), f"act_dropout_bwd_batched item M={M} N={N}"


SA_BATCHES = {2: [(2, 37, 8, 64), (1, 0, 2, 16)], 3: [(3, 5, 4, 32), (4, 1, 1, 256), (1, 50, 16, 4)],
              4: [(2, 0, 8, 64), (4, 33, 4, 256), (3, 17, 2, 8), (1, 3, 64, 16)]}


@pytest.mark.parametrize("n", [2, 3, 4], ids=lambda n: f"seqattn-batched-{n}items")
def test_seqattn_batched_equals_single_launches(hip, n):
    from grappa_amd import _lib
    lib, st = hip.lib, _st()
    gen = _gen(20 + n)
    fa, ba = (_lib.SeqAttnItem * n)(), (_lib.SeqAttnItem * n)()
    res = []
    for a, b, (s, T, nh, dh) in zip(fa, ba, SA_BATCHES[n]):
        Fd = nh * dh
        qkv, dout = torch.randn(s * T, 3 * Fd, generator=gen).cuda(), torch.randn(s * T, Fd, generator=gen).cuda()
        o, o1 = torch.empty(s * T, Fd, device="cuda"), torch.empty(s * T, Fd, device="cuda")
        d, d1 = torch.empty(s * T, 3 * Fd, device="cuda"), torch.empty(s * T, 3 * Fd, device="cuda")
        r = [torch.empty(s * T, dtype=torch.int32, device="cuda") for _ in range(4)]
        a.s, a.T, a.nheads, a.dh, a.qkv, a.out, a.amax = s, T, nh, dh, _i(qkv), _i(o), _i(r[0])
        b.s, b.T, b.nheads, b.dh, b.qkv, b.dout, b.dqkv, b.amax = s, T, nh, dh, _i(qkv), _i(dout), _i(d), _i(r[2])
        assert lib.grappa_seqattn_fwd_amax_f32(st, s, T, nh, dh, _i(qkv), _i(o1), _i(r[1])) == 0
        assert lib.grappa_seqattn_bwd_amax_f32(st, s, T, nh, dh, _i(qkv), _i(dout), _i(d1), _i(r[3])) == 0
        res.append(((s, T, nh, dh), o, o1, d, d1, r, (qkv, dout)))          # (the inputs stay alive until the batched launches ran)
    assert lib.grappa_seqattn_fwd_batched_f32(st, fa, n) == 0
    assert lib.grappa_seqattn_bwd_batched_f32(st, ba, n) == 0
    torch.cuda.synchronize()
    for key, o, o1, d, d1, r, _ in res:
        assert torch.equal(o, o1) and torch.equal(r[0], r[1]), f"seqattn_fwd_batched item {key}"
        assert torch.equal(d, d1) and torch.equal(r[2], r[3]), f"seqattn_bwd_batched item {key}"


# =============================================================================================================== F. Adam and loss
ADAM_CASES = [(1, 0.0, 1.0, "none", 1), (255, 1e-2, 0.25, "active", 1000), (255, 0.0, 1.0, "inactive", 1000),
              (1_000_003, 1e-2, 1.0, "active", 1), (1_000_003, 1e-2, 0.25, "inactive", 1000), (1, 1e-2, 0.25, "active", 1000)]


def _adam_id(n, wd, gs, clip, step):
    """e.g. adam-n1000003-gridrounds2-wd0.01-gs0.25-clip-inactive-step1000 (grid rounds: grid-stride trips of the 2048 x 256 threads)"""
    return f"adam-n{n}-gridrounds{-(-n // (2048 * 256))}-wd{wd}-gs{gs}-clip-{clip}-step{step}"


@pytest.mark.parametrize("dyn", [False, True], ids=["adam-static", "adam-dyn"])
@pytest.mark.parametrize("n,wd,gs,clip,step", [pytest.param(*c, id=_adam_id(*c)) for c in ADAM_CASES])
def test_adam_against_torch_optim_adam_float64(hip, n, wd, gs, clip, step, dyn):
    """adam_step / adam_step_dyn (learning rate and step read from device memory) against float64 torch.optim.Adam(weight_decay=wd) after
    clip_grad_norm_; the hyperparameters the kernel receives are fp32, so the reference gets the same fp32 values"""
    f32 = lambda v: float(np.float32(v))            # noqa: E731
    lr, b1, b2, eps, wd32 = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8), f32(wd)
    gen = _gen(n + step)
    p0, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 3
    m0 = 0.1 * torch.randn(n, generator=gen) if step > 1 else torch.zeros(n)
    v0 = 0.01 * torch.rand(n, generator=gen) + 1e-4 if step > 1 else torch.zeros(n)
    norm = float(g.double().norm()) * gs
    max_norm = {"none": 1.0, "active": 0.5 * norm, "inactive": 2.0 * norm}[clip]
    q = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd32, foreach=False)
    if step > 1:
        opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0.double().clone(), "exp_avg_sq": v0.double().clone()}
    q.grad = g.double() * gs
    if clip != "none":
        torch.nn.utils.clip_grad_norm_([q], max_norm)
    gterms = q.grad.abs() + wd32 * p0.double().abs()           # |clipped, scaled gradient| + |weight decay| (they may cancel)
    opt.step()
    p64, m64, v64 = q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]
    p, m, v, gd = p0.cuda(), m0.cuda(), v0.cuda(), g.cuda()
    ss = None
    if clip != "none":
        ss = torch.zeros(1, device="cuda")
        hip.sumsq(gd, ss, False)
    if dyn:
        hip.adam_step_dyn(p, gd, m, v, torch.tensor([lr], device="cuda"), b1, b2, eps, wd32, torch.tensor([step], dtype=torch.int32, device="cuda"),
                          gs, ss, max_norm)
    else:
        hip.adam_step(p, gd, m, v, lr, b1, b2, eps, wd32, step, gs, ss, max_norm)
    torch.cuda.synchronize()
    what = f"adam{'_dyn' if dyn else ''} n={n} wd={wd} grad_scale={gs} clip={clip} step={step}"
    # m, v: one fused multiply-add each over terms whose clip factor carries the sum of squares' roundings (<= 32 u): 64 u of the terms
    kr.assert_el(m, m64, 64, b1 * m0.double().abs() + (1 - b1) * gterms, what + " m")
    kr.assert_el(v, v64, 64, b2 * v0.double() + (1 - b2) * gterms * gterms, what + " v")
    # p: 4 u of p plus 64 u of the update (its sqrt, division, powf-based bias corrections)
    kr.assert_el(p, p64, 4, 16 * (p64 - p0.double()).abs(), what + " p")


def _loss_plan(sizes, dev):
    class P:
        pass
    p = P()
    p.B, p.N = len(sizes), int(sum(sizes))
    p.atom_molptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)
    return p


@pytest.mark.parametrize("dummies", [False, True], ids=["loss-C300-mol300-nodummy", "loss-C300-mol300-dummies"])
def test_loss_and_eval_strided_loops_against_float64(hip, ref, dummies):
    """loss_ef / eval_se with C = 300 > 256 conformations (the kernels' strided loops) and a molecule of 300 > 256 atoms"""
    sizes, C = [300, 7, 1, 40], 300
    pc, pg = _loss_plan(sizes, "cpu"), _loss_plan(sizes, "cuda")
    B, N = pc.B, pc.N
    gen = _gen(300)
    e, er = torch.randn(B, C, generator=gen) * 5 + 100, torch.randn(B, C, generator=gen) * 5 - 40
    gr, grr = torch.randn(N, C, 3, generator=gen) * 10, torch.randn(N, C, 3, generator=gen) * 10
    dm = None
    if dummies:
        dm = torch.zeros(B, C)
        dm[0, 250:] = 1
        dm[2, 1:] = 1
    inv_B, wE, wG = 1.0 / B, 1.0, 0.8

    # the reference: the loss stated directly in float64, gradients by autograd (kernel_refs.loss_ef_ref64, checked against
    # cpu_ref.RefMolwiseLoss on the CPU); the calibration: RefBackend's fp32 restatement
    r64 = kr.loss_ef_ref64(sizes, e, er, dm, gr, grr, wE, wG, inv_B)
    r32 = (torch.zeros(B), torch.zeros(B, C), torch.zeros(N, C, 3), torch.zeros(B, 4))
    ref.loss_ef(pc, e, er, dm, gr, grr, wE, wG, inv_B, r32[0], r32[1], r32[2])
    ref.eval_se(pc, e, er, dm, gr, grr, r32[3])
    lm, gE, gG, se = torch.zeros(B, device="cuda"), torch.zeros(B, C, device="cuda"), torch.zeros(N, C, 3, device="cuda"), torch.zeros(B, 4, device="cuda")
    cu = lambda t: None if t is None else t.cuda()        # noqa: E731
    hip.loss_ef(pg, cu(e), cu(er), cu(dm), cu(gr), cu(grr), wE, wG, inv_B, lm, gE, gG)
    hip.eval_se(pg, cu(e), cu(er), cu(dm), cu(gr), cu(grr), se)
    torch.cuda.synchronize()
    # per-molecule sums of up to 270,000 squares: summation order dominates -> self-calibrating gate, floor 256 u of the (positive) value
    kr.assert_calibrated(lm, r32[0], r64[0], 256, r64[0].abs(), "loss_ef loss_mol")
    kr.assert_calibrated(se, r32[3], r64[3], 256, kr.rowmax(r64[3]).reshape(-1), "eval_se")
    # gE: centred energies (offsets 100 and -40 cancel): 64 u of the molecule's energy magnitudes times the gradient's factor
    m = torch.ones(B, C) if dm is None else (dm == 0).double()
    nreal = m.sum(1, keepdim=True)
    kr.assert_el(gE, r64[1], 64, 2 * wE * inv_B / nreal * (kr.rowmax(e) + kr.rowmax(er)), "loss_ef gE")
    # gG: a difference and a scaling per element: 8 u of |grad| + |grad_ref| times the factor
    cnt = torch.tensor(sizes, dtype=torch.float64)
    seg = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))
    fac = (inv_B * wG * 2.0 / (cnt * nreal[:, 0] * 3.0))[seg][:, None, None]
    kr.assert_el(gG, r64[2], 8, fac * (gr.double().abs() + grr.double().abs()), "loss_ef gG")
