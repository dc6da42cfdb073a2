"""CPU: the float64 references of tests/kernel_refs.py (what the GPU domain tests compare the kernels with) agree with the op-by-op
restatement oracle/ops_ref.RefBackend run in float64 on the same inputs (the loss also with cpu_ref.RefMolwiseLoss), and the gates
reject what they must."""
import math

import numpy as np
import pytest
import torch

import kernel_refs as kr

D64 = torch.float64


@pytest.fixture(scope="module")
def ref():
    from oracle.ops_ref import RefBackend
    return RefBackend()


@pytest.fixture(scope="module")
def plan():
    from grappa_amd.datasets import build_batch_from_pool
    p = build_batch_from_pool([300, 301], n_confs=1, seed=0).plan()
    deg = (p.indptr[1:] - p.indptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(p.N), deg).numpy()
    N, s, d, hub, iso = kr.domain_graph(p.indices.long().numpy(), dst, p.N, hub_leaves=20)
    pc = kr.CsrPlan(N, s, d)
    assert int(pc.degree[hub]) == 20 and int(pc.degree[iso]) == 0
    # the reverse-edge slot of every edge holds the opposite edge
    assert torch.equal(pc.src[pc.rev.long()], pc.dst) and torch.equal(pc.dst[pc.rev.long()], pc.src)
    return pc


def _close(a, b, what, tol=1e-12):
    a, b = a.double(), b.double()
    err = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300) if b.numel() else 0.0
    assert err < tol, f"{what}: {err:.3e}"


@pytest.mark.parametrize("H,D", [(2, 8), (1, 4), (3, 16)])
def test_gat_reference(ref, plan, H, D):
    gen = torch.Generator().manual_seed(H * D)
    N, F = plan.N, H * D
    ft, dout = torch.randn(N, F, generator=gen, dtype=D64), torch.randn(N, F, generator=gen, dtype=D64)
    out, alpha, dft = kr.gat_ref64(ft, plan, H, D, dout)
    o, a, d = torch.empty(N, F, dtype=D64), torch.empty(plan.E, H, dtype=D64), torch.empty(N, F, dtype=D64)
    ref.gat_fwd(plan, ft, H, D, o, a)
    ref.gat_bwd(plan, ft, o, a, dout, H, D, d)
    _close(out, o, "out"), _close(alpha, a, "alpha"), _close(dft, d, "dft")


@pytest.mark.parametrize("flag", [False, True])
def test_neighbor_mean_reference(ref, plan, flag):
    x = torch.randn(plan.N, 12, generator=torch.Generator().manual_seed(1), dtype=D64)
    o = torch.empty_like(x)
    ref.neighbor_mean(plan, x, o, flag)
    _close(kr.neighbor_mean_ref64(x, plan, flag), o, f"neighbor_mean {flag}")


@pytest.mark.parametrize("M,W", [(7, 4), (5, 260), (1, 516)])
def test_layernorm_reference(ref, M, W):
    gen = torch.Generator().manual_seed(M + W)
    x, dy = torch.randn(M, W, generator=gen, dtype=D64) * 2 + 0.5, torch.randn(M, W, generator=gen, dtype=D64)
    g, b = 1 + 0.1 * torch.randn(W, generator=gen, dtype=D64), 0.1 * torch.randn(W, generator=gen, dtype=D64)
    y64, m64, r64, dx64, dg64, db64 = kr.layernorm_ref64(x, g, b, dy)
    y, m, r = torch.empty(M, W, dtype=D64), torch.empty(M, dtype=D64), torch.empty(M, dtype=D64)
    ref.layernorm_fwd(x, g, b, y, m, r)
    dx, dg, db = torch.empty(M, W, dtype=D64), torch.zeros(W, dtype=D64), torch.zeros(W, dtype=D64)
    ref.layernorm_bwd(dy, x, m, r, g, dx, dg, db, True)
    for u, v, n in ((y64, y, "y"), (m64, m, "mean"), (r64, r, "rstd"), (dx64, dx, "dx"), (dg64, dg, "dgamma"), (db64, db, "dbeta")):
        _close(u, v, n)


def test_act_dropout_reference(ref):
    gen = torch.Generator().manual_seed(3)
    dy, y = torch.randn(9, 130, generator=gen, dtype=D64), torch.nn.functional.elu(torch.randn(9, 130, generator=gen, dtype=D64))
    for p, yy in ((0.3, y), (0.3, None), (0.0, y)):
        o = torch.empty_like(dy)
        ref.act_dropout_bwd(dy, yy, p, 4242, o)
        want, keep = kr.act_dropout_ref64(dy, yy, p, 4242)
        _close(want, o, f"act_dropout p={p}")
        if keep is not None:
            assert abs(float(keep.double().mean()) - (1 - p)) < 0.05


@pytest.mark.parametrize("s,nh,dh,T", [(1, 2, 4, 3), (3, 2, 8, 5), (4, 1, 16, 1)])
def test_seqattn_reference(ref, s, nh, dh, T):
    gen = torch.Generator().manual_seed(s * dh)
    Fd = nh * dh
    qkv, dout = torch.randn(s * T, 3 * Fd, generator=gen, dtype=D64), torch.randn(s * T, Fd, generator=gen, dtype=D64)
    out, dq = kr.seqattn_ref64(qkv, dout, s, T, nh)
    o, d = torch.empty(s * T, Fd, dtype=D64), torch.empty(s * T, 3 * Fd, dtype=D64)
    ref.seqattn_fwd(qkv, s, T, nh, o)
    ref.seqattn_bwd(qkv, dout, s, T, nh, d)
    _close(out, o, "out"), _close(dq, d, "dqkv")
    if s == 1:
        _close(out, qkv[:, 2 * Fd:], "s = 1: the output is v")


@pytest.mark.parametrize("s,perms", [(1, [[0]]), (3, [[0, 1, 2], [2, 0, 1], [1, 2, 0]])])
def test_perm_concat_reference(ref, s, perms):
    gen = torch.Generator().manual_seed(s)
    T, Fd, P = 5, 8, len(perms)
    x, dz = torch.randn(s * T, Fd, generator=gen, dtype=D64), torch.randn(P * T, s * Fd, generator=gen, dtype=D64)
    z, dx = kr.perm_concat_ref64(x, s, T, perms, dz)
    z1, dx1 = torch.empty(P * T, s * Fd, dtype=D64), torch.empty(s * T, Fd, dtype=D64)
    ref.perm_concat_fwd(x, s, T, perms, z1)
    ref.perm_concat_bwd(dz, s, T, perms, dx1)
    assert torch.equal(z, z1)
    _close(dx, dx1, "perm_concat dx")


@pytest.mark.parametrize("n_per,offset", [((0, 0, 1, 8), False), ((0, 0, 6, 3), True)])
def test_mm_reference_autograd_equals_closed_forms(ref, n_per, offset):
    """autograd of the reference's formulas = the kernels' closed forms (RefBackend), both in float64: energy, dE/dx and the double
    backward's gk / geq"""
    from grappa_amd.datasets import build_batch_from_pool
    lv = ["n2", "n3", "n4", "n4_improper"]
    g = build_batch_from_pool([300, 301], n_confs=3, seed=1)
    p = g.plan()
    xyz = g.nodes["n1"].data["xyz"].double()
    gen = torch.Generator().manual_seed(5)
    ks = [700 + 100 * torch.rand(p.T["n2"], generator=gen, dtype=D64), 100 + 20 * torch.rand(p.T["n3"], generator=gen, dtype=D64),
          torch.randn(p.T["n4"], n_per[2], generator=gen, dtype=D64), torch.randn(p.T["n4_improper"], n_per[3], generator=gen, dtype=D64)]
    eqs = [1.2 + 0.1 * torch.randn(p.T["n2"], generator=gen, dtype=D64), 1.9 + 0.1 * torch.randn(p.T["n3"], generator=gen, dtype=D64), None, None]
    B, C, N = p.B, 3, p.N
    gE, gG = torch.randn(B, C, generator=gen, dtype=D64), torch.randn(N, C, 3, generator=gen, dtype=D64)
    want = kr.mm_ref64([p.idx32[l].long() for l in lv], [p.mol_ptr[l] for l in lv], B, xyz, ks, eqs, list(n_per), offset, gE, gG)
    e, terms, grad = torch.empty(B, C, dtype=D64), torch.empty(4, B, C, dtype=D64), torch.empty(N, C, 3, dtype=D64)
    te = [torch.empty(p.T[l], C, dtype=D64) for l in lv]
    tx = [torch.empty(p.T[l], C, dtype=D64) for l in lv]
    ref.mm_energy_fwd(p, xyz, ks, eqs, list(n_per), offset, e, terms, te, tx)
    ref.mm_gradient_fwd(p, xyz, ks, eqs, list(n_per), grad)
    gks, geqs = [torch.zeros_like(k) for k in ks], [torch.zeros_like(eqs[0]), torch.zeros_like(eqs[1]), None, None]
    ref.mm_bwd(p, xyz, ks, eqs, list(n_per), offset, gE, gG, gks, geqs)
    _close(want["E"], e, "energy", 1e-10), _close(want["G"], grad, "dE/dx", 1e-10)
    for l in range(4):
        _close(want["te"][l], te[l], f"tuple energy {lv[l]}", 1e-10), _close(want["tx"][l], tx[l], f"internal coordinate {lv[l]}", 1e-10)
        _close(want["gk"][l], gks[l], f"gk {lv[l]}", 1e-9)
    for l in range(2):
        _close(want["geq"][l], geqs[l], f"geq {lv[l]}", 1e-9)


def test_gates_reject_what_they_must():
    want = torch.linspace(-1, 1, 50, dtype=D64).reshape(5, 10)
    kr.assert_el(want.float(), want, 1, 0.0, "fp32 rounding of the values")
    bad = want.clone()
    bad[3, 7] += 1e-5
    with pytest.raises(AssertionError):
        kr.assert_el(bad, want, 64, kr.rowmax(want), "one wrong element")
    with pytest.raises(AssertionError):
        kr.assert_el(torch.full_like(want, float("nan")), want, 64, 1.0, "non-finite")
    # calibrated gate: the same distance as the fp32 reference passes, a row 10x further fails; angles compare modulo 2 pi
    r32 = want + 1e-6
    kr.assert_calibrated(want + 1.5e-6, r32, want, 0, 1.0, "within 2x")
    worse = want + 1e-6
    worse[2] += 1e-5
    with pytest.raises(AssertionError):
        kr.assert_calibrated(worse, r32, want, 0, 1.0, "a row 10x further")
    ang = torch.tensor([[math.pi - 1e-7], [0.5]], dtype=D64)
    kr.assert_calibrated(torch.tensor([[-math.pi + 1e-7], [0.5]]), ang, ang, 64, 1.0, "branch cut", period=2 * math.pi)
    with pytest.raises(AssertionError):
        kr.assert_calibrated(torch.tensor([[-math.pi + 1e-7], [0.5]]), ang, ang, 64, 1.0, "branch cut without the period")
    # bf16: the rounding of the value passes, two steps off fails
    w = torch.randn(1000, generator=torch.Generator().manual_seed(0), dtype=D64)
    kr.close_bf16(w.to(kr.BF), w, "bf16 rounding")
    with pytest.raises(AssertionError):
        kr.close_bf16((w * (1 + 3 * 2.0 ** -7)).to(kr.BF), w, "three steps off")


@pytest.mark.parametrize("dummies", [False, True])
def test_loss_reference_against_ref_molwise_loss(ref, dummies):
    """kernel_refs.loss_ef_ref64 (the GPU loss tests' float64 reference) = cpu_ref.RefMolwiseLoss run in float64: the loss per molecule
    and, by autograd through RefMolwiseLoss, the gradients of the batch loss; its eval_se = RefBackend.eval_se on float64 inputs"""
    from grappa_amd.datasets import build_batch_from_pool
    from oracle.cpu_ref import RefMolwiseLoss
    C = 5
    g = build_batch_from_pool([300, 301, 302], n_confs=C, seed=2)
    B, N = g.num_nodes("g"), g.num_nodes("n1")
    sizes = g.batch_num_nodes("n1").long()
    gen = torch.Generator().manual_seed(7)
    e, er = torch.randn(B, C, generator=gen, dtype=D64) * 5 + 100, torch.randn(B, C, generator=gen, dtype=D64) * 5 - 40
    gr, grr = torch.randn(N, C, 3, generator=gen, dtype=D64) * 10, torch.randn(N, C, 3, generator=gen, dtype=D64) * 10
    dm = None
    if dummies:
        dm = torch.zeros(B, C, dtype=D64)
        dm[0, 3:] = 1
        dm[2, 1:] = 1
    wE, wG = 1.0, 0.8
    loss, gE, gG, se = kr.loss_ef_ref64(sizes, e, er, dm, gr, grr, wE, wG, 1.0 / B)
    e_, g_ = e.clone().requires_grad_(True), gr.clone().requires_grad_(True)
    g.nodes["g"].data["energy"], g.nodes["g"].data["energy_ref"] = e_, er
    g.nodes["n1"].data["gradient"], g.nodes["n1"].data["gradient_ref"] = g_, grr
    if dm is not None:
        g.nodes["g"].data["is_dummy"] = dm
    lf = RefMolwiseLoss(gradient_weight=wG, energy_weight=wE, param_weight=0.0)
    total = lf(g)
    gE_r, gG_r = torch.autograd.grad(total, (e_, g_))
    _close(loss, lf.last_per_molecule, "loss per molecule"), _close(gE, gE_r, "d/d energy"), _close(gG, gG_r, "d/d gradient")
    se_r = torch.zeros(B, 4, dtype=D64)

    class P:
        pass
    p = P()
    p.B, p.N, p.atom_molptr = B, N, torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).int()
    old = torch.get_default_dtype()
    torch.set_default_dtype(D64)          # (RefBackend.eval_se makes its sums with the default dtype)
    try:
        ref.eval_se(p, e, er, dm, gr, grr, se_r)
    finally:
        torch.set_default_dtype(old)
    _close(se, se_r, "eval_se")


# ----------------------------------------------------------------------------------------------------------------------------- dense products
import gemm_routes as gr  # noqa: E402


def _gemm_case(form, layout="fwd", M=70, N=52, K=96, arith="f32_f16x3"):
    return gr.Case("cpu", "gate", form, M, N, K, layout=layout, arith=arith, scaled=1)


@pytest.mark.parametrize("form,layout", [(f, lay) for f in gr.FORMS if f not in gr.BF16_FORMS and f != "h" for lay in ("fwd", "dgrad", "wgrad")
                                         if f != "l" or lay == "wgrad"])
def test_gemm_reference_agrees_with_the_ref_backend(ref, form, layout):
    """every epilogue form RefBackend.gemm takes (it has no res_ln_* and no bf16 tensors; a_colsum on the wgrad layout only), in float64 on
    the same inputs"""
    c = _gemm_case(form, layout)
    o = gr.operands(c)
    f = c.f
    C64, OUT64, cs64, _ = gr.reference(c, o, seed=77)
    d = lambda t: None if t is None else t.double()          # noqa: E731
    out = d(o["old"]).clone() if o["old"] is not None else torch.full((c.M, c.N), float("nan"), dtype=D64)
    out2 = torch.full((c.M, c.N), float("nan"), dtype=D64) if f["c2"] else None
    colsum = d(o["colsum_old"]).clone() if f["colsum"] else None
    first = out if not f["c2"] else torch.full((c.M, c.N), float("nan"), dtype=D64)
    ref.gemm(d(o["A"]), d(o["B"]), first, M=c.M, N=c.N, K=c.K, a_kcontig=layout != "wgrad", b_kcontig=layout == "fwd", bias=d(o["bias"]), res=d(o["res"]),
             aux=d(o["aux"]), pre=d(o["pre"]), act=f["act"], drop_p=float(np.float32(f["drop"])), drop_seed=77, accumulate=bool(f["acc"]), out2=out2, a_colsum=colsum)
    _close(OUT64, out2 if f["c2"] else first, f"OUT {form}")
    if f["c2"]:
        _close(C64, first, f"C {form}")
    if f["colsum"]:
        _close(cs64, colsum, "a_colsum")


def test_gemm_reference_res_ln_and_salt():
    """what RefBackend has no argument for: the residual recomputed from the rows before their LayerNorm equals the residual given
    normalised; the salt moves the seed by salt * 0x9E3779B97F4A7C15"""
    c = _gemm_case("h")
    o = gr.operands(c)
    _, with_ln, _, _ = gr.reference(c, o, seed=5)
    y = torch.nn.functional.layer_norm(o["res"].double(), (c.N,), o["ln"][2].double(), o["ln"][3].double(), 1e-5)
    _, plain, _ = kr.gemm_ref64(o["A"], o["B"], "fwd", bias=o["bias"], drop_p=c.f["drop"], drop_seed=5, res=y)
    assert float((with_ln - plain).abs().max()) < 1e-5          # (mean / rstd travel as fp32)
    _, salted, _ = kr.gemm_ref64(o["A"], o["B"], "fwd", bias=o["bias"], drop_p=0.25, drop_seed=5, drop_salt=3)
    _, moved, _ = kr.gemm_ref64(o["A"], o["B"], "fwd", bias=o["bias"], drop_p=0.25, drop_seed=(5 + 3 * kr.GOLDEN64) & ((1 << 64) - 1))
    _, unsalted, _ = kr.gemm_ref64(o["A"], o["B"], "fwd", bias=o["bias"], drop_p=0.25, drop_seed=5)
    assert torch.equal(salted, moved) and not torch.equal(salted, unsalted)


def _fp32_product(c, o, seed, a=None, keep_shift=0, res_before_drop=False):
    """the documented product in fp32 on the CPU (torch.matmul + the epilogue), with the faults the gate must catch"""
    from oracle.ops_ref import dropout_keep
    f = c.f
    a64, b64 = kr.gemm_operands64(o["A"], o["B"], c.layout)
    v = (a64.float() if a is None else a) @ b64.float().t()
    if o["pre"] is not None:
        v = v + o["pre"]
    if o["bias"] is not None:
        v = v + o["bias"]
    if f["act"]:
        v = torch.nn.functional.elu(v)
    if o["aux"] is not None:
        v = v * torch.where(o["aux"] > 0, torch.ones_like(v), o["aux"] + 1.0)
    if res_before_drop and o["res"] is not None:
        v = v + o["res"]
    if f["drop"] > 0:
        p = float(np.float32(f["drop"]))
        keep = dropout_keep(seed, torch.arange(c.M * c.N).view(c.M, c.N) + keep_shift, p)
        v = torch.where(keep, v * np.float32(1.0 / (1.0 - p)), torch.zeros_like(v))
    if not res_before_drop and o["res"] is not None:
        v = v + o["res"]
    if o["old"] is not None:
        v = v + o["old"]
    return v


def _hi_only(a64):
    """A with its low piece lost: the fp16 HI part under the row scale of include/grappa_hip.h (ABI 5), s = 141 - exponent field of the row maximum"""
    am = a64.abs().amax(1, keepdim=True).float()
    s = 141 - ((am.view(torch.int32) >> 23) & 0xff)
    scale = torch.exp2(s.double())
    return ((a64 * scale).to(torch.float16).double() / scale).float()


@pytest.mark.parametrize("arith", kr.FP32_GRADE)
@pytest.mark.parametrize("form,K", [("a", 6), ("d", 96), ("i", 400), ("g", 1104), ("d", 5000)])
def test_gemm_gate_is_sharp(arith, form, K):
    """on the sweep's own operand generator: the fp32 CPU product passes assert_gemm; a product whose A lost its low fp16 piece (what a dropped
    hi * lo term or a flushed denormal gives, ~2^-12), one element with the neighbouring column's bias, a keep mask shifted by one index and
    a residual added before the dropout all fail, under every fp32-grade arithmetic"""
    c = _gemm_case(form, M=96, N=64, K=K, arith=arith)
    o = gr.operands(c)
    _, OUT64, _, terms = gr.reference(c, o, seed=9)
    good = _fp32_product(c, o, 9)
    kr.assert_gemm(good, OUT64, terms, arith, "fp32 CPU product", gr.C_ACC)
    a64, _ = kr.gemm_operands64(o["A"], o["B"], c.layout)
    with pytest.raises(AssertionError):
        kr.assert_gemm(_fp32_product(c, o, 9, a=_hi_only(a64)), OUT64, terms, arith, "A without its low piece", gr.C_ACC)
    if c.f["bias"]:
        bad = good.clone()
        keep = terms["gain"] > 1.0
        m, n = (int(x) for x in torch.nonzero(keep)[5])
        bad[m, n] = bad[m, n] + (o["bias"][(n + 1) % c.N] - o["bias"][n]) * float(terms["gain"][m, n])
        with pytest.raises(AssertionError):
            kr.assert_gemm(bad, OUT64, terms, arith, "one element with its neighbour's bias", gr.C_ACC)
    if c.f["drop"] > 0:
        with pytest.raises(AssertionError):
            kr.assert_gemm(_fp32_product(c, o, 9, keep_shift=1), OUT64, terms, arith, "keep mask shifted by one", gr.C_ACC)
        with pytest.raises(AssertionError):
            kr.assert_gemm(_fp32_product(c, o, 9, res_before_drop=True), OUT64, terms, arith, "residual before the dropout", gr.C_ACC)


def test_c_acc_is_twice_the_cpu_references_error():
    """gemm_routes.C_ACC = 2 x the larger error of two fp32 CPU summation orders over every product of the table, in units of u32 S; the
    block-of-8 chain is deterministic and must reproduce its tabulated figure, torch.matmul's blocking depends on the CPU and must stay
    inside the gate it calibrates"""
    assert gr.C_ACC == 2.0 * max(gr.R_MATMUL, gr.R_CHAIN)
    r_mm, r_ch = gr.calibrate()
    assert gr.R_CHAIN - 0.01 <= r_ch <= gr.R_CHAIN, r_ch
    assert r_mm <= gr.C_ACC, r_mm


# ----------------------------------------------------------------------------------------------------------------------------- output maps, parameter loss
import head_loss_cases as hc  # noqa: E402


@pytest.mark.parametrize("name,kind,n_per,gated,cutoff", [("bond", 0, 0, False, 0.0), ("angle", 1, 0, False, 0.0), ("torsion", 2, 3, False, 1e-4),
                                                           ("torsion-gated", 2, 3, True, 1e-4)])
def test_param_out_reference(ref, name, kind, n_per, gated, cutoff):
    """kernel_refs.param_out_ref64 (forward stated directly, gradients by autograd) = RefBackend's forward, closed-form backward and
    statistics gradient on float64 inputs; the closed-form terms whose magnitudes scale the statistics gate sum to that gradient"""
    T, P = 40, 3
    nout = 2 if kind != 2 else (2 if gated else 1) * n_per
    gen = torch.Generator().manual_seed(kind + 5)
    consts = torch.tensor(kr.BOND_CONSTS if kind == 0 else kr.ANGLE_CONSTS) if kind != 2 else torch.cat([0.1 + torch.rand(n_per, generator=gen), torch.randn(n_per, generator=gen)])
    o, dk, deq = kr.param_out_case(kind, T, P, nout, consts.tolist(), 3, n_per, gated)
    if kind == 2:
        consts[n_per:] *= torch.tensor([0.0, 1.0, 1.0])          # (no k_mean on the first periodicity ...)
        o.view(P, T, nout)[:, :5] *= 1e-6                        # (... where these tuples take the cutoff branch)
    o, consts, dk, deq = o.double(), consts.double(), dk.double(), None if deq is None else deq.double()
    k64, eq64, do64, dc64 = kr.param_out_ref64(kind, o, T, P, n_per, gated, cutoff, consts, dk, deq)
    k = torch.empty(k64.shape, dtype=D64)
    eq = None if kind == 2 else torch.empty(T, dtype=D64)
    d_o, d_c = torch.empty(P * T, nout, dtype=D64), torch.empty(consts.numel(), dtype=D64)
    cut = float(np.float32(cutoff))
    ref.param_out_fwd(kind, o, T, P, n_per, gated, cut, consts, k, eq)
    ref.param_out_bwd(kind, o, T, P, n_per, gated, cut, consts, dk, deq, d_o)
    ref.param_out_bwd_stats(kind, o, T, P, n_per, gated, cut, consts, dk, deq, d_c)
    _close(k64, k, name + " k"), _close(do64, d_o, name + " d_o"), _close(dc64, d_c, name + " d_consts")
    if eq is not None:
        _close(eq64, eq, name + " eq")
    terms = kr.param_out_stat_terms64(kind, o, T, P, n_per, gated, cutoff, consts, dk, deq)
    assert float((terms.sum(0) - dc64).abs().max()) <= 1e-12 * float(terms.abs().sum(0).max()), name + ": the terms do not sum to d_consts"
    if kind == 2:
        assert bool((k64 == 0).any()) and bool((k64 != 0).any())
    # no upstream gradient, no tuples
    z = kr.param_out_ref64(kind, o, T, P, n_per, gated, cutoff, consts, None, None)
    assert bool((z[2] == 0).all()) and bool((z[3] == 0).all())
    e = kr.param_out_ref64(kind, o[:0], 0, P, n_per, gated, cutoff, consts, dk[:0], None)
    assert e[0].numel() == 0 and e[2].shape == (0, nout) and bool((e[3] == 0).all())


def test_loss_param_reference_against_ref_molwise_loss():
    """kernel_refs.loss_param_ref64 = cpu_ref.RefMolwiseLoss run in float64 with param_weight, param_weights_by_dataset and both
    regularisers, per molecule and through autograd; k_ref / eq_ref tables with NaN entries and an n4 reference narrower than k.  A
    molecule without a single tuple (den == 0) is the documented deviation: 0 here, NaN in the reference loop."""
    from grappa_amd.batch import batch, single_graph
    from grappa_amd.datasets import graph_from_pool
    from oracle.cpu_ref import RefMolwiseLoss
    empty = lambda s: np.zeros((0, s), dtype=np.int64)          # noqa: E731
    bare = single_graph(2, np.array([[0, 1]]), {"n2": empty(2), "n3": empty(3), "n4": empty(4), "n4_improper": empty(4)}, {"partial_charge": torch.zeros(2)})
    g = batch([bare] + [graph_from_pool(i, 1, 0) for i in (300, 301, 302)])
    B = g.batch_size
    gen = torch.Generator().manual_seed(21)
    T = {l: g.num_nodes(l) for l in ("n2", "n3", "n4", "n4_improper")}
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=D64)          # noqa: E731
    params = [700 + 100 * rn(T["n2"]), 1.2 + 0.1 * rn(T["n2"]), 100 + 20 * rn(T["n3"]), 1.9 + 0.1 * rn(T["n3"]), rn(T["n4"], 6), rn(T["n4_improper"], 3)]
    refs = [p * (1 + 0.01 * rn(*p.shape)) for p in params[:4]] + [rn(T["n4"], 4), rn(T["n4_improper"], 3)]
    refs[2][:7] = float("nan")
    refs[1][3] = float("nan")
    refs[4][2, 1] = float("nan")
    live = [p.clone().requires_grad_(True) for p in params]
    for (lvl, name), p, r in zip(hc_levels(), live, refs):
        g.nodes[lvl].data[name], g.nodes[lvl].data[name + "_ref"] = p, r
    dsnames = ["x", "a", "b", "x"]
    lf = RefMolwiseLoss(gradient_weight=0.0, energy_weight=0.0, param_weight=1e-3, param_weights_by_dataset={"a": 0.0, "b": 5e-3},
                        proper_regularisation=1e-3, improper_regularisation=2e-3)
    old = torch.get_default_dtype()
    torch.set_default_dtype(D64)          # (RefMolwiseLoss makes its sums and weights with the default dtype)
    try:
        total = lf(g, dsnames)
    finally:
        torch.set_default_dtype(old)
    grads = torch.autograd.grad(total, live)
    pw = torch.tensor([1e-3, 0.0, 5e-3, 1e-3], dtype=D64)
    ptrs = [g.plan().mol_ptr[l] for l in hc.LV6]
    fac, reg = hc.FAC, [0, 0, 0, 0, 1e-3, 2 * 2e-3]          # (the reference adds the improper regulariser twice)
    loss, gp = kr.loss_param_ref64(ptrs, params, refs[:5] + [None], fac, reg, pw, 1.0 / B)
    per_mol = lf.last_per_molecule
    assert bool(torch.isnan(per_mol[0])) and float(loss[0]) == 0.0, "den == 0: the reference loop's NaN is 0 here"
    _close(loss[1:], per_mol[1:], "parameter loss per molecule")
    assert float(loss[1]) > 0 and float(loss[2]) > float(loss[3]) * 0.1
    for l in range(6):
        assert bool(torch.isfinite(grads[l]).all())
        _close(gp[l], grads[l], f"d/d params[{l}]")
    # the scale of the gradients' gate bounds the gradient itself, and is 0 exactly where there is no term
    sc = kr.loss_param_grad_scales(ptrs, params, refs[:5] + [None], fac, reg, pw, 1.0 / B)
    for l in range(6):
        assert bool((gp[l].abs() <= sc[l] * (1 + 1e-12)).all()), l
    assert bool((sc[2][:7] == 0).all()) and bool((gp[2][:7] == 0).all())


def hc_levels():
    return [("n2", "k"), ("n2", "eq"), ("n3", "k"), ("n3", "eq"), ("n4", "k"), ("n4_improper", "k")]


def test_colsum_chain_and_charge_reference(ref):
    assert kr.colsum_chain(1) == (1, 3, 1) and kr.colsum_chain(64) == (64, 3, 1) and kr.colsum_chain(65) == (33, 2 + 2, 2)
    assert kr.colsum_chain(4096) == (64, 16 + 2, 64) and kr.colsum_chain(4097) == (64, (3 + 2) + (5 + 2 + 2), 65)
    assert kr.colsum_chain(32768) == (64, (4 + 2) + (8 + 2), 512) and kr.colsum_chain(40000)[::2] == (79, 507)
    from oracle.cpu_ref import charge_encoding
    q = torch.linspace(-4, 4, 33, dtype=D64)
    for lo, hi, dim in ((-2.0, 2.0, 16), (-1.0, 3.0, 2), (0.0, 1.0, 16)):
        old = torch.get_default_dtype()
        torch.set_default_dtype(D64)          # (cpu_ref.charge_encoding allocates with the default dtype)
        try:
            want = charge_encoding(q, dim, lo, hi)
        finally:
            torch.set_default_dtype(old)
        assert float((kr.charge_encoding_ref64(q, dim, lo, hi) - want).abs().max()) < 1e-6          # (its frequencies are made in fp32)


# every gate of tests/test_gpu_head_and_loss_domains.py is reachable by a correct fp32 implementation: the same checks on RefBackend, CPU
@pytest.mark.parametrize("name", list(hc.MAP_CONSTS))
def test_fp32_ref_backend_passes_the_map_gates(ref, name):
    base = name.split("-")[0]
    for T in (1, 255, 256, 257):
        for P in (1, 2, 3, 6):
            hc.check_param_out_map(ref, "cpu", name, T, P, 2 + (P % 2))
    for drop in ("dk", "deq", "both"):
        hc.check_param_out_map(ref, "cpu", base, 257, 2, 2, drop)
    hc.check_param_out_map(ref, "cpu", base, 0, 2, 2)


@pytest.mark.parametrize("gated", [False, True])
def test_fp32_ref_backend_passes_the_cutoff_checks(ref, gated):
    hc.check_torsion_cutoff(ref, "cpu", gated)


@pytest.mark.parametrize("name", list(hc.STATS_KINDS))
def test_fp32_ref_backend_passes_the_statistics_gate(ref, name):
    for T, P in ((1, 2), (257, 6), (1003, 2), (65537, 2)):
        hc.check_param_out_stats(ref, "cpu", name, T, P)


@pytest.mark.parametrize("name", hc.LOSS_PARAM_CASES)
def test_fp32_ref_backend_passes_the_loss_param_gates(ref, name):
    hc.check_loss_param(ref, ref, "cpu", name)


def test_fp32_ref_backend_passes_the_loss_ef_colsum_and_charge_gates(ref):
    for C in (1, 6):
        for wE, wG in ((1.0, 0.0), (0.0, 0.8), (1.0, 0.8)):
            hc.check_loss_ef_off(ref, ref, "cpu", C, wE, wG)
    for shape in hc.COLSUM_SHAPES + [(0, 12, 12)]:
        for acc in (False, True):
            hc.check_colsum(ref, "cpu", *shape, acc)
    for lo, hi in ((-2.0, 2.0), (-1.0, 3.0), (0.0, 1.0)):
        for dim in (2, 16):
            for N, col0 in ((0, 0), (1, 0), (257, 0), (257, 5)):
                hc.check_charge_encoding(ref, "cpu", lo, hi, dim, N, col0)


def test_the_new_gates_reject_what_they_must():
    """a statistics sum that lost one block's partial, a loss increment divided by the wrong count, a gradient off by 1e-3 relative"""
    kind, n_per, gated, cutoff, consts, o, dk, deq, want, scale = hc.stats_case("bond", 1003, 2)
    terms = kr.param_out_stat_terms64(kind, o, 1003, 2, n_per, gated, cutoff, consts, dk, deq)
    kr.assert_sum(want.float(), want, kr.param_out_stats_c(1003), scale, "fp32 rounding of the sums")
    with pytest.raises(AssertionError):
        kr.assert_sum(terms[256:].sum(0), want, kr.param_out_stats_c(1003), scale, "the first block's partial left out")
    with pytest.raises(AssertionError):
        kr.assert_sum(want * (1 + 1e-3), want, kr.param_out_stats_c(1003), scale, "off by 1e-3")
