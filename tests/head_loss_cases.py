"""The cases and checks of the output maps (bond / angle / torsion, their statistics gradients), the parameter loss, the off branches of
the energy / force loss, the column sums and the charge encoding -- shared by tests/test_gpu_head_and_loss_domains.py (HipBackend on the
GPU) and tests/test_kernel_domain_refs.py (the fp32 RefBackend on the CPU: every gate is reachable by a correct fp32 implementation).

Each check takes the backend under test and its device, runs the op into sentinel-guarded buffers and compares with the float64
references of tests/kernel_refs.py.  It returns the largest error / bound it saw (the figures the GPU file's docstring records)."""
import functools
import math

import numpy as np
import torch

import kernel_refs as kr

FILL = 1024.0       # sentinel behind and inside every output buffer (exact in fp32): a kernel writing where it must not changes it
LV6 = ["n2", "n2", "n3", "n3", "n4", "n4_improper"]


def guarded(n, dev, guard=64, fill=FILL):
    """-> (flat fp32 buffer, view of n elements) with `fill` before, in and after the view"""
    buf = torch.full((guard + n + guard,), fill, dtype=torch.float32, device=dev)
    return buf, buf[guard:guard + n]


def guard_ok(buf, n, guard=64):
    return bool((buf[:guard] == FILL).all()) and bool((buf[guard + n:] == FILL).all())


def _sync(dev):
    if str(dev).startswith("cuda"):
        torch.cuda.synchronize()


def _to(t, dev):
    return None if t is None else t.to(dev)


# =============================================================================================================== A. bond and angle maps
MAP_CONSTS = {"bond": kr.BOND_CONSTS, "angle": kr.ANGLE_CONSTS,
              # a non-zero minimum on both outputs; the angle with a negative std_over_max (a learnable statistic may change sign)
              "bond-min": [6.3, 0.1953, 0.05, 4.7, 161.2, 12.5], "angle-min-negs": [-0.0292, math.pi, 0.0, 3.97, 26.6, 12.5]}
MAP_KIND = {"bond": kr.OUT_BOND, "angle": kr.OUT_ANGLE, "bond-min": kr.OUT_BOND, "angle-min-negs": kr.OUT_ANGLE}


def check_param_out_map(be, dev, name, T, P, nout, drop=""):
    """forward and backward of one bond / angle case.  drop: "dk", "deq" or "both": no upstream gradient on that output"""
    kind = MAP_KIND[name]
    consts = torch.tensor(MAP_CONSTS[name], dtype=torch.float32)
    o, dk, deq = kr.param_out_case(kind, T, P, nout, MAP_CONSTS[name], seed=1000 * T + 10 * P + nout)
    if drop in ("dk", "both"):
        dk = None
    if drop in ("deq", "both"):
        deq = None
    k64, eq64, do64, _ = kr.param_out_ref64(kind, o, T, P, 0, False, 0.0, consts, dk, deq)
    kb, k = guarded(T, dev)
    eb, eq = guarded(T, dev)
    db, d_o = guarded(P * T * nout, dev)
    d_o = d_o.view(P * T, nout)
    be.param_out_fwd(kind, o.to(dev), T, P, 0, False, 0.0, consts.to(dev), k, eq)
    be.param_out_bwd(kind, o.to(dev), T, P, 0, False, 0.0, consts.to(dev), _to(dk, dev), _to(deq, dev), d_o)
    _sync(dev)
    what = f"{name} T={T} P={P} nout={nout} drop={drop or '-'}"
    assert guard_ok(kb, T) and guard_ok(eb, T) and guard_ok(db, P * T * nout), what + ": written outside the outputs"
    if T == 0:
        return 0.0
    sk, seq = kr.param_out_scales(kind, o, T, P, consts)
    sd = kr.param_out_grad_scale(kind, o, T, P, consts, dk, deq)
    kr.assert_el(k, k64, 32, sk, what + " k")
    kr.assert_el(eq, eq64, 32, seq, what + " eq")
    kr.assert_el(d_o, do64, 32, sd, what + " d_o")
    if nout > 2:
        assert bool((d_o[:, 2:] == 0).all()), what + ": the columns behind k and eq have no gradient"
    if dk is None:
        assert bool((d_o[:, 1] == 0).all()), what + ": dk = None"
    if deq is None:
        assert bool((d_o[:, 0] == 0).all()), what + ": deq = None"
    return max(kr.el_ratio(k, k64, 32, sk), kr.el_ratio(eq, eq64, 32, seq), kr.el_ratio(d_o, do64, 32, sd))


# =============================================================================================================== B. torsion cutoff at equality
CUTOFF = 2.0 ** -10


def cutoff_case(gated, classes=("at", "above", "below"), reps=2):
    """P = 2, n_per = 2, k_std = 1, k_mean = 0, cutoff = 2^-10.  Every tuple's two rows sum (exactly, in fp32 and in float64) to
    +-2^-10 ("at": |v| == cutoff), the next fp32 above or the next below; column 1 has the opposite sign of column 0.  Gated: the gate
    rows are 20 + 20, where the sigmoid is exactly 1 in fp32 and in float64.  -> o (2T, nout), dk (T, 2), consts, the class of each tuple"""
    second = {"at": 1.0, "above": 1.0 + 2.0 ** -22, "below": 1.0 - 2.0 ** -23}
    cls = [c for c in classes for _ in range(2)] * reps
    T, n_per = len(cls), 2
    nout = (2 if gated else 1) * n_per
    o = torch.zeros(2 * T, nout)
    for t, c in enumerate(cls):
        sign = 1.0 if t % 2 == 0 else -1.0
        for n in range(n_per):
            s = sign if n == 0 else -sign
            o[t, n], o[T + t, n] = s * 2.0 ** -11, s * 2.0 ** -11 * second[c]
            if gated:
                o[t, n_per + n] = o[T + t, n_per + n] = 20.0
    dk = torch.randn(T, n_per, generator=torch.Generator().manual_seed(11 + int(gated)))
    dk = torch.sign(dk) * (dk.abs() + 0.1)
    return o, dk, torch.tensor([1.0, 1.0, 0.0, 0.0]), cls


def check_torsion_cutoff(be, dev, gated):
    n_per, P = 2, 2
    o, dk, consts, cls = cutoff_case(gated)
    T, nout = len(cls), o.shape[1]
    kept = torch.tensor([c == "above" for c in cls])
    k64, _, do64, dc64 = kr.param_out_ref64(2, o, T, P, n_per, gated, CUTOFF, consts, dk, None)
    assert bool((k64[~kept] == 0).all()) and bool((k64[kept].abs() > CUTOFF).all()), "the reference cuts at and below the cutoff only"
    kb, k = guarded(T * n_per, dev)
    db, d_o = guarded(P * T * nout, dev)
    cb, d_c = guarded(2 * n_per, dev)
    k, d_o = k.view(T, n_per), d_o.view(P * T, nout)
    args = (2, o.to(dev), T, P, n_per, gated, CUTOFF, consts.to(dev))
    be.param_out_fwd(*args, k, None)
    be.param_out_bwd(*args, dk.to(dev), None, d_o)
    be.param_out_bwd_stats(*args, dk.to(dev), None, d_c)
    _sync(dev)
    what = f"cutoff at equality gated={gated}"
    assert guard_ok(kb, T * n_per) and guard_ok(db, P * T * nout) and guard_ok(cb, 2 * n_per), what + ": written outside the outputs"
    # every kept value is the exact fp32 sum of its two rows: the forward is exact, not merely close
    assert torch.equal(k.cpu().double(), k64), what + ": k"
    cut_rows = (~kept).repeat(P)
    assert bool((d_o[cut_rows.to(dev)] == 0).all()), what + ": a cut element has a gradient"
    assert bool((d_o[kept.repeat(P).to(dev)][:, :n_per] != 0).all()), what + ": a kept element has none"
    kr.assert_el(d_o, do64, 32, kr.rowmax(do64), what + " d_o")
    terms = kr.param_out_stat_terms64(2, o, T, P, n_per, gated, CUTOFF, consts, dk, None)
    assert bool((terms[~kept] == 0).all())
    kr.assert_sum(d_c, dc64, kr.param_out_stats_c(T), terms.abs().sum(0), what + " d_consts")
    # ... and with nothing but cut elements the statistics get exactly nothing
    o2, dk2, _, cls2 = cutoff_case(gated, classes=("at", "below"))
    T2 = len(cls2)
    cb2, d_c2 = guarded(2 * n_per, dev)
    be.param_out_bwd_stats(2, o2.to(dev), T2, P, n_per, gated, CUTOFF, consts.to(dev), dk2.to(dev), None, d_c2)
    _sync(dev)
    assert guard_ok(cb2, 2 * n_per) and bool((d_c2 == 0).all()), what + ": cut elements reach the statistics"


# =============================================================================================================== C. statistics gradients
STATS_KINDS = {"bond": (kr.OUT_BOND, 0, False), "angle": (kr.OUT_ANGLE, 0, False),
               "torsion-nper1": (2, 1, False), "torsion-nper6": (2, 6, False), "torsion-nper8": (2, 8, False),
               "torsion-nper1-gated": (2, 1, True), "torsion-nper6-gated": (2, 6, True), "torsion-nper8-gated": (2, 8, True)}
STATS_CUTOFF = 1e-4


@functools.lru_cache(maxsize=4)
def stats_case(name, T, P):
    """inputs (fp32, CPU) and the float64 reference of one statistics case, computed once: randn rows plus the saturation rows of the
    maps (kernel_refs.param_out_case).  Torsions run with the hard cutoff 1e-4; a tuple whose |k| is within 2^-16 (relative to the
    magnitudes it is made of) of the cutoff, where fp32 and float64 could take different sides, has its rows zeroed."""
    kind, n_per, gated = STATS_KINDS[name]
    seed = 7 * T + P + 100 * n_per + int(gated)
    gen = torch.Generator().manual_seed(seed)
    if kind == 2:
        nout, cutoff = (2 if gated else 1) * n_per, STATS_CUTOFF
        consts = torch.cat([0.1 + torch.rand(n_per, generator=gen), torch.randn(n_per, generator=gen)])
    else:
        nout, cutoff = 2, 0.0
        consts = torch.tensor(kr.BOND_CONSTS if kind == kr.OUT_BOND else kr.ANGLE_CONSTS, dtype=torch.float32)
    o, dk, deq = kr.param_out_case(kind, T, P, nout, consts.tolist(), seed, n_per, gated)
    if kind == 2 and T:
        c64 = o.double().view(P, T, nout).sum(0)
        a64 = o.double().abs().view(P, T, nout).sum(0)
        cst = consts.double()
        v = c64[:, :n_per] * (torch.sigmoid(c64[:, n_per:]) if gated else 1.0) * cst[:n_per] + (0.0 if gated else cst[n_per:])
        mag = a64[:, :n_per] * cst[:n_per].abs() + cst[n_per:].abs() + cutoff
        near = ((v.abs() - float(np.float32(cutoff))).abs() < 2.0 ** -16 * mag).any(1)
        o.view(P, T, nout)[:, near, :n_per] = 0.0
    want = kr.param_out_ref64(kind, o, T, P, n_per, gated, cutoff, consts, dk, deq)[3]
    scale = kr.param_out_stat_terms64(kind, o, T, P, n_per, gated, cutoff, consts, dk, deq).abs().sum(0)
    return kind, n_per, gated, cutoff, consts, o, dk, deq, want, scale


def check_param_out_stats(be, dev, name, T, P):
    kind, n_per, gated, cutoff, consts, o, dk, deq, want, scale = stats_case(name, T, P)
    ncst = consts.numel()
    o_d, c_d, dk_d, deq_d = o.to(dev), consts.to(dev), _to(dk, dev), _to(deq, dev)
    runs = []
    for _ in range(2):
        cb, d_c = guarded(ncst, dev)          # (dirty: the sentinel)
        be.param_out_bwd_stats(kind, o_d, T, P, n_per, gated, cutoff, c_d, dk_d, deq_d, d_c)
        _sync(dev)
        assert guard_ok(cb, ncst), f"{name} T={T}: written outside d_consts"
        runs.append(d_c.cpu().clone())
    what = f"statistics gradient {name} T={T} P={P}"
    assert torch.equal(runs[0], runs[1]), what + ": two runs differ (the order of the sum is fixed)"
    if T == 0:
        assert bool((runs[0] == 0).all()), what + ": T = 0 leaves zeros"
        return 0.0
    return kr.assert_sum(runs[0], want, kr.param_out_stats_c(T), scale, what)


# =============================================================================================================== D. parameter loss
def _chain(n):
    i = np.arange(n)
    return {"n2": np.stack([i[:-1], i[1:]], 1), "n3": np.stack([i[:-2], i[1:-1], i[2:]], 1),
            "n4": np.stack([i[:-3], i[1:-2], i[2:-1], i[3:]], 1), "n4_improper": np.zeros((0, 4), dtype=np.int64)}


@functools.lru_cache(maxsize=1)
def loss_param_batch():
    """a 258-atom chain (257 bonds, 256 angles, 255 torsions, no impropers: the strided loop's edges and an empty level), a 2-atom
    molecule (one bond, nothing else), a 5-atom molecule with one improper, two pool molecules"""
    from grappa_amd.batch import batch, single_graph
    from grappa_amd.datasets import graph_from_pool
    n1 = lambda n: {"partial_charge": torch.zeros(n)}          # noqa: E731
    empty = lambda s: np.zeros((0, s), dtype=np.int64)         # noqa: E731
    chain = single_graph(258, _chain(258)["n2"], _chain(258), n1(258))
    two = single_graph(2, np.array([[0, 1]]), {"n2": [[0, 1]], "n3": empty(3), "n4": empty(4), "n4_improper": empty(4)}, n1(2))
    five = single_graph(5, np.array([[0, 1], [1, 2], [2, 3], [2, 4]]),
                        {"n2": [[0, 1], [1, 2], [2, 3], [2, 4]], "n3": [[0, 1, 2], [1, 2, 3], [1, 2, 4], [3, 2, 4]],
                         "n4": [[0, 1, 2, 3], [0, 1, 2, 4]], "n4_improper": [[1, 3, 2, 4]]}, n1(5))
    g = batch([chain, two, five, graph_from_pool(300, 1, 0), graph_from_pool(301, 1, 0)])
    assert g._bnn["n2"][0] == 257 and g._bnn["n3"][0] == 256 and g._bnn["n4"][0] == 255 and g._bnn["n4_improper"][0] == 0
    return g


FAC = [1e-3, 1.0, 1e-2, 1.0, 1e-4, 1.0]          # MolwiseLoss' default weights {"n2_k": 1e-3, "n3_k": 1e-2, "n4_k": 1e-4}
LOSS_PARAM_CASES = ["all-refs-working-regime", "all-refs-randn", "improper-p-without-ref-or-reg", "angle-k-ref-nan-for-the-chain",
                    "bond-eq-ref-all-nan", "no-refs-reg-only", "pw-zero-entry", "pw-none", "no-improper-params", "gps-level-none",
                    "reg-both-torsion-levels", "width-4-2-ref-wider-6", "width-4-2-ref-narrower-3"]


def loss_param_case(name):
    """-> params, refs, fac, reg, pw, the levels whose gradient is not asked for"""
    g = loss_param_batch()
    Ts = [g.num_nodes(l) for l in LV6]
    B = g.batch_size
    gen = torch.Generator().manual_seed(LOSS_PARAM_CASES.index(name))
    widths = [1, 1, 1, 1, 4, 2] if name.startswith("width-4-2") else [1, 1, 1, 1, 6, 3]
    rn = lambda *s: torch.randn(*s, generator=gen)          # noqa: E731
    params = [700 + 100 * rn(Ts[0]), 1.2 + 0.1 * rn(Ts[1]), 100 + 20 * rn(Ts[2]), 1.9 + 0.1 * rn(Ts[3]), rn(Ts[4], widths[4]), rn(Ts[5], widths[5])]
    if name == "all-refs-randn":
        refs = [rn(*p.shape) for p in params]
    else:
        refs = [p * (1 + 0.01 * rn(*p.shape)) for p in params]           # within 1 % of the parameters: the working regime
    if name not in ("all-refs-working-regime", "all-refs-randn"):
        refs[5] = None                                                    # (as MolwiseLoss: impropers never enter the MSE)
    reg = [0.0] * 6
    pw = torch.full((B,), 1e-3)
    no_grad = []
    if name == "angle-k-ref-nan-for-the-chain":
        refs[2][:256] = float("nan")
    elif name == "bond-eq-ref-all-nan":
        refs[1][:] = float("nan")
    elif name == "no-refs-reg-only":
        refs, reg = [None] * 6, [0, 0, 0, 0, 1e-3, 2e-3]
    elif name == "pw-zero-entry":
        pw[0], pw[3] = 0.0, 0.0
        reg = [0, 0, 0, 0, 1e-3, 0]
    elif name == "pw-none":
        pw, reg = None, [0, 0, 0, 0, 0, 2e-3]
    elif name == "no-improper-params":
        params[5] = None
    elif name == "gps-level-none":
        no_grad = [2]
    elif name == "reg-both-torsion-levels":
        reg = [0, 0, 0, 0, 1e-3, 2e-3]
    elif name == "width-4-2-ref-wider-6":
        refs[4] = rn(Ts[4], 6)
    elif name == "width-4-2-ref-narrower-3":
        refs[4] = rn(Ts[4], 3)
        refs[4][5, 1] = float("nan")
    return params, refs, FAC, reg, pw, no_grad


def check_loss_param(be, ref, dev, name):
    """be: the backend under test on dev; ref: the fp32 RefBackend (the calibration of the loss gate, run on the CPU)"""
    g = loss_param_batch()
    pc = g.plan()
    pd = pc if dev == "cpu" else g.to(dev).plan()
    B, inv_B = pc.B, 1.0 / pc.B
    params, refs, fac, reg, pw, no_grad = loss_param_case(name)
    ptrs = [pc.mol_ptr[l] for l in LV6]
    inc64, gp64 = kr.loss_param_ref64(ptrs, params, refs, fac, reg, pw, inv_B)
    scales = kr.loss_param_grad_scales(ptrs, params, refs, fac, reg, pw, inv_B)
    lm32 = torch.zeros(B)
    ref.loss_param(pc, params, refs, fac, reg, pw, inv_B, lm32, [None if p is None else torch.zeros_like(p) for p in params])
    what = f"loss_param {name}"
    got = {}
    for fill in (0.0, 3.0):
        lb, lm = guarded(B, dev)
        lm.fill_(fill)
        bufs = [guarded(params[l].numel() if params[l] is not None else 8, dev) for l in range(6)]
        gps = [None if l in no_grad else (b[1] if params[l] is None else b[1].view(params[l].shape)) for l, b in enumerate(bufs)]
        be.loss_param(pd, [_to(p, dev) for p in params], [_to(r, dev) for r in refs], fac, reg, _to(pw, dev), inv_B, lm, gps)
        _sync(dev)
        assert guard_ok(lb, B), what + ": written outside loss_mol"
        for l, (b, v) in enumerate(bufs):
            assert guard_ok(b, v.numel()), what + f": written outside gps[{l}]"
            if params[l] is None or l in no_grad:
                assert bool((v == FILL).all()), what + f": level {l} has no table / no gradient buffer and must stay untouched"
        got[fill] = (lm.cpu().clone(), [None if gp is None else gp.cpu().clone() for gp in gps])
    inc, gp = got[0.0]
    # loss_mol += loss: one fp32 addition onto what was there -- bit for bit the increment of the zero-filled run added to 3
    assert torch.equal(got[3.0][0], torch.full((B,), 3.0) + inc), what + ": loss_mol is not 3 + increment"
    assert all(a is None or torch.equal(a, b) for a, b in zip(gp, got[3.0][1])), what + ": the gradients depend on loss_mol"
    kr.assert_calibrated(inc, lm32, inc64, 256, inc64.abs(), what + " loss_mol increment")
    # the same gate on loss_mol - 3, with the one rounding of the addition onto 3 (u32 (3 + |increment|)) on its floor
    kr.assert_calibrated(got[3.0][0] - 3.0, lm32, inc64, 256, inc64.abs() + (3.0 + inc64.abs()) / 256.0, what + " loss_mol - 3")
    worst = 0.0
    for l in range(6):
        if params[l] is None or l in no_grad:
            continue
        kr.assert_el(gp[l], gp64[l], 16, scales[l], what + f" gps[{l}]")
        assert bool((gp[l][scales[l] == 0] == 0).all()), what + f": gps[{l}] of an element without an MSE or regulariser term"
        worst = max(worst, kr.el_ratio(gp[l], gp64[l], 16, scales[l]))
    return worst


# =============================================================================================================== E. loss_ef off branches
class _LossPlan:
    def __init__(self, sizes, dev):
        self.B, self.N = len(sizes), int(sum(sizes))
        self.atom_molptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)


def check_loss_ef_off(be, ref, dev, C, wE, wG):
    """B = 3 with a one-atom molecule; an off side (wE == 0 or wG == 0) must zero-fill its gradient buffer.  Dummy conformations
    (C = 6) on the off-branch cases only"""
    sizes = [1, 4, 3]
    pc, pd = _LossPlan(sizes, "cpu"), _LossPlan(sizes, dev)
    B, N = pc.B, pc.N
    gen = torch.Generator().manual_seed(10 * C + int(wE != 0) + 2 * int(wG != 0))
    e, er = torch.randn(B, C, generator=gen) * 5 + 100, torch.randn(B, C, generator=gen) * 5 - 40
    gr, grr = torch.randn(N, C, 3, generator=gen) * 10, torch.randn(N, C, 3, generator=gen) * 10
    dm = None
    if C > 1 and (wE == 0 or wG == 0):
        dm = torch.zeros(B, C)
        dm[1, 4:] = 1
    inv_B = 1.0 / B
    l64, gE64, gG64, _ = kr.loss_ef_ref64(sizes, e, er, dm, gr, grr, wE, wG, inv_B)
    l32, gE32, gG32 = torch.zeros(B), torch.zeros(B, C), torch.zeros(N, C, 3)
    ref.loss_ef(pc, e, er, dm, gr, grr, wE, wG, inv_B, l32, gE32, gG32)
    lb, lm = guarded(B, dev)
    eb, gE = guarded(B * C, dev)
    gb, gG = guarded(N * C * 3, dev)
    gE, gG = gE.view(B, C), gG.view(N, C, 3)
    be.loss_ef(pd, e.to(dev), er.to(dev), _to(dm, dev), gr.to(dev), grr.to(dev), wE, wG, inv_B, lm, gE, gG)
    _sync(dev)
    what = f"loss_ef C={C} wE={wE} wG={wG}"
    assert guard_ok(lb, B) and guard_ok(eb, B * C) and guard_ok(gb, N * C * 3), what + ": written outside the outputs"
    if wE == 0:
        assert bool((gE == 0).all()), what + ": gE of the energy term switched off"
    if wG == 0:
        assert bool((gG == 0).all()), what + ": gG of the force term switched off"
    if C == 1:
        assert bool((gE == 0).all()), what + ": one conformation, the centred energy difference is exactly 0"
    # the gates of test_gpu_kernel_domains.test_loss_and_eval_strided_loops_against_float64
    kr.assert_calibrated(lm, l32, l64, 256, l64.abs(), what + " loss_mol")
    m = torch.ones(B, C, dtype=torch.float64) if dm is None else (dm == 0).double()
    nreal = m.sum(1, keepdim=True)
    kr.assert_el(gE, gE64, 64, 2 * wE * inv_B / nreal * (kr.rowmax(e) + kr.rowmax(er)), what + " gE")
    cnt = torch.tensor(sizes, dtype=torch.float64)
    seg = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))
    fac = (inv_B * wG * 2.0 / (cnt * nreal[:, 0] * 3.0))[seg][:, None, None]
    kr.assert_el(gG, gG64, 8, fac * (gr.double().abs() + grr.double().abs()), what + " gG")


# =============================================================================================================== F. column sums
COLSUM_SHAPES = [(1, 4, 4), (63, 300, 300), (64, 301, 304), (65, 7, 12), (513, 130, 132), (4096, 8, 8), (4097, 8, 8), (32768, 8, 8),
                 (32769, 8, 8), (40000, 5, 8)]


def colsum_id(M, N, ldx):
    rpb, chain, used = kr.colsum_chain(M)
    return f"colsum-M{M}-N{N}-ld{ldx}-blocks{used}x{rpb}rows-{'two' if used > 64 else 'one'}stage"


def check_colsum(be, dev, M, N, ldx, accumulate):
    gen = torch.Generator().manual_seed(M + N)
    x = torch.randn(M, N, generator=gen)
    old = torch.randn(N, generator=gen) + 2.0
    buf = torch.full((M, ldx), FILL, device=dev)          # the columns behind N hold the sentinel: it must not leak into the sums
    xv = buf[:, :N]
    xv.copy_(x)
    ob, out = guarded(N, dev)
    out.copy_(old)
    be.colsum(xv, out, accumulate=accumulate)
    _sync(dev)
    what = f"colsum M={M} N={N} ldx={ldx} accumulate={accumulate}"
    assert guard_ok(ob, N), what + ": written outside out"
    assert bool((buf[:, N:] == FILL).all()) and torch.equal(xv.cpu(), x), what + ": x changed"
    if M == 0:
        assert torch.equal(out.cpu(), old if accumulate else torch.zeros(N)), what
        return 0.0
    want = x.double().sum(0) + (old.double() if accumulate else 0.0)
    terms = x.double().abs().sum(0) + (old.double().abs() if accumulate else 0.0)
    rpb, chain, _ = kr.colsum_chain(M)
    return kr.assert_sum(out, want, rpb + chain + 8, terms, what)


# =============================================================================================================== G. charge encoding
def check_charge_encoding(be, dev, lo, hi, dim, N, col0):
    span = hi - lo
    if N == 1:
        q = torch.tensor([hi + 1.0])
    else:
        q = torch.linspace(lo - 0.75 * span, hi + 0.75 * span, N)          # below lo, inside, above hi ...
        if N >= 4:
            q[1], q[2], q[N // 2], q[N - 2] = lo, hi, lo, hi               # ... and exactly at both ends
    W = col0 + dim + 3
    ob, out = guarded(N * W, dev)
    out = out.view(N, W)
    be.charge_encoding(q.to(dev), dim, lo, hi, out, col0)
    _sync(dev)
    what = f"charge_encoding [{lo}, {hi}] dim={dim} N={N} col0={col0}"
    assert guard_ok(ob, N * W), what + ": written outside out"
    assert bool((out[:, :col0] == FILL).all()) and bool((out[:, col0 + dim:] == FILL).all()), what + ": the other columns changed"
    if N == 0:
        return
    want = kr.charge_encoding_ref64(q, dim, lo, hi)
    if N >= 4:          # the quirk the encoding is trained with: the clamped range maps to [(lo + hi) / span, 2 hi / span], not to [0, 1]
        assert float(want[1, 0]) == math.sin((lo + hi) / span) and float(want[2, 0]) == math.sin(2 * hi / span)
        assert torch.equal(want[0], want[1]) and torch.equal(want[N - 1], want[N - 2]), "clamped on both sides"
    kr.assert_el(out[:, col0:col0 + dim], want, 16, 1.0, what)
