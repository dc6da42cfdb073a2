"""CPU: the references and gates of tests/writer_layer_refs.py (what tests/test_gpu_writer_layer_rows.py asserts the fused writer-head layer
with).  The float64 forward and its gradients agree with oracle/cpu_ref.TransformerLayer, the explicit backward chain with autograd; the two
fp32 restatements pass the row gates when each is calibrated by the other alone (the condition under which the gates are admissible); the
gates reject every mutant.  Whether the gates of tests/test_gpu_writer_layer.py (_close_bf16, 2e-2 of the largest magnitude) would have let
mutants (i), (ii), (iv), (vi) through was tried at s*T ~ 1000: they catch all four there, the figures stand beside each mutant."""
import functools

import pytest
import torch

import writer_layer_refs as wl

D64 = torch.float64
F = wl.F
CALIBRATION_CASES = [(s, T, p, False) for s, T in wl.CASES for p in (0.0, 0.3)] + [(s, 64 // s + 1, 0.0, True) for s in (2, 3, 4)]


def _close(a, b, what, tol=1e-10):
    a, b = a.double(), b.double()
    err = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)
    assert err < tol, f"{what}: {err:.3e}"


@functools.lru_cache(maxsize=4)
def _both(s, T, p, degenerate=False):
    """inputs, masks, float64 truth and the two restatements of the forward, and of the backward run on restatement a's saves"""
    if degenerate:
        T = max(T, 4)
    x, dout = wl.inputs(s, T, degenerate)
    P = wl.params()
    k1, k2 = wl.keep_masks(s, T, p)
    f64, fa, fb = wl.fwd64(x, P, s, T, p, k1, k2), wl.fwd32a(x, P, s, T, p), wl.fwd32b(x, P, s, T, p, k1, k2)
    sv = dict(fa, x=x)
    b64 = wl.with_partials(wl.bwd64(dout, sv, P, s, T, p, k1, k2), s, T)
    ba = wl.with_partials(wl.bwd32a(dout, sv, P, s, T, p, k1, k2), s, T)
    bb = wl.with_partials(wl.bwd32b(dout, sv, P, s, T, p, k1, k2), s, T, reverse=True)
    return dict(x=x, dout=dout, P=P, k1=k1, k2=k2, f64=f64, fa=fa, fb=fb, sv=sv, b64=b64, ba=ba, bb=bb, T=T)


# ----------------------------------------------------------------------------------------------------------------------------- a. cross-checks
@pytest.mark.parametrize("s", [2, 3, 4])
def test_float64_layer_equals_the_oracle_layer(s):
    """forward and autograd of writer_layer_refs.layer_fwd == oracle/cpu_ref.TransformerLayer in float64 (eval, p = 0)"""
    from oracle import cpu_ref
    T = 64 // s + 1
    x, dout = wl.inputs(s, T)
    P = wl.params()
    out, dx, g = wl.autograd64(x, P, dout, s, T)
    ref = cpu_ref.TransformerLayer(F, 8, F, 0.0).double()
    names = {"n1_w": "norm1.weight", "n1_b": "norm1.bias", "w_in": "attn.in_proj_weight", "b_in": "attn.in_proj_bias", "w_o": "attn.out_proj.weight",
             "b_o": "attn.out_proj.bias", "nf_w": "ff.norm1.weight", "nf_b": "ff.norm1.bias", "w1": "ff.linear1.weight", "b1": "ff.linear1.bias",
             "w2": "ff.linear2.weight", "b2": "ff.linear2.bias"}
    ref.load_state_dict({names[n]: P[n].double() for n in wl.ORDER})
    ref.eval()
    xr = x.double().view(s, T, F).clone().requires_grad_(True)
    yr = ref(xr)
    (yr * dout.double().view(s, T, F)).sum().backward()
    _close(out, yr.detach().view(s * T, F), "out")
    _close(dx, xr.grad.view(s * T, F), "dx")
    rp = dict(ref.named_parameters())
    for n in wl.ORDER:
        _close(g[n], rp[names[n]].grad, n)


@pytest.mark.parametrize("s,p", [(2, 0.0), (3, 0.3), (4, 0.0), (4, 0.3)])
def test_explicit_chain_equals_autograd(s, p):
    """the header's backward chain on the float64 forward's own tensors: dx, and through the by-products and the summed per-tile partials
    all twelve parameter gradients, equal autograd's"""
    T = 64 // s + 1
    x, dout = wl.inputs(s, T)
    P = wl.params()
    k1, k2 = wl.keep_masks(s, T, p)
    f64 = wl.fwd64(x, P, s, T, p, k1, k2)
    bw = wl.with_partials(wl.bwd64(dout, dict(f64, x=x), P, s, T, p, k1, k2), s, T)
    _, dx, g = wl.autograd64(x, P, dout, s, T, p, k1, k2)
    _close(bw["dx"], dx, "dx")
    mine = wl.param_grads(bw, f64)
    for n in wl.ORDER:
        _close(mine[n], g[n], n)
    assert bw["lnf_part"].shape == (wl.tiles(s, T), 2, F) and wl.tiles(s, T) == 2


@pytest.mark.parametrize("s", [3, 4])
def test_gathered_layer_is_the_layer_behind_its_first_two_stages(s):
    T = 64 // s + 1
    x, dout = wl.inputs(s, T)
    P = wl.params()
    f64 = wl.fwd64(x, P, s, T, 0.0, None, None)
    g64 = wl.fwd64(None, P, s, T, 0.0, None, None, gathered=(f64["x1"], f64["qkv"]))
    for n in ("att", "x2", "x3", "u", "out"):
        assert torch.equal(g64[n], f64[n]), n
    bw = wl.bwd64(dout, dict(f64, x=x), P, s, T, 0.0, None, None)
    bg = wl.bwd64(dout, dict(f64, x=x), P, s, T, 0.0, None, None, gather=True)
    assert torch.equal(bg["dqkv"], bw["dqkv"]) and torch.equal(bg["dx"], bw["dx2"]) and "ln1_rows" not in bg


def test_tile_rows_cover_every_token_once():
    for s, T in wl.CASES:
        rows = torch.cat([wl.tile_rows(s, T, b) for b in range(wl.tiles(s, T))])
        assert sorted(rows.tolist()) == list(range(s * T)), (s, T)
        assert wl.tile_rows(s, T, 0)[:2].tolist() == ([0, 1] if T > 1 else [0, T])


# ----------------------------------------------------------------------------------------------------------------------------- b. calibration
@pytest.mark.parametrize("s,T,p,degenerate", CALIBRATION_CASES)
def test_each_restatement_passes_the_gates_calibrated_by_the_other_alone(s, T, p, degenerate):
    c = _both(s, T, p, degenerate)
    x64, T = c["x"].double(), c["T"]
    for got, cal, tag in ((c["fb"], c["fa"], "b by a"), (c["fa"], c["fb"], "a by b")):
        wl.check_fwd(got, cal, None, c["f64"], x64, f"forward {tag}")
    for got, cal, tag in ((c["bb"], c["ba"], "b by a"), (c["ba"], c["bb"], "a by b")):
        wl.check_bwd(got, cal, None, c["b64"], s, T, f"backward {tag}")
    for r in (c["fa"], c["fb"], c["ba"], c["bb"]):
        assert all(bool(torch.isfinite(v).all()) for v in r.values() if torch.is_tensor(v))


@pytest.mark.parametrize("s", [3, 4])
def test_restatements_calibrate_each_other_behind_a_gather_with_repeats(s):
    T = 3 * (64 // s) + 1
    idx, x1_tab, qkv_tab = wl.gather_case(s, T)
    assert idx.unique().numel() < idx.numel()             # repeats
    rows = idx.t().reshape(-1)
    tabs = (x1_tab[rows], qkv_tab[rows])
    P, (k1, k2) = wl.params(), wl.keep_masks(s, T, 0.3)
    g64 = wl.fwd64(None, P, s, T, 0.3, k1, k2, gathered=tabs)
    ga, gb = wl.fwd32a_gathered(P, s, T, 0.3, k1, k2, tabs), wl.fwd32b(None, P, s, T, 0.3, k1, k2, gathered=tabs)
    names = ("att", "x2", "meanf", "rstdf", "x3", "u", "out")
    wl.check_fwd(gb, ga, None, g64, None, "gather b by a", names=names)
    wl.check_fwd(ga, gb, None, g64, None, "gather a by b", names=names)


# ----------------------------------------------------------------------------------------------------------------------------- c. mutants
BIG = {2: 16 * 32 + 1, 3: 16 * 21 + 1, 4: 16 * 16 + 1}          # s*T >= 1000, the last tile ragged (one tuple)


@functools.lru_cache(maxsize=2)
def _big(s, p=0.0):
    return _both(s, BIG[s], p)


def _new_gates_reject_fwd(c, mutant, s):
    with pytest.raises(AssertionError):
        wl.check_fwd(mutant, c["fa"], c["fb"], c["f64"], c["x"].double(), "mutant")


def _new_gates_reject_bwd(c, mutant, s, names=None):
    with pytest.raises(AssertionError):
        wl.check_bwd(mutant, c["ba"], c["bb"], c["b64"], s, c["T"], "mutant", names=names)


@pytest.mark.parametrize("s", [3, 4])
def test_mutant_i_dropped_last_partial(s):
    c = _big(s)
    m = wl.mutant_i(c["bb"], s, c["T"])
    _new_gates_reject_bwd(c, m, s, names=("lnf_part",))
    _new_gates_reject_bwd(c, m, s, names=("ln1_part",))
    # (not invisible to the old gates at this size: a tile's contribution to a sum over K rows falls like 1 / sqrt(K), not 1 / K, and the gate
    #  takes the largest of 512 columns -- nf_w is off by 7.9 % (s = 3) and 8.2 % (s = 4) of its largest magnitude at ~1000 rows, above 2e-2)
    _new_gates_reject_bwd(_both(s, 64 // s + 1, 0.0), wl.mutant_i(_both(s, 64 // s + 1, 0.0)["bb"], s, 64 // s + 1), s)      # ... and at a table case


@pytest.mark.parametrize("s", [3, 4])
def test_mutant_ii_swapped_heads(s):
    c = _big(s)
    T = c["T"]
    m = wl.fwd32b(c["x"], c["P"], s, T, 0.0, None, None, hook=wl.mutant_ii_hook(s, T))
    _new_gates_reject_fwd(c, m, s)
    for n in ("att", "x2", "out"):
        with pytest.raises(AssertionError):
            wl.check_fwd(m, c["fa"], c["fb"], c["f64"], c["x"].double(), "mutant", names=(n,))
    # (the old gates see this one too: the swapped heads differ by the tensor's own magnitude, 155 to 195 times _close_bf16's bound on att)


@pytest.mark.parametrize("s", [3, 4])
def test_mutant_iii_missing_bias_in_one_tile(s):
    T = 3 * (64 // s) + 1
    c = _both(s, T, 0.0)
    for tile in (1, wl.tiles(s, T) - 1):
        m = wl.fwd32b(c["x"], c["P"], s, T, 0.0, None, None, hook=wl.mutant_iii_hook(s, T, c["P"], tile))
        _new_gates_reject_fwd(c, m, s)


@pytest.mark.parametrize("s", [3, 4])
def test_mutant_iv_row_63_leaks_into_dbeta(s):
    c = _big(s)
    m = wl.mutant_iv(c["bb"], s, c["T"], 3)
    _new_gates_reject_bwd(c, m, s, names=("lnf_part",))
    _new_gates_reject_bwd(c, m, s, names=("ln1_part",))
    # (caught by the old gates at this size as well: one more row moves nf_b by 3.0 % (s = 3) and 2.5 % (s = 4) of its largest magnitude)


@pytest.mark.parametrize("s", [2, 4])
def test_mutant_v_mask_at_the_column_index(s):
    T = 3 * (64 // s) + 1
    c = _both(s, T, 0.3)
    for tile in (0, wl.tiles(s, T) - 1):
        k1, k2 = wl.mutant_v_masks(s, T, 0.3, tile)
        _new_gates_reject_fwd(c, wl.fwd32b(c["x"], c["P"], s, T, 0.3, k1, k2), s)
        m = wl.with_partials(wl.bwd32b(c["dout"], c["sv"], c["P"], s, T, 0.3, k1, k2), s, T)
        _new_gates_reject_bwd(c, m, s, names=("dz2",))
        _new_gates_reject_bwd(c, m, s, names=("dzo",))


@pytest.mark.parametrize("s", [3, 4])
def test_mutant_vi_dz1_row_from_its_neighbour(s):
    c = _big(s)
    m = wl.mutant_vi(c["bb"], s * c["T"] - 1)
    _new_gates_reject_bwd(c, m, s, names=("dz1",))
    # (caught by the old gates at this size as well: the wrong row's outer product moves dW_1 by 6.9 % (s = 3) and 7.3 % (s = 4) of its largest
    #  magnitude; the by-product itself was never looked at)
