"""GPU (-m gpu): the hand-written parameter-gradient logic of grappa_amd/ops.py on the HIP kernels, where its requires_grad branches also
choose the kernels' ROUTES (pair format, grouped and side-stream weight gradients, batched LayerNorm backward, fused LayerNorm + dropout
backward, fused bf16 writer layer, head streams) -- against the float64 oracle under the same requires_grad mask.  tests/autograd_refs.py
holds the helpers and the cached oracle runs, tests/test_host_autograd_contract.py is the twin on the test-only backend.
  1. freeze sets x routes (eval mode); the bf16 storage configuration at 512 features;
  2. train mode: the fused LayerNorm + dropout backward and its guard against a second consumer;
  3. accumulation over passes, zero_grad(set_to_none=True), a second pass over a retained graph;
  4. contiguous / broadcast / strided incoming gradients of every block Function;
  5. nested passes (re-entrant checkpoint, torch.autograd.grad inside a hook);
  6. the order of the head streams when no gradient of the atom embedding joins them (frozen GNN).
Gate: 1e-4 of each trainable tensor's largest entry (tests/test_gpu_e2e.py); every trainable tensor is compared.  Every test
that moves a backend or model setting restores it (autograd_refs.settings)."""
import numpy as np
import pytest
import torch

import autograd_refs as ar
import golden_utils as gu

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = ar.TOL


@pytest.fixture
def be():
    from grappa_amd.backend import get_backend
    return get_backend()


def _has_pairs(rec):
    return getattr(rec, "pairs", None) is not None


# what proves that a route ran: thin wrappers on the backend (autograd_refs.counting), read after the step
PROBES = dict(
    gemm_wgrad=lambda a, k, r: (_has_pairs(k.get("x_scales")), _has_pairs(k.get("dz_scales"))),
    _launch_wgrad_items=lambda a, k, r: len(a[0]),
    act_dropout_bwd=lambda a, k, r: bool(k.get("pairs", False)),
    _join_aside=None, layernorm_bwd_batched=lambda a, k, r: r is not None, gemm_group=None, colsum=None,
    layernorm_bwd=lambda a, k, r: k.get("drop") is not None,
    seqattn_fwd=lambda a, k, r: k.get("row_idx") is not None,
    credit=lambda a, k, r: a[0],
    _stream=lambda a, k, r: int(r),
    _route=lambda a, k, r: (r.name, r.layout, bool((a[1] if len(a) > 1 else k["b"]).requires_grad)),
)

ROUTES = {
    "defaults": {},
    "pairs": dict(training_pairs=True, pairs_min_rows=0, backward_pairs=False),
    "pairs_bwd": dict(training_pairs=True, pairs_min_rows=0, backward_pairs=True),
    "no_defer": dict(defer_wgrads=False),
    "aside_off": dict(wgrads_aside=False),
    "aside_on": dict(wgrads_aside=True),
    "streams1": dict(head_streams=1),
    "streams4": dict(head_streams=4),
    "merged": dict(merged_heads="1"),
    "indexed_off": dict(first_layer_indexed=False),
    "indexed_on": dict(first_layer_indexed=True),
    "token_first_layer": dict(first_layer_rows=False),
    "wpairs": dict(weight_pairs_min_rows=0),          # forward and input-gradient products read the WEIGHT from its cached pairs: parameters that train only
}


def _probe(be, model, g, aside_seen):
    """one step under the probes -> (loss, log)"""
    join = be._join_aside

    def joined():
        aside_seen.append(len(be._aside))
        return join()
    with ar.counting(be, **{k: (v or (lambda a, k_, r: 1)) for k, v in PROBES.items() if k != "_join_aside"}) as log:
        be._join_aside = joined
        try:
            loss = ar.step(model, g, be)
        finally:
            del be._join_aside
    return loss, log


def _route_ran(route, log, aside_seen, model, be):
    """the proof, per route"""
    named = dict(model.named_parameters())
    wg = log["gemm_wgrad"]
    if not any(p.requires_grad and p.dim() == 2 for p in named.values()):
        assert not wg and not log["_launch_wgrad_items"] and log["colsum"], "frozen matrices: bias gradients are lone column sums"
        return
    assert wg, "no weight-gradient product ran"
    heads_train = any(p.requires_grad for k, p in named.items() if k.startswith("parameter_writer."))
    gnn_train = any(p.requires_grad for k, p in named.items() if k.startswith("gnn."))
    if route in ("pairs", "pairs_bwd"):
        assert any(x for x, _ in wg), "no weight-gradient product read an operand the forward pass stored as pairs"
        # backward pairs: the ELU' / dropout backward in front of a TRAINABLE self_interaction.2.weight writes pairs only (ops._bwd_pairs)
        want = sum(blk.self_interaction[2].weight.requires_grad for blk in getattr(model.gnn, "att_blocks", [])) if route == "pairs_bwd" else 0
        assert sum(log["act_dropout_bwd"]) == want, (sum(log["act_dropout_bwd"]), want)
        assert sum(dz for _, dz in wg) >= want
    else:
        assert not any(log["act_dropout_bwd"])
    if route == "no_defer":
        assert not log["_launch_wgrad_items"], "a grouped weight-gradient launch with defer_wgrads off"
    else:
        assert sum(log["_launch_wgrad_items"]) > 0, "no grouped weight-gradient launch"
    if route == "aside_off":
        assert not any(aside_seen)
    elif route != "no_defer" and heads_train:
        # (with a frozen GNN this is the node that ends the heads' backward passes -- ops.JoinHeadsFn -- sending their queue aside)
        assert any(aside_seen), "nothing was launched beside the pass"
    streams = len(set(log["_stream"]))
    if route == "streams1" or route == "merged":
        assert streams <= 2, streams                         # the caller's stream (and the side stream of the weight gradients)
    elif heads_train or gnn_train:
        assert streams >= (4 if model.parameter_writer.head_streams >= 4 else 1), streams
    if route == "merged":
        assert log["gemm_group"], "the heads did not run layer-locked"
        norms = [p.requires_grad for k, p in named.items() if k.startswith("parameter_writer.") and "norm" in k]
        if all(norms):
            assert any(log["layernorm_bwd_batched"]), "the batched LayerNorm backward did not run with every norm trainable"
        if not any(norms):
            assert not any(log["layernorm_bwd_batched"])
    else:
        assert not log["gemm_group"]
    first_rows = [c for c in log["credit"] if c == "gemm_saved"]
    if route == "token_first_layer":
        assert not first_rows and not any(log["seqattn_fwd"])
    else:
        assert first_rows, "no head took the (atom, position) first layer"
        assert any(log["seqattn_fwd"]) == (route != "indexed_off"), route
    # (backend._route: a frozen weight stays off the routes that read a cached form of the weight)
    routes = [(n, g) for n, layout, g in log["_route"] if layout != "wgrad"]
    assert not any(n == "wpairs" and not g for n, g in routes), "a frozen weight was read from cached pairs"
    assert any(n == "wpairs" for n, g in routes) == (route == "wpairs"), route
    if route == "wpairs" and any(not p.requires_grad and p.dim() == 2 for p in named.values()):
        assert any(n in ("split", "native") and not g for n, g in routes)
    frozen_w_bias = [k for k, p in named.items() if k.endswith(ar._HEAD_MATRICES) and not p.requires_grad and named[k[:-6] + "bias"].requires_grad]
    if frozen_w_bias:
        assert len(log["colsum"]) >= len(frozen_w_bias), "a frozen weight's bias gradient did not come from a lone column sum"


def _run(case_name, freeze, route, be):
    c = ar.case(case_name)
    model = ar.product_model(c, DEV)
    train, frozen = ar.apply_freeze(model, freeze)
    aside_seen = []
    with ar.settings(be, model, **ROUTES[route]):
        loss, log = _probe(be, model, ar.batch_of(c).to(DEV), aside_seen)
        _route_ran(route, log, aside_seen, model, be)
    losses, ref = ar.oracle(case_name, freeze)
    assert abs(float(loss) - losses[0]) < TOL * abs(losses[0]), (float(loss), losses[0])
    worst = ar.check_against_oracle(model, train, frozen, ref, (case_name, freeze, route))
    ar.record(f"{case_name}: frozen {freeze}", route, worst)
    return model, train, frozen


# ---------------------------------------------------------------------------------------------------------------- 1. freeze sets x routes
@pytest.mark.parametrize("route", ["defaults", "pairs_bwd"])
@pytest.mark.parametrize("freeze", list(ar.FREEZE_SETS))
@pytest.mark.parametrize("case_name", list(ar.CASES))
def test_every_freeze_set_against_float64(be, case_name, freeze, route):
    _run(case_name, freeze, route, be)


@pytest.mark.parametrize("freeze", ar.ROUTE_FREEZE_SETS)
@pytest.mark.parametrize("route", [r for r in ROUTES if r not in ("defaults", "pairs_bwd")])
def test_every_route_against_float64(be, route, freeze):
    _run("att", freeze, route, be)


@pytest.mark.parametrize("freeze", ["gnn", "interleaved", "head_w_not_b", "biases"])
def test_frozen_parameters_keep_every_bit_through_an_optimiser_step(be, freeze):
    from grappa_amd.optim import FlatParams, FusedAdam
    c = ar.case("att")
    model = ar.product_model(c, DEV)
    train, frozen = ar.apply_freeze(model, freeze)
    named = dict(model.named_parameters())
    before = {k: p.detach().clone() for k, p in named.items()}
    flat = FlatParams(model)                                    # built after freezing: trainable elements only, each tensor rounded up to four
    assert flat.numel == sum((named[k].numel() + 3) // 4 * 4 for k in train) and len(flat.params) == len(train)
    opt = FusedAdam(flat, lr=1e-3)
    opt.zero_grad()
    ar.step(model, ar.batch_of(c).to(DEV), be)
    ar.check_against_oracle(model, train, frozen, ar.oracle("att", freeze)[1], ("flat", freeze))
    opt.step()
    torch.cuda.synchronize()
    assert all(torch.equal(named[k], before[k]) and named[k].grad is None for k in frozen)
    assert sum(not torch.equal(named[k], before[k]) for k in train) > len(train) // 2
    model = ar.product_model(c, DEV)                            # torch.optim.Adam over ALL parameters, no flat buffers
    train, frozen = ar.apply_freeze(model, freeze)
    named = dict(model.named_parameters())
    topt = torch.optim.Adam(model.parameters(), lr=1e-3)
    ar.step(model, ar.batch_of(c).to(DEV), be)
    topt.step()
    torch.cuda.synchronize()
    assert all(torch.equal(named[k], before[k]) and named[k].grad is None for k in frozen)
    assert sum(not torch.equal(named[k], before[k]) for k in train) > len(train) // 2


# ---- the bf16 storage configuration at 512 features: the fused writer layer, forward and backward
BF16_FREEZE = {
    "nothing": lambda k, p: False,
    "head_norms": lambda k, p: k.startswith("parameter_writer.") and "norm" in k,
    "head_matrices": lambda k, p: k.startswith("parameter_writer.") and p.dim() == 2 and "norm" not in k,
    "gnn": lambda k, p: k.startswith("gnn."),
}
_PROD = {}


def _prod_case():
    if not _PROD:
        from grappa_amd import get_default_model_config, model_from_config
        from grappa_amd.datasets import pool_atom_counts
        cfg = get_default_model_config()
        _PROD.update(cfg=cfg, sd=gu.keyed_state_dict(model_from_config(cfg)), oracle={},
                     ids=[int(i) for i in np.argsort(pool_atom_counts()[:300], kind="stable")[-4:]])      # four large molecules: the angle and proper heads take the table route
    return _PROD


def _prod_oracle(freeze):
    P = _prod_case()
    if freeze not in P["oracle"]:
        from grappa_amd.datasets import build_batch_from_pool
        model, _, loss = ar.oracle_step(P["cfg"], P["sd"], build_batch_from_pool(P["ids"], n_confs=2, seed=3), PROD_LK, True, BF16_FREEZE[freeze])
        P["oracle"][freeze] = (float(loss.detach()), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None})
    return P["oracle"][freeze]


PROD_LK = dict(gradient_weight=0.8, energy_weight=1.0, param_weight=0.0, proper_regularisation=1e-3)


@pytest.mark.parametrize("freeze", list(BF16_FREEZE))
def test_bf16_storage_with_frozen_parameters_against_float64(be, freeze):
    """gate: the one tests/test_gpu_bf16.py::test_bf16_configuration_end_to_end_against_the_oracle holds the bf16 configuration's parameter
    gradients to -- loss within 5e-2, cosine with the fp32-grade gradient > 0.98 (here: with float64's, over the trainable tensors)"""
    import os
    from grappa_amd import model_from_config, ops
    from grappa_amd.backend import DEFAULT_GEMM_PRECISION
    from grappa_amd.datasets import build_batch_from_pool
    P = _prod_case()
    model = model_from_config(P["cfg"])
    model.load_state_dict(P["sd"])
    model = model.to(DEV).eval()
    train, frozen = [], []
    for k, p in model.named_parameters():
        p.requires_grad_(not BF16_FREEZE[freeze](k, p))
        (train if p.requires_grad else frozen).append(k)
    g = build_batch_from_pool(P["ids"], n_confs=2, seed=3).to(DEV)
    try:
        ops.set_activation_dtype("bf16")
        be.set_gemm_precision("bf16")
        with ar.counting(be, "writer_layer_fwd", "writer_layer_bwd") as log:
            loss = ar.step(model, g, be, PROD_LK)
    finally:
        ops.set_activation_dtype("f32")
        be.set_gemm_precision(os.environ.get("GRAPPA_GEMM_PRECISION", DEFAULT_GEMM_PRECISION))
    assert len(log["writer_layer_fwd"]) >= 4 and len(log["writer_layer_bwd"]) >= 4, "the fused writer layer did not run forward and backward"
    want_loss, ref = _prod_oracle(freeze)
    named = dict(model.named_parameters())
    assert sorted(ref) == sorted(train) and len(train) == sum(p.requires_grad for p in named.values())
    assert all(named[k].grad is None for k in frozen)
    got = torch.cat([named[k].grad.detach().reshape(-1).cpu().double() for k in train])
    want = torch.cat([ref[k].reshape(-1) for k in train])
    assert torch.isfinite(got).all()
    cos = float((got * want).sum() / (got.norm() * want.norm()))
    worst = max(ar.grad_distance(named[k].grad, ref[k].numpy()) for k in train)
    print(f"bf16 storage, frozen {freeze}: loss {float(loss)} vs float64 {want_loss}; cosine {cos:.5f}; worst tensor distance {worst:.2e}")
    ar.record(f"bf16 storage F=512: frozen {freeze} (1 - cosine)", "fused writer layer", 1.0 - cos)
    assert abs(float(loss) - want_loss) < 5e-2 * abs(want_loss)
    assert cos > 0.98


# ---------------------------------------------------------------------------------------------------------------- 2. dropout on
_TRAIN_REF = {}


def _train_mode_reference(freeze, seed):
    """the product on the test-only backend (oracle/ops_ref.py shares the counter-based masks; the host twin pins that path to float64 in
    eval mode) with the same ops.manual_seed -> (loss, {key: gradient}), cached"""
    if (freeze, seed) not in _TRAIN_REF:
        from grappa_amd import backend, ops
        from oracle.ops_ref import RefBackend
        c = ar.case("att")
        old = backend._BACKEND
        backend.set_backend(RefBackend())
        try:
            model = ar.product_model(c, "cpu", train=True)
            ar.apply_freeze(model, freeze)
            ops.manual_seed(seed)
            loss = ar.step(model, ar.batch_of(c), backend.get_backend())
        finally:
            backend.set_backend(old)
        _TRAIN_REF[(freeze, seed)] = (float(loss), {k: p.grad.detach().numpy().astype(np.float64) for k, p in model.named_parameters() if p.grad is not None})
    return _TRAIN_REF[(freeze, seed)]


@pytest.mark.parametrize("route", ["defaults", "pairs_bwd"])
@pytest.mark.parametrize("freeze", ["nothing", "gnn", "writer", "head_w_not_b"])
def test_train_mode_dropout_backward_routes(be, freeze, route):
    """defaults: the LayerNorm backward writes the dropout backward of its result (fuse_ln_drop, ops._masked_grad picks it up);
    pairs_bwd: the dropout backward writes the pair format only in front of a TRAINABLE weight and fp32 rows in front of a frozen one
    whose bias still needs their column sums (ops._bwd_pairs; backend.drop_fusable turns the fused launch off under backward pairs)"""
    from grappa_amd import ops
    c = ar.case("att")
    model = ar.product_model(c, DEV, train=True)
    train, frozen = ar.apply_freeze(model, freeze)
    hits = []
    with ar.settings(be, model, fuse_ln_drop=True, **ROUTES[route]):
        ops.manual_seed(77)
        with ar.counting(be, layernorm_bwd=PROBES["layernorm_bwd"], act_dropout_bwd=PROBES["act_dropout_bwd"]) as log, \
                ar.counting(ops, _masked_grad=lambda a, k, r: hits.append(r is not None)):
            loss = ar.step(model, ar.batch_of(c).to(DEV), be)
    if route == "defaults":
        assert sum(log["layernorm_bwd"]) >= 4 and sum(hits) >= 4, "the LayerNorm backward did not write the dropout backward"
        assert not any(log["act_dropout_bwd"])
    else:
        assert not any(log["layernorm_bwd"]) and not any(hits)
        assert sum(log["act_dropout_bwd"]) > 0, "no dropout backward wrote the pair format"
    want_loss, ref = _train_mode_reference(freeze, 77)
    assert abs(float(loss) - want_loss) < TOL * abs(want_loss)
    worst = ar.check_against_oracle(model, train, frozen, ref, ("train mode", freeze, route))
    ar.record(f"att, train mode (dropout): frozen {freeze}", route + (" + fused LN/dropout backward" if route == "defaults" else ""), worst)


def _two_layers(dev, gen):
    from grappa_amd import model as M
    with torch.random.fork_rng():
        torch.manual_seed(5)
        layers = [ar._seeded(M.DottedAttWithMLP(64, 4, 64, 0.3), gen).to(dev).train() for _ in range(2)]
    return layers


def _chain(layers, x, d1, d2, consumers, swap_storage, masked_log):
    """x -> layer 1 -> y1 -> layer 2 -> y2; loss = <y2, d2> (+ <y1, d1>: a second consumer of y1, built BEFORE layer 2 runs so that layer 2's
    gradient reaches autograd's buffer first and the second one is added into it in place).  -> gradients"""
    from grappa_amd import ops
    ops.manual_seed(11)
    for t in [x] + [p for l in layers for p in l.parameters()]:
        t.grad = None
    s, T = 3, 40
    y1 = layers[0](x, s, T)
    extra = (y1 * d1).sum() if consumers == 2 else None
    if swap_storage:
        def swap(g):
            g.data = g.data.clone()                 # the same object, the same values, another buffer
            return None
        y1.register_hook(swap)
    y2 = layers[1](y1, s, T)
    loss = (y2 * d2).sum()
    if extra is not None:
        loss = loss + extra
    with ar.counting(ops, _masked_grad=lambda a, k, r: masked_log.append(r is not None)):
        loss.backward()
    if x.is_cuda:
        torch.cuda.synchronize()
    return {"x": x.grad.clone(), **{f"{i}.{k}": p.grad.clone() for i, l in enumerate(layers) for k, p in l.named_parameters()}}


@pytest.mark.parametrize("scenario", ["one_consumer", "two_consumers", "swapped_storage"])
def test_precomputed_dropout_backward_is_dropped_when_the_gradient_changed(be, scenario):
    """two transformer layers (s=3, T=40, 64 features, 4 heads, p=0.3): layer 2's LayerNorm backward also writes the dropout backward of its
    result for layer 1 (dx._grappa_masked).  A second consumer of layer 1's output makes autograd ADD into that dx: the precomputed part is
    then the backward of a part of the gradient, and ops._masked_grad must not return it.  Calls of _masked_grad in the backward pass:
    layer 2's last dropout (the caller's gradient: nothing precomputed), layer 2's first, LAYER 1's LAST (the guarded one), layer 1's first."""
    from grappa_amd import backend
    from oracle.ops_ref import RefBackend
    gen = torch.Generator().manual_seed(9)
    x0, d1, d2 = (torch.randn(120, 64, generator=gen) for _ in range(3))
    consumers = 2 if scenario == "two_consumers" else 1
    got_log = []
    with ar.settings(be, None, fuse_ln_drop=True):
        layers = _two_layers(DEV, torch.Generator().manual_seed(10))
        got = _chain(layers, x0.to(DEV).requires_grad_(True), d1.to(DEV), d2.to(DEV), consumers, scenario == "swapped_storage", got_log)
    assert ar.queues_empty(be)
    assert got_log == [False, True, scenario == "one_consumer", True], got_log
    old = backend._BACKEND
    backend.set_backend(RefBackend())
    try:
        ref = _chain(_two_layers("cpu", torch.Generator().manual_seed(10)), x0.clone().requires_grad_(True), d1, d2, consumers, False, [])
    finally:
        backend.set_backend(old)
    worst = max(ar.grad_distance(got[k], ref[k].numpy()) for k in ref)
    ar.record(f"two transformer layers, p=0.3: {scenario}", "fused LN/dropout backward", worst)
    assert sorted(got) == sorted(ref) and worst < TOL, worst


# ---------------------------------------------------------------------------------------------------------------- 3. accumulation
@pytest.mark.parametrize("flat_buffers", [False, True])
@pytest.mark.parametrize("freeze", ["nothing", "att_block0"])
def test_two_passes_without_zeroing_give_the_float64_sum(be, freeze, flat_buffers):
    from grappa_amd.optim import FlatParams
    c = ar.case("att")
    model = ar.product_model(c, DEV)
    train, frozen = ar.apply_freeze(model, freeze)
    flat = FlatParams(model) if flat_buffers else None
    losses, ref = ar.oracle("att", freeze, "accum")
    for sl, want in zip(ar.SPLIT, losses):
        loss = ar.step(model, ar.batch_of(c, sl).to(DEV), be)
        assert abs(float(loss) - want) < TOL * abs(want)
    worst = ar.check_against_oracle(model, train, frozen, ref, ("accum", freeze, flat_buffers))
    ar.record(f"att: two passes without zeroing, frozen {freeze}", "flat buffers" if flat_buffers else "plain .grad", worst)
    if flat is not None:
        named = dict(model.named_parameters())
        assert flat.numel == sum((named[k].numel() + 3) // 4 * 4 for k in train)            # a parameter frozen before is not in the buffer
        assert all(named[k].grad.data_ptr() == flat.grad.data_ptr() + 4 * flat._offsets[id(named[k])][0] for k in train)


def test_zero_grad_to_none_between_passes_restores_the_flat_views(be):
    from grappa_amd.optim import FlatParams
    c = ar.case("att")
    model = ar.product_model(c, DEV)
    train, frozen = ar.apply_freeze(model, "att_block0")
    flat = FlatParams(model)
    named = dict(model.named_parameters())
    ar.step(model, ar.batch_of(c, ar.SPLIT[0]).to(DEV), be)
    model.zero_grad(set_to_none=True)
    assert all(p.grad is None for p in named.values())
    ar.step(model, ar.batch_of(c).to(DEV), be)
    for k in train:
        assert named[k].grad.data_ptr() == flat.grad.data_ptr() + 4 * flat._offsets[id(named[k])][0], k
    worst = ar.check_against_oracle(model, train, frozen, ar.oracle("att", "att_block0")[1], "after zero_grad(set_to_none=True)")
    ar.record("att: zero_grad(set_to_none=True) between passes, frozen att_block0", "flat buffers", worst)


def test_a_second_backward_over_a_retained_graph_is_refused_by_name(be):
    """the contract (see the host twin): RuntimeError naming retain_graph at the first block the second pass reaches; the first pass is right"""
    from grappa_amd import Energy, MolwiseLoss
    c = ar.case("att")
    model = ar.product_model(c, DEV)
    train, frozen = ar.apply_freeze(model, "nothing")
    loss = MolwiseLoss(**ar.LK)(Energy()(model(ar.batch_of(c).to(DEV))))
    loss.backward(retain_graph=True)
    torch.cuda.synchronize()
    assert ar.queues_empty(be)
    ar.check_against_oracle(model, train, frozen, ar.oracle("att")[1], "first pass, graph retained")
    with pytest.raises(RuntimeError, match="retain_graph"):
        loss.backward()
    be.drop_deferred()
    assert ar.queues_empty(be)


# ---------------------------------------------------------------------------------------------------------------- 4. layouts
FUNCTION_CASES = [n for n, _ in ar.function_cases("cpu")]


@pytest.mark.parametrize("name", [n for n in FUNCTION_CASES if "T=0" not in n])
def test_incoming_gradient_layouts_give_the_same_bits_and_float64_values(be, name):
    worst = ar.check_function_layouts(dict(ar.function_cases(DEV))[name](), be, name)
    ar.record("function level, contiguous / broadcast / strided gradients", name, worst)


@pytest.mark.parametrize("name", [n for n in FUNCTION_CASES if "T=0" in n])
def test_empty_levels_return_zeros_and_launch_nothing(be, name):
    ar.check_empty_function(dict(ar.function_cases(DEV))[name](), be, name)


def test_input_and_statistics_gradients_are_computed_only_when_asked(be):
    ar.check_optional_gradients(be, DEV)


# ---------------------------------------------------------------------------------------------------------------- 5. nested passes
@pytest.mark.parametrize("around", ["parameter_writer", "gnn_block"])
def test_reentrant_checkpoint_gives_the_float64_gradients(be, around):
    c = ar.case("att")
    model = ar.product_model(c, DEV)
    train, frozen = ar.apply_freeze(model, "nothing")
    with ar.checkpointed(model, around) as ran:
        loss = ar.step(model, ar.batch_of(c).to(DEV), be)
    assert ran == [1]
    losses, ref = ar.oracle("att")
    assert abs(float(loss) - losses[0]) < TOL * abs(losses[0])
    worst = ar.check_against_oracle(model, train, frozen, ref, ("checkpoint", around))
    ar.record(f"att: re-entrant checkpoint around {around}", "defaults", worst)


def test_autograd_grad_inside_a_hook_of_the_outer_pass(be):
    c = ar.case("att")
    model = ar.product_model(c, DEV)
    train, frozen = ar.apply_freeze(model, "nothing")
    worst_inner = ar.step_with_inner_pass(model, ar.batch_of(c).to(DEV), be, DEV)
    worst = ar.check_against_oracle(model, train, frozen, ar.oracle("att")[1], "outer pass around an inner one")
    ar.record("att: torch.autograd.grad in a hook, outer pass", "defaults", worst)
    ar.record("att: torch.autograd.grad in a hook, inner pass", "defaults", worst_inner)


# ---------------------------------------------------------------------------------------------------------------- 6. stream order
@pytest.mark.parametrize("defer", [True, False])
def test_caller_stream_is_ordered_behind_every_head_stream_with_a_frozen_gnn(be, defer):
    """host-side and deterministic (no timing, no attempt at the race): with a frozen GNN no gradient of the atom embedding joins the four
    head streams, and the heads' kernels write p.grad themselves.  Everything that orders streams is recorded during backward(); when it
    returns, the caller's stream must be ordered behind the last launch on every other stream (vector clocks: autograd_refs.unjoined).
    The node that does it also tells the model that the heads are done: exactly once per pass."""
    from grappa_amd import Energy, MolwiseLoss
    c = ar.case("att")
    model = ar.product_model(c, DEV)
    train, frozen = ar.apply_freeze(model, "gnn")
    done = []
    model.on_heads_backward_done = lambda: done.append(1)
    with ar.settings(be, model, head_streams=4, defer_wgrads=defer):
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            loss = MolwiseLoss(**ar.LK)(Energy()(model(ar.batch_of(c).to(DEV))))
            main = torch.cuda.current_stream().cuda_stream
            with ar.stream_order_log(be) as log:
                loss.backward()
            torch.cuda.synchronize()
            assert ar.queues_empty(be)
            used = {s for what, s, _ in log if what == "launch"}
            assert len(used - {main}) >= 3, used                 # the three side streams of the heads did launch
            assert ar.unjoined(log, main) == []
    assert done == [1, 1]
    losses, ref = ar.oracle("att", "gnn")
    worst = ar.check_against_oracle(model, train, frozen, ref, ("frozen GNN on four streams", defer))
    ar.record("att: frozen gnn, four head streams", "defer_wgrads " + ("on" if defer else "off"), worst)


def test_heads_done_callback_fires_once_per_pass_with_a_trainable_gnn_too(be):
    c = ar.case("att")
    model = ar.product_model(c, DEV)
    ar.apply_freeze(model, "nothing")
    done = []
    model.on_heads_backward_done = lambda: done.append(1)
    for _ in range(2):
        ar.step(model, ar.batch_of(c).to(DEV), be)
    assert done == [1, 1]


def test_frozen_gnn_on_four_streams_equals_one_stream_bit_for_bit(be):
    """as tests/test_gpu_e2e.py::test_train_steps_on_four_streams_match_single_stream does for the all-trainable model: one summation order
    (no deferred grouping, tail launches pinned off), three optimiser steps, the same bits"""
    from grappa_amd.optim import FlatParams, FusedAdam
    c = ar.case("att")
    out = {}
    be.pin_tail_launches(False)
    try:
        with ar.settings(be, None, defer_wgrads=False):
            for streams in (1, 4):
                model = ar.product_model(c, DEV)
                ar.apply_freeze(model, "gnn")
                model.parameter_writer.head_streams = streams
                flat = FlatParams(model)
                opt = FusedAdam(flat, lr=1e-4)
                losses = []
                for _ in range(3):
                    opt.zero_grad()
                    losses.append(ar.step(model, ar.batch_of(c).to(DEV), be, sync=False).clone())
                    opt.step()
                torch.cuda.synchronize()
                out[streams] = (torch.stack(losses), flat.data.clone())
    finally:
        be.pin_tail_launches(None)
    assert torch.isfinite(out[4][1]).all() and float(out[1][0][-1]) != float(out[1][0][0])
    assert torch.equal(out[4][0], out[1][0]) and torch.equal(out[4][1], out[1][1])
