"""CPU: what autograd guarantees for parameter gradients elsewhere is hand-written in grappa_amd/ops.py (the Functions return None for
their weights; the kernels accumulate into `p.grad`), so it is tested like any other hand-written arithmetic -- here the host logic, on the
test-only backend (oracle/ops_ref.py), against the float64 oracle (oracle/cpu_ref.py) under the same requires_grad mask:
  1. freeze sets: every trainable tensor within 1e-4 of its float64 gradient, no frozen parameter with a gradient or a moved bit;
  3. accumulation over two passes, with and without flat buffers; zero_grad(set_to_none=True); a second pass over a retained graph;
  4. the block Functions one by one: contiguous, broadcast and strided incoming gradients give the same bits, and float64's values;
  5. nested passes: torch.utils.checkpoint (re-entrant) and torch.autograd.grad from inside a hook.
tests/test_gpu_autograd_contract.py is the twin on the HIP kernels, where these branches also choose the kernels' routes."""
import pytest
import torch

import autograd_refs as ar

TOL = ar.TOL        # 1e-4 of the tensor's largest entry (the measure of tests/test_gpu_e2e.py)


def _run(case_name, freeze, be, model=None):
    c = ar.case(case_name)
    model = ar.product_model(c) if model is None else model
    train, frozen = ar.apply_freeze(model, freeze)
    loss = ar.step(model, ar.batch_of(c), be)
    losses, ref = ar.oracle(case_name, freeze)
    assert abs(float(loss) - losses[0]) < TOL * abs(losses[0]), (float(loss), losses[0])
    worst = ar.check_against_oracle(model, train, frozen, ref, (case_name, freeze))
    ar.record(f"host {case_name}: frozen {freeze}", "reference backend", worst, write=False)
    return model, train, frozen


# ---------------------------------------------------------------------------------------------------------------- 1. freeze sets
@pytest.mark.parametrize("freeze", list(ar.FREEZE_SETS))
@pytest.mark.parametrize("case_name", list(ar.CASES))
def test_trainable_gradients_match_float64_under_every_freeze_set(ref_backend, case_name, freeze):
    _run(case_name, freeze, ref_backend)


@pytest.mark.parametrize("freeze", ["gnn", "interleaved", "head_w_not_b", "biases"])
def test_frozen_parameters_keep_every_bit_through_an_optimiser_step(ref_backend, freeze):
    from grappa_amd.optim import FlatParams, FusedAdam
    c = ar.case("att")
    # flat buffers built AFTER freezing: trainable elements only, each tensor rounded up to four
    model = ar.product_model(c)
    train, frozen = ar.apply_freeze(model, freeze)
    named = dict(model.named_parameters())
    before = {k: p.detach().clone() for k, p in named.items()}
    flat = FlatParams(model)
    assert flat.numel == sum((named[k].numel() + 3) // 4 * 4 for k in train)
    assert len(flat.params) == len(train) and all(not hasattr(named[k], "_grappa_flat") for k in frozen)
    lo, hi = flat.data.data_ptr(), flat.data.data_ptr() + 4 * flat.numel
    assert all(not (lo <= named[k].data_ptr() < hi) for k in frozen)
    opt = FusedAdam(flat, lr=1e-3)
    opt.zero_grad()
    _run("att", freeze, ref_backend, model)
    opt.step()
    assert all(torch.equal(named[k], before[k]) and named[k].grad is None for k in frozen)
    assert sum(not torch.equal(named[k], before[k]) for k in train) > len(train) // 2
    # torch.optim.Adam over ALL parameters, no flat buffers: it skips what has no gradient
    model = ar.product_model(c)
    named = dict(model.named_parameters())
    topt = torch.optim.Adam(model.parameters(), lr=1e-3)
    _, train, frozen = _run("att", freeze, ref_backend, model)
    topt.step()
    assert all(torch.equal(named[k], before[k]) and named[k].grad is None for k in frozen)
    assert sum(not torch.equal(named[k], before[k]) for k in train) > len(train) // 2


# ---------------------------------------------------------------------------------------------------------------- 3. accumulation
@pytest.mark.parametrize("flat_buffers", [False, True])
@pytest.mark.parametrize("freeze", ["nothing", "att_block0"])
def test_two_passes_without_zeroing_give_the_float64_sum(ref_backend, freeze, flat_buffers):
    from grappa_amd.optim import FlatParams
    c = ar.case("att")
    model = ar.product_model(c)
    train, frozen = ar.apply_freeze(model, freeze)
    flat = FlatParams(model) if flat_buffers else None
    losses, ref = ar.oracle("att", freeze, "accum")
    for sl, want in zip(ar.SPLIT, losses):
        loss = ar.step(model, ar.batch_of(c, sl), ref_backend)
        assert abs(float(loss) - want) < TOL * abs(want)
    worst = ar.check_against_oracle(model, train, frozen, ref, ("accum", freeze, flat_buffers))
    ar.record(f"host att: two passes, frozen {freeze}", "flat buffers" if flat_buffers else "plain .grad", worst, write=False)
    if flat is not None:
        named = dict(model.named_parameters())
        assert all(named[k].grad.data_ptr() == flat.grad.data_ptr() + 4 * flat._offsets[id(named[k])][0] for k in train)


def test_zero_grad_to_none_between_passes_restores_the_flat_views(ref_backend):
    from grappa_amd.optim import FlatParams
    c = ar.case("att")
    model = ar.product_model(c)
    train, frozen = ar.apply_freeze(model, "att_block0")
    flat = FlatParams(model)
    named = dict(model.named_parameters())
    ar.step(model, ar.batch_of(c, ar.SPLIT[0]), ref_backend)
    model.zero_grad(set_to_none=True)
    assert all(p.grad is None for p in named.values())
    ar.step(model, ar.batch_of(c), ref_backend)
    for k in train:
        lo = flat._offsets[id(named[k])][0]
        assert named[k].grad.data_ptr() == flat.grad.data_ptr() + 4 * lo, k
    # the views were zeroed when they were restored: the buffer holds the second pass alone
    ar.check_against_oracle(model, train, frozen, ar.oracle("att", "att_block0")[1], "after zero_grad(set_to_none=True)")


def test_a_second_backward_over_a_retained_graph_is_refused_by_name(ref_backend):
    """the contract: the blocks release their saved activations as the first pass goes, so a second pass over the same graph raises a
    RuntimeError that says so at the first block it reaches -- not a TypeError from unpacking None, not a silent partial sum (an attention
    block without its saved feed-forward part used to take itself for self_interaction=False)"""
    from grappa_amd import Energy, MolwiseLoss
    c = ar.case("att")
    model = ar.product_model(c)
    train, frozen = ar.apply_freeze(model, "nothing")
    loss = MolwiseLoss(**ar.LK)(Energy()(model(ar.batch_of(c))))
    loss.backward(retain_graph=True)
    ar.check_against_oracle(model, train, frozen, ar.oracle("att")[1], "first pass, graph retained")
    with pytest.raises(RuntimeError, match="retain_graph"):
        loss.backward()


@pytest.mark.parametrize("name", ["AttBlockFn", "TransformerLayerFn[s=4,T=40]", "SymmetriserFn[s=2,T=40]", "ProjFirstLayerFn[s=4,T=40]",
                                  "MultiTransformerLayerFn", "MultiSymmetriserFn"])
def test_every_function_that_releases_its_state_refuses_a_second_pass(ref_backend, name):
    c = dict(ar.function_cases("cpu"))[name]()
    outs = c["run"]()
    douts = [torch.ones_like(o) for o in outs]
    torch.autograd.backward(outs, douts, retain_graph=True)
    with pytest.raises(RuntimeError, match="retain_graph"):
        torch.autograd.backward(outs, douts)


# ---------------------------------------------------------------------------------------------------------------- 4. layouts
FUNCTION_CASES = [n for n, _ in ar.function_cases("cpu")]


@pytest.mark.parametrize("name", [n for n in FUNCTION_CASES if "T=0" not in n])
def test_incoming_gradient_layouts_give_the_same_bits_and_float64_values(ref_backend, name):
    ar.check_function_layouts(dict(ar.function_cases("cpu"))[name](), ref_backend, name)


@pytest.mark.parametrize("name", [n for n in FUNCTION_CASES if "T=0" in n])
def test_empty_levels_return_zeros_and_call_no_kernel(ref_backend, name):
    ar.check_empty_function(dict(ar.function_cases("cpu"))[name](), ref_backend, name)


def test_input_and_statistics_gradients_are_computed_only_when_asked(ref_backend):
    ar.check_optional_gradients(ref_backend, "cpu")


# ---------------------------------------------------------------------------------------------------------------- 5. nested passes
@pytest.mark.parametrize("around", ["parameter_writer", "gnn_block"])
def test_reentrant_checkpoint_gives_the_float64_gradients(ref_backend, around):
    c = ar.case("att")
    model = ar.product_model(c)
    train, frozen = ar.apply_freeze(model, "nothing")
    with ar.checkpointed(model, around) as ran:
        loss = ar.step(model, ar.batch_of(c), ref_backend)
    assert ran == [1]                                       # the wrapped part ran forward twice: once without a graph, once inside the backward pass
    losses, ref = ar.oracle("att")
    assert abs(float(loss) - losses[0]) < TOL * abs(losses[0])
    worst = ar.check_against_oracle(model, train, frozen, ref, ("checkpoint", around))
    ar.record(f"host att: re-entrant checkpoint around {around}", "reference backend", worst, write=False)


def test_autograd_grad_inside_a_hook_of_the_outer_pass(ref_backend):
    c = ar.case("att")
    model = ar.product_model(c)
    train, frozen = ar.apply_freeze(model, "nothing")
    worst_inner = ar.step_with_inner_pass(model, ar.batch_of(c), ref_backend, "cpu")
    worst = ar.check_against_oracle(model, train, frozen, ar.oracle("att")[1], "outer pass around an inner one")
    ar.record("host att: torch.autograd.grad in a hook, outer", "reference backend", worst, write=False)
    ar.record("host att: torch.autograd.grad in a hook, inner", "reference backend", worst_inner, write=False)


# ---------------------------------------------------------------------------------------------------------------- 6. the end of the heads
@pytest.mark.parametrize("freeze", ["nothing", "gnn"])
def test_heads_done_callback_fires_once_per_pass(ref_backend, freeze):
    """GrappaModel.on_heads_backward_done (the overlapped reducer bucket leaves on it): a hook on the atom embedding's gradient -- or, when a
    frozen GNN leaves that embedding without one, the node that joins the heads instead (ops.JoinHeadsFn)"""
    c = ar.case("att")
    model = ar.product_model(c)
    ar.apply_freeze(model, freeze)
    done = []
    model.on_heads_backward_done = lambda: done.append(1)
    for _ in range(2):
        ar.step(model, ar.batch_of(c), ref_backend)
    assert done == [1, 1]
    with torch.no_grad():
        model(ar.batch_of(c))
    assert done == [1, 1]


def test_the_stream_order_check_sees_a_missing_join():
    """autograd_refs.unjoined (the vector clocks of the GPU twin's stream-order test) on hand-made logs"""
    main, a, b = 1, 2, 3
    log = [("launch", main, None), ("record", main, 10), ("wait", a, 10), ("launch", a, None), ("launch", b, None)]
    assert ar.unjoined(log, main) == [a, b]
    log += [("record", a, 11), ("wait", main, 11)]
    assert ar.unjoined(log, main) == [b]
    log += [("record", b, 12), ("wait", a, 12), ("record", a, 13), ("wait", main, 13)]           # b -> a -> main: transitive
    assert ar.unjoined(log, main) == []
    assert ar.unjoined(log + [("launch", b, None)], main) == [b]                                    # a launch after the join is not covered
    assert ar.unjoined(log + [("wait", main, 99)], main) == []                                      # an event nobody recorded orders nothing
