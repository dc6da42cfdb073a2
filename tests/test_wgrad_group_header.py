"""CPU: the workspace of the grouped weight-gradient launch keeps its size and layout.  grappa_gemm_f32_grouped_workspace_bytes is host
code; tests/wgrad_group_cases.py workspace_bytes restates the layout of gemm_f32.hip plan_group (header, slabs, column-sum partials,
tickets) on gemm_routes.group_plan, and the figures the library gave when the cases were written are pinned beside it."""
import pytest

import gemm_routes as gr
import wgrad_group_cases as wc

# bytes of workspace per group, as the library answered when the cases were written
BEFORE = {"f32": 3162576, "pa": 1840788, "pb": 1840596, "pab": 1840788, "mixed": 2633680, "nine": 3156196, "nosplit": 1792}


@pytest.fixture(scope="module")
def lib():
    from grappa_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("group", list(wc.GROUPS))
def test_workspace_bytes_are_what_the_layout_says(lib, group):
    n = len(wc.GROUPS[group])
    for route in wc.ROUTES:                     # (the tickets are laid out whichever way the products are finished)
        got = int(lib.grappa_gemm_f32_grouped_workspace_bytes(wc.descs(group, route), n))
        assert got == wc.workspace_bytes(group), (group, route, got, wc.workspace_bytes(group))
        assert got == BEFORE[group], (group, route, got, BEFORE[group])


def test_the_layout_follows_the_plan():
    """slabs only where the plan splits: a group of unsplit members needs the header alone"""
    _, ns = gr.group_plan(wc.GROUPS["nosplit"])
    assert max(ns) == 1 and wc.workspace_bytes("nosplit") % 256 == 0 and wc.workspace_bytes("nosplit") < 4096
    for group, ms in wc.GROUPS.items():
        _, ns = gr.group_plan(ms)
        slabs = sum(n * -(-m.M // 256) * -(-m.N // 128) for m, n in zip(ms, ns) if n > 1)
        assert wc.workspace_bytes(group) >= slabs * 256 * 128 * 4


def test_counts_out_of_range_need_no_workspace(lib):
    from grappa_amd import _lib
    arr = wc.descs("nine", "reduce")
    assert lib.grappa_gemm_f32_grouped_workspace_bytes(arr, 0) == 0 and lib.grappa_gemm_f32_grouped_workspace_bytes(arr, _lib.GEMM_GROUP_MAX + 1) == 0
    assert lib.grappa_gemm_f32_grouped_workspace_bytes(None, 1) == 0
