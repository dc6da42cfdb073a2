"""GPU (-m gpu): the grouped weight-gradient launch through the C ABI on the cases of tests/wgrad_group_cases.py (operand formats x shapes
that reach every branch x both ways to finish a split product x two upload chunks), outputs between sentinels.  Per case:
  (a) every dW and db within the float64 gate of the dense products (kernel_refs.gemm_bound with gemm_routes.C_ACC);
  (b) nothing written outside the outputs, nor behind the workspace the library asked for;
  (c) a second run gives the same bits;
  (d) the SHA-256 of every output equals tests/golden/wgrad_group_bits.json -- written once by tools/wgrad_group_bits.py from the library
      BEFORE its operand loads and token maxima were changed (gemm_bf16x_impl.h as_global / load_token_maxima), never from the code under test.
Whether a member really splits is computed (gemm_routes.group_plan), and the table of cases must reach both."""
import json
import os

import numpy as np
import pytest
import torch

import gemm_routes as gr
import kernel_refs as kr
import wgrad_group_cases as wc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_group_bits.json")
_GROUPS, _REFS = {}, {}


@pytest.fixture(scope="module")
def lib():
    from grappa_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _group(lib, name):
    if name not in _GROUPS:
        _GROUPS[name] = wc.Group(lib, name)
    return _GROUPS[name]


def _refs(g):
    """float64 references and bound terms of a group's members, computed once for both routes"""
    if g.group not in _REFS:
        refs = []
        for m, (A, B, old, old_cs) in zip(g.members, g.ops):
            tA, tB, told = torch.from_numpy(A), torch.from_numpy(B), torch.from_numpy(old)
            _, want, cs = kr.gemm_ref64(tA, tB, "wgrad", old=told, a_colsum_old=torch.from_numpy(old_cs) if m.colsum else None)
            terms = kr.gemm_terms(tA, tB, "wgrad", old=told, amax_bcast=3)
            refs.append((want, cs, terms))
        _REFS[g.group] = refs
    return _REFS[g.group]


def test_the_cases_reach_split_and_unsplit_members_and_two_upload_chunks():
    ns = {name: gr.group_plan(ms)[1] for name, ms in wc.GROUPS.items()}
    assert max(ns["nosplit"]) == 1, ns
    for name in ("f32", "pa", "pb", "pab", "mixed", "nine"):
        assert max(ns[name]) == 3 and min(ns[name]) == 1, (name, ns[name])       # 2500 = 1024 + 1024 + 452 beside an unsplit member
    assert [gr.group_psrc(wc.GROUPS[n]) for n in ("f32", "pa", "pb", "pab", "mixed", "nine")] == [0, 1, 2, 3, 4, 4]
    assert len(wc.GROUPS["nine"]) == 9


@pytest.mark.parametrize("group,route", wc.CASES, ids=[wc.case_id(*c) for c in wc.CASES])
def test_grouped_wgrad_bits(lib, golden, group, route):
    cid = wc.case_id(group, route)
    g = _group(lib, group)
    assert wc.input_digest(group) == golden[cid]["inputs"], f"{cid}: the inputs are not the ones the golden digests were taken on"
    rc, outs, ws_ok, need = g.run(route)
    assert rc == 0, f"{cid}: status {rc}"
    assert need == wc.workspace_bytes(group), f"{cid}: workspace {need} bytes, the layout says {wc.workspace_bytes(group)}"
    assert ws_ok, f"{cid}: written behind the {need} bytes of workspace"                                     # (b)
    for m, (Cb, cs) in zip(g.members, outs):
        assert Cb.guard_ok(), f"{cid}/{m.tag}: dW written outside its {m.M} x {m.N} block (ld {m.c_ld})"
        assert cs is None or cs.guard_ok(), f"{cid}/{m.tag}: db written outside its {m.M} elements"
    for m, (Cb, cs), (want, cs64, terms) in zip(g.members, outs, _refs(g)):                                  # (a)
        kr.assert_gemm(torch.from_numpy(Cb.get()), want, terms, "f32_f16x3", f"{cid}/{m.tag}: dW", gr.C_ACC)
        if cs is not None:
            A = torch.from_numpy(g.ops[g.members.index(m)][0]).double()
            cterms = dict(S=A.abs().sum(0)[None, :], gain=torch.ones(1, m.M, dtype=torch.float64), res=torch.zeros(1, m.M, dtype=torch.float64),
                          old=torch.from_numpy(g.ops[g.members.index(m)][3]).double().abs()[None, :], h=(A.abs().amax() * m.K).expand(1, m.M))
            kr.assert_gemm(torch.from_numpy(cs.get()), cs64[None, :], cterms, "f32_f16x3", f"{cid}/{m.tag}: db", gr.C_ACC)
    first = g.digests(outs)
    rc, outs2, ws_ok, _ = g.run(route)                                                                       # (c)
    assert rc == 0 and ws_ok
    for m, (Cb, cs), (Cb2, cs2) in zip(g.members, outs, outs2):
        assert np.array_equal(Cb.get().view(np.uint32), Cb2.get().view(np.uint32)), f"{cid}/{m.tag}: dW differs between two runs"
        assert cs is None or np.array_equal(cs.get().view(np.uint32), cs2.get().view(np.uint32)), f"{cid}/{m.tag}: db differs between two runs"
    assert first == golden[cid]["outputs"], (                                                                # (d)
        f"{cid}: bits differ from the golden digests in {sorted(k for k in first if first[k] != golden[cid]['outputs'].get(k))}")
