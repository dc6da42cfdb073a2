"""CPU: the route table of the dense-product sweep (tests/gemm_routes.py) says what it claims -- every record reaches the route and the
epilogue site it declares, by the Python restatement of the host-side routing and, for fp32 operands, by the library's own plan query
(host only) -- and it is complete: every kernel family, tile, layout, load width and way to finish a product, and the whole matrix of
epilogue forms x epilogue sites, written out below.  Also: the 48 cases the fuzz generator of tools/gemm_fuzz.py draws for the GPU test meet none of the entry's refusal conditions."""
import os
import sys

import numpy as np
import pytest

import gemm_routes as gr

FINISH4 = ("nosplit", "splitk5-reduce", "splitk6-inkernel", "tail2")


def test_ids_are_unique_and_spell_the_route():
    assert len(gr.BY_ID) == len(gr.CASES)
    for c in gr.CASES:
        assert c.id.startswith(c.route + "-" + c.site), c.id


@pytest.mark.parametrize("cid", [c.id for c in gr.CASES])
def test_record_reaches_the_route_it_declares(cid):
    c = gr.BY_ID[cid]
    assert gr.route_of(c) == (c.route, c.site)
    if c.entry == "single" and c.fmt == "f32":
        # the library's own word on tile, split and tail (grappa_gemm_f32_plan_desc) against the declared route
        bm, bn, nsplit, tail_tiles, tail_nsplit = gr.plan_query(c)
        kern, tile, layout, loads, finish = c.route.split("-", 4)
        assert tile == f"{bm}x{bn}"
        want = f"tail{tail_nsplit}" if tail_tiles else ("nosplit" if nsplit == 1 else f"splitk{nsplit}-" + ("inkernel" if (c.reduce == 2 and kern != "native") else "reduce"))
        assert finish == want
        if tail_tiles:
            assert nsplit == 1 and tail_tiles == (-(-c.M // bm) * -(-c.N // bn)) % 256


def test_forced_plans_of_plane_and_pair_records_pin_the_plan():
    """route_of restates make_plan only under a forced split (and, for the pair kernels, a forced tile): the cost model has no say"""
    for c in gr.CASES:
        if c.entry == "single" and c.fmt != "f32":
            assert c.nsplit >= 1, c.id
            assert c.fmt != "pairs" or c.cfg in (7, 8, 9), c.id


def test_every_route_is_covered():
    have = {c.route for c in gr.CASES}
    want = set()
    # native fp32 kernel: cfg 0-4 x layout x loads (scalar: cfg 1-3) x {no split, split + reduction}
    for tile, scalar in (("128x128", False), ("64x64", True), ("128x32", True), ("32x128", True), ("128x64", False)):
        for layout in ("fwd", "dgrad", "wgrad"):
            for loads in ("vec", "scalar") if scalar else ("vec",):
                for finish in ("nosplit", "splitk3-reduce"):
                    want.add(f"native-{tile}-{layout}-{loads}-{finish}")
    # split-in-kernel: every arithmetic once; h3 and x6 on {128x128, 256x128} x layouts x loads x four ways to finish
    want |= {f"{k}-256x128-fwd-vec-nosplit" for k in ("x9", "x6", "x3", "x1", "h3")}
    for k in ("h3", "x6"):
        for tile in ("128x128", "256x128"):
            for layout in ("fwd", "dgrad", "wgrad"):
                for loads in ("vec", "scalar"):
                    want |= {f"{k}-{tile}-{layout}-{loads}-{f}" for f in FINISH4}
    # planes
    want |= {"wplanes_x6-256x128-fwd-dma-nosplit", "planes_x6-256x128-fwd-dma-nosplit", "planes_x6-256x128-wgrad-dma-splitk3-reduce",
             "planes_x6-256x128-wgrad-dma-nosplit", "bf16_il-256x128-fwd-dma-nosplit", "bf16_il-256x128-fwd-dma-splitk2-reduce",
             "planes_x1-256x128-fwd-dma-nosplit", "planes_x1-256x128-fwd-dma-splitk2-reduce", "planes_x1-256x128-fwd-dma-splitk3-reduce"}
    # pairs: three tiles x {pipeline, round-3 loop, split + reduction, main + tail}
    for tile in ("256x128", "256x256", "128x128"):
        want |= {f"pairs_il-{tile}-fwd-dma-nosplit", f"pairs_loop-{tile}-fwd-dma-nosplit", f"pairs_il-{tile}-fwd-dma-splitk3-reduce",
                 f"pairs_il-{tile}-fwd-dma-splitk5-reduce", f"pairs_loop-{tile}-fwd-dma-splitk6-reduce", f"pairs_loop-{tile}-fwd-dma-splitk2-reduce",
                 f"pairs_il-{tile}-fwd-dma-tail2"}
    # main + tail over several columns of tiles with several tail tiles; K below one slab on the split kernels' scalar path
    assert {c.route for c in gr.CASES if c.tag == "wide"} >= {"h3-128x128-fwd-vec-tail2", "h3-256x128-fwd-vec-tail2", "pairs_il-128x128-fwd-dma-tail2",
                                                              "pairs_il-256x256-fwd-dma-tail2", "wpairs_il-256x128-fwd-dma-tail2"}
    assert all(-(-c.N // int(c.route.split("-")[1].split("x")[1])) > 1 for c in gr.CASES if c.tag == "wide")
    assert {c.K for c in gr.CASES if c.route == "h3-256x128-fwd-scalar-nosplit"} >= {1, 6, 31}
    # weight pairs
    want |= {"wpairs_il-256x128-fwd-dma-nosplit", "wpairs_loop-256x128-fwd-dma-nosplit", "wpairs_il-256x128-fwd-dma-splitk3-reduce",
             "wpairs_loop-256x128-fwd-dma-splitk2-reduce", "wpairs_il_nseg-256x128-fwd-dma-nosplit", "wpairs_il-256x128-fwd-dma-tail2"}
    # group4 and grouped
    for n in (1, 2, 3, 4):
        want |= {f"group4_h3-256x128-fwd-n{n}", f"group4_h3-256x128-dgrad-n{n}", f"group4_pairs-256x128-fwd-n{n}"}
    want |= {f"grouped_h3-psrc0-vec-n{n}-chunk{(n + 7) // 8}-nosplit" for n in (1, 8, 9, 16)}
    want |= {"grouped_h3-psrc0-scalar-n2-chunk1-nosplit", "grouped_h3-psrc0-vec-n9-chunk2-mixedsplit", "grouped_h3-psrc1-vec-n2-chunk1-mixedsplit",
             "grouped_h3-psrc2-vec-n2-chunk1-mixedsplit", "grouped_h3-psrc3-vec-n2-chunk1-mixedsplit", "grouped_h3-psrc4-vec-n3-chunk1-mixedsplit"}
    assert not (want - have), sorted(want - have)
    by = {}
    for c in gr.CASES:
        by.setdefault(c.route, []).append(c)
    # the native kernel reached under the default arithmetic by M <= 32 and by N <= 32
    assert any(c.arith == "f32_f16x3" and c.M <= 32 for c in gr.CASES if c.route.startswith("native-"))
    assert any(c.arith == "f32_f16x3" and c.N <= 32 for c in gr.CASES if c.route.startswith("native-"))
    # weight planes with the planes of W and of W^T; k-major plane operands with a_colsum; the round-3 weight-pairs loop at K % 32 == 16
    assert {c.tag for c in by["wplanes_x6-256x128-fwd-dma-nosplit"]} >= {"", "dgrad_planes_of_Wt"}
    assert all(c.f["colsum"] for c in by["planes_x6-256x128-wgrad-dma-splitk3-reduce"])
    assert any(c.K % 32 == 16 for c in by["wpairs_loop-256x128-fwd-dma-nosplit"])
    # the grouped entry: both ways to sum a split group, products with different shapes and epilogues in one group4 launch
    sites = {c.site for c in gr.CASES if c.entry == "grouped"}
    assert sites >= {"grouped", "grouped_reduce", "grouped_inkernel"}
    for c in gr.CASES:
        if c.entry == "group4" and len(c.members) > 1:
            assert len({(m.M, m.form) for m in c.members}) == len(c.members)


FAST_SITE = {"a": "cls1", "b": "cls1", "c": "cls2", "d": "cls3", "e": "cls3", "f": "cls4", "g": "cls4", "h": "cls5", "i": "walk", "j": "walk",
             "k": "walk", "m1": "cls9", "m2": "cls11", "m3": "cls12", "m4": "walk", "m5": "cls10"}


def test_every_epilogue_form_runs_at_every_site_it_can():
    for carrier, in_kernel in (("h3-256x128-fwd-vec-", True), ("pairs_il-128x128-fwd-dma-", False)):
        have = {(c.form, c.site) for c in gr.CASES if c.route.startswith(carrier) and c.tag == "fx"}
        want = set()
        for form, site in FAST_SITE.items():
            want |= {(form, site), (form, "reduce"), (form, "tail_" + site)}
            if form != "h":                                    # res_ln_*: N % 4 == 0
                want.add((form, "ragged"))
            if form not in gr.BF16_FORMS:                      # bf16 tensors cannot be misaligned (refused)
                want.add((form, "misaligned"))
            if in_kernel:
                want.add((form, "inkernel"))
        assert not (want - have), (carrier, sorted(want - have))
    native = {(c.form, c.site) for c in gr.CASES if c.route.startswith("native-")}
    assert native >= {(f, s) for f in "abcdefgijk" for s in ("native", "native_reduce")} | {("l", "native"), ("l", "native_reduce")}
    assert {m.form for c in gr.CASES if c.entry == "grouped" for m in c.members} == {"k", "l"}
    # group4 member: every form a-k inside grappa_gemm_f32_group, fp32 operands (both layouts) and pairs
    for kern, layout in (("h3", "fwd"), ("h3", "dgrad"), ("pairs", "fwd")):
        g4 = {(m.form, s) for c in gr.CASES if c.route.startswith(f"group4_{kern}-256x128-{layout}-") for m, s in zip(c.members, c.site.split("+"))}
        want = {(f, "g4_" + FAST_SITE[f]) for f in "abcdefghijk"}
        assert not (want - g4), (kern, layout, sorted(want - g4))
    # the 3-plane bf16 output / residual on the plane kernels; about a third of the products also return row maxima
    assert {c.site for c in gr.CASES if c.form == "n"} >= {"walk", "reduce"}
    singles = [c for c in gr.CASES if not c.members and c.form not in gr.BF16_FORMS]
    assert len([c for c in singles if c.amax]) * 4 >= len(singles)
    assert any(c.amax == "parts" and "splitk" in c.route for c in singles)


def test_refusal_records_start_from_records_of_the_table():
    for name, (base, mutate) in gr.REFUSALS.items():
        assert base in gr.BY_ID and callable(mutate), name
        assert name.split("-")[0] == gr.BY_ID[base].entry


def test_fuzz_cases_meet_no_refusal_condition():
    """tools/gemm_fuzz.py, the generator alone: the 48 cases of seed 0 (tests/test_gpu_pairs.py) meet none of grappa_gemm_f32's refusal
    conditions as plan_accepted restates them on the host, so the GPU test insists on 0 refusals; and the check itself refuses what it must"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import gemm_fuzz
    rng = np.random.default_rng(0)
    kinds = set()
    for _ in range(48):
        p = gemm_fuzz.draw(rng)
        kinds.add(p["kind"])
        assert gemm_fuzz.plan_accepted(p), p
    assert kinds == {"pairs", "wpairs", "split"}
    ok = dict(kind="wpairs", M=300, N=200, K=64, plan={"plan_tail": 2})
    assert gemm_fuzz.plan_accepted(ok)
    for bad in (dict(ok, K=40), dict(ok, M=32), dict(ok, plan={"plan_cfg": 8}), dict(ok, kind="pairs", plan={"plan_cfg": 1}),
                dict(ok, kind="split", plan={"plan_cfg": 1}), dict(ok, kind="pairs", M=600000, K=2048)):
        assert not gemm_fuzz.plan_accepted(bad), bad
