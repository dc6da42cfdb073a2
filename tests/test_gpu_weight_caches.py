"""GPU (-m gpu): the forms of a weight that the Python front end caches (grappa_amd/backend.py: `_wamax` row / column maxima, `_wpairs` fp16
pairs in both orientations with the device table of their batched refresh, `_wplanes` bf16 planes plain and transposed), checked BY VALUE on
every route that reads them and after every way a weight can change or move.

The oracle: a cached form is a pure function of the weight's current contents, so a product on a backend with warm caches must equal, bit
for bit, the same product on a fresh backend with empty caches ("cold").  After every event `_check` sends every weight it is given through
every applicable route and layout on both, asserts the route (`HipBackend._route`) and that the route's cache now holds the weight, asserts
equal bits, and asserts the cold result against float64 within the project's gate of the arithmetic (`_rowrel < 2e-6` of
tests/test_gpu_f16x3.py for f32_f16x3, `GEMM_MODE_TOL` of tests/test_gpu_ops.py otherwise).  Where the cache holds something checkable on its
own it is: the maxima against torch, the pairs against `to_pairs` of the weight / of its transpose.

Every test runs once per MODE: one route alone on its own backend (so the first stale use is that route's), and "all" -- every route
interleaved on one backend.  A is 96 rows throughout.

THE MUTATION (`_mutate`): every 7th row and column times 2**12, every 5th times 2**-12 (exact in fp32; `up=False` is the exact inverse).
Maxima that are stale and too small overflow fp16, maxima that are stale and too large drop the low fp16 piece far beyond the gate:
test_raw_write_without_invalidation_is_seen (the negative control) shows that it changes bits."""
import gc
import os
import weakref

import pytest
import torch

from test_gpu_f16x3 import _rowrel
from test_gpu_ops import GEMM_MODE_TOL, REPORT as OPS_REPORT

pytestmark = pytest.mark.gpu

M = 96
ROUTES = ("split", "pairs", "wpairs", "weight_planes", "bf16_planes")
MODES = ROUTES + ("all",)
LAYOUTS = ("fwd", "dgrad")
READS_MAXIMA = ("split", "pairs", "wpairs")            # (these keep the weight alive: _AmaxEntry.w)
READS_PAIRS = ("pairs", "wpairs")
TOL = {"split": 2e-6, "pairs": 2e-6, "wpairs": 2e-6, "weight_planes": GEMM_MODE_TOL["f32_bf16x6"], "bf16_planes": GEMM_MODE_TOL["bf16"],
       "native": GEMM_MODE_TOL["f32"]}
BIG, SMALL = 2.0 ** 12, 2.0 ** -12
REPORT = os.path.join(os.path.dirname(OPS_REPORT), "weight_caches.txt")          # the reports directory of the op-level tests
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    try:
        os.makedirs(os.path.dirname(REPORT), exist_ok=True)
        with open(REPORT, "w") as f:
            f.write("# route taken, worst row-relative error of a cold product against float64, its gate, case\n")
            for took, (err, tag) in sorted(WORST.items()):
                f.write(f"{took:14s} {err:.3e}  {TOL[took]:.0e}  {tag}\n")
    except OSError:
        pass


def _backend():
    from grappa_amd.backend import HipBackend
    be = HipBackend()
    be.set_gemm_precision("f32_f16x3")
    be.set_gemm_precision_bwd(None)
    return be


def _routes(mode):
    return ROUTES if mode == "all" else (mode,)


def _raw(t):
    """magnitudes as the int32 bit patterns the maxima kernels write"""
    return t.detach().abs().contiguous().view(torch.int32)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


class _Inputs:
    """the A operand of every product of reduction length K, made once: fp32, bf16, and the pair format with its row maxima"""
    _made = {}

    def __init__(self, K):
        g = torch.Generator().manual_seed(1000 + K)
        self.f32 = torch.randn(M, K, generator=g).cuda()
        self.bf16 = self.f32.bfloat16()
        self.rec = _backend().to_pairs(self.f32) if K % 32 == 0 else None
        self.f64 = {False: self.f32.double().cpu(), True: self.bf16.double().cpu()}

    @classmethod
    def of(cls, K):
        if K not in cls._made:
            cls._made[K] = cls(K)
        return cls._made[K]


def _nk(w, layout):
    R, Cc = w.shape
    return (R, Cc) if layout == "fwd" else (Cc, R)


def _applies(route, layout, w):
    """split takes every weight (the native kernel where N <= 32); the routes that read pairs or planes need N > 32 and K % 32 == 0.  The view
    with row stride 66 stays on the split route, where its maxima are what the batched kernel cannot take"""
    N, K = _nk(w, layout)
    return route == "split" or (N > 32 and K % 32 == 0 and w.stride(0) % 4 == 0)


def _product(be, route, layout, w):
    """one product of the 96-row A with the weight on `route` -> (output, name of the route taken)"""
    fwd = layout == "fwd"
    N, K = _nk(w, layout)
    inp = _Inputs.of(K)
    be.weight_pairs_min_rows = 0 if route == "wpairs" else 1 << 30
    be.weight_planes = route == "weight_planes"
    precision = "f32_bf16x6" if route == "weight_planes" else None
    a = None if route == "pairs" else (inp.bf16 if route == "bf16_planes" else inp.f32)
    scales = inp.rec if route == "pairs" else None
    a_pairs = scales.pairs if scales is not None and be._pairs_readable(scales.pairs, w, M, N, K, True, precision, None) else None
    assert (a_pairs is not None) == (route == "pairs"), f"{route} {layout} {tuple(w.shape)}: A's pairs are not readable"
    took = be._route(a, w, M, N, K, True, fwd, a_pairs, None, precision).name
    want = "native" if route == "split" and N <= 32 else route
    assert took == want, f"{route} {layout} {tuple(w.shape)}: the front end takes {took}"
    out = torch.empty(M, N, device="cuda")
    be.gemm(a, w, out, M=M, N=N, K=K, a_kcontig=True, b_kcontig=fwd, precision=precision, a_scales=scales)
    return out, took


def _holds(be, took, layout, w):
    """does the cache that the route reads hold an entry of this weight now?"""
    R, Cc = w.shape
    fwd = layout == "fwd"
    if took == "split":
        return (w.data_ptr(), R, Cc, w.stride(0)) in be._wamax
    if took in READS_PAIRS:
        return (w.data_ptr(), R, Cc, "pairs" if fwd else "pairsT") in be._wpairs and (w.data_ptr(), R, Cc, w.stride(0)) in be._wamax
    if took == "native":
        return True
    return (w.data_ptr(), R, Cc, not fwd) in be._wplanes


def _exact(w, layout, bf16_a):
    N, K = _nk(w, layout)
    w64 = w.detach().double().cpu()
    return _Inputs.of(K).f64[bf16_a] @ (w64.t() if layout == "fwd" else w64)


def _check(warm, weights, mode, layouts=LAYOUTS, what=""):
    """every weight of the dict through every applicable route of the mode in the given layouts, warm against cold and cold against float64;
    then the cached maxima and pairs themselves"""
    cold = _backend()
    for name, w in weights.items():
        for layout in layouts:
            for route in _routes(mode):
                if not _applies(route, layout, w):
                    continue
                tag = f"{what}: {name} {tuple(w.shape)} {route} {layout}"
                got, took = _product(warm, route, layout, w)
                want, _ = _product(cold, route, layout, w)
                assert _holds(warm, took, layout, w), f"{tag}: the route left no entry of the weight in its cache"
                assert torch.equal(_bits(got), _bits(want)), f"{tag}: warm caches and empty caches give different bits"
                err = _rowrel(want, _exact(w, layout, route == "bf16_planes"))
                if not err < WORST.get(took, (0.0, ""))[0]:
                    WORST[took] = (err, tag)
                assert err < TOL[took], f"{tag}: {err:.3e} off float64, gate {TOL[took]}"
        R, Cc = w.shape
        if any(r in READS_MAXIMA for r in _routes(mode)):
            am = warm._amax_of_weight(w)
            assert torch.equal(am.row, _raw(w).amax(dim=1)) and torch.equal(am.col, _raw(w).amax(dim=0)), f"{what}: {name}: cached maxima"
        if any(r in READS_PAIRS for r in _routes(mode)) and w.stride(0) % 4 == 0:
            # (also the 6-row weight that no pair product accepts: its pairs are a registered item of the batched refresh all the same)
            if "fwd" in layouts and Cc % 32 == 0:
                assert torch.equal(warm._pairs_of_weight(w), cold.to_pairs(w.detach()).pairs), f"{what}: {name}: cached pairs"
            if "dgrad" in layouts and R % 32 == 0:
                assert torch.equal(warm._pairs_of_weight(w, transposed=True), cold.to_pairs(w.detach().t().contiguous()).pairs), f"{what}: {name}: cached pairsT"
    torch.cuda.synchronize()


def _mutate(t, up=True):
    """in place, through whatever tensor is given (the weight under no_grad, or its .data).  The tests only ever alternate between the two states
    (as made, `up` applied once).  The inverse applied to a weight as made would leave the 6-row weight with ONE large row, i.e. one dominant
    output column in the forward layout, and an error relative to a single sum that may cancel is not what the row-relative gates measure
    (seen once: 1.2e-5 against 1e-5 from the native fp32 kernel, which reads no cache)."""
    a, b = (BIG, SMALL) if up else (SMALL, BIG)
    t[::7] *= a
    t[::5] *= b
    t[:, ::7] *= a
    t[:, ::5] *= b


def _weights(seed=0):
    """the shapes at which the cache logic branches (all with requires_grad): batchable and pair-capable; not batchable (C % 4 != 0, C > 2048,
    row stride 66); 6 rows; two views of one matrix that share an address and differ in shape"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).cuda()      # noqa: E731
    ws = {"w64": r(64, 64), "w96": r(96, 256), "w300": r(300, 64), "odd": r(300, 85), "wide": r(40, 2052), "strided": r(64, 66)[:, :64], "six": r(6, 256)}
    both = r(128, 128)
    ws["rows_view"], ws["cols_view"] = both[:64], both[:, :64]
    assert ws["rows_view"].data_ptr() == ws["cols_view"].data_ptr() and ws["strided"].stride(0) == 66
    return {n: w.requires_grad_() for n, w in ws.items()}


def _with_a_live_tensor_below(shape):
    """-> (a new tensor, the tensors that must stay alive).  The caching allocator merges a freed block with free neighbours and hands the merged
    block out from its start: a block keeps its address for the next tensor of its size only while the block below it is in use, and is
    the best fit for that tensor while the block above it is in use too.  Of eight tensors allocated in a row, take one that lies between two
    others (else right above one)."""
    made = [torch.empty(shape, device="cuda") for _ in range(8)]
    nbytes = made[0].numel() * 4
    at = {t.data_ptr() for t in made}
    above = [t for t in made if t.data_ptr() - nbytes in at]
    pick = next((t for t in above if t.data_ptr() + nbytes in at), above[0] if above else made[-1])
    return pick, [t for t in made if t is not pick]


def _land_on(ptr, shape, version):
    """allocate tensors of the shape until one lies at `ptr` (64 tries, the misses held alive); give it the version count asked for
    -> (tensor or None, misses)"""
    held = []
    for _ in range(64):
        t = torch.empty(shape, device="cuda")
        if t.data_ptr() == ptr:
            with torch.no_grad():
                while t._version < version:
                    t.zero_()
            return t, held
        held.append(t)
    return None, held


# ---------------------------------------------------------------------------------------------------- 1: in-place torch ops
@pytest.mark.parametrize("mode", MODES)
def test_in_place_ops_move_the_version_counter(mode):
    """w.mul_-style writes and w.copy_ under no_grad: no call is needed; the weights that were not touched keep matching"""
    hip, ws = _backend(), _weights(1)
    _check(hip, ws, mode, what="first use")
    _check(hip, ws, mode, what="hit")
    with torch.no_grad():
        for n in ("w96", "odd", "rows_view", "six"):
            _mutate(ws[n])
    _check(hip, ws, mode, what="after mul_")
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for n in ("w64", "wide", "strided", "cols_view"):
            ws[n].copy_(torch.randn(ws[n].shape, generator=g) * 300.0)
        _mutate(ws["w96"], up=False)
    _check(hip, ws, mode, what="after copy_")


# ---------------------------------------------------------------------------------------------------- 2: raw writes
@pytest.mark.parametrize("mode", MODES)
def test_raw_write_then_invalidate_weights(mode):
    """a write through w.data moves no version counter: invalidate_weights() is the caller's duty, and enough"""
    hip, ws = _backend(), _weights(3)
    _check(hip, ws, mode, what="first use")
    versions = {n: w._version for n, w in ws.items()}
    for up in (True, False):
        for n in ("w64", "w300", "odd", "strided", "cols_view"):
            _mutate(ws[n].data, up)
        hip.invalidate_weights()
        _check(hip, ws, mode, what=f"raw write up={up}")
    assert versions == {n: w._version for n, w in ws.items()}, "the raw write moved a version counter: the epoch was not what refreshed"


@pytest.mark.parametrize("route", ["split", "weight_planes"])
def test_raw_write_without_invalidation_is_seen(route):
    """NEGATIVE CONTROL: the same raw write without the call leaves stale maxima / planes behind, and the mutation is large enough for that to
    change bits of the product in both layouts.  With the call the results agree again."""
    hip, cold = _backend(), _backend()
    ws = {n: w for n, w in _weights(4).items() if n in ("w64", "w96")}
    _check(hip, ws, route, what="first use")
    for w in ws.values():
        _mutate(w.data)
    for name, w in ws.items():
        for layout in LAYOUTS:
            got, _ = _product(hip, route, layout, w)
            want, _ = _product(cold, route, layout, w)
            assert not torch.equal(_bits(got), _bits(want)), f"{name} {route} {layout}: a stale cache went unnoticed: the mutation does not discriminate"
    hip.invalidate_weights()
    _check(hip, ws, route, what="after the call")


@pytest.mark.parametrize("mode", MODES)
def test_fused_adam_step_on_a_flat_buffer(mode, monkeypatch):
    """hip.adam_step writes the flat buffer through raw pointers; FusedAdam.step tells the backend.  A step of learning rate 64 moves every
    element by 64 (first step: lr * sign(g)), i.e. every maximum by 2**6 or so"""
    from grappa_amd import backend
    from grappa_amd.optim import FlatParams, FusedAdam
    hip = _backend()
    monkeypatch.setattr(backend, "_BACKEND", hip)              # FusedAdam reaches the backend through get_backend()
    mod = torch.nn.Module()
    for n, w in _weights(5).items():
        if n in ("w64", "w96", "w300", "odd", "six"):
            mod.register_parameter(n, torch.nn.Parameter(w.detach().clone()))
    flat = FlatParams(mod)
    ws = dict(mod.named_parameters())
    _check(hip, ws, mode, what="first use")
    before, versions = flat.data.clone(), {n: w._version for n, w in ws.items()}
    flat.grad.copy_(torch.randn(flat.numel, generator=torch.Generator().manual_seed(6)))
    FusedAdam(flat, lr=64.0, max_grad_norm=None).step()
    assert float((flat.data - before).abs().min()) > 1.0 and versions == {n: w._version for n, w in ws.items()}
    _check(hip, ws, mode, what="after the step")


# ---------------------------------------------------------------------------------------------------- 3: a parameter moves
@pytest.mark.parametrize("mode", MODES)
def test_parameter_rehomed_and_its_old_address_reused(mode):
    """FlatParams re-points a parameter into its flat buffer (`p.data = ...`): the Parameter object lives on at a new address, its old storage
    is freed.  Another tensor of the same shape and version count that lands on the old address must get its own maxima, pairs and planes,
    and so must the parameter where it lives now."""
    from grappa_amd.optim import FlatParams
    hip = _backend()
    g = torch.Generator().manual_seed(7)
    mod, keep = torch.nn.Module(), []
    for n, shape in (("a", (96, 256)), ("b", (64, 64))):
        t, live = _with_a_live_tensor_below(shape)
        t.copy_(torch.randn(shape, generator=g))
        mod.register_parameter(n, torch.nn.Parameter(t))
        keep += live
        del t, live
    ps = dict(mod.named_parameters())
    _check(hip, ps, mode, what="before the move")
    old = {n: (p.data_ptr(), p._version, p.detach().clone()) for n, p in ps.items()}
    flat = FlatParams(mod)
    assert all(p.data_ptr() != old[n][0] and p._version == old[n][1] for n, p in ps.items()) and flat.data.data_ptr() == ps["a"].data_ptr()
    landed = {}
    for n, (ptr, version, contents) in old.items():
        t, held = _land_on(ptr, contents.shape, version)
        keep += held
        assert t is not None, f"{n}: the allocator did not hand the old address out again: the test would prove nothing"
        t.requires_grad_()
        t.data.copy_(contents)
        _mutate(t.data)
        assert t._version == version and t.data_ptr() == ptr and not torch.equal(t.detach(), contents)
        landed["on_old_" + n] = t
    _check(hip, landed, mode, what="the tensor on the old address")
    _check(hip, ps, mode, what="the parameter at its new address")
    _check(hip, {**landed, **ps}, mode, what="both")


# ---------------------------------------------------------------------------------------------------- 4: free and replace
@pytest.mark.parametrize("mode", MODES)
def test_weight_freed_and_replaced(mode):
    """del, gc.collect(), another tensor of the same shape and version count.  The planes are held by weak reference only, so there the address
    is handed out again (asserted); an entry of the maxima keeps its weight alive, so on the other routes it is not.  Either way the new tensor
    gets its own forms."""
    hip = _backend()
    shape = (96, 256)
    w, keep = _with_a_live_tensor_below(shape)
    w.copy_(torch.randn(shape, generator=torch.Generator().manual_seed(8)))
    w.requires_grad_()
    _check(hip, {"first": w}, mode, what="first")
    ptr, version, contents, gone = w.data_ptr(), w._version, w.detach().clone(), weakref.ref(w)
    del w
    gc.collect()
    t, held = _land_on(ptr, shape, version)
    if not any(r in READS_MAXIMA for r in _routes(mode)):
        assert gone() is None, "something other than the maxima keeps the weight alive"
        assert t is not None, "the allocator did not hand the address out again: the test would prove nothing"
    if t is None:
        t = held[0]
        with torch.no_grad():
            while t._version < version:
                t.zero_()
    t.requires_grad_()
    t.data.copy_(contents)
    _mutate(t.data)
    assert t._version == version
    _check(hip, {"replacement": t}, mode, what="replacement")


# ---------------------------------------------------------------------------------------------------- 5: ageing and re-registration
def _raw_step(hip, ws, names, up):
    for n in names:
        _mutate(ws[n].data, up)
    hip.invalidate_weights()


@pytest.mark.parametrize("mode", MODES)
def test_ageing_and_reregistration(mode):
    """a weight unused for two epochs leaves the maxima, the pairs and both device tables; changed and used again it registers anew, the tables
    are rebuilt and the others refresh in the same launch.  A weight that registers while the others are stale does the same to the tables.
    Batchable and not batchable weights side by side."""
    hip = _backend()
    ws = {n: w for n, w in _weights(9).items() if n in ("w96", "w64", "odd", "w300", "six")}
    w1 = {n: ws[n] for n in ("w96", "odd")}
    w2 = {n: ws[n] for n in ("w64", "six")}
    w3 = {"w300": ws["w300"]}
    _check(hip, {**w1, **w2}, mode, what="epoch 0")
    for up in (True, False):
        _raw_step(hip, ws, w2, up)
        _check(hip, w2, mode, what="only w2")
    W = ws["w96"]
    if mode == "split":                  # (a batched refresh of the pairs reads the maxima of every registered weight, which keeps them a step longer)
        assert (W.data_ptr(), 96, 256, 256) not in hip._wamax and (ws["odd"].data_ptr(), 300, 85, 85) not in hip._wamax
    if mode in READS_PAIRS + ("all",):
        assert not any(k[0] == W.data_ptr() for k in hip._wpairs)
    _raw_step(hip, ws, w1, True)
    _check(hip, w1, mode, what="w1 again")
    _check(hip, {**w2, **w1}, mode, what="w2 beside w1")
    for n in w1:
        _mutate(ws[n].data, up=False)
    _raw_step(hip, ws, w2, True)
    _check(hip, w3, mode, what="w3 registers while w1 and w2 are stale")
    _raw_step(hip, ws, w3, True)
    _check(hip, {**w2, **w1, **w3}, mode, what="all three")


def test_pairs_follow_maxima_that_registered_again():
    """across routes: a weight that only pair products read (one orientation), beside a weight on the split route whose refreshes age the
    maxima.  After two epochs without the first, its maxima are gone while its pairs -- and the device table that names the old maxima arrays
    -- are still registered.  Used again it gets new maxima arrays, and the batched refresh of the pairs must split by those."""
    hip = _backend()
    ws = _weights(10)
    w1, w2 = {"w96": ws["w96"]}, {"w64": ws["w64"]}
    fwd = ("fwd",)
    _check(hip, w1, "pairs", fwd, what="epoch 0")
    _check(hip, w2, "split", what="epoch 0")
    _raw_step(hip, ws, ("w96", "w64"), True)
    _check(hip, w1, "pairs", fwd, what="epoch 1")                    # (a batched refresh: the device table of the pairs exists from here on)
    _check(hip, w2, "split", what="epoch 1")
    for up in (False, True):
        _raw_step(hip, ws, w2, up)
        _check(hip, w2, "split", what="only w2")
    _raw_step(hip, ws, w1, False)
    _check(hip, w1, "pairs", fwd, what="w1 again")
    _check(hip, {**w1, **w2}, "all", what="both, every route")


# ---------------------------------------------------------------------------------------------------- 6: both orientations
@pytest.mark.parametrize("mode", MODES)
def test_both_orientations_refreshed_by_one_stale_use(mode):
    """"pairs" and "pairsT", plain and transposed planes, row and column maxima of one weight alive together: after a change the first stale
    use is in one layout, and the product in the other layout that follows must read refreshed forms too -- each layout first once"""
    hip = _backend()
    ws = {n: w for n, w in _weights(11).items() if n in ("w64", "w96", "rows_view", "cols_view", "odd")}
    _check(hip, ws, mode, what="first use")
    for first, up in (("fwd", True), ("dgrad", False)):
        other = "dgrad" if first == "fwd" else "fwd"
        _raw_step(hip, ws, ("w96", "cols_view", "odd"), up)
        _check(hip, {"w96": ws["w96"]}, mode, (first,), what=f"stale use in {first}")
        _check(hip, ws, mode, (other, first), what=f"{other} after a stale use in {first}")


# ---------------------------------------------------------------------------------------------------- 7: another stream
def test_other_stream_after_a_batched_pairs_refresh():
    """32 weights of 1024 x 1024 registered in the pair format, all changed; the first stale use, on stream A with the first weight, refreshes
    all of them in one launch on A; the last weight's product follows at once on stream B and must wait for that launch.  Correct ordering
    always passes; a missing wait fails only with some probability (the refresh may happen to finish first), so this runs once and is not looped."""
    hip = _backend()
    g = torch.Generator().manual_seed(12)
    ws = [torch.randn(1024, 1024, generator=g).cuda().requires_grad_() for _ in range(32)]
    for w in ws:
        _product(hip, "pairs", "fwd", w)
    for w in ws:
        _mutate(w.data)
    hip.invalidate_weights()
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(sa):
        first, _ = _product(hip, "pairs", "fwd", ws[0])
    with torch.cuda.stream(sb):
        last, _ = _product(hip, "pairs", "fwd", ws[-1])
    torch.cuda.synchronize()
    assert len(hip._wpairs) == 32 and hip._wptable.n == 32
    cold = _backend()
    for got, w in ((first, ws[0]), (last, ws[-1])):
        want, _ = _product(cold, "pairs", "fwd", w)
        assert torch.equal(_bits(got), _bits(want))
        assert _rowrel(want, _exact(w, "fwd", False)) < TOL["pairs"]
    assert torch.equal(hip._pairs_of_weight(ws[-1]), cold.to_pairs(ws[-1].detach()).pairs)
