"""GPU (-m gpu): every route of the dense products (tests/gemm_routes.py: kernel family x tile x operand layout and loads x way to finish the
product x epilogue site x epilogue form) run once through the C ABI with an explicit descriptor -- operand format and forced plan are exactly
what the record says -- and compared with float64 element by element (kernel_refs.gemm_ref64 / assert_gemm).  Outputs live in guarded,
strided buffers: the columns N..ld, the rows beyond M and the words in front of the base must keep the sentinel, an element the kernel
does not write keeps its NaN.  No case is skipped: a record the library refuses fails, a record that declares a refusal asserts
GRAPPA_ERR_ARG and untouched outputs.  gemm_routes.txt, beside the op_errors.txt of tests/test_gpu_ops.py, receives per case and per arithmetic and route the worst
|gpu - f64| / (u32 gain S) and the part of it that c_acc has to cover (kernel_refs.gemm_c_acc_used: the error left after the arithmetic's
representation term and the epilogue's roundings)."""
import ctypes as C
import os

import pytest
import torch

import gemm_routes as gr
import kernel_refs as kr
from test_gpu_ops import REPORT as OPS_REPORT

pytestmark = pytest.mark.gpu

FILL = 1024.0            # as tests/test_gpu_kernel_domains.py: exact in fp32 and bf16
LEAD = 64                # sentinel elements in front of every buffer (keeps the base 16-byte aligned)
REPORT = os.path.join(os.path.dirname(OPS_REPORT), "gemm_routes.txt")          # the reports directory of the op-level tests
WORST = {}
BF = torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    from grappa_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def _report():
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "w") as f:
        f.write(f"# arithmetic, worst |gpu - f64| / (u32 gain S), c_acc used (the gate allows c_acc = {gr.C_ACC:.1f}), case\n")
    yield
    with open(REPORT, "a") as f:
        f.write("# ---- worst per arithmetic and route\n")
        for (arith, route), (used, r, cid) in sorted(WORST.items()):
            f.write(f"{arith:12s} {route:55s} ratio {r:10.3f}  c_acc used {used:7.3f} of {gr.C_ACC:.1f}  {cid}\n")


def _st():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """a guarded, strided 2-D (planes x rows x cols) device buffer: FILL in front of the base, between the rows (columns cols..ld) and behind"""

    def __init__(self, rows, cols, ld, dtype, off=0, planes=1, init=None):
        assert ld >= cols
        self.rows, self.cols, self.ld, self.off, self.planes = rows, cols, ld, off, planes
        self.flat = torch.full((LEAD + off + planes * rows * ld + LEAD,), FILL, dtype=dtype, device="cuda")
        self.body = self.flat[LEAD + off:LEAD + off + planes * rows * ld].view(planes, rows, ld)
        self.view = self.body[:, :, :cols]
        if init is not None:
            self.view.copy_(init.to(dtype).reshape(-1, rows, cols) if torch.is_tensor(init) else torch.full_like(self.view, init))
        assert (self.flat.data_ptr() & 15) == 0

    @property
    def ptr(self):
        return self.body.data_ptr()

    @property
    def plane_stride(self):
        return self.rows * self.ld

    def get(self):
        v = self.view.detach().cpu()
        return v[0] if self.planes == 1 else v

    def guard_ok(self):
        lo, hi = LEAD + self.off, LEAD + self.off + self.planes * self.rows * self.ld
        return bool((self.flat[:lo] == FILL).all()) and bool((self.flat[hi:] == FILL).all()) and bool((self.body[:, :, self.cols:] == FILL).all())


def _bits(x):
    """fp32 bit patterns of magnitudes, as the library's amax arrays hold them"""
    return x.float().abs().contiguous().view(torch.int32)


def _split3(x):
    p0 = x.to(BF)
    p1 = (x - p0.float()).to(BF)
    p2 = (x - p0.float() - p1.float()).to(BF)
    return torch.stack([p0, p1, p2])


def _pairs_of(lib, x_dev, ldx, R, Cc, amax_dev, transpose=False):
    rows, cols = (Cc, R) if transpose else (R, Cc)
    out = torch.zeros((rows, 2 * ((cols + 31) // 32 * 32)), dtype=torch.float16, device="cuda")
    assert lib.grappa_split_pairs_f32(_st(), R, Cc, x_dev.data_ptr(), ldx, amax_dev.data_ptr(), out.data_ptr(), out.stride(0), int(transpose)) == 0
    return out


def _planes_of(lib, x_dev, R, Cc, transpose=False, kcontig=True):
    rows, cols = (Cc, R) if transpose else (R, Cc)
    ld = (cols + 31) // 32 * 32 if kcontig else (cols + 7) // 8 * 8
    out = torch.zeros((3, rows, ld), dtype=BF, device="cuda")
    assert lib.grappa_split_planes_f32(_st(), R, Cc, x_dev.data_ptr(), x_dev.stride(0), out.data_ptr(), ld, rows * ld, int(transpose)) == 0
    return out


class Product:
    """one descriptor with everything it points to, and the checks of what the kernel left"""

    def __init__(self, lib, c, key=None, seed=1234):
        from grappa_amd import _lib
        self.c, self.lib, self.key = c, lib, key
        self.what = c.id if key is None else key
        self.seed = seed + (gr._seed(self.what) & 0xffff)
        self.salt_value = 3 if c.f["drop"] and (gr._seed(self.what) & 2) else 0
        o = self.o = gr.operands(c, key)
        f, M, N, K = c.f, c.M, c.N, c.K
        d = self.d = _lib.GemmDesc()
        keep = self.keep = []
        d.M, d.N, d.K = M, N, K
        d.a_kcontig, d.b_kcontig = int(c.layout != "wgrad"), int(c.layout == "fwd")
        d.precision = _lib.GEMM_PRECISIONS[c.arith]
        d.plan_cfg, d.plan_nsplit, d.plan_tail, d.splitk_reduce = c.cfg, c.nsplit, c.tail, c.reduce
        a64, b64 = kr.gemm_operands64(o["A"], o["B"], c.layout)
        # ---- operands
        a_is_f32 = c.fmt in ("f32", "wplanes", "wpairs", "pb")
        b_is_f32 = c.fmt in ("f32", "pa")
        if a_is_f32:
            ra, ca = o["A"].shape
            lda = c.op_ld("a") if c.fmt in ("f32", "pb") else (ca + 3) // 4 * 4
            A = Buf(ra, ca, lda, torch.float32, off=c.a_off, init=o["A"])
            keep.append(A)
            d.A, d.lda = A.ptr, lda
        if b_is_f32:
            rb, cb = o["B"].shape
            B = Buf(rb, cb, c.op_ld("b"), torch.float32, init=o["B"])
            keep.append(B)
            d.B, d.ldb = B.ptr, B.ld
        am_a, am_b = _bits(a64.abs().amax(1)).cuda(), _bits(b64.abs().amax(1)).cuda()
        if c.fmt in ("pairs", "wpairs"):
            Bd = o["B"].cuda()
            bp = _pairs_of(lib, Bd, Bd.stride(0), N, K, am_b)
            keep += [Bd, bp]
            d.B, d.ldb, d.b_planes = bp.data_ptr(), bp.stride(0), 1
            if c.fmt == "pairs":
                Ad = o["A"].cuda()
                ap = _pairs_of(lib, Ad, Ad.stride(0), M, K, am_a)
                keep += [Ad, ap]
                d.A, d.lda, d.a_planes = ap.data_ptr(), ap.stride(0), 1
        elif c.fmt in ("wplanes", "planes"):
            if c.tag == "dgrad_planes_of_Wt":                   # the weight as stored, W^T[K][N], split into the planes of its transpose
                Wt = o["B"].t().contiguous().cuda()
                bp = _planes_of(lib, Wt, K, N, transpose=True)
            else:
                Bd = o["B"].cuda()
                bp = _planes_of(lib, Bd, *o["B"].shape, kcontig=c.layout == "fwd")
            keep.append(bp)
            d.B, d.ldb, d.b_planes, d.b_plane_stride = bp.data_ptr(), bp.stride(1), 1, bp.stride(0)
            if c.fmt == "planes":
                ap = _planes_of(lib, o["A"].cuda(), *o["A"].shape, kcontig=c.layout == "fwd")
                keep.append(ap)
                d.A, d.lda, d.a_planes, d.a_plane_stride = ap.data_ptr(), ap.stride(1), 1, ap.stride(0)
        elif c.fmt in ("pa", "pb", "pab"):                      # grouped weight gradients: token-major operands, every token row under its own scale
            for which, stored, feat in (("a", o["A"], M), ("b", o["B"], N)):
                if which not in c.fmt[1:]:
                    continue
                xd = stored.cuda()
                rowmax = _bits(stored.abs().amax(1)).cuda()
                pp = _pairs_of(lib, xd, xd.stride(0), K, feat, rowmax)
                keep += [xd, rowmax, pp]
                if which == "a":
                    d.A, d.lda, d.a_planes, d.a_rowmax = pp.data_ptr(), pp.stride(0), 1, rowmax.data_ptr()
                else:
                    d.B, d.ldb, d.b_planes, d.b_rowmax = pp.data_ptr(), pp.stride(0), 1, rowmax.data_ptr()
        if c.arith == "f32_f16x3":
            if c.bcast & 1:
                am_a = _bits(a64.abs().amax().reshape(1)).cuda()
            if c.bcast & 2:
                am_b = _bits(b64.abs().amax().reshape(1)).cuda()
            if c.a_nseg > 1:                                     # per-segment partial maxima whose maximum is the row's
                rm = a64.abs().amax(1).float()
                parts = torch.stack([torch.where(torch.arange(M) % c.a_nseg == s, rm, rm * 0.5 ** (s + 1)) for s in range(c.a_nseg)])
                am_a = _bits(parts).cuda()
                d.a_amax_nseg = c.a_nseg
            keep += [am_a, am_b]
            d.a_amax, d.b_amax, d.amax_bcast = am_a.data_ptr(), am_b.data_ptr(), c.bcast
        # ---- epilogue tensors
        nan = float("nan")
        self.C = self.C2 = self.Cp = self.C1p = self.colsum = self.amax = None
        ldp = (N + c.ld_extra + 3) // 4 * 4
        if not f["cp"]:
            self.C = Buf(M, N, c.ldc, torch.float32, off=c.c_off, init=o["old"] if (f["acc"] and not f["c2"]) else nan)
            d.C, d.ldc = self.C.ptr, c.ldc
            if f["c2"]:
                self.C2 = Buf(M, N, c.ldc, torch.float32, off=c.c_off, init=nan)
                d.C2, d.ldc2 = self.C2.ptr, c.ldc
        else:
            self.Cp = Buf(M, N, ldp, BF, planes=f["cp"], init=nan)
            d.Cp, d.ldcp, d.cp_plane_stride, d.cp_nplanes = self.Cp.ptr, ldp, self.Cp.plane_stride, f["cp"]
            if f["c1p"]:
                self.C1p = Buf(M, N, ldp, BF, init=nan)
                d.C1p, d.ldc1p = self.C1p.ptr, ldp
        for name in ("res", "aux", "pre"):
            bf = f.get(name + "p", 0)
            if o[name] is None:
                continue
            if bf:
                t = Buf(M, N, ldp, BF, planes=bf, init=o[name].to(BF) if bf == 1 else _split3(o[name]))
                setattr(d, name + "p", t.ptr), setattr(d, "ld" + name + "p", ldp), setattr(d, name + "p_plane_stride", t.plane_stride)
                setattr(d, name + "p_nplanes", bf)
            else:
                t = Buf(M, N, c.ldc, torch.float32, off=c.c_off, init=o[name])
                setattr(d, name, t.ptr), setattr(d, "ld" + name, c.ldc)
            keep.append(t)
        if o["bias"] is not None:
            bias = o["bias"].cuda()
            keep.append(bias)
            d.bias = bias.data_ptr()
        if o["ln"] is not None:
            ln = [t.cuda() for t in o["ln"]]
            keep.append(ln)
            d.res_ln_mean, d.res_ln_rstd, d.res_ln_gamma, d.res_ln_beta = (t.data_ptr() for t in ln)
        d.act, d.drop_p, d.drop_seed, d.accumulate = f["act"], f["drop"], self.seed, f["acc"]
        if self.salt_value:
            salt = torch.tensor([self.salt_value], dtype=torch.int64, device="cuda")
            keep.append(salt)
            d.drop_salt = salt.data_ptr()
        if f["colsum"]:
            self.colsum = Buf(1, M, M, torch.float32, init=o["colsum_old"])
            d.a_colsum = self.colsum.ptr
        if c.amax:
            nseg = (N + 31) // 32 if c.amax == "parts" else 1
            self.amax = Buf(nseg, M, M, torch.int32, init=-1)
            if c.amax == "parts":
                d.out_amax_parts = self.amax.ptr
            else:
                d.out_amax = self.amax.ptr
        self.outputs = [(n, b) for n, b in (("C", self.C), ("C2", self.C2), ("Cp", self.Cp), ("C1p", self.C1p), ("a_colsum", self.colsum), ("amax", self.amax)) if b is not None]

    def snapshot(self):
        return [b.flat.clone() for _, b in self.outputs]

    def check(self):
        c, f, o = self.c, self.c.f, self.o
        for name, b in self.outputs:
            assert b.guard_ok(), f"{self.what}: {name} written outside its {b.rows} x {b.cols} block (ld {b.ld}, offset {b.off})"
        C64, OUT64, cs64, terms = gr.reference(c, o, self.seed, self.salt_value)
        arith = c.arith if gr.use_bf16x(c) else "f32"          # ("shapes with M <= 32 or N <= 32 always take the native fp32 path")
        if c.fmt == "planes" and c.arith == "bf16":
            arith = "bf16_given"                               # both operands GIVEN as bf16 (one plane): nothing left for the kernel to round
        pre_terms = dict(terms, gain=torch.ones_like(terms["S"]), res=torch.zeros_like(terms["S"]), old=torch.zeros_like(terms["S"]))
        ratio, used = 0.0, 0.0
        out = None
        if self.C is not None:
            first = self.C.get()
            if self.C2 is not None:
                kr.assert_gemm(first, C64, pre_terms, arith, f"{self.what}: C (before dropout)", gr.C_ACC)
                ratio, used = max(ratio, kr.gemm_ratio(first, C64, pre_terms)), max(used, kr.gemm_c_acc_used(first, C64, pre_terms, arith))
                out = self.C2.get()
            else:
                out = first
            kr.assert_gemm(out, OUT64, terms, arith, f"{self.what}: OUT", gr.C_ACC)
            ratio, used = max(ratio, kr.gemm_ratio(out, OUT64, terms)), max(used, kr.gemm_c_acc_used(out, OUT64, terms, arith))
        if self.Cp is not None:
            got = self.Cp.get().float()
            got = got if f["cp"] == 1 else (got[0] + got[1]) + got[2]
            kr.assert_gemm(got, OUT64, terms, arith, f"{self.what}: Cp", gr.C_ACC, bf16_out=f["cp"] == 1)
            ratio, used = max(ratio, kr.gemm_ratio(got, OUT64, terms)), max(used, kr.gemm_c_acc_used(got, OUT64, terms, arith, f["cp"] == 1))
            out = got
            if self.C1p is not None:
                kr.assert_gemm(self.C1p.get().float(), C64, pre_terms, arith, f"{self.what}: C1p", gr.C_ACC, bf16_out=True)
        if f["drop"] > 0:
            # the zero pattern of the dropout is the documented counter hash, exactly: a dropped element holds the residual alone (bit for bit; with
            # res_ln_* the LayerNorm row the epilogue recomputes in fp32, i.e. float64's within the residual's share of the bound), a kept one does not
            dropped = terms["gain"] == 1.0
            base = o["res"].double() if o["res"] is not None else torch.zeros_like(OUT64)
            tol = torch.zeros_like(OUT64)
            if f["res_ln"]:
                mean, rstd, gamma, beta = (t.double() for t in o["ln"])
                base = (base - mean[:, None]) * rstd[:, None] * gamma[None, :] + beta[None, :]
                tol = 4.0 * kr.U32 * terms["res"]
            if self.Cp is not None and f["cp"] == 1:
                base = kr.bf16_round(base)
            same = (out.double() - base).abs() <= tol
            assert bool(same[dropped].all()), f"{self.what}: {int((~same[dropped]).sum())} dropped elements carry a value"
            bound = kr.gemm_bound(OUT64, terms, arith, gr.C_ACC, self.Cp is not None and f["cp"] == 1)
            stray = same & ~dropped & ((OUT64 - base).abs() > torch.maximum(bound + tol, torch.full_like(tol, 1e-6)))
            assert not bool(stray.any()), f"{self.what}: {int(stray.sum())} kept elements were dropped"
        if self.colsum is not None:
            a64, _ = kr.gemm_operands64(o["A"], o["B"], c.layout)
            am = a64.abs().amax(1) if not (c.bcast & 1) else a64.abs().amax().expand(c.M)
            cterms = dict(S=a64.abs().sum(1)[None, :], gain=torch.ones(1, c.M, dtype=torch.float64), res=torch.zeros(1, c.M, dtype=torch.float64),
                          old=o["colsum_old"].double().abs()[None, :], h=(am * c.K)[None, :])
            kr.assert_gemm(self.colsum.get(), cs64[None, :], cterms, arith, f"{self.what}: a_colsum", gr.C_ACC)
        if self.amax is not None:
            parts = self.amax.body[0].contiguous()
            if c.amax == "parts":
                nseg = (c.N + 31) // 32
                comb = torch.empty(c.M, dtype=torch.int32, device="cuda")
                assert self.lib.grappa_amax_combine(_st(), c.M, nseg, parts.data_ptr(), comb.data_ptr()) == 0
                torch.cuda.synchronize()
                segs = torch.stack([_bits(out[:, 32 * s:32 * s + 32].abs().amax(1)) for s in range(nseg)])
                assert torch.equal(parts.cpu(), segs), f"{self.what}: out_amax_parts are not the maxima of the 32-column segments of OUT"
            else:
                comb = parts[0]
            got_amax = comb.cpu()
            assert torch.equal(got_amax, _bits(out.abs().amax(1))), f"{self.what}: out_amax is not the row maxima of the output the kernel wrote"
            bound = kr.gemm_bound(OUT64, terms, arith, gr.C_ACC).amax(1)
            err = (got_amax.view(torch.float32).double() - OUT64.abs().amax(1)).abs()
            assert bool((err <= bound).all()), f"{self.what}: out_amax off the reference's row maxima by up to {float((err / bound).max()):.3g}x the gate"
        return used, ratio


def _record(c, route, what, used, ratio):
    with open(REPORT, "a") as fh:
        fh.write(f"{c.arith:12s} ratio {ratio:10.3f}  c_acc used {used:7.3f}  {what}\n")
    key = (c.arith, route)
    if (used, ratio) >= WORST.get(key, (-1.0, -1.0, ""))[:2]:
        WORST[key] = (used, ratio, what)


def _workspace(nbytes):
    return torch.empty(max(int(nbytes), 16) + 256, dtype=torch.uint8, device="cuda")


def _launch(lib, c, prods):
    from grappa_amd import _lib
    if c.entry == "single":
        d = prods[0].d
        ws = _workspace(lib.grappa_gemm_f32_workspace_bytes_desc(C.byref(d)))
        return lib.grappa_gemm_f32(_st(), C.byref(d), ws.data_ptr(), ws.numel() - 256), ws
    arr = (_lib.GemmDesc * len(prods))(*[p.d for p in prods])
    if c.entry == "group4":
        ws = _workspace(lib.grappa_gemm_f32_group_workspace_bytes(arr, len(prods)))
        return lib.grappa_gemm_f32_group(_st(), arr, len(prods), ws.data_ptr(), ws.numel() - 256), ws
    ws = _workspace(lib.grappa_gemm_f32_grouped_workspace_bytes(arr, len(prods)))
    return lib.grappa_gemm_f32_grouped(_st(), arr, len(prods), ws.data_ptr(), ws.numel() - 256), ws


def _products(lib, c):
    if c.members:
        return [Product(lib, m, key=f"{c.id}/{m.tag}") for m in c.members]
    return [Product(lib, c)]


@pytest.mark.parametrize("cid", [c.id for c in gr.CASES])
def test_route_against_float64(lib, cid):
    c = gr.BY_ID[cid]
    prods = _products(lib, c)
    torch.cuda.synchronize()
    rc, ws = _launch(lib, c, prods)
    torch.cuda.synchronize()
    assert rc == 0, f"{cid}: the library refused the record (status {rc})"
    for p in prods:
        _record(p.c, c.route, p.what, *p.check())


@pytest.mark.parametrize("name", list(gr.REFUSALS))
def test_refusal_leaves_the_outputs_alone(lib, name):
    """one case per `return GRAPPA_ERR_ARG` a caller can reach in grappa_gemm_f32, group4_desc_ok and group_desc_ok: a valid record, one
    field changed, the status, and every guarded output bit for bit as it was.  Only the status is observable: a change that an earlier line
    than the one named in gemm_routes.REFUSALS refuses passes as well.  Left out on purpose: the refusals of operands of 4 GiB and more
    (rows * ld * element size >= 2^32: buffers of that size for a status code)"""
    base_id, mutate = gr.REFUSALS[name]
    c = gr.BY_ID[base_id]
    prods = _products(lib, c)
    mutate(prods)
    before = [p.snapshot() for p in prods]
    torch.cuda.synchronize()
    rc, ws = _launch(lib, c, prods)
    torch.cuda.synchronize()
    assert rc == -1, f"{name}: status {rc}, expected GRAPPA_ERR_ARG"
    for p, snap in zip(prods, before):
        for (n, b), s in zip(p.outputs, snap):
            assert torch.equal(b.flat.view(torch.uint8), s.view(torch.uint8)), f"{name}: {n} was written although the call was refused"


def test_group_entries_refuse_counts_out_of_range(lib):
    """n <= 0 and n above GRAPPA_GEMM_GROUP_MAX / the four products of grappa_gemm_f32_group: refused before a descriptor is read"""
    from grappa_amd import _lib
    arr = (_lib.GemmDesc * 17)()
    ws = _workspace(0)
    for n in (0, -1, _lib.GEMM_GROUP4_MAX + 1):
        assert lib.grappa_gemm_f32_group(_st(), arr, n, ws.data_ptr(), 16) == -1, n
    for n in (0, -1, _lib.GEMM_GROUP_MAX + 1):
        assert lib.grappa_gemm_f32_grouped(_st(), arr, n, ws.data_ptr(), 16) == -1, n
    assert lib.grappa_gemm_f32_group(_st(), None, 1, ws.data_ptr(), 16) == -1 and lib.grappa_gemm_f32_grouped(_st(), None, 1, ws.data_ptr(), 16) == -1
