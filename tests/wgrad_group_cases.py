"""The grouped weight-gradient launch (grappa_gemm_f32_grouped) on small groups that reach every branch of it: the cases shared by
tests/test_gpu_wgrad_group_bits.py, tests/test_wgrad_group_header.py and tools/wgrad_group_bits.py.

A case is ONE grouped call.  Its members are weight gradients dW[M, N] += dZ[K, M]^T X[K, N] (+ the bias gradient db[M] += sum_k dZ[k, :])
in the arithmetic of the headline configuration (f32_f16x3, one scale per operand), each operand given as fp32 rows ("f32") or in the pair
format under per-token scales ("pa": A, "pb": B, "pab": both).

Operands: standard normal from a fixed seed (numpy PCG64 keyed by case and member), every token row scaled by 2^U(-6, 6).  One token row of
each operand is scaled by a further 2^-10 -- the rows' own spread reaches 12 - 13 binades, the second factor of the per-token rescale
(gemm_bf16x_impl.h store_quads_pairs, d > 14) needs more -- and one token row of each operand is all zeros.

Shapes (the tile is 256 x 128, a slab 16 tokens, the K chunk of these small groups 1024: gemm_routes.group_plan says what really splits):
  edge        M, N just above the limit of 32 (a pair operand's rows are a multiple of 32: 64 there, 40 / 36 for fp32 rows), K = 1030
              (with a 1024-token chunk: a second range of one 6-token slab)
  two_tiles   288 x 160: two tile rows, two tile columns, ragged in both; K = 2500 = 1024 + 1024 + 452
  one_range   K = 1014: one range whose last slab holds 6 tokens
  odd         fp32 rows of M = 511 in a 512-column table and N = 85 in 88 (the odd widths of the workload), dW contiguous (ldc = 85)
"""
import hashlib
import zlib
from dataclasses import dataclass

import numpy as np

SEED = 20240611
FILL = 1024.0
LEAD = 64                    # sentinel words in front of and behind every output
WS_GUARD = 256               # sentinel bytes behind the workspace
ROUTES = {"reduce": 1, "inkernel": 2}          # grappa_gemm_desc.splitk_reduce


@dataclass(frozen=True)
class Member:
    tag: str
    fmt: str                 # "f32" | "pa" | "pb" | "pab"  (the names gemm_routes.group_psrc reads)
    M: int
    N: int
    K: int
    colsum: bool
    lda: int = 0             # fp32 operands: leading dimensions (0 = the rows rounded up to 4)
    ldb: int = 0
    ldc: int = 0             # 0 = N rounded up to 4, plus 4 columns of sentinel

    @property
    def a_ld(self):
        return self.lda or (self.M + 3) // 4 * 4

    @property
    def b_ld(self):
        return self.ldb or (self.N + 3) // 4 * 4

    @property
    def c_ld(self):
        return self.ldc or (self.N + 3) // 4 * 4 + 4


def _small(fmt):
    return (64 if "a" in fmt[1:] else 40), (64 if "b" in fmt[1:] else 36)


def _uniform(fmt):
    m, n = _small(fmt)
    ms = [Member("edge", fmt, m, n, 1030, True), Member("two_tiles", fmt, 288, 160, 2500, True), Member("one_range", fmt, m, n, 1014, False)]
    if fmt == "f32":
        ms.append(Member("odd", fmt, 511, 85, 2500, True, lda=512, ldb=88, ldc=85))
        ms.append(Member("odd_nobias", fmt, 511, 85, 1030, False, lda=512, ldb=88, ldc=85))
    return ms


def _nine():
    fmts, ks = ("f32", "pa", "pb", "pab"), (1030, 1014, 2500)
    return [Member(f"m{i}", fmts[i % 4], *(_small(fmts[i % 4]) if i != 5 else (288, 160)), ks[i % 3], i % 2 == 0) for i in range(9)]


GROUPS = {
    "f32": _uniform("f32"),
    "pa": _uniform("pa"),
    "pb": _uniform("pb"),
    "pab": _uniform("pab"),
    "mixed": [Member("odd", "f32", 511, 85, 2500, True, lda=512, ldb=88, ldc=85), Member("two_tiles", "pa", 288, 160, 2500, True),
              Member("edge", "pb", 40, 64, 1030, False), Member("one_range", "pab", 64, 64, 1014, True)],
    "nine": _nine(),
    "nosplit": [Member("one_range", "pab", 64, 64, 1014, True), Member("two_tiles", "f32", 288, 160, 1014, False),
                Member("short", "pa", 64, 36, 70, True)],
}
CASES = [(g, r) for g in GROUPS for r in ROUTES]


def case_id(group, route):
    return f"{group}-{route}"


def operands(group, member):
    """-> A[K, M], B[K, N], old dW[M, N], old db[M] (float32 numpy), the same on every machine"""
    rng = np.random.Generator(np.random.PCG64([SEED, zlib.crc32(f"{group}/{member.tag}".encode())]))
    out = []
    for cols in (member.M, member.N):
        x = rng.standard_normal((member.K, cols)).astype(np.float32)
        scale = np.exp2(rng.uniform(-6.0, 6.0, member.K)).astype(np.float32)
        small, zero = rng.choice(member.K, 2, replace=False)
        scale[small] *= np.float32(2.0 ** -10)
        x *= scale[:, None]
        x[zero] = 0.0
        out.append(x)
    out.append(rng.standard_normal((member.M, member.N)).astype(np.float32))
    out.append(rng.standard_normal(member.M).astype(np.float32))
    return out


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def input_digest(group):
    return sha(*[x for m in GROUPS[group] for x in operands(group, m)])


def descs(group, route):
    """the descriptor array of a group with the shapes, formats and options alone (what plan_group reads): the host-only test's input"""
    from grappa_amd import _lib
    ms = GROUPS[group]
    arr = (_lib.GemmDesc * len(ms))()
    for d, m in zip(arr, ms):
        d.M, d.N, d.K = m.M, m.N, m.K
        d.a_planes, d.b_planes = int("a" in m.fmt[1:]), int("b" in m.fmt[1:])
        d.accumulate, d.precision, d.splitk_reduce = 1, _lib.GEMM_PRECISIONS["f32_f16x3"], ROUTES[route]
        d.amax_bcast = 3
    return arr


def workspace_bytes(group):
    """the workspace of grappa_gemm_f32_grouped as gemm_f32.hip plan_group lays it out, from gemm_routes.group_plan: header (descriptors of
    sizeof(GemmParams) and the two index arrays of GRAPPA_GEMM_GROUP_MAX + 1 words, rounded up to 256 bytes), per split member nsplit tile
    slabs of 256 x 128 floats and nsplit x M column-sum partials, one ticket per tile of every split member"""
    import ctypes as C

    import gemm_routes as gr
    from grappa_amd import _lib
    ms = GROUPS[group]
    _, ns = gr.group_plan(ms)
    # GemmParams (gemm_common.h): the descriptor, k_per_split, nsplit, two pointers, drop_scale, tiles_m, tiles_n, tile_begin, ntiles_launch, bm,
    # bn, vec_io, a pointer, amax_seg, epi_class, two pointers -- laid out by the C rules ctypes applies to the same list
    class GemmParams(C.Structure):
        _fields_ = [("d", _lib.GemmDesc), ("k_per_split", C.c_int), ("nsplit", C.c_int), ("slab", C.c_void_p), ("cs_slab", C.c_void_p),
                    ("drop_scale", C.c_float), ("tiles_m", C.c_int), ("tiles_n", C.c_int), ("tile_begin", C.c_int), ("ntiles_launch", C.c_int),
                    ("bm", C.c_int), ("bn", C.c_int), ("vec_io", C.c_int), ("amax_part", C.c_void_p), ("amax_seg", C.c_int), ("epi_class", C.c_int),
                    ("tickets", C.c_void_p), ("drop_salt", C.c_void_p)]
    header = (len(ms) * C.sizeof(GemmParams) + 2 * (_lib.GEMM_GROUP_MAX + 1) * 4 + 255) // 256 * 256
    floats = tickets = 0
    for m, n in zip(ms, ns):
        tiles = -(-m.M // 256) * -(-m.N // 128)
        if n > 1:
            floats += n * tiles * 256 * 128 + n * m.M
            tickets += tiles
    return header + 4 * floats + 4 * tickets


class Guarded:
    """an output between sentinels: FILL in front of the base, in the columns cols..ld of every row and behind the last row"""

    def __init__(self, rows, cols, ld, init):
        import torch
        self.rows, self.cols, self.ld = rows, cols, ld
        self.flat = torch.full((LEAD + rows * ld + LEAD,), FILL, dtype=torch.float32, device="cuda")
        self.body = self.flat[LEAD:LEAD + rows * ld].view(rows, ld)
        self.body[:, :cols].copy_(torch.from_numpy(init).reshape(rows, cols))

    @property
    def ptr(self):
        return self.body.data_ptr()

    def get(self):
        return self.body[:, :self.cols].contiguous().cpu().numpy()

    def guard_ok(self):
        f = self.flat
        return bool((f[:LEAD] == FILL).all()) and bool((f[LEAD + self.rows * self.ld:] == FILL).all()) and bool((self.body[:, self.cols:] == FILL).all())


def _bits(t):
    import torch
    return t.float().abs().contiguous().view(torch.int32)


class Group:
    """a group's operands on the device (built once) and a call of it with fresh outputs"""

    def __init__(self, lib, group):
        import torch
        self.lib, self.group, self.members = lib, group, GROUPS[group]
        self.ops = [operands(group, m) for m in self.members]
        self.keep, self.dev = [], []
        st = torch.cuda.current_stream().cuda_stream
        for m, (A, B, _, _) in zip(self.members, self.ops):
            e = {}
            for which, x, ld in (("a", A, m.a_ld), ("b", B, m.b_ld)):
                t = torch.from_numpy(x)
                e[which + "_amax"] = _bits(t.abs().amax().reshape(1)).cuda()
                if which in m.fmt[1:]:
                    xd, rowmax = t.cuda(), _bits(t.abs().amax(1)).cuda()
                    pairs = torch.zeros((m.K, 2 * ((x.shape[1] + 31) // 32 * 32)), dtype=torch.float16, device="cuda")
                    rc = lib.grappa_split_pairs_f32(st, m.K, x.shape[1], xd.data_ptr(), xd.stride(0), rowmax.data_ptr(), pairs.data_ptr(), pairs.stride(0), 0)
                    assert rc == 0, rc
                    e[which], e[which + "_ld"], e[which + "_rowmax"] = pairs, pairs.stride(0), rowmax
                else:
                    xd = torch.zeros((m.K, ld), dtype=torch.float32, device="cuda")
                    xd[:, :x.shape[1]].copy_(t)
                    e[which], e[which + "_ld"], e[which + "_rowmax"] = xd, ld, None
            self.dev.append(e)
        torch.cuda.synchronize()

    def run(self, route):
        """one grouped call -> (status, [(C, a_colsum or None) as Guarded], workspace guard intact)"""
        import torch
        from grappa_amd import _lib
        lib = self.lib
        arr = descs(self.group, route)
        outs = []
        for d, m, e, (_, _, old, old_cs) in zip(arr, self.members, self.dev, self.ops):
            d.A, d.lda, d.B, d.ldb = e["a"].data_ptr(), e["a_ld"], e["b"].data_ptr(), e["b_ld"]
            if e["a_rowmax"] is not None:
                d.a_rowmax = e["a_rowmax"].data_ptr()
            if e["b_rowmax"] is not None:
                d.b_rowmax = e["b_rowmax"].data_ptr()
            d.a_amax, d.b_amax = e["a_amax"].data_ptr(), e["b_amax"].data_ptr()
            Cb = Guarded(m.M, m.N, m.c_ld, old)
            cs = Guarded(1, m.M, m.M, old_cs) if m.colsum else None
            d.C, d.ldc = Cb.ptr, m.c_ld
            if cs is not None:
                d.a_colsum = cs.ptr
            outs.append((Cb, cs))
        need = int(lib.grappa_gemm_f32_grouped_workspace_bytes(arr, len(self.members)))
        ws = torch.full((need + WS_GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = lib.grappa_gemm_f32_grouped(torch.cuda.current_stream().cuda_stream, arr, len(self.members), ws.data_ptr(), need)
        torch.cuda.synchronize()
        return rc, outs, bool((ws[need:] == 0xA5).all()), need

    def digests(self, outs):
        """{"<member>/C": sha256, "<member>/a_colsum": sha256}"""
        dg = {}
        for m, (Cb, cs) in zip(self.members, outs):
            dg[f"{m.tag}/C"] = sha(Cb.get())
            if cs is not None:
                dg[f"{m.tag}/a_colsum"] = sha(cs.get())
        return dg
