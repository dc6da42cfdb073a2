"""The recorder behind the call-trace tests (test_dense_front_end_trace.py, test_ops_trace.py): a real `HipBackend` over a stub library whose
every symbol records its call, on CPU tensors, with `torch.cuda`'s stream / event entry points replaced through pytest's `monkeypatch`.

A trace is the ordered list of library calls.  Every structure passed is dumped field by field, non-zero fields only.  Pointers are
position-independent: `name+byte_offset` into a tensor the scenario supplied, `new<k>+offset` into a tensor the code under test allocated
itself (numbered in order of first appearance), `#<n>` for a stream handle, `-` for null."""
import contextlib
import ctypes as C
import hashlib
import os

import torch

from grappa_amd import _lib, backend
from grappa_amd.backend import Amax

F32, BF16, F16, I32 = torch.float32, torch.bfloat16, torch.float16, torch.int32

# device tables of the batched refreshes (include/grappa_hip.h grappa_split_pairs_item / grappa_amax_item)
_TABLES = {"grappa_split_pairs_f32_batched": (1, [("x", "<u8"), ("amax", "<u8"), ("pairs", "<u8"), ("R", "<i4"), ("C", "<i4"), ("ldx", "<i4"), ("ldp", "<i4"),
                                                  ("transpose", "<i4"), ("tile_begin", "<i4")]),
           "grappa_amax_f32_batched": (1, [("x", "<u8"), ("R", "<i4"), ("C", "<i4"), ("ld", "<i4"), ("pad", "<i4"), ("row", "<u8"), ("col", "<u8")])}

_TUPLES_PER_TILE = {2: 32, 3: 21, 4: 16}          # of the fused writer layer's 64-row tiles (csrc/writer_layer.hip)


def _special_return(cx, name, args):
    """what the stub returns where 0 would not do; None: 0"""
    if name.endswith("workspace_bytes") or name.endswith("workspace_bytes_desc"):
        return 4096
    if name == "grappa_layernorm_bwd_partial_rows":
        return 8
    if name == "grappa_gemm_f32_group":
        return cx.group_rc
    if name == "grappa_writer_head_tiles":
        s, T = args
        return -(-T // _TUPLES_PER_TILE[s])
    return None


class _Stream:
    def __init__(self, cx, handle, device=None):
        self.cx, self.cuda_stream, self.device = cx, handle, torch.device("cpu")

    def wait_event(self, ev):
        self.cx.trace.append(["wait_event", f"#{self.cuda_stream}"])

    def wait_stream(self, other):
        self.cx.trace.append(["wait_stream", f"#{self.cuda_stream}", f"#{other.cuda_stream}"])


class _Event:
    def __init__(self, enable_timing=False):
        pass

    def record(self, stream=None):
        pass

    def elapsed_time(self, other):
        return 0.0


class _Lib:
    """the recorder: every symbol of the C ABI records its call"""

    def __init__(self, cx):
        self._cx = cx

    def __getattr__(self, name):
        if name not in _lib.SIGNATURES:
            raise AttributeError(name)
        return lambda *args: self._cx.lib_call(name, args)


class _Cx:
    """one scenario: a fresh HipBackend over the recorder, the tensors it is given, the trace"""

    def __init__(self, mp):
        self.mp, self.trace, self.out = mp, [], []
        self.supplied, self.news, self.ids, self.naming = [], [], {}, None
        self.records = {}
        self.group_rc = 0
        self.streams = {7: _Stream(self, 7)}
        self.cur = self.streams[7]
        for k in [k for k in os.environ if k.startswith("GRAPPA_")]:
            mp.delenv(k)
        mp.setattr(_lib, "load", lambda: _Lib(self))
        mp.setattr(torch.cuda, "is_available", lambda: True)
        mp.setattr(backend, "_raw_stream", lambda _idx: self.cur.cuda_stream)
        mp.setattr(torch._C, "_cuda_getDevice", lambda: 0, raising=False)
        mp.setattr(torch.cuda, "current_stream", lambda device=None: self.cur)
        mp.setattr(torch.cuda, "Event", _Event)
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
        mp.setattr(torch.cuda, "synchronize", lambda *a: None)
        mp.setattr(torch.cuda, "Stream", lambda device=None: self.stream(100 + len(self.streams)))
        mp.setattr(torch.cuda, "stream", self.on)
        for fn in ("empty", "zeros", "empty_like", "zeros_like", "from_numpy"):
            mp.setattr(torch, fn, self._noting(getattr(torch, fn)))
        self.be = backend.HipBackend()
        self.be.start_profile()

    # ---- streams
    def stream(self, handle):
        if handle not in self.streams:
            self.streams[handle] = _Stream(self, handle)
        return self.streams[handle]

    @contextlib.contextmanager
    def on(self, st):
        old, self.cur = self.cur, (st if isinstance(st, _Stream) else self.stream(st))
        try:
            yield
        finally:
            self.cur = old

    # ---- tensors and pointers
    def _noting(self, fn):
        def f(*a, **k):
            t = fn(*a, **k)
            if isinstance(t, torch.Tensor) and t.untyped_storage().nbytes():
                (self.supplied if self.naming else self.news).append((self.naming, t))
            return t
        return f

    def mat(self, name, dtype, shape, ld=None, off=0, grad=False):
        """a (rows, cols) view, `ld` elements between rows, `off` elements into its buffer (which is 64-byte aligned)"""
        rows, cols = shape
        ld = cols if ld is None else ld
        self.naming = name
        base = torch.zeros(off + max(rows, 1) * max(ld, cols, 1) + 16, dtype=dtype)
        self.naming = None
        assert base.data_ptr() % 64 == 0
        t = base.as_strided((rows, cols), (ld, 1), off)
        return t.requires_grad_() if grad else t

    def vec(self, name, n, dtype=F32):
        self.naming = name
        t = torch.zeros(n, dtype=dtype)
        self.naming = None
        return t

    def ptr(self, p):
        if p is None or p == 0:
            return None
        p = int(p)
        for name, t in self.supplied:
            s = t.untyped_storage()
            if s.data_ptr() <= p < s.data_ptr() + s.nbytes():
                return f"{name}+{p - s.data_ptr()}"
        for _, t in self.news:
            s = t.untyped_storage()
            if s.data_ptr() <= p < s.data_ptr() + s.nbytes():
                k = self.ids.setdefault(s.data_ptr(), len(self.ids))
                return f"new{k}+{p - s.data_ptr()}"
        return f"#{p}" if p < 4096 else "?"

    def tensor_at(self, p):
        for _, t in self.supplied + self.news:
            s = t.untyped_storage()
            if s.data_ptr() <= p < s.data_ptr() + s.nbytes():
                return t
        return None

    def tens(self, t):
        return f"{self.ptr(t.data_ptr())}{list(t.shape)}"

    # ---- the recorder's side
    def struct(self, o):
        d = {}
        for f, ty in o._fields_:
            v = getattr(o, f)
            if ty is C.c_void_p:
                v = self.ptr(v)
            if v:
                d[f] = v
        return d

    def arg(self, v, ty):
        if isinstance(v, C.Array):
            if issubclass(v._type_, C.Structure):
                return [self.struct(e) for e in v]
            return [self.ptr(e) if v._type_ is C.c_void_p else e for e in v]
        if hasattr(v, "_obj"):                         # ctypes.byref(...)
            return self.struct(v._obj)
        if isinstance(v, C.Structure):
            return self.struct(v)
        if ty is C.c_void_p:
            return self.ptr(v)
        return v

    def lib_call(self, name, args):
        sig = _lib.SIGNATURES[name][1]
        assert len(args) == len(sig), name
        ev = [name] + [self.arg(v, ty) for v, ty in zip(args, sig)]
        if name in _TABLES:
            import numpy as np
            ncol, fields = _TABLES[name]
            tab = self.tensor_at(args[-1]).numpy().view(np.dtype(fields))[:args[ncol]]
            ev.append([{f: (self.ptr(int(r[f])) if ty == "<u8" else int(r[f])) for f, ty in fields if r[f]} for r in tab])
        self.trace.append(ev)
        r = _special_return(self, name, args)
        return 0 if r is None else r

    # ---- steps
    def ret(self, r):
        if isinstance(r, Amax):
            d = {k: self.tens(getattr(r, k)) for k in ("row", "col", "tmax", "pairs", "parts") if getattr(r, k) is not None}
            if r.nseg:
                d["nseg"] = r.nseg
            for n, rec in self.records.items():
                if rec is r:
                    d["is"] = n
            return {"Amax": d}
        if isinstance(r, (tuple, list)):
            return [self.ret(x) for x in r]
        if isinstance(r, torch.Tensor):
            return self.tens(r)
        return r

    def step(self, label, fn):
        n0 = len(self.trace)
        rec = {"step": label}
        try:
            rec["ret"] = self.ret(fn())
        except Exception as e:          # noqa: BLE001 -- the type and the message are what is pinned
            rec["error"] = [type(e).__name__, str(e)]
        prof = self.be.stop_profile()
        rec["timed"] = {k: [v[0], v[2], v[3]] for k, v in sorted(prof.items())}
        rec["details"] = [[f, d, fl, by] for f, d, _ms, fl, by in self.be.last_profile_details]
        self.be.start_profile()
        self.out += self.trace[n0:] + [rec]

    def set(self, **attrs):
        for k, v in attrs.items():
            assert hasattr(self.be, k), k
            setattr(self.be, k, v)
        return self


def txt(o):
    """compact text of a dumped value: {field=value ...} for structures and records, [a b] for arrays, - for null"""
    if isinstance(o, dict):
        return "{" + " ".join(f"{k}={txt(v)}" for k, v in o.items()) + "}"
    if isinstance(o, (list, tuple)):
        return "[" + " ".join(txt(v) for v in o) + "]"
    return "-" if o is None else str(o)


def lines(cx):
    """the trace as lines of text: `symbol(arguments)` per library call (without the grappa_ prefix), `{step=...}` after the calls of a step"""
    return [txt(e) if isinstance(e, dict) else f"{e[0].replace('grappa_', '')}({', '.join(txt(v) for v in e[1:])})" for e in cx.out]


def digest(ls):
    return f"{len(ls)} lines, sha256 {hashlib.sha256(chr(10).join(ls).encode()).hexdigest()[:20]}"
