"""GPU: the six families of grappa_md_steps_* entries (csrc/dynamics_steps.hip) are ONE call.  A family takes the optional pointers of
the one before it plus one, and a call through a wider family with the added pointers NULL is the call of the narrower one:
  a. every configuration of cutoff, constraints and solvent gives, through every family that can express it, the bits and the launches
     of the narrowest one;
  b. every refusal an option can meet is GRAPPA_ERR_ARG through every family that takes the option, on init, run and finish, for an
     empty batch too, with nothing launched and nothing written;
  c. frames_esolv of a restrained run without a solvent is no output of the run, as it is none through every other route.
Shapes: s65_C3 (one molecule of 65 atoms: two blocks, 3 conformations) and, with constraints, span64 of md_steps_cons_refs."""
import ctypes as C
import functools

import pytest
import torch

import md_cons_refs as mc
import md_cut_refs as mcut
import md_gb_cut_refs as mgc
import md_gb_refs as mg
import md_restr_refs as mr
import md_steps_cons_refs as msc
from test_gpu_md_restr import THERMO, _abi
from test_gpu_md_steps import FILL_B, GUARD_B, _bits, _fill_of, _guarded

pytestmark = pytest.mark.gpu

FAMILIES = ("", "_cut", "_cons", "_gb", "_gbcut", "_restr")          # narrowest first
TAKES = {"": (), "_cut": ("cut",), "_cons": ("cut", "cons"), "_gb": ("cut", "cons", "gb"), "_gbcut": ("cut", "cons", "gb", "gbcut"),
         "_restr": ("cut", "cons", "gb", "gbcut", "r")}              # the optional structs of a family's head (cut stands in front of the options)
N_OPT = {"": 0, "_cut": 0, "_cons": 0, "_gb": 1, "_gbcut": 1, "_restr": 3}      # of (esolv, er, phi) and of their frames
ENDS = ("xyz", "vel", "epot", "ekin", "steps", "status", "esolv", "er", "phi")
FRAMES = ("frames_xyz", "frames_epot", "frames_ekin", "frames_esolv", "frames_er", "frames_phi")
OPTS = dict(n_steps=6, save_every=3, dt=0.001, **THERMO)
CONS_CASE = "span64"


@pytest.fixture(scope="module")
def hip():
    from grappa_amd.backend import HipBackend
    return HipBackend()


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> batch, masses, keys, the case's constraints (or None)"""
    if name == CONS_CASE:
        return msc.case(name)[0], msc.case(name)[2], msc.case(name)[3], msc.case(name)[1]
    c = mr.case(name)
    return c["batch"], c["masses"], c["keys"], None


def _structs(hip, name, cut=False, cons=False, gb=False, gbcut=False):
    """the option structs of a configuration on the case (and what keeps their tensors alive)"""
    from grappa_amd import _lib
    from grappa_amd.backend_mm import _cut_struct, _opts_struct
    from grappa_amd.constraints import ConstraintBatch
    from grappa_amd.solvent import GBBatch, as_implicit_solvent
    b = _case(name)[0]
    s, keep = {}, []
    if cut:          # beside a cut-off solvent the nonbonded cutoff is the one placed with it
        s["cut"] = _cut_struct((mgc.nb_cutoff(name) if gbcut else (msc.cutoff(name) if name == CONS_CASE else mcut.cutoff(name))), "test")
    if cons:
        cb = ConstraintBatch(_case(name)[3], tolerance=mc.TOL).to("cuda")
        s["cons"] = hip._md_cons(cb, b.B, cb.cluster_atoms.device, True, "test")
        keep.append(cb)
    if gb or gbcut:
        g = GBBatch(list(mg.cons_gb()) if name == CONS_CASE else mg.gb_params(name)).to("cuda")
        sv = mgc.solvent(name) if gbcut else as_implicit_solvent(mg.MODEL)
        s["gb"] = _lib.GbDesc(radius=g.radius.data_ptr(), scale=g.scale.data_ptr(), **sv.as_opts())
        if gbcut:
            s["gbcut"] = _opts_struct(_lib.GbCut, sv.cut_opts(), "test")
        keep.append(g)
    return s, keep


def _ref(x):
    return None if x is None else C.byref(x)


def _head(hip, fam, a, s, mm=None, nb="given"):
    opt = [_ref(s.get(k)) for k in TAKES[fam]]
    return (hip._stream(), _ref(a["d"] if mm is None else mm), _ref(a["nd"] if nb == "given" else nb), *opt[:1], C.byref(a["mo"]), *opt[1:])


def _buffers(a, b, R=1):
    N, B, Cc, F = b.N, b.B, a["Cc"], OPTS["n_steps"] // OPTS["save_every"]
    f32, i32 = torch.float32, torch.int32
    shapes = {"xyz": ((N, Cc, 3), f32), "vel": ((N, Cc, 3), f32), "epot": ((B, Cc), f32), "ekin": ((B, Cc), f32), "steps": ((B, Cc), i32),
              "status": ((B, Cc), i32), "esolv": ((B, Cc), f32), "er": ((B, Cc), f32), "phi": ((R, Cc), f32),
              "frames_xyz": ((F, N, Cc, 3), f32), "frames_epot": ((F, B, Cc), f32), "frames_ekin": ((F, B, Cc), f32),
              "frames_esolv": ((F, B, Cc), f32), "frames_er": ((F, B, Cc), f32), "frames_phi": ((F, R, Cc), f32)}
    return {k: _guarded(*v) for k, v in shapes.items()}


def _workspace(need):
    wbuf = torch.full((GUARD_B + need + GUARD_B,), FILL_B, dtype=torch.uint8, device="cuda")
    return wbuf, wbuf[GUARD_B:GUARD_B + need]


def _calls(hip, fam, a, head, ws, bufs, step0=0, n=OPTS["n_steps"], frames=FRAMES, er="given"):
    """the family's init, run and finish as callables, with every output the family takes (frames: the names it is given)"""
    lib = hip.lib
    p = {k: v[1].data_ptr() for k, v in bufs.items()}
    tail = (a["table"].data_ptr(), a["n_items"], a["n_blocks"], ws.data_ptr(), ws.numel())
    fr = [p[k] if k in frames else None for k in FRAMES[:3 + N_OPT[fam]]]
    ends = [p[k] for k in ENDS[:6 + N_OPT[fam]]]
    if er != "given":
        ends[7] = er
    return (lambda: getattr(lib, f"grappa_md_steps_init{fam}_f32")(*head, a["mass"].data_ptr(), a["key"].data_ptr(), None, *tail),
            lambda: getattr(lib, f"grappa_md_steps_run{fam}_f32")(*head, a["mass"].data_ptr(), a["key"].data_ptr(), *tail, step0, n, *fr),
            lambda: getattr(lib, f"grappa_md_steps_finish{fam}_f32")(*head, *tail, *ends))


def _counted(hip, call):
    before = hip.lib.grappa_launch_count(0)
    rc = call()
    return rc, int(hip.lib.grappa_launch_count(0) - before)


def _guards_intact(bufs, wbuf):
    for k, (buf, _) in bufs.items():
        assert bool((buf[:64] == _fill_of(buf)).all()) and bool((buf[-64:] == _fill_of(buf)).all()), f"written outside {k}"
    assert bool((wbuf[:GUARD_B] == FILL_B).all()) and bool((wbuf[-GUARD_B:] == FILL_B).all()), "written outside the workspace"


def _untouched(bufs, wbuf, what):
    for k, (buf, _) in bufs.items():
        assert bool((buf == _fill_of(buf)).all()), f"{what}: {k} was written"
    assert bool((wbuf == FILL_B).all()), f"{what}: the workspace was written"


# ------------------------------------------------------------------------------------------------ a. every family gives the narrowest one's run
# configuration -> (case, the options it has, the narrowest family that expresses it, the arguments of that family's workspace_bytes)
CONFIGS = {
    "none": ("s65_C3", {}, "", lambda K: ()),
    "cut": ("s65_C3", dict(cut=True), "_cut", lambda K: ()),
    "cons": (CONS_CASE, dict(cons=True), "_cons", lambda K: (K, 0)),
    "cons+cut": (CONS_CASE, dict(cons=True, cut=True), "_cons", lambda K: (K, 1)),
    "gb": ("s65_C3", dict(gb=True), "_gb", lambda K: (0,)),
    "gb+cons": (CONS_CASE, dict(gb=True, cons=True), "_gb", lambda K: (K,)),
    "gbcut": ("s65_C3", dict(gbcut=True), "_gbcut", lambda K: (0,)),
    "gbcut+cut": ("s65_C3", dict(gbcut=True, cut=True), "_gbcut", lambda K: (0,)),
    "gbcut+cut+cons": (CONS_CASE, dict(gbcut=True, cut=True, cons=True), "_gbcut", lambda K: (K,)),
}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_every_family_gives_the_run_of_the_narrowest(hip, config):
    """6 steps with frames every 3 and every frame output asked for, through the narrowest family and through every wider one with the
    added pointers NULL: equal bits in every output, equal launches (finish through _restr_: one more, the zero write of erestr), the
    outputs of an absent option untouched, the guards intact.  The workspace is the size the NARROWEST family asks for: a wider
    family with NULL pointers needs no more."""
    name, has, first, size_args = CONFIGS[config]
    b, m, k, _ = _case(name)
    a = _abi(hip, b, m, k, OPTS)
    s, keep = _structs(hip, name, **has)
    K = s["cons"].K if "cons" in s else 0
    need = int(getattr(hip.lib, f"grappa_md_steps{first}_workspace_bytes")(b.N, a["Cc"], b.B, a["n_blocks"], *size_args(K)))
    assert need > 0
    solvent = "gb" in s
    base = None
    for fam in FAMILIES[FAMILIES.index(first):]:
        bufs = _buffers(a, b)
        wbuf, ws = _workspace(need)
        rcs, counts = zip(*(_counted(hip, call) for call in _calls(hip, fam, a, _head(hip, fam, a, s), ws, bufs)))
        torch.cuda.synchronize()
        assert rcs == (0, 0, 0), (config, fam, rcs)
        _guards_intact(bufs, wbuf)
        got = {kk: v[1].cpu().clone() for kk, v in bufs.items()}
        written = ENDS[:6] + FRAMES[:3] + (("esolv", "frames_esolv") if solvent else ()) + (("er",) if fam == "_restr" else ())
        for kk in ENDS + FRAMES:
            if kk not in written:
                assert bool((got[kk] == _fill_of(got[kk])).all()), f"{config} through {fam or 'plain'}: {kk} was written"
        if fam == "_restr":
            assert not got["er"].any(), f"{config}: erestr without restraints"
        if base is None:
            base = (got, counts)
            assert bool((got["steps"] == OPTS["n_steps"]).all()) and not got["status"].any(), (config, got["steps"], got["status"])
            assert counts[0] > 0 and counts[1] >= 2 * OPTS["n_steps"] and counts[2] > 0, counts
            continue
        for kk in written:
            if kk != "er":
                assert torch.equal(_bits(got[kk]), _bits(base[0][kk])), f"{config} through {fam}: {kk} differs from the {first or 'plain'} family's"
        assert counts == (base[1][0], base[1][1], base[1][2] + (1 if fam == "_restr" else 0)), (config, fam, counts, base[1])
    del keep


# ------------------------------------------------------------------------------------------------ b. refusals
def _restr_struct(rb, **kw):
    from grappa_amd import _lib
    f = dict(pos_k=rb.pos_k.data_ptr(), pos_ref=None, dih_molptr=rb.dih_molptr.data_ptr(), dih_atoms=rb.dih_atoms.data_ptr(), dih_k=rb.dih_k.data_ptr(),
             dih_target=rb.dih_target.data_ptr(), R=int(rb.dih_atoms.shape[0]))
    f.update(kw)
    return _lib.MdRestr(**f)


@pytest.mark.parametrize("empty", [False, True], ids=["s65_C3", "N=0"])
def test_refusals_are_the_same_through_every_family_and_come_before_the_empty_batch(hip, empty):
    """every refusal of an option, through every family that takes the option's pointer, on init, run and finish: -1, no launch, nothing
    written -- for s65_C3 and for a batch with N = 0, which the same calls without the refused option answer with 0"""
    from grappa_amd import _lib
    name = "s65_C3"
    c = mr.case(name)
    b, m, k = c["batch"], c["masses"], c["keys"]
    rb = c["rb"].to("cuda")
    a = _abi(hip, b, m, k, OPTS)
    good, keep = _structs(hip, name, cut=True, gbcut=True)
    table = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    atoms = torch.tensor([[0, 1, -1, -1, -1]], dtype=torch.int32, device="cuda")
    dist = torch.ones(1, 4, dtype=torch.float32, device="cuda")

    def cons(**kw):
        f = dict(cluster_molptr=table.data_ptr(), cluster_atoms=atoms.data_ptr(), cluster_d=dist.data_ptr(), K=1, tolerance=mc.TOL, constrain_start=1)
        f.update(kw)
        return _lib.MdCons(**f)

    mm, nd = None, a["nd"]
    if empty:
        mm, nd = _lib.MMDesc.from_buffer_copy(a["d"]), _lib.NbDesc.from_buffer_copy(a["nd"])
        mm.N = nd.N = 0
    need = int(hip.lib.grappa_md_steps_restr_workspace_bytes(b.N, a["Cc"], b.B, a["n_blocks"], 1, 1, 1, 1))
    bufs = _buffers(a, b, R=rb.R)
    wbuf, ws = _workspace(need)
    ref = b.xyz.to("cuda")
    # what: (the pointer whose families meet the refusal, the option structs of the call, nb)
    refusals = {
        "gb with cut but without gbcut": ("gb", dict(cut=good["cut"], gb=good["gb"]), nd),
        "gbcut without gb": ("gbcut", dict(gbcut=good["gbcut"]), nd),
        "a cut without nb": ("cut", dict(cut=good["cut"]), None),
        "K < 0": ("cons", dict(cons=cons(K=-1)), nd),
        "a NULL cluster_molptr with K > 0": ("cons", dict(cons=cons(cluster_molptr=None)), nd),
        "a NULL cluster_atoms with K > 0": ("cons", dict(cons=cons(cluster_atoms=None)), nd),
        "a NULL cluster_d with K > 0": ("cons", dict(cons=cons(cluster_d=None)), nd),
        "a NaN tolerance": ("cons", dict(cons=cons(tolerance=float("nan"))), nd),
        "R < 0": ("r", dict(r=_restr_struct(rb, R=-1)), nd),
        "pos_ref without pos_k": ("r", dict(r=_restr_struct(rb, pos_k=None, pos_ref=ref.data_ptr())), nd),
    }
    before = hip.lib.grappa_launch_count(0)
    for what, (pointer, s, nb) in refusals.items():
        for fam in FAMILIES:
            if pointer in TAKES[fam]:
                rcs = tuple(call() for call in _calls(hip, fam, a, _head(hip, fam, a, s, mm=mm, nb=nb), ws, bufs))
                assert rcs == (-1, -1, -1), f"{what} through {fam}: {rcs}"
    for what, s in (("restraints", dict(r=_restr_struct(rb))), ("r == NULL", {}), ("a solvent", dict(gb=good["gb"]))):
        finish = _calls(hip, "_restr", a, _head(hip, "_restr", a, s, mm=mm, nb=nd), ws, bufs, er=None)[2]
        assert finish() == -1, f"a NULL erestr at finish with {what}"
    torch.cuda.synchronize()
    assert hip.lib.grappa_launch_count(0) == before, "a refused call launched something"
    _untouched(bufs, wbuf, "a refused call")
    if empty:          # the refusals above were the options' own: the empty batch itself is accepted by every family, without a launch
        full = dict(good, cons=cons(), r=_restr_struct(rb))
        for fam in FAMILIES:          # (the _gb_ family takes no cutoff beside its solvent)
            s = {kk: full[kk] for kk in TAKES[fam] if not (fam == "_gb" and kk == "cut")}
            rcs = tuple(call() for call in _calls(hip, fam, a, _head(hip, fam, a, s, mm=mm, nb=nd), ws, bufs))
            assert rcs == (0, 0, 0), f"the empty batch through {fam}: {rcs}"
        assert hip.lib.grappa_launch_count(0) == before, "an empty batch launched something"
        _untouched(bufs, wbuf, "an empty batch")
    del keep


# ------------------------------------------------------------------------------------------------ c. the normalised edge
def test_frames_esolv_without_a_solvent_is_no_output_of_a_restrained_run(hip):
    """run_restr with restraints and no solvent, frames_esolv given and every other frame output NULL: the launches of the same call with
    frames_esolv == NULL, nothing written into frames_esolv, and a step0 off the frame period is accepted -- as through every other
    family, which drops frames_esolv without a solvent"""
    name = "s65_C3"
    c = mr.case(name)
    b, m, k = c["batch"], c["masses"], c["keys"]
    rb = c["rb"].to("cuda")
    a = _abi(hip, b, m, k, OPTS)
    s = dict(r=_restr_struct(rb))
    need = int(hip.lib.grappa_md_steps_restr_workspace_bytes(b.N, a["Cc"], b.B, a["n_blocks"], 0, 0, 0, 0))
    bufs = _buffers(a, b, R=rb.R)
    wbuf, ws = _workspace(need)
    head = _head(hip, "_restr", a, s)
    counts = {}
    for frames in ((), ("frames_esolv",)):
        init, run, _ = _calls(hip, "_restr", a, head, ws, bufs, frames=frames)
        assert init() == 0
        rc, counts[frames] = _counted(hip, run)
        assert rc == 0
    init, first, _ = _calls(hip, "_restr", a, head, ws, bufs, step0=0, n=1, frames=())
    off_period = _calls(hip, "_restr", a, head, ws, bufs, step0=1, n=2, frames=("frames_esolv",))[1]
    assert init() == 0 and first() == 0
    rc = off_period()
    torch.cuda.synchronize()
    print(f"launches of the run call: {counts}; run call at step0 = 1 with frames_esolv: {rc}")
    assert counts[("frames_esolv",)] == counts[()], counts
    assert bool((bufs["frames_esolv"][0] == _fill_of(bufs["frames_esolv"][0])).all()), "frames_esolv was written without a solvent"
    assert rc == 0, "a step0 off the frame period was refused though the run writes no frame"
    _guards_intact(bufs, wbuf)
