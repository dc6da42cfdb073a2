"""GPU: the nonbonded term under a cutoff (grappa_nonbonded_fwd_cut_f32 through HipBackend.nonbonded(cutoff=)) against the float64
restatement of tests/nb_cut_refs.py, and the tile pruning against the host restatement of the skip rule.  Cases, cutoffs and variants
are nb_cut_refs'; tests/test_host_nb_cut.py asserts on the CPU what these tests need of their inputs (the gap around every cutoff, no
tile at the threshold, fewer tiles than all on the 513-atom chain)."""
import ctypes as C

import numpy as np
import pytest
import torch

import nb_cut_refs as nc
import nonbonded_refs as nr
from grappa_amd import _lib

pytestmark = pytest.mark.gpu

FILL, FILL_I, FILL_B = 1024.0, 12345, 0xA5
GUARD_B = 4096


@pytest.fixture(scope="module")
def hip():
    from grappa_amd.backend import HipBackend
    return HipBackend()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _evaluate(hip, nb, x, cut, gradient=True):
    """-> dict of CPU tensors: energy (B,C), terms (2,B,C), grad (N,C,3), tiles (n_items)"""
    x = x.to("cuda")
    Cc = x.shape[1]
    plan = hip.nonbonded_plan(nb.atom_molptr_host, nb.N, Cc, x.device)
    e = torch.full((nb.B, Cc), FILL, device="cuda")
    te = torch.full((2, nb.B, Cc), FILL, device="cuda")
    g = torch.full_like(x, FILL) if gradient else None
    tiles = torch.full((plan[1],), FILL_I, dtype=torch.int32, device="cuda")
    hip.nonbonded(x, nb.atom_molptr, nb.charge, nb.sigma, nb.epsilon, nb.exc_ptr, nb.exc_atom, nb.exc_qq, nb.exc_sigma, nb.exc_eps, e, te, g,
                  plan=plan, cutoff=cut, tiles=tiles)
    torch.cuda.synchronize()
    return dict(energy=e.cpu(), terms=te.cpu(), grad=None if g is None else g.cpu(), tiles=tiles.cpu())


@pytest.mark.parametrize("name,nominal", nc.CASES, ids=[f"{n}-{c}A" for n, c in nc.CASES])
def test_energy_terms_gradient_and_tiles(hip, name, nominal):
    """every variant (switch or none, eps 78.3 or 1): energy, both terms and every gradient row through nonbonded_refs' gate; `tiles`
    equals the host restatement item for item; prune = 0 gives the same bits and evaluates every tile"""
    params, nb, x = nc.inputs(name)
    nbd = nc.NonbondedBatch(params).to("cuda")
    for switch, eps in nc.VARIANTS:
        r64, r32 = nc.refs(name, nominal, switch, eps)
        cut = nc.cutoff_of(name, nominal, switch, eps)
        got = _evaluate(hip, nbd, x, cut)
        what = f"{name} rc {cut.distance} switch {cut.switch_distance} eps {eps}"
        nr.gate_all(got["energy"], got["terms"], got["grad"], r64, r32, what)
        want, full, _ = nc.expected_tiles(params, x.numpy(), cut)
        assert got["tiles"].tolist() == want.tolist(), f"{what}: tiles {got['tiles'].tolist()} expected {want.tolist()}"
        every = _evaluate(hip, nbd, x, nc.cutoff_of(name, nominal, switch, eps, prune=False))
        assert every["tiles"].tolist() == full.tolist(), f"{what}: prune = 0 skipped a tile"
        for k in ("energy", "terms", "grad"):
            assert torch.equal(_bits(got[k]), _bits(every[k])), f"{what}: {k} differs between prune = 1 and prune = 0"


def test_the_second_batch_of_verdicts(hip):
    """a molecule of 257 tiles (nb_cut_refs.BIG): a work item decides its tiles 256 at a time, so tile 256 belongs to a second batch.
    `tiles` equals the host restatement item for item, and energy, terms and gradient have the bits of the call that evaluates every
    tile (no dense reference at this size: the formulas are gated on the smaller cases)"""
    params, nb, x = nc.inputs(nc.BIG)
    nbd = nc.NonbondedBatch(params).to("cuda")
    cut = nc.Cutoff(nc.BIG_CUTOFF, 0.8 * nc.BIG_CUTOFF)
    got = _evaluate(hip, nbd, x, cut)
    want, full, _ = nc.expected_tiles(params, x.numpy(), cut)
    assert got["tiles"].tolist() == want.tolist(), f"tiles {got['tiles'].tolist()} expected {want.tolist()}"
    every = _evaluate(hip, nbd, x, nc.Cutoff(nc.BIG_CUTOFF, 0.8 * nc.BIG_CUTOFF, prune=False))
    assert every["tiles"].tolist() == full.tolist() and full.tolist() == [257] * 257, "prune = 0 skipped a tile"
    for k in ("energy", "terms", "grad"):
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(_bits(got[k]), _bits(every[k])), f"{k} differs between prune = 1 and prune = 0"


def test_the_same_call_twice_gives_the_same_bits(hip):
    params, nb, x = nc.inputs("c513_C3")
    nbd = nc.NonbondedBatch(params).to("cuda")
    cut = nc.cutoff_of("c513_C3", 9.0, True, 78.3)
    a, b = _evaluate(hip, nbd, x, cut), _evaluate(hip, nbd, x, cut)
    for k in ("energy", "terms", "grad", "tiles"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


def test_a_molecule_alone_and_inside_the_mixed_batch_gives_the_same_bits(hip):
    params, nb, x = nc.inputs("chain_mixed")
    cut = nc.cutoff_of("chain_mixed", 9.0, True, 78.3)
    whole = _evaluate(hip, nc.NonbondedBatch(params).to("cuda"), x, cut)
    ptr = np.concatenate([[0], np.cumsum([p.n_atoms for p in params])])
    for b, p in enumerate(params):
        alone = _evaluate(hip, nc.NonbondedBatch([p]).to("cuda"), x[ptr[b]:ptr[b + 1]], cut)
        assert torch.equal(_bits(alone["energy"][0]), _bits(whole["energy"][b])), b
        assert torch.equal(_bits(alone["terms"][:, 0]), _bits(whole["terms"][:, b])), b
        assert torch.equal(_bits(alone["grad"]), _bits(whole["grad"][ptr[b]:ptr[b + 1]])), b


def test_the_energy_alone_has_the_bits_of_the_call_with_the_gradient(hip):
    params, nb, x = nc.inputs("c129_C3")
    nbd = nc.NonbondedBatch(params).to("cuda")
    cut = nc.cutoff_of("c129_C3", 6.0, False, 78.3)
    a, b = _evaluate(hip, nbd, x, cut), _evaluate(hip, nbd, x, cut, gradient=False)
    assert torch.equal(_bits(a["energy"]), _bits(b["energy"])) and torch.equal(_bits(a["terms"]), _bits(b["terms"]))


def test_refusals_launch_nothing_and_write_nothing(hip):
    """options outside the ranges of grappa_nb_cut, a NULL cut, a misaligned or short workspace: GRAPPA_ERR_ARG / _WORKSPACE, no launch
    (grappa_launch_count), nothing written (guarded buffers)"""
    params, nb, x = nc.inputs("nTp1_C3")
    nbd = nc.NonbondedBatch(params).to("cuda")
    xd = x.to("cuda")
    Cc = xd.shape[1]
    table, n_items, n_blocks, _ = hip.nonbonded_plan(nbd.atom_molptr_host, nbd.N, Cc, xd.device)
    lib = hip.lib
    need = int(lib.grappa_nonbonded_cut_workspace_bytes(Cc, n_blocks))
    assert need >= 56 * n_blocks * Cc and lib.grappa_nonbonded_cut_workspace_bytes(0, n_blocks) == 0
    d = _lib.NbDesc()
    d.N, d.C, d.B, d.xyz = nbd.N, Cc, nbd.B, xd.data_ptr()
    for n in ("atom_molptr", "charge", "sigma", "epsilon", "exc_ptr", "exc_atom", "exc_qq", "exc_sigma", "exc_eps"):
        setattr(d, n, getattr(nbd, n).data_ptr())
    bufs = {"energy": torch.full((64 + nbd.B * Cc + 64,), FILL, device="cuda"), "terms": torch.full((64 + 2 * nbd.B * Cc + 64,), FILL, device="cuda"),
            "grad": torch.full((64 + xd.numel() + 64,), FILL, device="cuda"),
            "tiles": torch.full((64 + n_items + 64,), FILL_I, dtype=torch.int32, device="cuda")}
    ws = torch.full((GUARD_B + need + GUARD_B,), FILL_B, dtype=torch.uint8, device="cuda")
    ptr = lambda t, off=64: t.data_ptr() + off * t.element_size()      # noqa: E731

    def call(cut, ws_off=GUARD_B, ws_bytes=need):
        return lib.grappa_nonbonded_fwd_cut_f32(None, C.byref(d), None if cut is None else C.byref(cut), table.data_ptr(), n_items, n_blocks,
                                                ptr(bufs["energy"]), ptr(bufs["terms"]), ptr(bufs["grad"]), ptr(bufs["tiles"]),
                                                ws.data_ptr() + ws_off, ws_bytes)

    good = dict(cutoff=4.0, switch_distance=3.2, rf_dielectric=78.3, prune=1)
    bad = [dict(good, cutoff=0.0), dict(good, cutoff=-1.0), dict(good, cutoff=float("inf")), dict(good, cutoff=float("nan")),
           dict(good, switch_distance=4.0), dict(good, switch_distance=5.0), dict(good, switch_distance=-0.5), dict(good, switch_distance=float("nan")),
           dict(good, rf_dielectric=0.5), dict(good, rf_dielectric=float("inf")), dict(good, rf_dielectric=float("nan")), dict(good, prune=2),
           dict(good, prune=-1)]
    torch.cuda.synchronize()
    before = lib.grappa_launch_count(0)
    for o in bad:
        assert call(_lib.NbCut(**o)) == -1, o
    assert call(None) == -1
    assert call(_lib.NbCut(**good), ws_off=GUARD_B + 4) == -1          # a workspace that is not 16-byte aligned
    assert call(_lib.NbCut(**good), ws_bytes=need - 1) == -3           # GRAPPA_ERR_WORKSPACE
    assert lib.grappa_launch_count(0) == before, "a refused call launched something"
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert bool((t == (FILL_I if t.dtype == torch.int32 else FILL)).all()), f"a refused call wrote {k}"
    assert bool((ws == FILL_B).all()), "a refused call wrote to the workspace"
    # the same buffers with good options: 3 launches, everything written, nothing outside
    assert call(_lib.NbCut(**good)) == 0
    assert lib.grappa_launch_count(0) == before + 3
    torch.cuda.synchronize()
    for k, t in bufs.items():
        fill = FILL_I if t.dtype == torch.int32 else FILL
        assert bool((t[:64] == fill).all()) and bool((t[-64:] == fill).all()), f"written outside {k}"
        assert not bool((t[64:-64] == fill).any()), f"{k} was not written everywhere"
    assert bool((ws[:GUARD_B] == FILL_B).all()) and bool((ws[-GUARD_B:] == FILL_B).all()), "written outside the workspace"


def test_the_numpy_door_takes_a_cutoff(hip):
    """nonbonded_energy(..., cutoff=) and NonbondedBatch.evaluate(..., cutoff=): a plain float is a Cutoff"""
    from grappa_amd.nonbonded import nonbonded_energy
    params, nb, x = nc.inputs("c129_C3")
    rc, _ = nc.placed("c129_C3", 9.0)
    r64, r32 = nc.nb_cut_ref(params, x, nc.Cutoff(rc), torch.float64), nc.nb_cut_ref(params, x, nc.Cutoff(rc), torch.float32)
    e, g = nonbonded_energy(params[0], x.numpy().transpose(1, 0, 2), cutoff=rc)
    nr.gate_all(torch.from_numpy(e)[None], None, torch.from_numpy(g.transpose(1, 0, 2)), r64, r32, "nonbonded_energy(cutoff=float)")
    e2, _ = nc.NonbondedBatch(params).to("cuda").evaluate(x.to("cuda"), cutoff=nc.Cutoff(rc))
    assert torch.equal(_bits(e2.cpu()), _bits(torch.from_numpy(e).float()[None]))
