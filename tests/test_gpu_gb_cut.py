"""GPU: the GB/SA implicit solvent under a cutoff (grappa_gb_obc_fwd_cut_f32 through HipBackend.gb_obc(cut=)) against the float64
restatement of tests/gb_cut_refs.py, whose gradient is autograd of the restated, truncated energy.  Cases, placed cutoffs and the
scales of the gate are gb_cut_refs'; tests/test_host_gb_cut.py asserts on the CPU what these tests need of their inputs (a real share
of the pairs on each side of every cutoff, no pair within 1e-4 A of it, no tile at the threshold, the chain skips most of its tiles)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gb_cut_refs as gc
import gb_refs as gr
from grappa_amd import _lib
from grappa_amd.solvent import GBBatch, ImplicitSolvent, solvent_energy

pytestmark = pytest.mark.gpu

FILL, FILL_B, FILL_I = 1024.0, 0xA5, -77
GUARD_B = 4096
KEYS = ("energy", "terms", "grad", "born")


@pytest.fixture(scope="module")
def hip():
    from grappa_amd.backend import HipBackend
    return HipBackend()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _evaluate(hip, nbp, gbp, x, solvent, gradient=True, born=True, gb=None):
    """-> dict of CPU tensors: energy (B,C), terms (2,B,C), grad (N,C,3) or None, born (N,C) or None, tiles (n_items,)"""
    nb = gr.NonbondedBatch(nbp).to("cuda")
    gb = GBBatch(gbp).to("cuda") if gb is None else gb
    x = x.to("cuda")
    Cc = x.shape[1]
    plan = hip.nonbonded_plan(nb.atom_molptr_host, nb.N, Cc, x.device)
    e = torch.full((nb.B, Cc), FILL, device="cuda")
    te = torch.full((2, nb.B, Cc), FILL, device="cuda")
    g = torch.full_like(x, FILL) if gradient else None
    br = torch.full((nb.N, Cc), FILL, device="cuda") if born else None
    tl = torch.full((plan[1],), FILL_I, dtype=torch.int32, device="cuda")
    hip.gb_obc(x, nb.atom_molptr, nb.charge, gb.radius, gb.scale, solvent.as_opts(), e, te, g, br, plan=plan, cut=solvent.cut_opts(), tiles=tl)
    torch.cuda.synchronize()
    return dict(energy=e.cpu(), terms=te.cpu(), grad=None if g is None else g.cpu(), born=None if br is None else br.cpu(), tiles=tl.cpu())


def _report(name, got, r64, r32):
    u = gr.C_GATE * 2.0 ** -24
    for key, scale, width in (("grad", "abs_g", 3), ("born", "abs_born", 1), ("energy", "abs_e", 1)):
        dg = (got[key].double() - r64[key]).abs().reshape(-1, width).amax(1)
        dr = (r32[key].double() - r64[key]).abs().reshape(-1, width).amax(1)
        bound = 2 * dr + u * r64[scale].reshape(-1)
        live = bound > 0
        if bool(live.any()):
            print(f"{name} {key}: largest |gpu - f64| {float(dg.max()):.3e}, |f32 - f64| {float(dr.max()):.3e}, floor {float((u * r64[scale]).max()):.3e}; "
                  f"largest |gpu - f64| / bound {float((dg[live] / bound[live]).max()):.3f}")


@pytest.mark.parametrize("name,nominal", gc.CASES)
def test_energy_terms_gradient_and_born_radii_under_the_cutoff(hip, name, nominal):
    """every case at its placed cutoff: energy, both terms, every gradient row and every Born radius through the calibrated gate, with
    the scales of the truncated restatement"""
    nbp, gbp, x = gr.inputs(name)
    r64, r32 = gc.refs(name, nominal)
    got = _evaluate(hip, nbp, gbp, x, gc.solvent_of(name, nominal))
    _report(f"{name} @ {nominal}", got, r64, r32)
    gr.gate_all(got, r64, r32, f"{name} @ {nominal}")


def test_obc1_under_the_cutoff(hip):
    nbp, gbp, x = gr.inputs("n257")
    sv = gc.solvent_of("n257", 6.0, model="obc1")
    r64, r32 = gc.gb_cut_ref(nbp, gbp, x, sv, torch.float64), gc.gb_cut_ref(nbp, gbp, x, sv, torch.float32)
    gr.gate_all(_evaluate(hip, nbp, gbp, x, sv), r64, r32, "n257 obc1 @ 6")


@pytest.mark.parametrize("name,nominal", gc.PRUNING)
def test_tiles_are_those_of_the_host_restatement(hip, name, nominal):
    """item for item, with and without pruning"""
    nbp, gbp, x = gr.inputs(name)
    rc = gc.placed(name, nominal)[0]
    want, full, _ = gc.expected_tiles(gc.counts_of(name), x.numpy(), rc)
    got = _evaluate(hip, nbp, gbp, x, gc.solvent_of(name, nominal))["tiles"].numpy()
    assert np.array_equal(got, want), (got, want)
    every = _evaluate(hip, nbp, gbp, x, gc.solvent_of(name, nominal, prune=False))["tiles"].numpy()
    assert np.array_equal(every, full)


@pytest.mark.parametrize("name,nominal", [("chain513", 9.0), ("n257", 6.0), ("mixed", 6.0)])
def test_pruning_does_not_change_a_bit(hip, name, nominal):
    nbp, gbp, x = gr.inputs(name)
    a = _evaluate(hip, nbp, gbp, x, gc.solvent_of(name, nominal, prune=True))
    b = _evaluate(hip, nbp, gbp, x, gc.solvent_of(name, nominal, prune=False))
    for k in KEYS:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


def test_the_second_batch_of_verdicts(hip):
    """16,448 atoms are 257 j-tiles: a work item asks for its verdicts twice.  No dense reference: tiles against the host restatement,
    and prune 0 against 1 bit for bit"""
    nbp, gbp, x = gc.big_inputs()
    sv1, sv0 = ImplicitSolvent(cutoff=gc.BIG_CUTOFF), ImplicitSolvent(cutoff=gc.BIG_CUTOFF, prune=False)
    want, full, closest = gc.expected_tiles([nbp[0].n_atoms], x.numpy(), gc.BIG_CUTOFF)
    assert full[0] == 257 and closest > 1e-5 and want.sum() < full.sum() // 10
    a, b = _evaluate(hip, nbp, gbp, x, sv1), _evaluate(hip, nbp, gbp, x, sv0)
    assert np.array_equal(a["tiles"].numpy(), want) and np.array_equal(b["tiles"].numpy(), full)
    for k in KEYS:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    assert bool(torch.isfinite(a["grad"]).all()) and bool(torch.isfinite(a["energy"]).all())


@pytest.mark.parametrize("name", ["n2Tp1_C3", "mixed", "n257"])
def test_a_cutoff_beyond_the_diameter_is_the_all_pairs_energy(hip, name):
    """through the same gate against the ALL-PAIRS restatement.  (Not the bits of grappa_gb_obc_fwd_f32: the cut passes form r2 with a
    fixed order of roundings, the all-pairs passes leave its contraction to the compiler -- DESIGN.md section 22.)"""
    nbp, gbp, x = gr.inputs(name)
    r64, r32 = gr.refs(name)
    got = _evaluate(hip, nbp, gbp, x, ImplicitSolvent(cutoff=100.0))
    _report(f"{name} @ 100", got, r64, r32)
    gr.gate_all(got, r64, r32, f"{name} @ 100")


def test_the_same_call_twice_gives_the_same_bits(hip):
    nbp, gbp, x = gr.inputs("chain513")
    sv = gc.solvent_of("chain513", 9.0)
    a, b = _evaluate(hip, nbp, gbp, x, sv), _evaluate(hip, nbp, gbp, x, sv)
    for k in KEYS + ("tiles",):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


def test_a_molecule_alone_and_inside_the_mixed_batch_gives_the_same_bits(hip):
    nbp, gbp, x = gr.inputs("mixed")
    sv = gc.solvent_of("mixed", 6.0)
    whole = _evaluate(hip, nbp, gbp, x, sv)
    ptr = np.concatenate([[0], np.cumsum([p.n_atoms for p in nbp])])
    assert 0 in np.diff(ptr), "the mixed case lost its empty molecule"
    for b, (p, g) in enumerate(zip(nbp, gbp)):
        if p.n_atoms == 0:
            assert bool((whole["energy"][b] == 0).all()) and bool((whole["terms"][:, b] == 0).all())
            continue
        alone = _evaluate(hip, [p], [g], x[ptr[b]:ptr[b + 1]], sv)
        assert torch.equal(_bits(alone["energy"][0]), _bits(whole["energy"][b])), b
        assert torch.equal(_bits(alone["terms"][:, 0]), _bits(whole["terms"][:, b])), b
        assert torch.equal(_bits(alone["grad"]), _bits(whole["grad"][ptr[b]:ptr[b + 1]])), b
        assert torch.equal(_bits(alone["born"]), _bits(whole["born"][ptr[b]:ptr[b + 1]])), b


def test_the_energy_alone_has_the_bits_of_the_call_with_the_gradient(hip):
    nbp, gbp, x = gr.inputs("n257")
    sv = gc.solvent_of("n257", 6.0)
    a, b = _evaluate(hip, nbp, gbp, x, sv), _evaluate(hip, nbp, gbp, x, sv, gradient=False, born=False)
    assert torch.equal(_bits(a["energy"]), _bits(b["energy"])) and torch.equal(_bits(a["terms"]), _bits(b["terms"]))
    assert torch.equal(a["tiles"], b["tiles"])


def test_refusals_launch_nothing_and_write_nothing(hip):
    """gbcut == NULL, a cutoff that is not finite and > 0 or whose square overflows, a prune other than 0 or 1, and refusals of the entry
    it extends: GRAPPA_ERR_ARG / _WORKSPACE, no launch, nothing written between the guard words; then the same buffers with good options:
    4 launches without the gradient, 5 with it, everything written, nothing outside"""
    nbp, gbp, x = gr.inputs("nTp1_C3")
    nb, gb = gr.NonbondedBatch(nbp).to("cuda"), GBBatch(gbp).to("cuda")
    xd = x.to("cuda")
    Cc = xd.shape[1]
    table, n_items, n_blocks, _ = hip.nonbonded_plan(nb.atom_molptr_host, nb.N, Cc, xd.device)
    lib = hip.lib
    need = int(lib.grappa_gb_obc_cut_workspace_bytes(nb.N, Cc, n_blocks))
    assert need >= int(lib.grappa_gb_obc_workspace_bytes(nb.N, Cc, n_blocks)) + 32 * n_blocks * Cc
    assert lib.grappa_gb_obc_cut_workspace_bytes(0, Cc, n_blocks) == 0 and lib.grappa_gb_obc_cut_workspace_bytes(nb.N, Cc, 0) == 0
    d = _lib.NbDesc()
    d.N, d.C, d.B, d.xyz, d.atom_molptr, d.charge = nb.N, Cc, nb.B, xd.data_ptr(), nb.atom_molptr.data_ptr(), nb.charge.data_ptr()
    bufs = {"energy": torch.full((64 + nb.B * Cc + 64,), FILL, device="cuda"), "terms": torch.full((64 + 2 * nb.B * Cc + 64,), FILL, device="cuda"),
            "grad": torch.full((64 + xd.numel() + 64,), FILL, device="cuda"), "born": torch.full((64 + nb.N * Cc + 64,), FILL, device="cuda"),
            "tiles": torch.full((64 + n_items + 64,), FILL_I, dtype=torch.int32, device="cuda")}
    fill = {k: (FILL_I if k == "tiles" else FILL) for k in bufs}
    ws = torch.full((GUARD_B + need + GUARD_B,), FILL_B, dtype=torch.uint8, device="cuda")
    ptr = lambda t, off=64: t.data_ptr() + off * t.element_size()      # noqa: E731
    g_ok = _lib.GbDesc(radius=gb.radius.data_ptr(), scale=gb.scale.data_ptr(), **ImplicitSolvent().as_opts())
    rc = gc.placed("nTp1_C3", 6.0)[0]

    def call(cut, g=g_ok, nbd=d, ws_off=GUARD_B, ws_bytes=need, tab=table.data_ptr(), grad=True):
        return lib.grappa_gb_obc_fwd_cut_f32(None, None if nbd is None else C.byref(nbd), None if g is None else C.byref(g),
                                             None if cut is None else C.byref(cut), tab, n_items, n_blocks, ptr(bufs["energy"]),
                                             ptr(bufs["terms"]), ptr(bufs["grad"]) if grad else None, ptr(bufs["born"]), ptr(bufs["tiles"]),
                                             ws.data_ptr() + ws_off, ws_bytes)

    nan, inf = float("nan"), float("inf")
    torch.cuda.synchronize()
    before = lib.grappa_launch_count(0)
    for cutoff, prune in ((0.0, 1), (-1.0, 1), (nan, 1), (inf, 1), (1e20, 1), (rc, 2), (rc, -1)):
        assert call(_lib.GbCut(cutoff=cutoff, prune=prune)) == -1, (cutoff, prune)
    good = _lib.GbCut(cutoff=rc, prune=1)
    assert call(None) == -1
    assert call(good, g=None) == -1 and call(good, nbd=None) == -1 and call(good, tab=None) == -1
    bad_g = _lib.GbDesc(radius=gb.radius.data_ptr(), scale=gb.scale.data_ptr(), **{**ImplicitSolvent().as_opts(), "eps_in": 0.0})
    assert call(good, g=bad_g) == -1
    assert call(good, ws_off=GUARD_B + 4) == -1            # a workspace that is not 16-byte aligned
    assert call(good, ws_bytes=need - 1) == -3             # GRAPPA_ERR_WORKSPACE
    assert lib.grappa_launch_count(0) == before, "a refused call launched something"
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert bool((t == fill[k]).all()), f"a refused call wrote {k}"
    assert bool((ws == FILL_B).all()), "a refused call wrote to the workspace"
    assert call(good, grad=False) == 0
    assert lib.grappa_launch_count(0) == before + 4
    torch.cuda.synchronize()
    assert bool((bufs["grad"] == FILL).all()), "grad == NULL wrote a gradient"
    assert call(good) == 0
    assert lib.grappa_launch_count(0) == before + 4 + 5
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert bool((t[:64] == fill[k]).all()) and bool((t[-64:] == fill[k]).all()), f"written outside {k}"
        assert not bool((t[64:-64] == fill[k]).any()), f"{k} was not written everywhere"
    assert bool((ws[:GUARD_B] == FILL_B).all()) and bool((ws[-GUARD_B:] == FILL_B).all()), "written outside the workspace"


def test_a_nan_coordinate_is_found_in_its_molecule_only(hip):
    """a NaN coordinate makes its block's box NaN, which counts as near: the pairs are evaluated and the molecule's results are
    non-finite, with and without pruning; the other molecules keep their bits"""
    nbp, gbp, x = gr.inputs("mixed")
    sv = gc.solvent_of("mixed", 6.0)
    whole = _evaluate(hip, nbp, gbp, x, sv)
    ptr = np.concatenate([[0], np.cumsum([p.n_atoms for p in nbp])])
    b_bad = 4
    xb = x.clone()
    xb[int(ptr[b_bad]) + 3, 1, 2] = float("nan")
    for prune in (True, False):
        got = _evaluate(hip, nbp, gbp, xb, ImplicitSolvent(cutoff=sv.cutoff, prune=prune))
        assert bool(torch.isnan(got["energy"][b_bad, 1])) and not bool(torch.isfinite(got["grad"][ptr[b_bad]:ptr[b_bad + 1], 1]).all())
        assert torch.equal(_bits(got["energy"][b_bad, 0]), _bits(whole["energy"][b_bad, 0]))          # the other conformations are untouched
        for b in range(len(nbp)):
            if b != b_bad:
                assert torch.equal(_bits(got["energy"][b]), _bits(whole["energy"][b])), b
                assert torch.equal(_bits(got["grad"][ptr[b]:ptr[b + 1]]), _bits(whole["grad"][ptr[b]:ptr[b + 1]])), b


def test_parameters_outside_the_model_give_nan_for_their_molecule_only(hip):
    nbp, gbp, x = gr.inputs("mixed")
    sv = gc.solvent_of("mixed", 6.0)
    whole = _evaluate(hip, nbp, gbp, x, sv)
    gb = GBBatch(gbp).to("cuda")
    ptr = np.concatenate([[0], np.cumsum([p.n_atoms for p in nbp])])
    b_bad = 3
    gb.radius[int(ptr[b_bad]) + 2] = 0.05
    got = _evaluate(hip, nbp, gbp, x, sv, gb=gb)
    assert bool(torch.isnan(got["energy"][b_bad]).all())
    for b in range(len(nbp)):
        if b != b_bad:
            assert torch.equal(_bits(got["energy"][b]), _bits(whole["energy"][b])), b
            assert torch.equal(_bits(got["grad"][ptr[b]:ptr[b + 1]]), _bits(whole["grad"][ptr[b]:ptr[b + 1]])), b


def test_the_numpy_door(hip):
    """solvent_energy with an ImplicitSolvent that carries a cutoff: numpy in and out, against the truncated restatement, with tiles"""
    name, nominal = "n257", 6.0
    nbp, gbp, x = gr.inputs(name)
    r64, r32 = gc.refs(name, nominal)
    (e, g, ep, es, br), tiles = solvent_energy(nbp[0], gbp[0], x.numpy().transpose(1, 0, 2), model=gc.solvent_of(name, nominal), terms=True,
                                               born_radii=True, tiles=True)
    got = dict(energy=torch.from_numpy(e)[None], terms=torch.from_numpy(np.stack([ep, es]))[:, None], grad=torch.from_numpy(g.transpose(1, 0, 2)),
               born=torch.from_numpy(br.T))
    gr.gate_all(got, r64, r32, "solvent_energy under a cutoff")
    assert np.array_equal(tiles, gc.expected_tiles(gc.counts_of(name), x.numpy(), gc.placed(name, nominal)[0])[0])
    with pytest.raises(ValueError, match="tiles"):
        solvent_energy(nbp[0], gbp[0], x.numpy().transpose(1, 0, 2), tiles=True)
