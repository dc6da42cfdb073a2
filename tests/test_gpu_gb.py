"""GPU: the GB/SA implicit solvent (grappa_gb_obc_fwd_f32 through HipBackend.gb_obc) against the float64 restatement of
tests/gb_refs.py, whose gradient is autograd of the restated energy.  Cases and the scales of the gate are gb_refs';
tests/test_host_gb.py asserts on the CPU what these tests need of their inputs (every branch of H occurs, no pair sits on a branch
border, the saturated and the unsaturated regime are both covered)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gb_refs as gr
from grappa_amd import _lib
from grappa_amd.solvent import GBBatch, ImplicitSolvent, solvent_energy

pytestmark = pytest.mark.gpu

FILL, FILL_B = 1024.0, 0xA5
GUARD_B = 4096


@pytest.fixture(scope="module")
def hip():
    from grappa_amd.backend import HipBackend
    return HipBackend()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _evaluate(hip, nbp, gbp, x, solvent="obc2", gradient=True, born=True):
    """-> dict of CPU tensors: energy (B,C), terms (2,B,C), grad (N,C,3) or None, born (N,C) or None"""
    nb, gb = gr.NonbondedBatch(nbp).to("cuda"), GBBatch(gbp).to("cuda")
    x = x.to("cuda")
    Cc = x.shape[1]
    plan = hip.nonbonded_plan(nb.atom_molptr_host, nb.N, Cc, x.device)
    e = torch.full((nb.B, Cc), FILL, device="cuda")
    te = torch.full((2, nb.B, Cc), FILL, device="cuda")
    g = torch.full_like(x, FILL) if gradient else None
    br = torch.full((nb.N, Cc), FILL, device="cuda") if born else None
    hip.gb_obc(x, nb.atom_molptr, nb.charge, gb.radius, gb.scale, gr.as_implicit_solvent(solvent).as_opts(), e, te, g, br, plan=plan)
    torch.cuda.synchronize()
    return dict(energy=e.cpu(), terms=te.cpu(), grad=None if g is None else g.cpu(), born=None if br is None else br.cpu())


@pytest.mark.parametrize("name", gr.CASES)
def test_energy_terms_gradient_and_born_radii(hip, name):
    """every case: energy, both terms, every gradient row and every Born radius through the calibrated gate"""
    nbp, gbp, x = gr.inputs(name)
    r64, r32 = gr.refs(name)
    got = _evaluate(hip, nbp, gbp, x)
    u = gr.C_GATE * 2.0 ** -24
    for key, scale, width in (("grad", "abs_g", 3), ("born", "abs_born", 1), ("energy", "abs_e", 1)):
        dg = (got[key].double() - r64[key]).abs().reshape(-1, width).amax(1)
        dr = (r32[key].double() - r64[key]).abs().reshape(-1, width).amax(1)
        bound = 2 * dr + u * r64[scale].reshape(-1)
        live = bound > 0
        if bool(live.any()):
            print(f"{name} {key}: largest |gpu - f64| {float(dg.max()):.3e}, |f32 - f64| {float(dr.max()):.3e}, floor {float((u * r64[scale]).max()):.3e}; "
                  f"largest |gpu - f64| / bound {float((dg[live] / bound[live]).max()):.3f}")
    gr.gate_all(got, r64, r32, name)


@pytest.mark.parametrize("name", ["branches", "nTp1_C3"])
def test_obc1(hip, name):
    """the other parameter set of the same formula"""
    nbp, gbp, x = gr.inputs(name)
    r64, r32 = gr.refs(name, "obc1")
    gr.gate_all(_evaluate(hip, nbp, gbp, x, "obc1"), r64, r32, f"{name} obc1")


def test_the_same_call_twice_gives_the_same_bits(hip):
    nbp, gbp, x = gr.inputs("chain513")
    a, b = _evaluate(hip, nbp, gbp, x), _evaluate(hip, nbp, gbp, x)
    for k in ("energy", "terms", "grad", "born"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


def test_a_molecule_alone_and_inside_the_mixed_batch_gives_the_same_bits(hip):
    nbp, gbp, x = gr.inputs("mixed")
    whole = _evaluate(hip, nbp, gbp, x)
    ptr = np.concatenate([[0], np.cumsum([p.n_atoms for p in nbp])])
    assert 0 in np.diff(ptr), "the mixed case lost its empty molecule"
    for b, (p, g) in enumerate(zip(nbp, gbp)):
        if p.n_atoms == 0:
            assert bool((whole["energy"][b] == 0).all()) and bool((whole["terms"][:, b] == 0).all())
            continue
        alone = _evaluate(hip, [p], [g], x[ptr[b]:ptr[b + 1]])
        assert torch.equal(_bits(alone["energy"][0]), _bits(whole["energy"][b])), b
        assert torch.equal(_bits(alone["terms"][:, 0]), _bits(whole["terms"][:, b])), b
        assert torch.equal(_bits(alone["grad"]), _bits(whole["grad"][ptr[b]:ptr[b + 1]])), b
        assert torch.equal(_bits(alone["born"]), _bits(whole["born"][ptr[b]:ptr[b + 1]])), b


def test_the_energy_alone_has_the_bits_of_the_call_with_the_gradient(hip):
    nbp, gbp, x = gr.inputs("n2Tp1_C3")
    a, b = _evaluate(hip, nbp, gbp, x), _evaluate(hip, nbp, gbp, x, gradient=False, born=False)
    assert torch.equal(_bits(a["energy"]), _bits(b["energy"])) and torch.equal(_bits(a["terms"]), _bits(b["terms"]))


def test_equal_dielectrics_and_no_surface_tension_give_exact_zeros(hip):
    nbp, gbp, x = gr.inputs("nTp1_C3")
    got = _evaluate(hip, nbp, gbp, x, ImplicitSolvent("obc2", 2.0, 2.0, 0.0))
    for k in ("energy", "terms", "grad"):
        assert bool((got[k] == 0).all()), k
    assert bool((got["born"] > 0).all())


def test_refusals_launch_nothing_and_write_nothing(hip):
    """options outside the ranges of grappa_gb_desc, NULL descriptors or tables, a misaligned or short workspace: GRAPPA_ERR_ARG /
    _WORKSPACE, no launch (grappa_launch_count), nothing written (guarded buffers); then the same buffers with good options: 4 launches
    (3 without the gradient), everything written, nothing outside"""
    nbp, gbp, x = gr.inputs("nTp1_C3")
    nb, gb = gr.NonbondedBatch(nbp).to("cuda"), GBBatch(gbp).to("cuda")
    xd = x.to("cuda")
    Cc = xd.shape[1]
    table, n_items, n_blocks, _ = hip.nonbonded_plan(nb.atom_molptr_host, nb.N, Cc, xd.device)
    lib = hip.lib
    need = int(lib.grappa_gb_obc_workspace_bytes(nb.N, Cc, n_blocks))
    assert need >= 12 * nb.N * Cc + 16 * n_blocks * Cc and lib.grappa_gb_obc_workspace_bytes(0, Cc, n_blocks) == 0
    d = _lib.NbDesc()
    d.N, d.C, d.B, d.xyz, d.atom_molptr, d.charge = nb.N, Cc, nb.B, xd.data_ptr(), nb.atom_molptr.data_ptr(), nb.charge.data_ptr()
    bufs = {"energy": torch.full((64 + nb.B * Cc + 64,), FILL, device="cuda"), "terms": torch.full((64 + 2 * nb.B * Cc + 64,), FILL, device="cuda"),
            "grad": torch.full((64 + xd.numel() + 64,), FILL, device="cuda"), "born": torch.full((64 + nb.N * Cc + 64,), FILL, device="cuda")}
    ws = torch.full((GUARD_B + need + GUARD_B,), FILL_B, dtype=torch.uint8, device="cuda")
    ptr = lambda t, off=64: t.data_ptr() + off * t.element_size()      # noqa: E731
    good = ImplicitSolvent().as_opts()

    def desc(**over):
        return _lib.GbDesc(radius=gb.radius.data_ptr(), scale=gb.scale.data_ptr(), **{**good, **over})

    def call(g, nbd=d, ws_off=GUARD_B, ws_bytes=need, tab=table.data_ptr(), grad=True):
        return lib.grappa_gb_obc_fwd_f32(None, None if nbd is None else C.byref(nbd), None if g is None else C.byref(g), tab, n_items, n_blocks,
                                         ptr(bufs["energy"]), ptr(bufs["terms"]), ptr(bufs["grad"]) if grad else None, ptr(bufs["born"]),
                                         ws.data_ptr() + ws_off, ws_bytes)

    nan, inf = float("nan"), float("inf")
    bad = [dict(offset=nan), dict(offset=inf), dict(alpha=nan), dict(beta=inf), dict(gamma=nan), dict(eps_in=0.0), dict(eps_in=-1.0),
           dict(eps_in=nan), dict(eps_out=0.0), dict(eps_out=inf), dict(surface_tension=-0.1), dict(surface_tension=nan), dict(probe=-1.0),
           dict(probe=inf)]
    torch.cuda.synchronize()
    before = lib.grappa_launch_count(0)
    for o in bad:
        assert call(desc(**o)) == -1, o
    assert call(None) == -1 and call(desc(), nbd=None) == -1 and call(desc(), tab=None) == -1
    no_r = desc()
    no_r.radius = None
    assert call(no_r) == -1
    assert call(desc(), ws_off=GUARD_B + 4) == -1          # a workspace that is not 16-byte aligned
    assert call(desc(), ws_bytes=need - 1) == -3           # GRAPPA_ERR_WORKSPACE
    assert lib.grappa_launch_count(0) == before, "a refused call launched something"
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert bool((t == FILL).all()), f"a refused call wrote {k}"
    assert bool((ws == FILL_B).all()), "a refused call wrote to the workspace"
    assert call(desc(), grad=False) == 0
    assert lib.grappa_launch_count(0) == before + 3
    torch.cuda.synchronize()
    assert bool((bufs["grad"] == FILL).all()), "grad == NULL wrote a gradient"
    assert call(desc()) == 0
    assert lib.grappa_launch_count(0) == before + 3 + 4
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert bool((t[:64] == FILL).all()) and bool((t[-64:] == FILL).all()), f"written outside {k}"
        assert not bool((t[64:-64] == FILL).any()), f"{k} was not written everywhere"
    assert bool((ws[:GUARD_B] == FILL_B).all()) and bool((ws[-GUARD_B:] == FILL_B).all()), "written outside the workspace"


def test_parameters_outside_the_model_give_nan_for_their_molecule_only(hip):
    """radius and scale are device memory: a radius <= offset or a scale <= 0 that slipped past GBParameters.validate makes the results
    of ITS molecule NaN and leaves the other molecules' bits as they are"""
    nbp, gbp, x = gr.inputs("mixed")
    whole = _evaluate(hip, nbp, gbp, x)
    nb, gb = gr.NonbondedBatch(nbp).to("cuda"), GBBatch(gbp).to("cuda")
    ptr = np.concatenate([[0], np.cumsum([p.n_atoms for p in nbp])])
    b_bad = 3
    gb.radius[int(ptr[b_bad]) + 2] = 0.05
    xd = x.to("cuda")
    Cc = xd.shape[1]
    plan = hip.nonbonded_plan(nb.atom_molptr_host, nb.N, Cc, xd.device)
    e, g = torch.zeros(nb.B, Cc, device="cuda"), torch.zeros_like(xd)
    hip.gb_obc(xd, nb.atom_molptr, nb.charge, gb.radius, gb.scale, ImplicitSolvent().as_opts(), e, None, g, None, plan=plan)
    e, g = e.cpu(), g.cpu()
    assert bool(torch.isnan(e[b_bad]).all())
    for b in range(nb.B):
        if b != b_bad:
            assert torch.equal(_bits(e[b]), _bits(whole["energy"][b])) and torch.equal(_bits(g[ptr[b]:ptr[b + 1]]), _bits(whole["grad"][ptr[b]:ptr[b + 1]])), b


def test_the_numpy_door(hip):
    """solvent_energy: numpy in and out, against the restatement; a list of molecules gives each molecule's own results"""
    nbp, gbp, x = gr.inputs("nTp1_C3")
    r64, r32 = gr.refs("nTp1_C3")
    e, g, ep, es, br = solvent_energy(nbp[0], gbp[0], x.numpy().transpose(1, 0, 2), terms=True, born_radii=True)
    got = dict(energy=torch.from_numpy(e)[None], terms=torch.from_numpy(np.stack([ep, es]))[:, None], grad=torch.from_numpy(g.transpose(1, 0, 2)),
               born=torch.from_numpy(br.T))
    gr.gate_all(got, r64, r32, "solvent_energy")
    both = solvent_energy([nbp[0], nbp[0]], [gbp[0], gbp[0]], [x.numpy().transpose(1, 0, 2)] * 2, model=ImplicitSolvent("obc2"))
    assert len(both) == 2 and np.array_equal(both[0][0], e) and np.array_equal(both[1][1], g)
