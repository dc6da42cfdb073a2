"""GPU (-m gpu): the MM energy, its coordinate gradient and its double backward (csrc/mm_energy.hip) against float64 autograd of the
reference's formulas (oracle/cpu_ref.bond_length / bond_angle / dihedral, tests/kernel_refs.mm_ref64): every lane count of mm_bwd
(C = 1..1025), the energy kernel's loop over C > 1024, n_per = 1..8 with and without offset_torsion, and the geometries where the
formulas change regime (torsions at the atan2 branch cut on both sides, near 0, near-linear angles).

Gate (summation order and conditioning dominate): per row, the GPU's distance to float64 <= 2 x that of the farther of two fp32
implementations (the RefBackend closed forms, and the same autograd formulas run in fp32) + a stated floor."""
import math

import numpy as np
import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from grappa_amd.backend import HipBackend
    return HipBackend()


@pytest.fixture(scope="module")
def ref():
    from oracle.ops_ref import RefBackend
    return RefBackend()


LV = ["n2", "n3", "n4", "n4_improper"]


def _run(be, plan, xyz, ks, eqs, n_per, offset, gE, gG, dev):
    B, C, N = plan.B, xyz.shape[1], xyz.shape[0]
    c = lambda t: None if t is None else t.to(dev)        # noqa: E731
    e, terms, grad = torch.empty(B, C, device=dev), torch.empty(4, B, C, device=dev), torch.empty(N, C, 3, device=dev)
    te = [torch.empty(plan.T[l], C, device=dev) for l in LV]
    tx = [torch.empty(plan.T[l], C, device=dev) for l in LV]
    kk, ee = [c(k) for k in ks], [c(q) for q in eqs]
    be.mm_energy_fwd(plan, c(xyz), kk, ee, n_per, offset, e, terms, te, tx)
    be.mm_gradient_fwd(plan, c(xyz), kk, ee, n_per, grad)
    gks = [torch.zeros_like(k) for k in kk]
    geqs = [torch.zeros_like(ee[0]), torch.zeros_like(ee[1]), None, None]
    be.mm_bwd(plan, c(xyz), kk, ee, n_per, offset, c(gE), c(gG), gks, geqs)
    return dict(E=e, terms=terms, G=grad, te=te, tx=tx, gk=gks, geq=geqs[:2])


def _check(hip, ref, g, xyz, ks, eqs, n_per, offset, what):
    pc, pg = g.plan(), g.to("cuda").plan()
    B, C, N = pc.B, xyz.shape[1], xyz.shape[0]
    gen = torch.Generator().manual_seed(C + sum(n_per))
    gE, gG = torch.randn(B, C, generator=gen), torch.randn(N, C, 3, generator=gen)
    args = ([pc.idx32[l].long() for l in LV], [pc.mol_ptr[l] for l in LV], B, xyz, ks, eqs, n_per, offset, gE, gG)
    want, a32 = kr.mm_ref64(*args), kr.mm_ref64(*args, dtype=torch.float32)
    r32 = _run(ref, pc, xyz, ks, eqs, n_per, offset, gE, gG, "cpu")
    got = _run(hip, pg, xyz, ks, eqs, n_per, offset, gE, gG, "cuda")
    torch.cuda.synchronize()
    mx = lambda t: float(t.abs().max()) if t.numel() else 0.0     # noqa: E731

    def gate(name, c, l=None, **kw):
        pick = (lambda d: d[name]) if l is None else (lambda d: d[name][l])
        kr.assert_calibrated(pick(got), pick(r32), pick(want), c, max(mx(pick(want)), kw.pop("min_scale", 0.0)),
                             what + f" {name}" + ("" if l is None else f" {LV[l]}"), ref32b=pick(a32), **kw)

    # floors: 64 u of the tensor's largest value (energies and gradients are sums over a molecule's tuples); gk / geq sum over C
    # conformations: 256 u
    gate("E", 64)
    gate("G", 64)
    for l in range(4):
        gate("terms", 64, l)
        gate("te", 64, l)
        # internal coordinates modulo 2 pi: at the branch cut fp32 and float64 may return +pi and -pi
        gate("tx", 64, l, period=2 * math.pi, min_scale=1.0)
        gate("gk", 256, l)
    for l in range(2):
        gate("geq", 256, l)
    # translation invariance: zero net force per molecule and conformation, within 64 u of the sum of |dE/dx| over its atoms
    ptr = pc.atom_molptr.long()
    seg = torch.repeat_interleave(torch.arange(B), ptr[1:] - ptr[:-1])
    G = got["G"].cpu().double()
    net = torch.zeros(B, C, 3, dtype=torch.float64).index_add(0, seg, G)
    tot = torch.zeros(B, C, 1, dtype=torch.float64).index_add(0, seg, G.abs().sum(-1, keepdim=True))
    assert bool((net.abs() <= 64 * kr.U32 * tot).all()), what + ": net force"


def _params(plan, n_per, seed):
    gen = torch.Generator().manual_seed(seed)
    T = plan.T
    ks = [700 + 100 * torch.rand(T["n2"], generator=gen), 100 + 20 * torch.rand(T["n3"], generator=gen),
          torch.randn(T["n4"], n_per[2], generator=gen), torch.randn(T["n4_improper"], n_per[3], generator=gen)]
    eqs = [1.2 + 0.1 * torch.randn(T["n2"], generator=gen), 1.9 + 0.1 * torch.randn(T["n3"], generator=gen), None, None]
    return ks, eqs


def _lanes(c):
    """mm_bwd's lanes per tuple (csrc/mm_energy.hip lanes_per_tuple)"""
    return 64 if c > 32 else 32 if c > 16 else 16 if c > 8 else 8


@pytest.mark.parametrize("C", [1, 8, 9, 16, 17, 32, 33, 64, 1025], ids=lambda c: f"mm-C{c}-lanes{_lanes(c)}" + ("-energyloop" if c > 1024 else ""))
def test_mm_conformation_counts(hip, ref, C):
    from grappa_amd.datasets import build_batch_from_pool
    g = build_batch_from_pool(list(range(300, 304)) if C <= 64 else [300, 301], n_confs=C, seed=C)
    xyz = g.nodes["n1"].data["xyz"].contiguous()
    n_per = [0, 0, 6, 3]
    ks, eqs = _params(g.plan(), n_per, C)
    _check(hip, ref, g, xyz, ks, eqs, n_per, False, f"C={C}")


@pytest.mark.parametrize("offset", [False, True], ids=["plain", "offset"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8], ids=lambda n: f"mm-nper{n}")
def test_mm_periodicities(hip, ref, n, offset):
    """propers with n_per = n and impropers with 9 - n: every periodicity 1..8 on both levels"""
    from grappa_amd.datasets import build_batch_from_pool
    g = build_batch_from_pool([300, 301, 302], n_confs=12, seed=n)
    xyz = g.nodes["n1"].data["xyz"].contiguous()
    n_per = [0, 0, n, 9 - n]
    ks, eqs = _params(g.plan(), n_per, 100 + n)
    _check(hip, ref, g, xyz, ks, eqs, n_per, offset, f"n_per={n_per[2:]} offset={offset}")


# (angle (0,1,2), proper torsion (0,1,2,3)) per conformation
EDGE_CASES = [(1.9, math.pi - d) for d in (1e-4, 3e-5, 1e-5)] + [(1.9, -math.pi + d) for d in (1e-4, 3e-5, 1e-5)] + \
             [(1.9, d) for d in (1e-4, -1e-4, 1e-6)] + [(math.pi - 1e-2, 1.0), (math.pi - 1e-3, -2.0), (math.pi - 1e-2, math.pi - 1e-4),
                                                       (2.1, 0.7), (1.7, -1.3)]


def edge_molecules():
    """two 5-atom molecules (chain 0-1-2-3, atom 4 on 2) whose conformations put the proper torsion (0,1,2,3) within 1e-4 rad of +pi
    and of -pi (both sides of the atan2 branch cut) and near 0, and the angle (0,1,2) at pi - 1e-2 and pi - 1e-3 (never exactly
    collinear: the derivative is undefined there)"""
    from grappa_amd.batch import batch, single_graph
    C = len(EDGE_CASES)
    xyz = np.zeros((5, C, 3))
    for c, (th, phi) in enumerate(EDGE_CASES):
        p1, p2 = np.array([0.0, 0.0, 0.0]), np.array([1.5, 0.0, 0.0])
        p0 = p1 + 1.1 * np.array([math.cos(th), math.sin(th), 0.0])
        p3 = p2 + 1.2 * np.array([-math.cos(1.9), math.sin(1.9) * math.cos(phi), math.sin(1.9) * math.sin(phi)])
        p4 = p2 + np.array([0.4, -0.7, 0.9])
        xyz[:, c] = np.stack([p0, p1, p2, p3, p4])
    bonds = np.array([[0, 1], [1, 2], [2, 3], [2, 4]])
    idxs = {"n2": [[0, 1], [1, 2], [2, 3], [2, 4]], "n3": [[0, 1, 2], [1, 2, 3], [1, 2, 4], [3, 2, 4]],
            "n4": [[0, 1, 2, 3], [0, 1, 2, 4]], "n4_improper": [[1, 3, 2, 4]]}
    g1 = single_graph(5, bonds, idxs, {"xyz": torch.from_numpy(xyz.astype(np.float32))})
    g2 = single_graph(5, bonds, idxs, {"xyz": torch.from_numpy((xyz[:, ::-1] * 1.01 + 0.3).astype(np.float32))})
    return batch([g1, g2])


@pytest.mark.parametrize("offset", [False, True], ids=["mm-edges-branchcut-linear", "mm-edges-branchcut-linear-offset"])
def test_mm_regime_edges(hip, ref, offset):
    from oracle.cpu_ref import bond_angle, dihedral
    g = edge_molecules()
    xyz = g.nodes["n1"].data["xyz"].contiguous()
    x64 = xyz.double()
    phi = dihedral(x64[0], x64[1], x64[2], x64[3])
    th = bond_angle(x64[0], x64[1], x64[2])
    # the fp32 positions really are at the edges the case list names
    assert bool((((math.pi - phi) < 2e-4) & (phi < math.pi)).any()) and bool((((phi + math.pi) < 2e-4) & (phi > -math.pi)).any())
    assert bool(((math.pi - th) < 2e-3).any()) and bool((phi.abs() < 2e-4).any())
    n_per = [0, 0, 6, 3]
    ks, eqs = _params(g.plan(), n_per, 7)
    eqs[1] = torch.full_like(eqs[1], 3.0)          # near-linear equilibrium angles: the angle terms stay moderate
    _check(hip, ref, g, xyz, ks, eqs, n_per, offset, f"edge geometries offset={offset}")


def test_mm_refuses_n_per_9(hip):
    """n_per = 9 is the first periodicity outside the kernels' domain: an error before anything is launched"""
    from grappa_amd.backend import GrappaHipError
    from grappa_amd.datasets import build_batch_from_pool
    g = build_batch_from_pool([300], n_confs=2, seed=0)
    n_per = [0, 0, 9, 3]
    ks, eqs = _params(g.plan(), n_per, 0)
    with pytest.raises(GrappaHipError):
        _run(hip, g.to("cuda").plan(), g.nodes["n1"].data["xyz"].contiguous(), ks, eqs, n_per, False, torch.zeros(1, 2),
             torch.zeros(g.num_nodes("n1"), 2, 3), "cuda")
