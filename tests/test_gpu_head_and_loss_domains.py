"""GPU (-m gpu): the kernels that turn network outputs into force-field parameters and score them, against float64 at the edges of
their domains -- the bond and angle output maps and every kind's statistics gradients (csrc/tuples.hip), the parameter loss and the
off branches of the energy / force loss (csrc/loss.hip), the column sums and the charge encoding (csrc/rowwise.hip).  The cases, the
checks and the gates live in tests/head_loss_cases.py and tests/kernel_refs.py; tests/test_kernel_domain_refs.py runs the same checks
on the fp32 RefBackend on the CPU (every gate is reachable by a correct fp32 implementation).  Parameter ids name the branch a case is for.

Gates.
  A  maps: elementwise |gpu - f64| <= 32 u32 (|f64| + scale), scale = std (|mos| + sum_p |o_p| + 1) + |min| (ToPositive),
     max (1 + |s| sum_p |o_p|) (angle eq), the same times |upstream| for d_o: at most P + 8 roundings (P <= 6) and a <= 2 ulp
     transcendental.
  C  statistics gradients: per constant |gpu - f64| <= c u32 sum_t |term_t|, c = ceil(T / 65536) + min(256, ceil(T / 256)) + 8 + 16:
     the longest chain of additions (a thread's serial sum over its tuples, the final serial sum over the blocks, the wave's six
     butterfly steps plus two additions for the four waves) and 16 for a term's own arithmetic.  Two runs are bit-equal.
  D  parameter loss: loss_mol by the self-calibrating gate (2 x the fp32 RefBackend's distance + 256 u32 |f64|) on the increment;
     loss_mol += is one fp32 addition, so the run on loss_mol = 3 must equal 3 + the increment of the run on 0 BIT FOR BIT (a gate of
     256 u32 |increment| on loss_mol - 3 itself is out of any fp32 implementation's reach: the addition onto 3 alone rounds by up to
     u32 (3 + |increment|) = 1.8e-7, the working regime's increments are 4e-8 .. 1.3e-7: the fp32 RefBackend's own (3 + inc) - 3 is
     off by up to 1.1e-7 there, against a bound of 2e-12; that one rounding is added to the floor of the gate on loss_mol - 3).  gps elementwise, 16 u32 (|f64| + inv_B (pw fac^2 2 (|p| + |ref|) / den + reg / n 2 |p|)): <= 10 roundings.
  F  column sums: per column |gpu - f64| <= c u32 (sum_r |x| [+ |out| when accumulating]), c = rows per block + the additions of
     reduce_rows' longest path + 8 (kernel_refs.colsum_chain states the chain).
  G  charge encoding: 16 u32 (|f64| + 1).

Largest observed error / bound on an MI355X (gfx950), over all cases of a section: A 0.029 (bond), 0.028 (angle); C 0.040; D 0.15 (gps);
F 0.044.  (The module prints them at its end: run with -s.)"""
import pytest
import torch

import head_loss_cases as hc
import kernel_refs as kr

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    from grappa_amd.backend import HipBackend
    return HipBackend()


@pytest.fixture(scope="module")
def ref():
    from oracle.ops_ref import RefBackend
    return RefBackend()


@pytest.fixture(scope="module")
def ratios():
    """the largest error / bound per section, printed at the end of the module (-s shows it)"""
    r = {}
    yield r
    print("\nlargest error / bound:", {k: round(v, 4) for k, v in sorted(r.items())})


def _note(ratios, key, value):
    ratios[key] = max(ratios.get(key, 0.0), value)


# =============================================================================================================== A. bond and angle maps
MAP_CASES = [pytest.param(name, T, P, 2, "", id=f"{name}-T{T}-P{P}-blocks{-(-T // 256)}")
             for name in ("bond", "angle") for T in (1, 255, 256, 257) for P in (1, 2, 3, 6)] + \
            [pytest.param(name, 257, P, 3, "", id=f"{name}-nout3-zero-column-P{P}") for name in ("bond", "angle") for P in (1, 2, 3, 6)] + \
            [pytest.param(name, 257, 2, 2, drop, id=f"{name}-no-upstream-{drop}") for name in ("bond", "angle") for drop in ("dk", "deq", "both")] + \
            [pytest.param("bond-min", 257, 3, 2, "", id="bond-nonzero-min"), pytest.param("angle-min-negs", 257, 3, 3, "", id="angle-nonzero-min-negative-std-over-max")]


@pytest.mark.parametrize("name,T,P,nout,drop", MAP_CASES)
def test_bond_and_angle_maps_against_float64(hip, ratios, name, T, P, nout, drop):
    _note(ratios, "A " + name.split("-")[0], hc.check_param_out_map(hip, DEV, name, T, P, nout, drop))


@pytest.mark.parametrize("name", ["bond", "angle"], ids=["bond-T0-no-launch", "angle-T0-no-launch"])
def test_maps_without_tuples_write_nothing(hip, name):
    hc.check_param_out_map(hip, DEV, name, 0, 2, 2)


# =============================================================================================================== B. torsion cutoff at equality
@pytest.mark.parametrize("gated", [False, True], ids=["torsion-cutoff-at-equality-ungated", "torsion-cutoff-at-equality-gated"])
def test_torsion_cutoff_at_equality(hip, gated):
    hc.check_torsion_cutoff(hip, DEV, gated)


# =============================================================================================================== C. statistics gradients
def _stats_id(name, T, P):
    blocks = min(256, -(-T // 256))
    return f"stats-{name}-T{T}-P{P}-blocks{blocks}" + ("-gridstride" if T > 65536 else "")


STATS_CASES = [pytest.param(name, T, 2, id=_stats_id(name, T, 2)) for name in hc.STATS_KINDS for T in (1, 255, 257, 1003, 65536, 65537, 2 * 65536 + 77)] + \
              [pytest.param(name, 257, 6, id=_stats_id(name, 257, 6)) for name in hc.STATS_KINDS]


@pytest.mark.parametrize("name,T,P", STATS_CASES)
def test_statistics_gradients_against_float64(hip, ratios, name, T, P):
    _note(ratios, "C", hc.check_param_out_stats(hip, DEV, name, T, P))


@pytest.mark.parametrize("name", list(hc.STATS_KINDS), ids=lambda n: f"stats-{n}-T0-memset")
def test_statistics_gradients_without_tuples_are_zero(hip, name):
    hc.check_param_out_stats(hip, DEV, name, 0, 2)


# =============================================================================================================== D. parameter loss
@pytest.mark.parametrize("name", hc.LOSS_PARAM_CASES, ids=lambda n: f"loss-param-{n}")
def test_loss_param_against_float64(hip, ref, ratios, name):
    _note(ratios, "D gps", hc.check_loss_param(hip, ref, DEV, name))


# =============================================================================================================== E. loss_ef off branches
@pytest.mark.parametrize("wE,wG", [(1.0, 0.0), (0.0, 0.8), (1.0, 0.8)], ids=["force-term-off-zero-fills-gG", "energy-term-off-zero-fills-gE", "both-on-no-dummies"])
@pytest.mark.parametrize("C", [1, 6], ids=["loss-ef-C1", "loss-ef-C6"])
def test_loss_ef_off_branches(hip, ref, C, wE, wG):
    hc.check_loss_ef_off(hip, ref, DEV, C, wE, wG)


# =============================================================================================================== F. column sums
@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite-dirty-out", "accumulate"])
@pytest.mark.parametrize("M,N,ldx", [pytest.param(*s, id=hc.colsum_id(*s)) for s in hc.COLSUM_SHAPES])
def test_colsum_against_float64(hip, ratios, M, N, ldx, accumulate):
    _note(ratios, "F", hc.check_colsum(hip, DEV, M, N, ldx, accumulate))


@pytest.mark.parametrize("accumulate", [False, True], ids=["colsum-M0-zeroes-dirty-out", "colsum-M0-accumulate-untouched"])
def test_colsum_without_rows(hip, accumulate):
    hc.check_colsum(hip, DEV, 0, 12, 12, accumulate)


# =============================================================================================================== G. charge encoding
@pytest.mark.parametrize("N,col0", [(0, 0), (1, 0), (257, 0), (257, 5)], ids=["N0", "N1", "N257", "N257-col0-5"])
@pytest.mark.parametrize("dim", [2, 16], ids=["dim2", "dim16"])
@pytest.mark.parametrize("lo,hi", [(-2.0, 2.0), (-1.0, 3.0), (0.0, 1.0)], ids=["charge-symmetric", "charge-asymmetric-m1-3", "charge-0-1"])
def test_charge_encoding_against_float64(hip, lo, hi, dim, N, col0):
    hc.check_charge_encoding(hip, DEV, lo, hi, dim, N, col0)
