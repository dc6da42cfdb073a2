"""The bootstrapped `Evaluator` (grappa_amd/evaluation.py; the reference's training/evaluation.py:164-386) against what the reference's own
Evaluator produced on four batches (tests/golden/ref_evaluator.npz, written by tools/make_evaluator_golden.py) and against the same
quantities in float64.  CPU: the host logic through a test-only backend (tests/eval_refs.py); GPU (-m gpu): the kernels
grappa_eval_moments_f32 / grappa_eval_bootstrap_f64.

Tolerances.  Every sum of the feature is a double sum of fewer than 10^6 terms of one sign (or compared on the scale of the sum of
their magnitudes), whose relative error is bounded by n * 2^-53 < 1.2e-10: TOL = 1e-10 relative to the float64 value is that bound, not
a fit to what the code gives.  Against the reference (float32 tensors, float32 means) the bound is the reference's own recorded
distance to float64 plus TOL -- the triangle inequality."""
import types

import numpy as np
import pytest
import torch

import golden_utils as gu
from eval_refs import NMET, NMOM, EvalRefBackend
from test_host_train import TINY

TOL = 1e-10
SUFFIXES = dict(suffix="", suffix_ref="_ref", suffix_classical="_classical_ff", suffix_classical_ref="_qm")
METRICS = ("std_energies", "std_gradients", "rmse_energies", "mae_energies", "rmse_gradients", "crmse_gradients", "mae_gradients")
CLASSICAL = ("rmse_classical_energies_from_ref", "rmse_classical_gradients_from_ref", "crmse_classical_gradients_from_ref")


@pytest.fixture
def eval_backend():
    from grappa_amd import backend
    old = backend._BACKEND
    backend.set_backend(EvalRefBackend())
    yield backend.get_backend()
    backend.set_backend(old)


class _Graph:
    """the slice of MolBatch the evaluator touches: plan() (B, N, atom_molptr) and the 'g' / 'n1' data dicts"""

    def __init__(self, fx, bi, device):
        t = lambda k: torch.from_numpy(fx[f"b{bi}::{k}"].copy()).to(device)   # noqa: E731
        counts = fx[f"b{bi}::atoms_per_mol"]
        ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(device)
        self._plan = types.SimpleNamespace(B=len(counts), N=int(counts.sum()), atom_molptr=ptr, device=device)
        self.nodes = {"g": types.SimpleNamespace(data={k: t(k) for k in ("energy", "energy_ref", "energy_classical_ff", "energy_qm", "is_dummy")}),
                      "n1": types.SimpleNamespace(data={k: t(k) for k in ("gradient", "gradient_ref", "gradient_classical_ff", "gradient_qm")})}

    def plan(self):
        return self._plan


def _stepped(fx, device, batches=None, **kw):
    from grappa_amd.evaluation import Evaluator
    ev = Evaluator(calculate_classical=True, **SUFFIXES, **kw)
    first = 0
    for bi in range(int(fx["n_batches"][0])):
        names = [str(x) for x in fx[f"b{bi}::dsnames"]]
        if batches is None or bi in batches:
            ev.step(_Graph(fx, bi, device), names, order=list(range(first, first + len(names))))
        first += len(names)
    return ev


def _close(got, fx, key, what):
    """within TOL of the float64 value, and within (the reference's distance to float64 + TOL) of the reference's value"""
    f64, ref = float(fx[f"f64::{key}"][0]), float(fx[f"ref::{key}"][0])
    print(f"{what:70s} got {got:.17g}  f64 {f64:.17g}  ref {ref:.9g}  |got-f64|/|f64| {abs(got - f64) / max(abs(f64), 1e-300):.2e}")
    assert abs(got - f64) <= TOL * abs(f64), (what, got, f64)
    assert abs(got - ref) <= abs(ref - f64) + TOL * abs(f64), (what, got, ref, f64)


def _check(fx, device):
    names = [str(x) for x in fx["ds_names"]]
    plain = _stepped(fx, device).pool(0)
    assert list(plain) == names                                           # datasets in the order of their first molecule
    for j, ds in enumerate(names):
        assert list(plain[ds]) == ["n_confs", "n_mols"] + list(METRICS + CLASSICAL)          # get_metrics' keys, in its order
        assert plain[ds]["n_mols"] == int(fx["ds_counts"][j]) == int(fx[f"ref::pool0::{ds}::n_mols"][0])
        assert plain[ds]["n_confs"] == int(fx[f"ref::pool0::{ds}::n_confs"][0]) and isinstance(plain[ds]["n_confs"], int)
        for m in METRICS + CLASSICAL:
            _close(plain[ds][m], fx, f"pool0::{ds}::{m}", f"pool(0) {ds} {m}")
    ev = _stepped(fx, device)
    boot = ev.pool(n_bootstrap=64, seed=3)
    assert list(boot) == names
    for ds in names:
        assert list(boot[ds]) == list(METRICS + CLASSICAL) + ["n_confs", "n_mols"]
        assert boot[ds]["n_confs"] == plain[ds]["n_confs"] and boot[ds]["n_mols"] == plain[ds]["n_mols"]
        for m in METRICS + CLASSICAL:
            assert set(boot[ds][m]) == {"mean", "std"}
            _close(boot[ds][m]["mean"], fx, f"boot::{ds}::{m}::mean", f"pool(64, 3) {ds} {m} mean")
            _close(boot[ds][m]["std"], fx, f"boot::{ds}::{m}::std", f"pool(64, 3) {ds} {m} std")
    single = names[int(np.argmin(fx["ds_counts"]))]
    assert int(fx["ds_counts"].min()) == 1
    for m in METRICS + CLASSICAL:                                         # one molecule: every resample is that molecule
        assert boot[single][m]["std"] == 0.0 and boot[single][m]["mean"] == plain[single][m], (m, boot[single][m], plain[single][m])
    again = ev.pool(n_bootstrap=64, seed=3)                               # pooling keeps the storage (as the reference): same bits again
    assert again == boot
    # without the classical pair, or without its reference suffix, the three classical metrics are not emitted (evaluation.py:379-384)
    from grappa_amd.evaluation import Evaluator
    for kw in (dict(), dict(calculate_classical=True), dict(suffix_classical_ref="_qm")):
        e2 = Evaluator(**kw)
        e2.step(_Graph(fx, 0, device), [str(x) for x in fx["b0::dsnames"]])
        assert all(list(v) == ["n_confs", "n_mols"] + list(METRICS) for v in e2.pool().values())


def test_bootstrap_indices_are_the_references_draws_and_leave_numpy_alone():
    from grappa_amd.evaluation import bootstrap_indices
    fx = gu.load("ref_evaluator.npz")
    np.random.seed(1234)
    np.random.rand(3)
    before = np.random.get_state()
    idx = bootstrap_indices([int(c) for c in fx["ds_counts"]], 64, seed=3)
    after = np.random.get_state()
    assert idx.dtype == np.int32 and idx.shape == fx["index_matrix"].shape == (64, 22)
    assert np.array_equal(idx, fx["index_matrix"])
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert bootstrap_indices([3, 1], 1).tolist() == [[0, 1, 2, 0]] and bootstrap_indices([3, 1], 0).tolist() == [[0, 1, 2, 0]]


def test_evaluator_matches_float64_and_the_reference_cpu(eval_backend):
    _check(gu.load("ref_evaluator.npz"), "cpu")


def test_index_chunks_and_step_order_do_not_change_the_result(eval_backend, monkeypatch):
    """the index table uploaded one replicate at a time, and the batches stepped in another order with their ordinals: the same dict"""
    from grappa_amd import evaluation
    fx = gu.load("ref_evaluator.npz")
    want = _stepped(fx, "cpu").pool(n_bootstrap=64, seed=3)
    monkeypatch.setattr(evaluation, "INDEX_CHUNK_BYTES", 4 * 22)
    calls = []
    orig = eval_backend.eval_bootstrap
    monkeypatch.setattr(eval_backend, "eval_bootstrap", lambda *a: calls.append(a[4:6]) or orig(*a))
    assert _stepped(fx, "cpu").pool(n_bootstrap=64, seed=3) == want
    assert calls[:4] == [(0, 1), (0, 1), (1, 2), (1, 2)] and len(calls) == 128          # two tables (classical) per chunk
    ev = evaluation.Evaluator(calculate_classical=True, **SUFFIXES)
    first = np.concatenate([[0], np.cumsum([len(fx[f"b{bi}::dsnames"]) for bi in range(4)])])
    for bi in (2, 0, 3, 1):
        ev.step(_Graph(fx, bi, "cpu"), [str(x) for x in fx[f"b{bi}::dsnames"]], order=list(range(first[bi], first[bi + 1])))
    assert ev.pool(n_bootstrap=64, seed=3) == want


def test_keep_data_and_constructor(eval_backend):
    from grappa_amd import Evaluator
    fx = gu.load("ref_evaluator.npz")
    with pytest.raises(NotImplementedError):
        Evaluator(plot_dir="plots")
    with pytest.raises(RuntimeError):
        _stepped(fx, "cpu").collect()
    with pytest.raises(ValueError):
        Evaluator().step(_Graph(fx, 0, "cpu"), ["dsA"])
    ev = _stepped(fx, "cpu", keep_data=True)
    plain = ev.pool(0)
    ev.collect()
    for ds, m in plain.items():
        e, er, g, gr = ev.all_energies[ds], ev.all_reference_energies[ds], ev.all_gradients[ds], ev.all_reference_gradients[ds]
        assert e.shape == er.shape == (m["n_confs"],) and g.shape == gr.shape and g.shape[1] == 3 and ev.n_mols[ds] == m["n_mols"]
        assert abs(float(er.double().std()) - m["std_energies"]) <= 1e-5 * m["std_energies"]
        assert abs(float((e - er).double().square().mean().sqrt()) - m["rmse_energies"]) <= 1e-5 * m["rmse_energies"]
        assert abs(float((g - gr).double().square().sum(-1).sqrt().mean()) - m["mae_gradients"]) <= 1e-5 * m["mae_gradients"]
    ev.collect(bootstrap_seed=5)
    assert all(ev.all_gradients[ds].shape[1] == 3 for ds in plain)


def _dp_worker(rank, world, port, out_q):
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    import torch.distributed as dist
    from grappa_amd import backend
    from grappa_amd.dist import init_process_group_from_env
    backend.set_backend(EvalRefBackend())
    init_process_group_from_env("gloo")
    fx = gu.load("ref_evaluator.npz")
    ev = _stepped(fx, "cpu", batches=[b for b in range(4) if b % world == rank])           # batches dealt round-robin, with their ordinals
    out_q.put((rank, ev.pool(n_bootstrap=64, seed=3)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_pool_the_bits_of_one_rank(eval_backend):
    import torch.multiprocessing as mp
    from test_host_train import _free_port
    want = _stepped(gu.load("ref_evaluator.npz"), "cpu").pool(n_bootstrap=64, seed=3)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in range(2)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    assert res[0][1] == want and res[1][1] == want and list(res[0][1]) == list(want)          # float for float, key for key


def _trainer_test(device):
    from grappa_amd import GrappaModel, eval_model, ops
    from grappa_amd.device_dataset import DeviceDataset
    from grappa_amd.trainer import Trainer
    from test_trainer import _items
    torch.manual_seed(0)
    ops.manual_seed(5)
    model = GrappaModel(**TINY).to(device)
    train = DeviceDataset(_items(list(range(300, 308))), device=device)
    items = _items(list(range(340, 349)))
    test = DeviceDataset(items, device=device)
    tr = Trainer(model, train, None, batch_size=4, conf_strategy=4, val_batch_size=4, lr=2e-3, start_qm_epochs=0, warmup_steps=2,
                 energy_weight=1.0, gradient_weight=0.8, param_weight=0.0)
    model.train()
    m = tr.test(test, n_bootstrap=16, seed=1)
    assert model.training                                                  # the mode the caller had is back
    assert list(m) == ["ds0", "ds1"] and m["ds0"]["n_mols"] == 5 and m["ds1"]["n_mols"] == 4
    assert m["ds0"]["n_confs"] == sum(4 + (j % 3) for j in range(0, 9, 2))                  # every conformation of every molecule
    for ds in m:
        assert list(m[ds]) == list(METRICS) + ["n_confs", "n_mols"]
        for k in METRICS:
            assert set(m[ds][k]) == {"mean", "std"} and np.isfinite(m[ds][k]["mean"]) and m[ds][k]["std"] > 0
    plain = tr.test(test, n_bootstrap=0, batch_size=2)
    assert list(plain["ds1"]) == ["n_confs", "n_mols"] + list(METRICS)
    # eval_model: the same model over the same molecules, batched by its own rule, one dataset object per name
    by_name = {"a": DeviceDataset(items[:5], device=device), "b": DeviceDataset(items[5:][::-1], device=device)}
    em = eval_model(model, by_name, n_bootstrap=0, forces_per_batch=400)
    assert list(em) == ["test"] and set(em["test"]) == {"ds0", "ds1"} and model.training
    for ds in plain:
        assert em["test"][ds]["n_confs"] == plain[ds]["n_confs"] and em["test"][ds]["n_mols"] == plain[ds]["n_mols"]
        for k in METRICS:
            assert abs(em["test"][ds][k] - plain[ds][k]) <= 1e-4 * abs(plain[ds][k]), (ds, k, em["test"][ds][k], plain[ds][k])
    return m


def test_trainer_test_and_eval_model_cpu(eval_backend):
    _trainer_test("cpu")


# ---------------------------------------------------------------------------------------------------------------------- GPU
def _random_batch(seed, B, Cc, lo, hi, big_atoms=None):
    g = torch.Generator().manual_seed(seed)
    counts = torch.randint(lo, hi, (B,), generator=g)
    if big_atoms:
        counts[B // 2] = big_atoms
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)]).int()
    N = int(counts.sum())
    e, er = torch.randn(B, Cc, generator=g) * 30 + 100, torch.randn(B, Cc, generator=g) * 30 - 50
    gr, grr = torch.randn(N, Cc, 3, generator=g) * 10, torch.randn(N, Cc, 3, generator=g) * 10
    nreal = torch.randint(1, Cc + 1, (B,), generator=g)
    dummy = (torch.arange(Cc)[None, :] >= nreal[:, None]).float()
    e[dummy != 0] = float("nan")                                           # a dummy slot may hold anything
    gr[torch.repeat_interleave(dummy != 0, counts, dim=0)] = 1e30
    return types.SimpleNamespace(B=B, N=N, atom_molptr=ptr), (e, er, dummy, gr, grr)


def _moments_close(got, want):
    """columns of one sign: TOL relative; the two plain sums (3: sum r, 8: sum g) on the scale of sqrt(n * sum of squares) >= sum |term|"""
    got, want = got.cpu(), want.cpu()
    assert torch.equal(got[:, 0], want[:, 0]) and torch.equal(got[:, 5], want[:, 5])          # counts: exact
    for c in (1, 2, 4, 6, 7, 9):
        err = ((got[:, c] - want[:, c]).abs() / want[:, c].abs().clamp_min(1e-300)).max()
        print(f"moment column {c}: max relative error {float(err):.2e}")
        assert (got[:, c] - want[:, c]).abs().le(TOL * want[:, c].abs()).all(), c
    for c, n, sq in ((3, 0, 4), (8, 5, 9)):
        scale = (want[:, n] * (3.0 if c == 8 else 1.0) * want[:, sq]).sqrt()
        assert (got[:, c] - want[:, c]).abs().le(TOL * scale).all(), c


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["256x32", "C300_and_300_atoms", "no_gradients_no_mask"])
def test_moments_kernel_matches_the_float64_restatement(case):
    from grappa_amd.backend import HipBackend
    if case == "256x32":
        plan, (e, er, dummy, gr, grr) = _random_batch(5, 256, 32, 3, 90)
    elif case == "C300_and_300_atoms":                                     # the strided loops: more conformations / 3-vectors than threads
        plan, (e, er, dummy, gr, grr) = _random_batch(6, 6, 300, 3, 40, big_atoms=300)
    else:
        plan, (e, er, dummy, gr, grr) = _random_batch(7, 9, 5, 3, 20)
        dummy, gr, grr, e = None, None, None, torch.nan_to_num(e, nan=3.0)
    want = torch.zeros(plan.B, NMOM, dtype=torch.float64)
    EvalRefBackend().eval_moments(plan, e, er, dummy, gr, grr, want)
    cu = lambda t: None if t is None else t.cuda()                         # noqa: E731
    plan_d = types.SimpleNamespace(B=plan.B, N=plan.N, atom_molptr=plan.atom_molptr.cuda())
    hip = HipBackend()
    got, again = (torch.zeros(plan.B, NMOM, dtype=torch.float64, device="cuda") for _ in range(2))
    hip.eval_moments(plan_d, cu(e), cu(er), cu(dummy), cu(gr), cu(grr), got)
    hip.eval_moments(plan_d, cu(e), cu(er), cu(dummy), cu(gr), cu(grr), again)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))     # the same input: the same bits
    assert torch.isfinite(got).all()
    _moments_close(got, want)
    if gr is None:
        assert (got[:, 5:] == 0).all()


@pytest.mark.gpu
def test_bootstrap_kernel_matches_the_float64_restatement():
    """moment rows of 256 molecules x 32 conformations in five datasets (one of a single molecule, one EMPTY: its metrics are NaN, as
    torch's statistics of nothing), 37 replicates sent in three ranges; twice: the same bits"""
    from grappa_amd.backend import HipBackend
    plan, (e, er, dummy, gr, grr) = _random_batch(5, 256, 32, 3, 90)
    mom = torch.zeros(plan.B, NMOM, dtype=torch.float64)
    ref = EvalRefBackend()
    ref.eval_moments(plan, e, er, dummy, gr, grr, mom)
    ds_ptr = torch.tensor([0, 100, 101, 101, 180, 256], dtype=torch.int32)
    n_rep, n_ds, M = 37, 5, 256
    g = torch.Generator().manual_seed(11)
    idx = torch.zeros(n_rep, M, dtype=torch.int32)
    for d in range(n_ds):
        n = int(ds_ptr[d + 1] - ds_ptr[d])
        if n:
            idx[:, ds_ptr[d]:ds_ptr[d + 1]] = torch.randint(0, n, (n_rep, n), generator=g).int()
            idx[0, ds_ptr[d]:ds_ptr[d + 1]] = torch.arange(n).int()
    want = [torch.zeros(n_rep, n_ds, NMET, dtype=torch.float64), torch.zeros(n_ds, NMET, dtype=torch.float64), torch.zeros(n_ds, NMET, dtype=torch.float64)]
    ref.eval_bootstrap(mom, ds_ptr, idx, n_rep, 0, n_rep, *want)
    hip = HipBackend()
    runs = []
    for _ in range(2):
        out = [torch.full_like(w, -7.0).cuda() for w in want]
        for r0, r1 in ((0, 1), (1, 20), (20, 37)):
            hip.eval_bootstrap(mom.cuda(), ds_ptr, idx[r0:r1].contiguous(), n_rep, r0, r1, *out)          # host tables: checked, then uploaded
        torch.cuda.synchronize()
        runs.append([o.cpu() for o in out])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    for name, got, w in zip(("replicates", "mean", "std"), runs[0], want):
        assert torch.equal(torch.isnan(got), torch.isnan(w)) and torch.isnan(w[..., 2, :]).all() and not torch.isnan(w[..., [0, 1, 3, 4], :]).any()
        ok = ~torch.isnan(w)
        print(f"bootstrap {name}: max relative error {float(((got[ok] - w[ok]).abs() / w[ok].abs().clamp_min(1e-300)).max()):.2e}")
        assert (got[ok] - w[ok]).abs().le(TOL * w[ok].abs()).all(), name
    assert (runs[0][2][1] == 0).all() and torch.equal(runs[0][1][1], runs[0][0][0, 1])          # the single molecule: std exactly 0, mean = its value
    # device-resident tables are not read back: an index out of range is clamped into its dataset, as documented
    bad = idx[:1].clone()
    bad[0, 5], bad[0, 150] = 100000, -3
    clamped = idx[:1].clone()
    clamped[0, 5], clamped[0, 150] = 99, 0
    outs = []
    for t in (bad, clamped):
        out = [torch.zeros(1, n_ds, NMET, dtype=torch.float64, device="cuda"), torch.zeros(n_ds, NMET, dtype=torch.float64, device="cuda"),
               torch.zeros(n_ds, NMET, dtype=torch.float64, device="cuda")]
        hip.eval_bootstrap(mom.cuda(), ds_ptr.cuda(), t.cuda(), 1, 0, 1, *out)
        torch.cuda.synchronize()
        outs.append(out[0].cpu())
    assert torch.equal(outs[0].view(torch.int64), outs[1].view(torch.int64))


@pytest.mark.gpu
def test_entry_points_refuse_bad_arguments():
    from grappa_amd import _lib
    from grappa_amd.backend import GrappaHipError, HipBackend
    hip = HipBackend()
    lib = _lib.load()
    mom = torch.ones(8, NMOM, dtype=torch.float64, device="cuda")
    ds_ptr = torch.tensor([0, 5, 8], dtype=torch.int32, device="cuda")
    idx = torch.zeros(2, 8, dtype=torch.int32, device="cuda")
    rep, mean, std = (torch.zeros(s, dtype=torch.float64, device="cuda") for s in ((2, 2, NMET), (2, NMET), (2, NMET)))
    p = lambda t: t.data_ptr()                                             # noqa: E731
    good = [None, p(mom), 8, 2, p(ds_ptr), p(idx), 2, 0, 2, p(rep), p(mean), p(std)]
    assert lib.grappa_eval_bootstrap_f64(*good) == 0
    for pos in (1, 4, 5, 9, 10, 11):                                       # a NULL pointer
        a = list(good)
        a[pos] = None
        assert lib.grappa_eval_bootstrap_f64(*a) == -1, pos
    for pos, v in ((6, 0), (6, -1), (2, 0), (3, 0), (7, -1), (7, 2), (8, 3), (8, 0)):          # n_rep < 1, no rows, no datasets, ranges outside [0, n_rep]
        a = list(good)
        a[pos] = v
        assert lib.grappa_eval_bootstrap_f64(*a) == -1, (pos, v)
    torch.cuda.synchronize()
    host_idx = torch.zeros(2, 8, dtype=torch.int32)
    hip.eval_bootstrap(mom, ds_ptr.cpu(), host_idx, 2, 0, 2, rep, mean, std)
    for r, c, v in ((1, 6, 3), (0, 0, -1), (1, 4, 5)):                     # an index outside its dataset's range (datasets of 5 and 3 rows)
        t = host_idx.clone()
        t[r, c] = v
        with pytest.raises(GrappaHipError, match="GRAPPA_ERR_ARG"):
            hip.eval_bootstrap(mom, ds_ptr.cpu(), t, 2, 0, 2, rep, mean, std)
    with pytest.raises(GrappaHipError, match="GRAPPA_ERR_ARG"):
        hip.eval_bootstrap(mom, torch.tensor([0, 5, 7], dtype=torch.int32), host_idx, 2, 0, 2, rep, mean, std)
    e = torch.zeros(2, 4, device="cuda")
    gr = torch.zeros(6, 4, 3, device="cuda")
    ptr = torch.tensor([0, 3, 6], dtype=torch.int32, device="cuda")
    out = torch.zeros(2, NMOM, dtype=torch.float64, device="cuda")
    assert lib.grappa_eval_moments_f32(None, 2, 4, 6, p(ptr), p(e), p(e), None, p(gr), p(gr), p(out)) == 0
    assert lib.grappa_eval_moments_f32(None, 2, 4, 6, p(ptr), p(e), p(e), None, p(gr), None, p(out)) == -1
    assert lib.grappa_eval_moments_f32(None, 0, 4, 6, p(ptr), p(e), p(e), None, None, None, p(out)) == -1
    assert lib.grappa_eval_moments_f32(None, 2, 4, 6, p(ptr), None, p(e), None, None, None, p(out)) == -1
    assert lib.grappa_eval_moments_f32(None, 2, 4, 6, p(ptr), p(e), p(e), None, None, None, None) == -1
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_evaluator_matches_float64_and_the_reference_gpu():
    _check(gu.load("ref_evaluator.npz"), "cuda")


@pytest.mark.gpu
def test_trainer_test_and_eval_model_gpu():
    gpu = _trainer_test("cuda")
    # ... and the recorded eval step where validate() would use it: the same metrics from replayed graphs
    from grappa_amd import GrappaModel, ops
    from grappa_amd.device_dataset import DeviceDataset
    from grappa_amd.trainer import Trainer
    from test_trainer import _items
    torch.manual_seed(0)
    ops.manual_seed(5)
    model = GrappaModel(**TINY).to("cuda")
    train = DeviceDataset(_items(list(range(300, 308))), device="cuda")
    test = DeviceDataset(_items(list(range(340, 349))), device="cuda")
    tr = Trainer(model, train, None, batch_size=4, conf_strategy=4, val_batch_size=4, lr=2e-3, start_qm_epochs=0, warmup_steps=2,
                 energy_weight=1.0, gradient_weight=0.8, param_weight=0.0, recorded=True)
    rec = tr.test(test, n_bootstrap=16, seed=1)
    assert tr.recorded_stats.get("eval_replayed", 0) >= 1
    for ds in gpu:
        assert rec[ds]["n_confs"] == gpu[ds]["n_confs"]
        for k in METRICS:
            assert abs(rec[ds][k]["mean"] - gpu[ds][k]["mean"]) <= 1e-4 * abs(gpu[ds][k]["mean"]), (ds, k, rec[ds][k], gpu[ds][k])
