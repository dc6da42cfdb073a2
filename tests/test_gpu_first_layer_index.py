"""GPU (-m gpu): the unfused fp32 first layer of a writer head with q | k | v kept on the (atom, position) table (HipBackend.first_layer_indexed).
Nothing here may move a bit, so every comparison is torch.equal:
  1. the attention kernels reading q | k | v rows through an index == the same kernels on the gathered copy;
  2. the token sums with several rows in flight (grappa_tuple_gather_bwd2_f32) == the one-row-at-a-time kernel == a sequential fp32 sum,
     with the row maxima they write == grappa_amax_f32 on the result;
  3. ops.ProjFirstLayerFn with the switch on == off, output and every gradient;
  4. one train step of the tiny model, switch on == off, eagerly on 1 and 4 head streams and recorded in a hipGraph."""
import types

import numpy as np
import pytest
import torch

import golden_utils as gu

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT_F, SENT_I = -7.0e4, 0x5A5A5A5A      # what the guard rows hold: nothing may be written in front of or behind an output


@pytest.fixture
def be():
    from grappa_amd.backend import get_backend
    b = get_backend()
    keep = (b.first_layer_indexed, b.training_pairs, b.pairs_min_rows)
    yield b
    b.first_layer_indexed, b.training_pairs, b.pairs_min_rows = keep


class _Guarded:
    """a (rows, cols) output between two guard blocks of 64 rows each"""

    def __init__(self, rows, cols, dtype=torch.float32, guard=64):
        fill = {torch.float32: SENT_F, torch.int32: SENT_I, torch.float16: -3.0e4}[dtype]
        self.fill, self.g, self.rows = fill, guard, rows
        self.buf = torch.full((rows + 2 * guard, cols), fill, dtype=dtype, device=DEV)
        self.t = self.buf[guard:guard + rows]

    def intact(self):
        return bool((self.buf[:self.g] == self.fill).all()) and bool((self.buf[self.g + self.rows:] == self.fill).all())


def _chk(rc):
    assert rc == 0, rc


def _st():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------- 1. indexed attention
@pytest.mark.parametrize("T", [1, 5, 67])                                  # a single wave, a ragged last block, several blocks
@pytest.mark.parametrize("F,heads", [(64, 2), (96, 3), (512, 8)])          # 96: idle lanes in a trip; 512: both trips of the pairs kernel
@pytest.mark.parametrize("s", [2, 3, 4])
def test_indexed_attention_equals_attention_on_the_gathered_copy(be, s, F, heads, T):
    lib, dh, R = be.lib, F // heads, 7
    gen = torch.Generator().manual_seed(1000 * s + 10 * F + T)
    qkv_tab = torch.randn(R, 3 * F, generator=gen).to(DEV)
    idx = torch.randint(0, R, (T, s), generator=gen, dtype=torch.int32)
    flat = idx.reshape(-1)
    flat[0], flat[-1] = R - 1, 0                                           # rows 0 and R-1 are used, and the order is not monotone
    if flat.numel() > 2:
        flat[1] = 0
    row_idx = idx.to(DEV).contiguous()
    qkv_tok = qkv_tab[row_idx.t().reshape(-1).long()].contiguous()         # token row pos*T + t
    dout = torch.randn(s * T, F, generator=gen).to(DEV)
    got, want = {}, {}
    for res, indexed in ((want, False), (got, True)):
        qkv = qkv_tab if indexed else qkv_tok
        out, am = _Guarded(s * T, F), _Guarded(s * T, 1, torch.int32)
        if indexed:
            _chk(lib.grappa_seqattn_fwd_idx_f32(_st(), s, T, heads, dh, qkv.data_ptr(), row_idx.data_ptr(), out.t.data_ptr(), am.t.data_ptr()))
        else:
            _chk(lib.grappa_seqattn_fwd_amax_f32(_st(), s, T, heads, dh, qkv.data_ptr(), out.t.data_ptr(), am.t.data_ptr()))
        pr, pam = _Guarded(s * T, 2 * F, torch.float16), _Guarded(s * T, 1, torch.int32)
        if indexed:
            _chk(lib.grappa_seqattn_fwd_pairs_idx_f32(_st(), s, T, heads, dh, qkv.data_ptr(), row_idx.data_ptr(), pr.t.data_ptr(), 2 * F, pam.t.data_ptr()))
        else:
            _chk(lib.grappa_seqattn_fwd_pairs_f32(_st(), s, T, heads, dh, qkv.data_ptr(), pr.t.data_ptr(), 2 * F, pam.t.data_ptr()))
        dq, dam = _Guarded(s * T, 3 * F), _Guarded(s * T, 1, torch.int32)
        if indexed:
            _chk(lib.grappa_seqattn_bwd_idx_f32(_st(), s, T, heads, dh, qkv.data_ptr(), row_idx.data_ptr(), dout.data_ptr(), dq.t.data_ptr(), dam.t.data_ptr()))
        else:
            _chk(lib.grappa_seqattn_bwd_amax_f32(_st(), s, T, heads, dh, qkv.data_ptr(), dout.data_ptr(), dq.t.data_ptr(), dam.t.data_ptr()))
        torch.cuda.synchronize()
        for name, gd in (("out", out), ("out_amax", am), ("pairs", pr), ("pairs_amax", pam), ("dqkv", dq), ("dqkv_amax", dam)):
            assert gd.intact(), (name, indexed)
            res[name] = gd.t.clone()
    for name in want:
        a, b = got[name], want[name]
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else a, b.view(torch.int16) if b.dtype == torch.float16 else b), name
    assert torch.isfinite(want["out"]).all() and float(want["dqkv"].abs().max()) > 0
    assert torch.equal(want["out_amax"], want["pairs_amax"])
    # without the maxima (NULL) the indexed kernels write the same rows
    out2, dq2 = _Guarded(s * T, F), _Guarded(s * T, 3 * F)
    _chk(lib.grappa_seqattn_fwd_idx_f32(_st(), s, T, heads, dh, qkv_tab.data_ptr(), row_idx.data_ptr(), out2.t.data_ptr(), None))
    _chk(lib.grappa_seqattn_bwd_idx_f32(_st(), s, T, heads, dh, qkv_tab.data_ptr(), row_idx.data_ptr(), dout.data_ptr(), dq2.t.data_ptr(), None))
    torch.cuda.synchronize()
    assert out2.intact() and dq2.intact() and torch.equal(out2.t, want["out"]) and torch.equal(dq2.t, want["dqkv"])


def test_indexed_attention_refuses_what_cannot_work(be):
    lib = be.lib
    q = torch.zeros(8, 3 * 64, device=DEV)
    o = torch.zeros(8, 64, device=DEV)
    am = torch.zeros(8, dtype=torch.int32, device=DEV)
    pr = torch.zeros(8, 128, dtype=torch.float16, device=DEV)
    idx = torch.zeros(4, 2, dtype=torch.int32, device=DEV)
    ERR_ARG = lib.grappa_seqattn_fwd_f32(_st(), 9, 4, 2, 32, q.data_ptr(), o.data_ptr())          # (s = 9: the library's argument error)
    assert ERR_ARG != 0
    a = (_st(), 2, 4, 2, 32, q.data_ptr())
    assert lib.grappa_seqattn_fwd_idx_f32(*a, None, o.data_ptr(), am.data_ptr()) == ERR_ARG                      # no index
    assert lib.grappa_seqattn_fwd_pairs_idx_f32(*a, None, pr.data_ptr(), 128, am.data_ptr()) == ERR_ARG
    assert lib.grappa_seqattn_bwd_idx_f32(*a, None, o.data_ptr(), q.data_ptr(), am.data_ptr()) == ERR_ARG
    i = idx.data_ptr()
    assert lib.grappa_seqattn_fwd_idx_f32(_st(), 2, 4, 2, 24, q.data_ptr(), i, o.data_ptr(), am.data_ptr()) == ERR_ARG       # dh / 4 not a power of two
    assert lib.grappa_seqattn_fwd_idx_f32(_st(), 2, 4, 32, 64, q.data_ptr(), i, o.data_ptr(), am.data_ptr()) == ERR_ARG      # F = 2048 > 1024
    assert lib.grappa_seqattn_bwd_idx_f32(_st(), 2, 4, 32, 64, q.data_ptr(), i, o.data_ptr(), q.data_ptr(), am.data_ptr()) == ERR_ARG
    assert lib.grappa_seqattn_fwd_pairs_idx_f32(_st(), 2, 4, 16, 64, q.data_ptr(), i, pr.data_ptr(), 2048, am.data_ptr()) == ERR_ARG     # F = 1024 > 512
    # and the Python front end checks the index as tuple_gather_fwd checks its own
    with pytest.raises(ValueError):
        be.seqattn_fwd(q, 2, 4, 2, o, row_idx=idx.long())
    with pytest.raises(ValueError):
        be.seqattn_fwd(q, 2, 4, 2, o, row_idx=idx.t())
    with pytest.raises(ValueError):
        be.seqattn_fwd(q, 2, 4, 2, o, row_idx=idx.cpu())
    with pytest.raises(ValueError):
        be.seqattn_bwd(q, o, 2, 4, 2, torch.zeros_like(q), row_idx=idx[:3])
    with pytest.raises(ValueError):
        be.seqattn_fwd(q, 2, 4, 2, o, row_idx=idx, table_rows=9)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 2. the token sums
COUNTS = [7, 0, 40, 1, 2, 0]              # incident rows per destination: skew and empty destinations, two workgroups of destinations


def _incidence(gen):
    nrows = sum(COUNTS)
    ptr = np.concatenate(([0], np.cumsum(COUNTS))).astype(np.int32)
    rows = torch.randperm(nrows, generator=gen).numpy().astype(np.int32)
    return ptr, rows


def _sequential_sum(dx, ptr, rows, start, has_pe):
    """fp32 adds in list order on the CPU (numpy float32 arithmetic, one add per row)"""
    out = start.copy()
    W = dx.shape[1]
    for n in range(len(COUNTS)):
        acc = out[n, :W].copy()
        for j in range(ptr[n], ptr[n + 1]):
            v = dx[rows[j]].copy()
            if has_pe:
                v[W - 1] = np.float32(0)
            acc = (acc + v).astype(np.float32)
        out[n, :W] = acc
    return out


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("has_pe", [False, True])
@pytest.mark.parametrize("W", [4, 516, 512, 1536])                          # 516: 129 chunks, not a multiple of 64
def test_token_sums_new_equal_old_equal_the_sequential_sum(be, W, has_pe, accumulate):
    lib, N = be.lib, len(COUNTS)
    W2 = {4: 516, 516: 4, 512: 1536, 1536: 512}[W]
    gen = torch.Generator().manual_seed(7 * W + 2 * has_pe + accumulate)
    ptr, rows = _incidence(gen)
    nrows = int(ptr[-1])
    dxs = [(torch.randn(nrows, w, generator=gen) * torch.logspace(-3, 3, nrows).view(-1, 1)).contiguous() for w in (W, W2)]
    dxs[0][torch.from_numpy(rows[ptr[2]:ptr[3]][::2].copy()).long()] *= -1.0       # (mixed signs inside the long list)
    starts = [torch.randn(N, w, generator=gen) if accumulate else torch.zeros(N, w) for w in (W, W2)]
    dptr, drows = torch.from_numpy(ptr).to(DEV), torch.from_numpy(rows).to(DEV)
    ddx = [d.to(DEV) for d in dxs]
    want = [_sequential_sum(d.numpy(), ptr, rows, st.numpy(), has_pe) for d, st in zip(dxs, starts)]

    def guarded(k):
        gd = _Guarded(N, (W, W2)[k], guard=8)
        gd.t.copy_(starts[k])
        return gd

    def single(k, new):
        w, da, am = (W, W2)[k], guarded(k), _Guarded(N, 1, torch.int32, guard=8)
        if new:
            _chk(lib.grappa_tuple_gather_bwd2_f32(_st(), N, dptr.data_ptr(), drows.data_ptr(), int(has_pe), int(accumulate), w, ddx[k].data_ptr(), w,
                                                  da.t.data_ptr(), w, am.t.data_ptr(), 0, None, 0, None, 0, None))
        else:
            _chk(lib.grappa_tuple_gather_bwd_f32(_st(), N, w, dptr.data_ptr(), drows.data_ptr(), ddx[k].data_ptr(), w, da.t.data_ptr(), w, int(has_pe),
                                                 int(accumulate)))
        torch.cuda.synchronize()
        assert da.intact() and am.intact()
        return da.t.clone(), am.t.clone().view(-1)

    old = [single(k, False)[0] for k in (0, 1)]
    new = [single(k, True) for k in (0, 1)]
    # the two tables in one launch
    da, da2 = guarded(0), guarded(1)
    am, am2 = _Guarded(N, 1, torch.int32, guard=8), _Guarded(N, 1, torch.int32, guard=8)
    _chk(lib.grappa_tuple_gather_bwd2_f32(_st(), N, dptr.data_ptr(), drows.data_ptr(), int(has_pe), int(accumulate), W, ddx[0].data_ptr(), W, da.t.data_ptr(), W,
                                          am.t.data_ptr(), W2, ddx[1].data_ptr(), W2, da2.t.data_ptr(), W2, am2.t.data_ptr()))
    torch.cuda.synchronize()
    assert da.intact() and da2.intact() and am.intact() and am2.intact()
    both = [(da.t.clone(), am.t.clone().view(-1)), (da2.t.clone(), am2.t.clone().view(-1))]
    for k in (0, 1):
        w = (W, W2)[k]
        ref = torch.from_numpy(want[k])
        assert torch.equal(old[k].cpu().view(torch.int32), ref.view(torch.int32)), ("old kernel vs the sequential sum", k)
        assert torch.equal(new[k][0].view(torch.int32), old[k].view(torch.int32)), ("new vs old", k)
        assert torch.equal(both[k][0].view(torch.int32), old[k].view(torch.int32)), ("two tables in one launch", k)
        # the maxima: grappa_amax_f32 on the result, the has_pe column left out
        res = old[k].clone()
        if has_pe:
            res[:, w - 1] = 0
        row, _ = be._amax_launch(res, True, False)
        torch.cuda.synchronize()
        assert torch.equal(new[k][1], row) and torch.equal(both[k][1], row), k
        if has_pe and accumulate and w > 4:
            assert float(old[k][:, w - 1].abs().max()) > 0                   # (the column the maximum leaves out is not empty here)
    if not accumulate:
        assert float(old[0][1].abs().max()) == 0 and int(new[0][1][1]) == 0 and int(new[0][1][5]) == 0      # an empty destination: zeros, maximum 0


def test_token_sums_front_end_returns_the_maxima_record(be):
    """HipBackend.tuple_gather_bwd: the record of the first table's row maxima when asked, both tables written; with the switch off the same rows
    through the old kernel and no record"""
    gen = torch.Generator().manual_seed(5)
    ptr, rows = _incidence(gen)
    N, nrows = len(COUNTS), int(ptr[-1])
    dptr, drows = torch.from_numpy(ptr).to(DEV), torch.from_numpy(rows).to(DEV)
    dx, dx2 = torch.randn(nrows, 192, generator=gen).to(DEV), torch.randn(nrows, 64, generator=gen).to(DEV)
    res = {}
    for on in (False, True):
        be.first_layer_indexed = on
        da, da2 = torch.empty(N, 192, device=DEV), torch.empty(N, 64, device=DEV)
        rec = be.tuple_gather_bwd(dptr, drows, dx, da, False, False, amax=True, second=(dx2, da2))
        torch.cuda.synchronize()
        res[on] = (da, da2, rec)
    assert res[False][2] is None and res[True][2] is not None
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    row, _ = be._amax_launch(res[False][0], True, False)
    assert torch.equal(res[True][2].row, row)


# ---------------------------------------------------------------------------------------------------------------- 3. ProjFirstLayerFn
def _first_layer_case(s, seed):
    import importlib
    batch = importlib.import_module("grappa_amd.batch")         # (grappa_amd.batch the attribute is the function of that name)
    N, T, R, Fd, H = 9, 11, 16, 64, 96
    gen = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, N, (T, s), generator=gen, dtype=torch.int32).to(DEV)
    lvl = {3: "n3", 4: "n4"}[s]
    plan = types.SimpleNamespace(N=N, T={lvl: T}, idx32={lvl: idx})
    tabs = batch._position_tables(plan, lvl)
    r = lambda *shape, scale=1.0: (torch.randn(*shape, generator=gen) * scale).to(DEV).requires_grad_(True)      # noqa: E731
    h = r(N, R)
    params = dict(w=r(Fd - 1, R, scale=0.3), b=r(Fd - 1, scale=0.1), n1_w=r(Fd), n1_b=r(Fd, scale=0.1), w_in=r(3 * Fd, Fd, scale=0.15), b_in=r(3 * Fd, scale=0.1),
                  w_o=r(Fd, Fd, scale=0.15), b_o=r(Fd, scale=0.1), nf_w=r(Fd), nf_b=r(Fd, scale=0.1), w1=r(H, Fd, scale=0.15), b1=r(H, scale=0.1),
                  w2=r(Fd, H, scale=0.15), b2=r(Fd, scale=0.1))
    pe = torch.linspace(-1.0, 1.0, s).to(DEV)
    dout = torch.randn(s * T, Fd, generator=gen).to(DEV)
    return h, params, tabs, pe, dout, (N, T, Fd)


@pytest.mark.parametrize("training_pairs", [True, False])
@pytest.mark.parametrize("s", [3, 4])
def test_first_layer_with_the_table_index_equals_the_token_copy(be, s, training_pairs):
    from grappa_amd import backend as B, ops
    h, P, tabs, pe, dout, (N, T, Fd) = _first_layer_case(s, 40 + s)
    be.training_pairs, be.pairs_min_rows = training_pairs, 0             # (the pair format as the operands' storage format at this size too)
    assert be.training_pairs_ok(s * T, Fd) == training_pairs
    order = ["w", "b", "n1_w", "n1_b", "w_in", "b_in", "w_o", "b_o", "nf_w", "nf_b", "w1", "b1", "w2", "b2"]
    res, logs, idx_calls = {}, {}, {}
    fwd = be.seqattn_fwd
    for on in (False, True):
        be.first_layer_indexed = on
        for t in [h] + list(P.values()):
            t.grad = None
        seen = []
        be.seqattn_fwd = lambda *a, **k: (seen.append(k.get("row_idx") is not None), fwd(*a, **k))[1]      # noqa: B023
        B._AMAX_LOG = []
        ops.mark_mode()
        try:
            out = ops.ProjFirstLayerFn.apply(h, P["w"], P["b"], tabs, s, T, pe, None, 2, 0.1, 1234567, 7654321, P["n1_w"], P["n1_b"], P["w_in"], P["b_in"],
                                             P["w_o"], P["b_o"], P["nf_w"], P["nf_b"], P["w1"], P["b1"], P["w2"], P["b2"])
            out.backward(dout)
            be.flush_wgrads()
            torch.cuda.synchronize()
        finally:
            logs[on], B._AMAX_LOG = B._AMAX_LOG, None
            del be.seqattn_fwd
        idx_calls[on] = seen
        res[on] = [out.detach().clone(), h.grad.clone()] + [P[k].grad.clone() for k in order]
    assert idx_calls[False] == [False] and idx_calls[True] == [True]
    for name, a, b in zip(["out", "h"] + order, res[True], res[False]):
        assert torch.isfinite(b).all() and float(b.abs().max()) > 0, name
        assert torch.equal(a, b), name
    # the table of q | k | v gradients no longer gets a maxima pass of its own: the token sum wrote its row maxima
    tab_shape = (s * N, 3 * Fd)
    assert any((R, Cc) == tab_shape for R, Cc, *_ in logs[False])
    assert not any((R, Cc) == tab_shape for R, Cc, *_ in logs[True])


# ---------------------------------------------------------------------------------------------------------------- 4. a train step
def _tiny_setup():
    from grappa_amd import Energy, MolwiseLoss, get_default_model_config, model_from_config
    from grappa_amd.datasets import build_batch_from_pool, pool_atom_counts
    from grappa_amd.optim import FlatParams, FusedAdam
    cfg = get_default_model_config()
    cfg.update(graph_node_features=16, gnn_width=32, gnn_attentional_layers=1, gnn_attention_heads=2,
               **{f"{hd}_{k}": v for hd in ("bond", "angle", "proper", "improper")
                  for k, v in (("transformer_depth", 1), ("n_heads", 2), ("transformer_width", 32), ("symmetriser_depth", 2), ("symmetriser_width", 16))})
    model = model_from_config(cfg)
    model.load_state_dict(gu.keyed_state_dict(model))
    model = model.to(DEV)
    flat = FlatParams(model)
    opt = FusedAdam(flat, lr=1e-3, max_grad_norm=10.0)
    ids = [int(i) for i in np.argsort(pool_atom_counts()[:300], kind="stable")[-4:]]      # four large molecules: angles and propers outnumber 4/3 N
    g = build_batch_from_pool(ids, n_confs=2, seed=3).to(DEV)
    loss_fn = MolwiseLoss(gradient_weight=0.8, energy_weight=1.0, param_weight=0.0, proper_regularisation=1e-3)
    return model, flat, opt, g, Energy(), loss_fn


def _count_indexed(be, counter):
    fwd = be.seqattn_fwd

    def wrapped(*a, **k):
        counter.append(k.get("row_idx") is not None)
        return fwd(*a, **k)
    be.seqattn_fwd = wrapped


@pytest.mark.parametrize("streams", [1, 4])
def test_tiny_train_step_with_the_table_index_equals_the_token_copy(be, streams):
    from grappa_amd import ops
    res, used = {}, {}
    for on in (False, True):
        be.first_layer_indexed = on
        model, flat, opt, g, energy, loss_fn = _tiny_setup()
        model.train()
        model.parameter_writer.head_streams = streams
        ops.manual_seed(99)
        seen = []
        _count_indexed(be, seen)
        try:
            flat.zero_grad()
            g = energy(model(g))
            loss = loss_fn(g)
            loss.backward()
            torch.cuda.synchronize()
        finally:
            del be.seqattn_fwd
        used[on] = seen
        res[on] = (loss.detach().clone(), g.nodes["g"].data["energy"].detach().clone(), g.nodes["n1"].data["gradient"].detach().clone(), flat.grad.clone())
    plan = g.plan()
    on_rows = sum(4 * plan.N <= 3 * plan.T[lvl] for lvl in ("n2", "n3", "n4", "n4_improper"))
    assert on_rows >= 2 and sum(used[True]) == on_rows and sum(used[False]) == 0      # the angle and the proper head took the table route
    for name, a, b in zip(("loss", "energy", "forces", "flat gradient"), res[True], res[False]):
        assert torch.isfinite(b).all() and float(b.abs().max()) > 0, name
        assert torch.equal(a, b), name


def test_recorded_tiny_train_step_with_the_table_index_equals_the_eager_steps(be):
    """2 warm-up steps + 2 replays of the recorded step == 4 eager steps (no dropout: the same arithmetic), with the table index and -- the
    eager steps -- without it"""
    from grappa_amd.capture import CapturedTrainStep, _drop_outputs
    want = {}
    for on in (False, True):
        be.first_layer_indexed = on
        model, flat, opt, g, energy, loss_fn = _tiny_setup()
        model.eval()
        opt.enable_dynamic()
        for _ in range(4):
            opt.zero_grad()
            _drop_outputs(g)
            loss_fn(energy(model(g))).backward()
            opt.step()
        torch.cuda.synchronize()
        want[on] = flat.data.clone()
    assert torch.isfinite(want[False]).all() and torch.equal(want[True], want[False])
    be.first_layer_indexed = True
    model, flat, opt, g, energy, loss_fn = _tiny_setup()
    model.eval()
    step = CapturedTrainStep(model, energy, loss_fn, opt, g, warmup=2)
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    assert torch.equal(flat.data, want[True])
