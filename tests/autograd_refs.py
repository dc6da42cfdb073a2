"""Helpers of the autograd-contract tests (test_host_autograd_contract.py on the test-only backend, test_gpu_autograd_contract.py on
the HIP kernels): grappa_amd/ops.py keeps parameter gradients out of autograd's hands (every Function returns None for its weights
and the kernels accumulate into `p.grad`), so what autograd guarantees elsewhere -- frozen parameters, accumulation over passes,
non-contiguous incoming gradients, nested passes -- is hand-written there and is checked here against the float64 oracle
(oracle/cpu_ref.py) under the same `requires_grad` mask.

Measure: the project's own (tests/test_gpu_e2e.py): for every trainable tensor max|g - ref| / max(max|ref|, 1e-8) < 1e-4."""
import contextlib
import os

import numpy as np
import torch

import golden_utils as gu

TOL = 1e-4

# (fixture, conformations, parameter references): the shapes of tests/test_gpu_e2e.py
CASES = {"att": ("ref_small_att.npz", 4, False), "conv": ("ref_small_conv.npz", 5, False)}
LK = dict(gradient_weight=0.8, energy_weight=1.0, param_weight=0.0, proper_regularisation=1e-3, improper_regularisation=1e-3)

_HEAD_MATRICES = ("attn.out_proj.weight", "ff.linear2.weight")

# freeze sets: predicates on (state-dict key, parameter) -> frozen?
FREEZE_SETS = {
    "nothing": lambda k, p: False,
    "gnn": lambda k, p: k.startswith("gnn."),
    "writer": lambda k, p: k.startswith("parameter_writer."),
    "matrices": lambda k, p: p.dim() == 2 and "norm" not in k,                 # only biases and norms train
    "biases": lambda k, p: k.endswith("bias"),
    "norms": lambda k, p: "norm" in k,
    "interleaved": lambda k, p: sum(map(ord, k)) % 2 == 0,
    "all_but_angle": lambda k, p: not k.startswith("parameter_writer.angle_writer."),
    "proper_layer0": lambda k, p: k.startswith("parameter_writer.proper_writer.") and ".transformer.0." in k,      # a frozen layer between trainable ones
    "head_w_not_b": lambda k, p: k.startswith("parameter_writer.") and k.endswith(_HEAD_MATRICES),               # frozen weight, trainable bias
    "att_block0": lambda k, p: k.startswith("gnn.att_blocks.0."),                                              # a frozen block whose input still takes a gradient
}
ROUTE_FREEZE_SETS = ("nothing", "gnn", "interleaved", "head_w_not_b")


def apply_freeze(model, name):
    """requires_grad of every parameter by FREEZE_SETS[name] -> (keys of the trainable ones, keys of the frozen ones)"""
    pred = FREEZE_SETS[name]
    train, frozen = [], []
    for k, p in model.named_parameters():
        f = bool(pred(k, p))
        p.requires_grad_(not f)
        (frozen if f else train).append(k)
    assert train and (frozen or name == "nothing"), name
    return train, frozen


_CASE = {}


def case(name):
    """-> dict(cfg, sd, mols, n_confs, refs) of a small fixture (cached; the tensors are never written)"""
    if name not in _CASE:
        from grappa_amd import GrappaModel
        fixture, n_confs, refs = CASES[name]
        fx = gu.load(fixture)
        cfg = gu.config_of(fx)
        sd = gu.weights_for(fx, GrappaModel(**cfg))
        _CASE[name] = dict(cfg=cfg, sd=sd, mols=gu.molecules_of(fx), n_confs=n_confs, refs=refs)
    return _CASE[name]


def batch_of(c, sl=slice(None)):
    return gu.build_batch(c["mols"][sl], c["n_confs"], c["refs"], (c["cfg"]["n_periodicity_proper"], c["cfg"]["n_periodicity_improper"]))


def product_model(c, device="cpu", train=False):
    from grappa_amd import GrappaModel
    model = GrappaModel(**c["cfg"])
    model.load_state_dict(c["sd"])
    model = model.to(device)
    return model.train() if train else model.eval()


def oracle_step(cfg, sd, g_cpu, loss_kwargs, double=True, frozen=None):
    """tests/test_gpu_e2e.py's `_oracle_step` with a `frozen` predicate on (key, parameter): the oracle (float64: ground truth) under the
    same requires_grad mask as the product"""
    from oracle import cpu_ref
    model = cpu_ref.RefGrappaModel(**cfg)
    model.load_state_dict(sd)
    model.eval()
    if double:
        model = model.double()
        for nt in g_cpu.ntypes:
            for k, v in list(g_cpu.nodes[nt].data.items()):
                if torch.is_tensor(v) and v.dtype == torch.float32:
                    g_cpu.nodes[nt].data[k] = v.double()
    if frozen is not None:
        for k, p in model.named_parameters():
            p.requires_grad_(not frozen(k, p))
    g = cpu_ref.RefEnergy()(model(g_cpu))
    loss = cpu_ref.RefMolwiseLoss(**loss_kwargs)(g)
    loss.backward()
    return model, g, loss


_ORACLE = {}
SPLIT = (slice(0, 2), slice(2, None))          # the two micro-batches of the accumulation scenario


def oracle(case_name, freeze="nothing", scenario="full"):
    """-> (losses, {key: float64 gradient}) of the float64 oracle, cached per (config, freeze set, scenario).  scenario "full": one pass over
    the batch (losses: [loss]); "accum": the passes over mols[:2] and mols[2:] summed (losses: one per pass).  A frozen parameter has no
    entry."""
    key = (case_name, freeze, scenario)
    if key not in _ORACLE:
        c = case(case_name)
        losses, grads = [], {}
        for sl in ((slice(None),) if scenario == "full" else SPLIT):
            model, _, loss = oracle_step(c["cfg"], c["sd"], batch_of(c, sl), LK, True, FREEZE_SETS[freeze])
            losses.append(float(loss.detach()))
            for k, p in model.named_parameters():
                if p.grad is not None:
                    grads[k] = grads.get(k, 0) + p.grad.detach().numpy().astype(np.float64)
                else:
                    assert not p.requires_grad, k
        for v in grads.values():
            v.setflags(write=False)
        _ORACLE[key] = (losses, grads)
    return _ORACLE[key]


def grad_distance(got, ref):
    """max|g - ref| / max(max|ref|, 1e-8): the measure of test_small_configs_against_reference_goldens"""
    ref = np.asarray(ref, dtype=np.float64)
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape
    return float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-8)


def check_against_oracle(model, train, frozen, ref_grads, label, tol=TOL):
    """every trainable tensor against the oracle (none skipped: the count is asserted), no frozen one with a gradient -> worst distance"""
    named = dict(model.named_parameters())
    assert sorted(ref_grads) == sorted(train), label
    worst, n, where = 0.0, 0, None
    for k in train:
        p = named[k]
        assert p.requires_grad and p.grad is not None, (label, k)
        assert torch.isfinite(p.grad).all(), (label, k)
        d = grad_distance(p.grad, ref_grads[k])
        if d > worst:
            worst, where = d, k
        n += 1
    assert n == len(train) == sum(p.requires_grad for p in named.values()), label
    for k in frozen:
        assert named[k].grad is None, (label, k)
    assert worst < tol, (label, where, worst)
    return worst


def queues_empty(be) -> bool:
    """the HIP backend's deferred work after a backward pass: nothing queued, no end-of-pass callback pending"""
    if not hasattr(be, "_wq"):
        return True
    return not be._wq and not be._lnq and be._wq_task is None


def step(model, g, be, lk=LK, sync=True):
    """forward, loss, backward on the product -> loss; the backend's queues must be empty afterwards"""
    from grappa_amd import Energy, MolwiseLoss
    loss = MolwiseLoss(**lk)(Energy()(model(g)))
    loss.backward()
    if sync and loss.is_cuda:
        torch.cuda.synchronize()
    assert queues_empty(be)
    return loss.detach()


@contextlib.contextmanager
def settings(be=None, model=None, **kw):
    """set and restore: backend attributes by name; head_streams / merged_heads of model.parameter_writer; first_layer_rows =
    ops.FIRST_LAYER_ON_ATOM_ROWS"""
    from grappa_amd import ops
    old = []
    try:
        for k, v in kw.items():
            if k in ("head_streams", "merged_heads"):
                tgt, name = model.parameter_writer, k
            elif k == "first_layer_rows":
                tgt, name = ops, "FIRST_LAYER_ON_ATOM_ROWS"
            else:
                tgt, name = be, k
                assert hasattr(be, k), k
            old.append((tgt, name, getattr(tgt, name)))
            setattr(tgt, name, v)
        yield
    finally:
        for tgt, name, v in reversed(old):
            setattr(tgt, name, v)


@contextlib.contextmanager
def counting(obj, *names, **summaries):
    """thin wrappers on methods of `obj` (a backend, a module of functions) -> {name: [summary of each call]}; summaries: name -> f(args,
    kwargs, result), default 1.  Removed on exit."""
    log = {}
    own = []
    try:
        for n in list(names) + list(summaries):
            f = summaries.get(n) or (lambda a, k, r: 1)
            orig = getattr(obj, n)
            own.append((n, n in vars(obj), vars(obj).get(n)))
            log[n] = []

            def wrapped(*a, _orig=orig, _log=log[n], _f=f, **k):
                r = _orig(*a, **k)
                _log.append(_f(a, k, r))
                return r
            setattr(obj, n, wrapped)
        yield log
    finally:
        for n, had, val in own:
            if had:
                setattr(obj, n, val)
            else:
                delattr(obj, n)


_DIST = {}
DIST_NAME = "autograd_contract_distances.txt"


def record(scenario, route, worst, write=True):
    """worst distance per (scenario, route), printed and (GPU tests) kept as autograd_contract_distances.txt in the suite's report directory
    (where tests/test_gpu_ops.py keeps its per-op errors)"""
    key = (scenario, route)
    _DIST[key] = max(_DIST.get(key, 0.0), float(worst))
    print(f"autograd contract: {scenario} | {route}: worst distance {worst:.2e}")
    if write:
        import test_gpu_ops
        out_dir = os.path.dirname(test_gpu_ops.REPORT)
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, DIST_NAME), "w") as fh:
            fh.write("# worst max|g - ref| / max|ref| over the trainable tensors, per (scenario, route)\n")
            for (s, r), v in sorted(_DIST.items()):
                fh.write(f"{s} | {r}: {v:.2e}\n")


# ------------------------------------------------------------------------------------------------------------ function level
# Every block Function of grappa_amd/ops.py on its own, at the smallest shapes (37 atoms, 64 features, tuples of 2 and 4 tokens, 1 and 40
# tuples), against float64 autograd of the oracle's module for the same block (oracle/cpu_ref.py), for the incoming-gradient layouts.
N_ATOMS, FEATS, HEADS = 37, 64, 4
GRAPH_IDS = (301, 397)                          # two pool molecules of 18 + 19 atoms
PERMS = {2: [[0, 1], [1, 0]], 4: [[0, 1, 2, 3], [3, 2, 1, 0]]}
PE = {2: None, 4: [0.0, 1.0, 1.0, 0.0]}


def _seeded(module_or_tensors, gen):
    """move LayerNorm weights off 1 and biases off 0 (default initialisation would hide a swapped or missing affine term)"""
    with torch.no_grad():
        for k, p in module_or_tensors.named_parameters():
            if "norm" in k or k.endswith("bias"):
                p.add_(0.1 * torch.randn(p.shape, generator=gen))
    return module_or_tensors


def _tokens_ref(h, w, b, idx, s, pe):
    """ProjGatherFn in plain torch: a = ELU(h W^T + b); x[pos*T + t] = [a[idx[t, pos]], pe[pos]]"""
    a = torch.nn.functional.elu(h @ w.t() + b)
    x = a[idx.long().t().reshape(-1)]
    if pe is not None:
        x = torch.cat([x, pe.to(x.dtype).repeat_interleave(idx.shape[0]).unsqueeze(1)], dim=1)
    return x


def _incidence(idx, N):
    """inverse incidence atom -> token rows (pos*T + t), as grappa_amd/batch.py builds it"""
    atoms = idx.numpy().astype(np.int64).T.reshape(-1)
    rows = np.argsort(atoms, kind="stable")
    ptr = np.zeros(N + 1, dtype=np.int64)
    np.add.at(ptr, atoms + 1, 1)
    return torch.from_numpy(np.cumsum(ptr).astype(np.int32)), torch.from_numpy(rows.astype(np.int32))


def _param_out_ref(kind, o, T, P, n_per, gated, cutoff, consts):
    """oracle/cpu_ref.py's output maps (BondWriter / AngleWriter / TorsionWriter) on the sum over the permuted copies"""
    elu = torch.nn.functional.elu
    c = o.view(P, T, -1).sum(0)
    to_pos = lambda x, mos, std, mn: std * (elu(mos + x - 1) + 1) + mn      # noqa: E731
    if kind == 0:
        return to_pos(c[:, 1], consts[3], consts[4], consts[5]), to_pos(c[:, 0], consts[0], consts[1], consts[2])
    if kind == 1:
        return to_pos(c[:, 1], consts[3], consts[4], consts[5]), consts[1] * torch.sigmoid(consts[0] * c[:, 0])
    k_std, k_mean = consts[:n_per], consts[n_per:]
    c = c[:, :n_per] * torch.sigmoid(c[:, n_per:]) * k_std if gated else c * k_std + k_mean
    return (torch.where(c.abs() > cutoff, c, torch.zeros_like(c)) if cutoff > 0 else c),


def function_cases(dev):
    """-> [(name, build)]; build() -> dict(run: () -> outputs of the product Function(s), leaves: {name: leaf tensor}, ref: () -> (float64
    outputs, {name: float64 leaf}), T)"""
    from grappa_amd import model as M, ops
    from grappa_amd.datasets import build_batch_from_pool
    from oracle import cpu_ref
    import importlib
    import types
    batch = importlib.import_module("grappa_amd.batch")
    cases = []

    def leaf(t):
        return t.detach().to(dev).requires_grad_(True)

    def leaf64(t):
        return t.detach().cpu().double().requires_grad_(True)

    def named(mod, **extra):
        return {**extra, **dict(mod.named_parameters())}

    def add(name):
        def deco(f):
            def build():
                with torch.random.fork_rng():
                    torch.manual_seed(sum(map(ord, name)))
                    return f(torch.Generator().manual_seed(sum(map(ord, name)) + 1))
            cases.append((name, build))
            return f
        return deco

    @add("LinearFn")
    def _(gen):
        x, w, b = (leaf(torch.randn(N_ATOMS, FEATS, generator=gen)), leaf(torch.randn(FEATS, FEATS, generator=gen) / 8), leaf(0.1 * torch.randn(FEATS, generator=gen)))
        leaves = dict(x=x, w=w, b=b)

        def ref():
            l64 = {k: leaf64(v) for k, v in leaves.items()}
            return (torch.nn.functional.elu(l64["x"] @ l64["w"].t() + l64["b"]),), l64
        return dict(run=lambda: (ops.LinearFn.apply(x, w, b, ops.ELU, 0.0, 0),), leaves=leaves, ref=ref, T=N_ATOMS)

    def graph_block(name, make_prod, make_ref):
        @add(name)
        def _(gen):
            g_cpu = build_batch_from_pool(list(GRAPH_IDS), n_confs=2, seed=1)
            plan = g_cpu.to(dev).plan()
            assert plan.N == N_ATOMS
            prod = _seeded(make_prod(), gen).to(dev)
            x = leaf(torch.randn(N_ATOMS, FEATS, generator=gen))
            src, dst = cpu_ref.n1_edges(g_cpu)

            def ref():
                r = _twin64_from(prod, make_ref())
                x64 = leaf64(x)
                return (r(src.long(), dst.long(), x64),), named(r, x=x64)
            return dict(run=lambda: (prod(plan, x),), leaves=named(prod, x=x), ref=ref, T=N_ATOMS)

    def _twin64_from(prod, ref):
        ref.load_state_dict({k: v.detach().cpu() for k, v in prod.state_dict().items()})
        return ref.double()

    graph_block("AttBlockFn", lambda: M.ResidualAttentionBlock(FEATS, HEADS, 0.0), lambda: cpu_ref.AttBlock(FEATS, HEADS, 0.0))
    graph_block("ConvBlockFn", lambda: M.ResidualConvBlock(FEATS, 0.0), lambda: cpu_ref.ConvBlock(FEATS, 0.0))

    def layer_pair(gen):
        prod = _seeded(M.DottedAttWithMLP(FEATS, HEADS, FEATS, 0.0), gen).to(dev)
        return prod, lambda: _twin64_from(prod, cpu_ref.TransformerLayer(FEATS, HEADS, FEATS, 0.0))

    def sym_pair(gen, s, n_out=6):
        perms = torch.tensor(PERMS[s], dtype=torch.int32)
        prod = _seeded(M.SymmetrisedTransformer(FEATS, HEADS, FEATS, 0, n_out, perms, 0.0, 3, 32, None), gen).to(dev)

        def twin():
            r = cpu_ref._Symmetriser(FEATS, n_out, perms, 32, 3)
            r.load_state_dict({k[len("symmetriser."):]: v.detach().cpu() for k, v in prod.state_dict().items()})
            return r.double()
        return prod, twin

    def sym_ref(r, x64, s, T):
        """cpu_ref._Symmetriser.forward without the sum over the permuted copies (ParamOutFn takes it): rows p*T + t"""
        xs = x64.view(s, T, -1)
        xp = torch.stack([xs[p.long()] for p in r.permutations], dim=0).transpose(1, 2).contiguous().view(len(r.permutations) * T, -1)
        return r.mlp(xp)

    for s in (2, 4):
        for T in (1, 40, 0):
            tag = f"[s={s},T={T}]"
            idx = torch.randint(0, N_ATOMS, (T, s), generator=torch.Generator().manual_seed(10 * s + T), dtype=torch.int32)
            pe = None if PE[s] is None else torch.tensor(PE[s])
            Wp = FEATS - (pe is not None)

            @add("TransformerLayerFn" + tag)
            def _(gen, s=s, T=T):
                prod, twin = layer_pair(gen)
                x = leaf(torch.randn(s * T, FEATS, generator=gen))

                def ref():
                    r, x64 = twin(), leaf64(x)
                    return (r(x64.view(s, T, FEATS)).reshape(s * T, FEATS),), named(r, x=x64)
                return dict(run=lambda: (prod(x, s, T),), leaves=named(prod, x=x), ref=ref, T=T)

            @add("SymmetriserFn" + tag)
            def _(gen, s=s, T=T):
                prod, twin = sym_pair(gen, s)
                x = leaf(torch.randn(s * T, FEATS, generator=gen))

                def ref():
                    r, x64 = twin(), leaf64(x)
                    return (sym_ref(r, x64, s, T),), {"x": x64, **{"symmetriser." + k: p for k, p in r.named_parameters()}}
                return dict(run=lambda: (prod(x, s, T),), leaves=named(prod, x=x), ref=ref, T=T)

            @add("ProjGatherFn" + tag)
            def _(gen, s=s, T=T, idx=idx, pe=pe, Wp=Wp):
                h, w, b = leaf(torch.randn(N_ATOMS, 32, generator=gen)), leaf(torch.randn(Wp, 32, generator=gen) / 5), leaf(0.1 * torch.randn(Wp, generator=gen))
                ptr, rows = _incidence(idx, N_ATOMS)
                d = lambda t: None if t is None else t.to(dev)      # noqa: E731
                leaves = dict(h=h, w=w, b=b)

                def ref():
                    l64 = {k: leaf64(v) for k, v in leaves.items()}
                    return (_tokens_ref(l64["h"], l64["w"], l64["b"], idx, s, pe),), l64
                return dict(run=lambda: (ops.ProjGatherFn.apply(h, w, b, d(idx), d(ptr), d(rows), s, d(pe), None),), leaves=leaves, ref=ref, T=T)

            if T:
                @add("ProjFirstLayerFn" + tag)
                def _(gen, s=s, T=T, idx=idx, pe=pe, Wp=Wp):
                    h, w, b = leaf(torch.randn(N_ATOMS, 32, generator=gen)), leaf(torch.randn(Wp, 32, generator=gen) / 5), leaf(0.1 * torch.randn(Wp, generator=gen))
                    l0, twin = layer_pair(gen)
                    lvl = {2: "n2", 4: "n4"}[s]
                    tabs = batch._position_tables(types.SimpleNamespace(N=N_ATOMS, T={lvl: T}, idx32={lvl: idx.to(dev)}), lvl)
                    leaves = named(l0, h=h, w=w, b=b)

                    def run():
                        ops.mark_mode()
                        return (ops.ProjFirstLayerFn.apply(h, w, b, tabs, s, T, None if pe is None else pe.to(dev), None, HEADS, 0.0, 0, 0, l0.norm1.weight, l0.norm1.bias,
                                                           l0.attn.in_proj_weight, l0.attn.in_proj_bias, l0.attn.out_proj.weight, l0.attn.out_proj.bias, *l0.ff.params()),)

                    def ref():
                        r = twin()
                        l64 = {k: leaf64(leaves[k]) for k in ("h", "w", "b")}
                        x = _tokens_ref(l64["h"], l64["w"], l64["b"], idx, s, pe)
                        return (r(x.view(s, T, FEATS)).reshape(s * T, FEATS),), named(r, **l64)
                    return dict(run=run, leaves=leaves, ref=ref, T=T)

        for kind, T in ((0, 40), (1, 40), (2, 40), (2, 1), (0, 0), (2, 0)):
            if s == 4 and kind != 2 or s == 2 and kind == 2 and T != 40:
                continue
            @add(f"ParamOutFn[kind={kind},T={T},s={s}]")
            def _(gen, kind=kind, T=T):
                P, n_per, gated, cutoff = 2, (3 if kind == 2 else 0), kind == 2, (1e-4 if kind == 2 else 0.0)
                width = 2 if kind < 2 else 2 * n_per
                o = leaf(torch.randn(P * T, width, generator=gen))
                consts = leaf(torch.tensor([[1.1, 0.2, 0.0, 2.0, 150.0, 0.0], [0.05, 3.14159, 0.0, 2.5, 40.0, 0.0], [0.8, 0.5, 0.3, 0.1, -0.2, 0.05]][kind]))      # learnable statistics
                leaves = dict(o=o, consts=consts)

                def ref():
                    l64 = {k: leaf64(v) for k, v in leaves.items()}
                    return _param_out_ref(kind, l64["o"], T, P, n_per, gated, cutoff, l64["consts"]), l64

                def run():
                    out = ops.ParamOutFn.apply(o, kind, T, P, n_per, gated, cutoff, consts)
                    return out if isinstance(out, tuple) else (out,)
                return dict(run=run, leaves=leaves, ref=ref, T=T)

    @add("MultiTransformerLayerFn")
    def _(gen):
        heads = [(2, 40), (4, 17)]
        pairs = [layer_pair(gen) for _ in heads]
        xs = [leaf(torch.randn(s * T, FEATS, generator=gen)) for s, T in heads]
        leaves = {}
        for i, ((l, _tw), x) in enumerate(zip(pairs, xs)):
            leaves.update({f"{i}.{k}": v for k, v in named(l, x=x).items()})

        def run():
            flat = []
            for (l, _tw), x in zip(pairs, xs):
                flat += [x, l.norm1.weight, l.norm1.bias, l.attn.in_proj_weight, l.attn.in_proj_bias, l.attn.out_proj.weight, l.attn.out_proj.bias, *l.ff.params()]
            ops.mark_mode()
            return ops.MultiTransformerLayerFn.apply(tuple((s, T, HEADS, 0.0, 0, 0) for s, T in heads), *flat)

        def ref():
            outs, l64 = [], {}
            for i, ((_l, tw), x, (s, T)) in enumerate(zip(pairs, xs, heads)):
                r, x64 = tw(), leaf64(x)
                outs.append(r(x64.view(s, T, FEATS)).reshape(s * T, FEATS))
                l64.update({f"{i}.{k}": v for k, v in named(r, x=x64).items()})
            return tuple(outs), l64
        return dict(run=run, leaves=leaves, ref=ref, T=40)

    @add("MultiSymmetriserFn")
    def _(gen):
        heads = [(2, 40), (4, 17)]
        pairs = [sym_pair(gen, s) for s, _ in heads]
        xs = [leaf(torch.randn(s * T, FEATS, generator=gen)) for s, T in heads]
        leaves = {}
        for i, ((m, _tw), x) in enumerate(zip(pairs, xs)):
            leaves.update({f"{i}.{k}": v for k, v in named(m, x=x).items()})

        def run():
            cfgs, flat = [], []
            for (m, _tw), x, (s, T) in zip(pairs, xs, heads):
                sym = m.symmetriser
                cfgs.append((s, T, sym._perm_list, len(sym.mlp)))
                flat += [x] + [t for ff in sym.mlp for t in ff.params()]
            ops.mark_mode()
            return ops.MultiSymmetriserFn.apply(tuple(cfgs), *flat)

        def ref():
            outs, l64 = [], {}
            for i, ((_m, tw), x, (s, T)) in enumerate(zip(pairs, xs, heads)):
                r, x64 = tw(), leaf64(x)
                outs.append(sym_ref(r, x64, s, T))
                l64.update({f"{i}.x": x64, **{f"{i}.symmetriser." + k: p for k, p in r.named_parameters()}})
            return tuple(outs), l64
        return dict(run=run, leaves=leaves, ref=ref, T=40)

    return cases


def gradient_layouts(outs, gen):
    """-> {"random": {layout: [dout per output]}, "rows": {...}}: the same values as a contiguous tensor, as a strided slice of a wider
    buffer (NaN around it) and -- "rows": one random row for all rows, what a broadcast can carry -- as an expanded view with stride 0"""
    def strided(v):
        if v.dim() == 1:
            wide = torch.full((v.shape[0], 3), float("nan"), dtype=v.dtype, device=v.device)
            wide[:, 1] = v
            return wide[:, 1]
        wide = torch.full((v.shape[0], v.shape[1] + 7), float("nan"), dtype=v.dtype, device=v.device)
        wide[:, 3:3 + v.shape[1]] = v
        return wide[:, 3:3 + v.shape[1]]
    rnd = [torch.randn(o.shape, generator=gen).to(o.device) for o in outs]
    rows = [torch.randn(o.shape[1:] if o.dim() > 1 else (), generator=gen).to(o.device) for o in outs]
    sets = {"random": {"contiguous": rnd, "strided": [strided(v) for v in rnd]},
            "rows": {"contiguous": [r.expand(o.shape).contiguous() for r, o in zip(rows, outs)], "expanded": [r.expand(o.shape) for r, o in zip(rows, outs)],
                     "strided": [strided(r.expand(o.shape).contiguous()) for r, o in zip(rows, outs)]}}
    for o, e, st in zip(outs, sets["rows"]["expanded"], sets["rows"]["strided"]):
        assert o.numel() <= 1 or not e.is_contiguous() or o.shape[0] == 1
        assert o.numel() <= 1 or not st.is_contiguous() or o.shape[0] <= 1
    return sets


def function_grads(c, douts, be):
    """one forward and backward of a function case -> {leaf name: gradient (clone) or None}"""
    for t in c["leaves"].values():
        t.grad = None
    outs = c["run"]()
    torch.autograd.backward(outs, douts)
    if hasattr(be, "flush_wgrads"):
        be.flush_wgrads()
    if outs[0].is_cuda:
        torch.cuda.synchronize()
    assert queues_empty(be)
    return {k: (None if t.grad is None else t.grad.detach().clone()) for k, t in c["leaves"].items()}, outs


def check_function_layouts(c, be, name, tol=TOL):
    """contiguous / strided (and, for values a broadcast can carry, expanded) incoming gradients: bit-identical input and parameter
    gradients; the contiguous case within `tol` of float64 autograd of the oracle's module (1e-4 of each tensor's largest entry: the
    project's gate for gradients; float32 kernels on <= 256-term sums sit two orders below it) -> worst distance"""
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + 2)
    sets = gradient_layouts(c["run"](), gen)
    base = None
    for values, layouts in sets.items():
        got = {}
        for layout, douts in layouts.items():
            got[layout], _ = function_grads(c, douts, be)
        first = got["contiguous"]
        assert all(g is not None and torch.isfinite(g).all() for g in first.values()), (name, values)
        assert any(float(g.abs().max()) > 0 for g in first.values()), (name, values)
        for layout, grads in got.items():
            for k, g in grads.items():
                assert torch.equal(g, first[k]), (name, values, layout, k)
        if values == "random":
            base = (first, layouts["contiguous"])
    grads, douts = base
    outs64, leaves64 = c["ref"]()
    assert sorted(leaves64) == sorted(c["leaves"]), name
    outs = c["run"]()
    for o, o64 in zip(outs, outs64):
        assert grad_distance(o, o64.detach().numpy()) < tol, (name, "forward")
    keys = sorted(leaves64)
    ref = torch.autograd.grad(outs64, [leaves64[k] for k in keys], [d.detach().cpu().double() for d in douts], allow_unused=True)
    worst = 0.0
    for k, r in zip(keys, ref):
        assert r is not None, (name, k)
        d = grad_distance(grads[k], r.numpy())
        worst = max(worst, d)
        assert d < tol, (name, k, d)
    return worst


@contextlib.contextmanager
def kernel_calls(be):
    """-> [count] of the kernels the backend launched inside the block (the HIP library's own launch counter; the test-only backend:
    calls of its methods)"""
    n = [0]
    lib = getattr(be, "lib", None)
    if lib is not None:
        torch.cuda.synchronize()
        lib.grappa_launch_count(1)
        try:
            yield n
        finally:
            n[0] = int(lib.grappa_launch_count(1))
        return
    names = [k for k in dir(be) if not k.startswith("_") and callable(getattr(be, k))]
    with counting(be, *names) as log:
        try:
            yield n
        finally:
            n[0] = sum(len(v) for v in log.values())


def check_empty_function(c, be, name):
    """T = 0: outputs without rows, a backward pass that returns zeros of the input's shape and type and launches nothing"""
    outs = c["run"]()
    assert all(o.shape[0] == 0 for o in outs), name
    with kernel_calls(be) as n:
        torch.autograd.backward(outs, [torch.zeros_like(o) for o in outs])
    assert n[0] == 0, (name, n[0])
    assert queues_empty(be)
    inputs = [k for k in ("x", "h", "o") if k in c["leaves"]]
    assert inputs
    for k, t in c["leaves"].items():
        if k in inputs:
            assert t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == t.dtype and not bool(t.grad.any()), (name, k)
        else:
            assert t.grad is None or not bool(t.grad.any()), (name, k)


OUT_KEYS = (("n2", "k"), ("n2", "eq"), ("n3", "k"), ("n3", "eq"), ("n4", "k"), ("n4_improper", "k"))


@contextlib.contextmanager
def checkpointed(model, around):
    """torch.utils.checkpoint (use_reentrant=True) around the parameter writer or around the model's last GNN block: its forward pass runs
    again inside the backward pass and its backward pass is a pass of its own inside the outer one -> [re-computations seen]"""
    from torch.utils.checkpoint import checkpoint
    ran = []
    if around == "parameter_writer":
        mod = model.parameter_writer
        inner = mod.forward

        def forward(g, **kw):
            calls = []

            def run(h):
                calls.append(1)
                g.nodes["n1"].data["h"] = h
                inner(g, **kw)
                return tuple(g.nodes[lvl].data[k] for lvl, k in OUT_KEYS)
            h = g.nodes["n1"].data["h"]
            outs = checkpoint(run, h, use_reentrant=True)
            for (lvl, k), o in zip(OUT_KEYS, outs):
                g.nodes[lvl].data[k] = o
            g.nodes["n1"].data["h"] = h
            ran.append(calls)
            return g
    else:
        mod = model.gnn.blocks[len(model.gnn.blocks) - 1]
        inner = mod.forward

        def forward(plan, h):
            calls = []

            def run(hh):
                calls.append(1)
                return inner(plan, hh)
            ran.append(calls)
            return checkpoint(run, h, use_reentrant=True)
    mod.forward = forward
    seen = []
    try:
        yield seen
    finally:
        del mod.forward
        seen.extend(len(c) - 1 for c in ran)


def step_with_inner_pass(model, g, be, dev):
    """a train step whose backward pass runs ANOTHER pass from a hook on the atom embedding: torch.autograd.grad over a transformer layer
    of its own (product-backed: its weight gradients are queued by the inner pass and land in the inner parameters only).  -> the inner
    pass's worst distance to float64"""
    from grappa_amd import Energy, MolwiseLoss
    name = "TransformerLayerFn[s=4,T=40]"
    c = dict(function_cases(dev))[name]()
    douts = [torch.randn(4 * 40, FEATS, generator=torch.Generator().manual_seed(3)).to(dev)]
    inner, outer_before = {}, {}
    named = dict(model.named_parameters())

    def hook(grad):
        # (the outer pass is half-way: the heads are done, the GNN is still to come)
        outer_before.update({k: (None if p.grad is None else p.grad.detach().clone()) for k, p in named.items() if k.startswith("gnn.")})
        outer = torch._C._current_graph_task_id()
        with torch.enable_grad():                                # (hooks run with gradients disabled)
            outs = c["run"]()
        with counting(be, **({"flush_wgrads": lambda a, k, r: a[0] if a else k.get("task")} if hasattr(be, "flush_wgrads") else {})) as log:
            inner["dx"], = torch.autograd.grad(outs, [c["leaves"]["x"]], douts)
        # the inner pass launched what IT had queued at ITS end (a pass id of its own); what the outer pass has queued so far is still waiting
        inner["flushed"] = [t for t in log.get("flush_wgrads", [outer + 1]) if t is not None and t != outer]
        inner["queues"] = all(t == outer for t, _ in getattr(be, "_wq", {})) and all(it.task == outer for it in getattr(be, "_lnq", []))
        inner["outer_after"] = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in named.items() if k.startswith("gnn.")}
        return None

    def forward_hook(_m, _i, out):
        out.nodes["n1"].data["h"].register_hook(hook)
    handle = model.gnn.register_forward_hook(forward_hook)
    try:
        loss = MolwiseLoss(**LK)(Energy()(model(g)))
        loss.backward()
    finally:
        handle.remove()
    if loss.is_cuda:
        torch.cuda.synchronize()
    assert queues_empty(be)
    assert "dx" in inner and inner["queues"] and len(inner["flushed"]) == 1
    for k, v in inner["outer_after"].items():               # ... and touched nothing of the outer pass's targets
        assert (v is None and outer_before[k] is None) or torch.equal(v, outer_before[k]), k
    outs64, leaves64 = c["ref"]()
    keys = sorted(leaves64)
    ref = torch.autograd.grad(outs64, [leaves64[k] for k in keys], [d.cpu().double() for d in douts])
    worst = 0.0
    for k, r in zip(keys, ref):
        got = inner["dx"] if k == "x" else c["leaves"][k].grad
        assert got is not None, k
        worst = max(worst, grad_distance(got, r.numpy()))
    assert c["leaves"]["x"].grad is None                      # torch.autograd.grad returns the input's gradient instead of accumulating it
    assert worst < TOL, worst
    return worst


@contextlib.contextmanager
def stream_order_log(be):
    """what orders HIP streams, as the host issues it: every kernel launch of the backend with the stream it goes to, every event recorded
    on a stream and every wait of a stream for an event (torch.cuda.Stream.wait_stream is those two).  -> the log, for `unjoined`"""
    log = []
    rec, wait, stream = torch.cuda.Event.record, torch.cuda.Event.wait, be._stream

    def record(self, stream=None):
        s = torch.cuda.current_stream() if stream is None else stream
        log.append(("record", s.cuda_stream, id(self)))
        return rec(self, s)

    def wait_(self, stream=None):
        s = torch.cuda.current_stream() if stream is None else stream
        log.append(("wait", s.cuda_stream, id(self)))
        return wait(self, s)

    def launch():
        h = stream()
        log.append(("launch", int(h), None))
        return h
    torch.cuda.Event.record, torch.cuda.Event.wait, be._stream = record, wait_, launch
    try:
        yield log
    finally:
        torch.cuda.Event.record, torch.cuda.Event.wait = rec, wait
        del be._stream


def unjoined(log, main):
    """vector clocks over the log: clock[S][B] = position of the last launch on stream B that stream S is ordered behind.  -> the streams
    whose last launch the stream `main` is NOT ordered behind at the end of the log"""
    clock, events, last = {}, {}, {}
    for i, (what, s, ev) in enumerate(log):
        c = clock.setdefault(s, {})
        if what == "launch":
            c[s] = last[s] = i
        elif what == "record":
            events[ev] = dict(c)
        elif ev in events:
            for b, pos in events[ev].items():
                c[b] = max(c.get(b, -1), pos)
    seen = clock.get(main, {})
    return sorted(b for b, pos in last.items() if b != main and seen.get(b, -1) < pos)


def check_optional_gradients(be, dev):
    """the two gradients a Function computes only when asked: LinearFn's input gradient (ctx.needs_input_grad[0]: the model's first product
    reads input features that take none) and ParamOutFn's gradient of the statistics (needs_input_grad[7]: learnable_statistics) -- the
    product / the reduction must not run when nobody asked, and must when somebody did"""
    from grappa_amd import ops
    gen = torch.Generator().manual_seed(21)
    for ask in (False, True):
        x = torch.randn(N_ATOMS, FEATS, generator=gen).to(dev).requires_grad_(ask)
        w, b = (torch.randn(FEATS, FEATS, generator=gen) / 8).to(dev).requires_grad_(True), torch.zeros(FEATS, device=dev, requires_grad=True)
        y = ops.LinearFn.apply(x, w, b, ops.ELU, 0.0, 0)
        with counting(be, gemm=lambda a, k, r: (k.get("a_kcontig", True), k.get("b_kcontig", True))) as log:
            y.backward(torch.ones_like(y))
        assert sum(1 for ak, bk in log["gemm"] if ak and not bk) == int(ask), (ask, log["gemm"])
        assert (x.grad is not None) == ask and w.grad is not None and b.grad is not None
        o = torch.randn(2 * 40, 2, generator=gen).to(dev).requires_grad_(True)
        consts = torch.tensor([1.1, 0.2, 0.0, 2.0, 150.0, 0.0], device=dev, requires_grad=ask)
        k_, eq = ops.ParamOutFn.apply(o, 0, 40, 2, 0, False, 0.0, consts)
        with counting(be, "param_out_bwd", "param_out_bwd_stats") as log:
            (k_.sum() + eq.sum()).backward()
        assert len(log["param_out_bwd"]) == 1 and len(log["param_out_bwd_stats"]) == int(ask), ask
        assert (consts.grad is not None) == ask and o.grad is not None
    if hasattr(be, "flush_wgrads"):
        be.flush_wgrads()
    assert queues_empty(be)
