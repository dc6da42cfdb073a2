"""`FastEvaluator`: per-dataset RMSE of energies and forces over batched graphs.

Drop-in for the reference's training/evaluation.py:16-159 (same constructor keywords, `step(g, dsnames)`,
`pool() -> {dsname: {'rmse_energies', 'rmse_gradients', 'crmse_gradients'}, 'avg': {...}}`), but `step` is ONE
kernel launch per batch (`grappa_eval_se_f32`, one workgroup per molecule: centred-energy and force squared errors with
dummy conformations masked) plus one device-side `index_add_` into per-dataset accumulators, instead of
`dgl.unbatch` and a Python loop of ~10 tiny kernels per molecule.  Nothing is copied to the host before `pool()`.

`Evaluator` (training/evaluation.py:164-386) is the test-time counterpart: seven metrics per dataset with bootstrap error bars, from
per-molecule moment rows (`grappa_eval_moments_f32`) resampled on the device (`grappa_eval_bootstrap_f64`); `eval_model` runs it over
resident datasets (training/eval_model.py).
"""
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib
from .backend import get_backend


class FastEvaluator:
    def __init__(self, log_parameters: bool = False, log_classical_values: bool = False, metric_names: Optional[List[str]] = None,
                 gradients: bool = True):
        if log_parameters:
            raise NotImplementedError("Logging of parameters is not supported anymore.")      # evaluation.py:33-34
        self.log_classical_values = log_classical_values
        self.metric_names = metric_names
        self.gradients = gradients
        self.init_storage()

    def init_storage(self):
        self._ds_index: Dict[str, int] = {}
        self._acc: Optional[torch.Tensor] = None          # (n_datasets, 8) float64 on the graphs' device: se_E, n_E, se_G, n_G, then the
        #                                                   same four for the classical force field vs the PREDICTION (evaluation.py:80-87)

    def register(self, dsnames: List[str], device) -> None:
        """fix the row of every dataset name up front (data parallel validation: every rank must use the same rows, whatever share of
        the batches it sees, so that `all_reduce()` adds like to like)"""
        self._index_of(list(dsnames), device)

    def all_reduce(self) -> None:
        """sum the accumulators over the ranks of the default process group (each rank has stepped through ITS share of the batches)"""
        import torch.distributed as tdist
        if self._acc is not None and tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
            tdist.all_reduce(self._acc, op=tdist.ReduceOp.SUM)

    def _index_of(self, dsnames: List[str], device) -> torch.Tensor:
        for n in dsnames:
            if n not in self._ds_index:
                self._ds_index[n] = len(self._ds_index)
        need = len(self._ds_index)
        if self._acc is None:
            self._acc = torch.zeros((max(need, 8), 8), dtype=torch.float64, device=device)
        elif self._acc.shape[0] < need:
            grown = torch.zeros((2 * need, 8), dtype=torch.float64, device=device)
            grown[: self._acc.shape[0]] = self._acc
            self._acc = grown
        return torch.tensor([self._ds_index[n] for n in dsnames], dtype=torch.int64).to(device, non_blocking=True)

    @torch.no_grad()
    def step(self, g, dsnames: List[str]):
        plan = g.plan()
        # a batch padded to a fixed shape (DeviceDataset.collate(pad_to=...)) ends in a padding molecule that is no molecule of any dataset
        nB = plan.B if getattr(plan, "n_real_mols", None) is None else int(plan.n_real_mols)
        assert len(dsnames) == nB, f"one dataset name per molecule: {len(dsnames)} names for {nB} molecules"
        gd, n1 = g.nodes["g"].data, g.nodes["n1"].data
        energy, energy_ref = gd["energy"].detach().float().contiguous(), gd["energy_ref"].detach().float().contiguous()
        assert energy.dim() == 2 and energy.shape[1] > 0, f"energies must be a tensor of shape (n_mols, n_confs) but is {tuple(energy.shape)}"
        assert energy.shape == energy_ref.shape, f"energies and energies_ref must have the same shape but are {energy.shape} and {energy_ref.shape}"
        grad = grad_ref = None
        if self.gradients:
            grad, grad_ref = n1["gradient"].detach().float().contiguous(), n1["gradient_ref"].detach().float().contiguous()
            assert grad.dim() == 3, f"gradients must be a tensor of shape (n_atoms,n_confs, 3) but is {tuple(grad.shape)}"
            assert grad.shape == grad_ref.shape, f"gradients and gradients_ref must have the same shape but are {grad.shape} and {grad_ref.shape}"
        is_dummy = gd["is_dummy"].float().contiguous() if "is_dummy" in gd else None
        out = torch.zeros((plan.B, 8), dtype=torch.float32, device=energy.device)
        be = get_backend()
        first = torch.zeros((plan.B, 4), dtype=torch.float32, device=energy.device)
        be.eval_se(plan, energy, energy_ref, is_dummy, grad, grad_ref, first)
        out[:, :4] = first
        if self.log_classical_values:
            e_cl = gd["energy_classical_ff"].detach().float().contiguous()
            g_cl = n1["gradient_classical_ff"].detach().float().contiguous() if self.gradients else None
            be.eval_se(plan, e_cl, energy, is_dummy, g_cl, grad, first)
            out[:, 4:] = first
        idx = self._index_of(list(dsnames), energy.device)
        self._acc.index_add_(0, idx, out[:nB].double())

    def pool(self):
        """per-dataset metrics (energies: per conformation; gradients: per 3-vector; crmse: per component) and their unweighted
        average over datasets; resets the storage (evaluation.py:115-159)."""
        metrics: Dict[str, Dict[str, Optional[float]]] = {}
        acc = self._acc.cpu().numpy() if self._acc is not None else np.zeros((0, 8))
        for dsname, i in self._ds_index.items():
            se_e, n_e, se_g, n_g, cse_e, _, cse_g, _ = (float(x) for x in acc[i])
            m = {"rmse_energies": float(np.sqrt(np.float32(se_e) / np.float32(n_e))),
                 "rmse_gradients": float(np.sqrt(np.float32(se_g) / np.float32(n_g))) if self.gradients else None,
                 "crmse_gradients": float(np.sqrt(np.float32(se_g) / np.float32(n_g) / np.float32(3.0))) if self.gradients else None}
            if self.log_classical_values:
                m["rmse_classical_gradients"] = float(np.sqrt(np.float32(cse_g) / np.float32(n_g))) if self.gradients else None
                m["rmse_classical_energies"] = float(np.sqrt(np.float32(cse_e) / np.float32(n_e)))
            if self.metric_names is not None:
                m = {k: v for k, v in m.items() if k in self.metric_names}
            metrics[dsname] = m
        metrics["avg"] = {}
        for key in ["rmse_energies", "rmse_gradients"]:
            if self.metric_names is not None and key not in self.metric_names:
                continue
            mlist = [metrics[d][key] for d in metrics if d not in ("avg", "all") and metrics[d][key] is not None]
            metrics["avg"][key] = None if len(mlist) == 0 else np.mean(mlist)
        self.init_storage()
        return metrics


def early_stopping_loss(metrics, energy_weight: float = 2.0) -> float:
    """the reference's model-selection criterion (training/lightning_model.py:257-262): energy_weight * <rmse_E> + <rmse_F>,
    each averaged over datasets with equal weight."""
    return float(energy_weight * metrics["avg"]["rmse_energies"] + metrics["avg"]["rmse_gradients"])


INDEX_CHUNK_BYTES = 64 << 20           # the resample indices go to the device in replicate chunks of at most this size


def bootstrap_indices(counts: List[int], n_bootstrap: int, seed: int = 0) -> np.ndarray:
    """the (n_bootstrap, sum(counts)) int32 resample table of `Evaluator.pool`, dataset by dataset in the order of `counts`, local to each
    dataset.  Row 0 is the full dataset; the other rows are drawn exactly as the reference draws them (training/evaluation.py:328-331 and
    :266-273): np.random.seed(seed), randint(0, 2**32, n_bootstrap - 1) replicate seeds, and per replicate np.random.seed(s) followed by one
    np.random.choice(n, n, replace=True) per dataset.  The reference leaves numpy's global generator in the state of its last draw; here the
    caller's state is saved before the first draw and restored after the last, so a pool() in the middle of a run changes nothing else."""
    idx = np.empty((max(int(n_bootstrap), 1), int(sum(counts))), dtype=np.int32)
    idx[0] = np.concatenate([np.arange(n, dtype=np.int32) for n in counts]) if len(counts) else 0
    if n_bootstrap > 1:
        state = np.random.get_state()
        try:
            np.random.seed(seed)
            seeds = np.random.randint(0, 2**32, size=n_bootstrap - 1).tolist()
            for r, s in enumerate(seeds, start=1):
                np.random.seed(s)
                o = 0
                for n in counts:
                    idx[r, o:o + n] = np.random.choice(n, size=n, replace=True)
                    o += n
        finally:
            np.random.set_state(state)
    return idx


class Evaluator:
    """Drop-in for the reference's `Evaluator` (training/evaluation.py:164-386): per-dataset test metrics -- std_energies, std_gradients,
    rmse_energies, mae_energies, rmse_gradients, crmse_gradients, mae_gradients, with `calculate_classical` and `suffix_classical_ref` the
    three `*_classical_*_from_ref` -- plain (`pool()`) or as mean and std over bootstrap resamples of the molecules (`pool(n_bootstrap)`).

    The reference keeps every molecule's energies and gradients and, per replicate and dataset, concatenates the resampled tensors before
    it takes means.  All of these metrics are functions of ten sums per molecule, so `step` is ONE kernel launch per batch
    (`grappa_eval_moments_f32`: a row of ten doubles per molecule, arithmetic in double) and a replicate is a gather-and-add of rows
    (`grappa_eval_bootstrap_f64`: one workgroup per (dataset, replicate), metrics, their mean and np.std finalised on the device).  Rows stay
    on the device; `pool` reads back once.  Molecules keep the order in which they were stepped (or, with `order=`, their global ordinals),
    datasets the order of their first molecule -- with that the resamples are the reference's, index for index.

    keep_data=True additionally keeps the flattened per-molecule tensors (one host read of the dummy mask per batch): `collect()` then
    exposes `all_energies`, `all_gradients`, `all_reference_energies`, `all_reference_gradients` per dataset, as the reference does.
    `device` is accepted for signature compatibility: the rows live where the graphs live.  Plotting (`plot_dir`) is out of scope."""

    def __init__(self, keep_data: bool = False, device="cpu", suffix: str = "", suffix_ref: str = "_ref", suffix_classical: str = "_classical_ff",
                 suffix_classical_ref: Optional[str] = None, calculate_classical: bool = False, plot_dir: Optional[str] = None):
        if plot_dir is not None:
            raise NotImplementedError("plotting the parameters (plot_dir) is not part of this engine (DESIGN.md section 7)")
        self.keep_data, self.device = keep_data, device
        self.suffix, self.suffix_ref = suffix, suffix_ref
        self.log_classical_values = calculate_classical
        self.suffix_classical, self.suffix_classical_ref = suffix_classical, suffix_classical_ref
        self.plot_dir = plot_dir
        self.init_storage()

    @property
    def _classical(self) -> bool:
        return bool(self.log_classical_values) and self.suffix_classical_ref is not None          # evaluation.py:379-384

    def init_storage(self):
        self._rows: List[torch.Tensor] = []             # per step (molecules, EVAL_NMOM) float64, on the graphs' device
        self._rows_cl: List[torch.Tensor] = []          # the same for the classical force field against ITS reference
        self._names: List[str] = []                     # per molecule: dataset name, ordinal (host values: they came from the host)
        self._ordinals: List[int] = []
        self._gathered = False
        self._kept: Dict[str, Dict[str, List[torch.Tensor]]] = {}          # keep_data: name -> quantity -> per-molecule tensors

    # ------------------------------------------------------------------------------------------------------------------
    def _moments(self, be, plan, gd, n1, sfx, sfx_ref, is_dummy):
        e, er = (gd[f"energy{s}"].detach().float().contiguous() for s in (sfx, sfx_ref))
        g, gr = (n1[f"gradient{s}"].detach().float().contiguous() for s in (sfx, sfx_ref))
        assert e.dim() == 2 and e.shape[1] > 0, f"energies must be a tensor of shape (n_mols, n_confs) but is {tuple(e.shape)}"
        assert e.shape == er.shape and g.dim() == 3 and g.shape == gr.shape, "prediction and reference must have the same shapes"
        out = torch.zeros((plan.B, _lib.EVAL_NMOM), dtype=torch.float64, device=e.device)
        be.eval_moments(plan, e, er, is_dummy, g, gr, out)
        return out, (e, er, g, gr)

    @torch.no_grad()
    def step(self, g, dsnames: List[str], order: Optional[List[int]] = None):
        """one batch: a moment row per molecule (one launch; a second one for the classical pair).  order: the global ordinal of every
        molecule of the batch -- data-parallel runs, where each rank steps through its share and `gather()` restores the global order."""
        plan = g.plan()
        nB = plan.B if getattr(plan, "n_real_mols", None) is None else int(plan.n_real_mols)      # (a padded batch ends in a padding molecule)
        if len(dsnames) != nB:
            raise ValueError(f"Number of graphs and dsnames must be equal but are {nB} and {len(dsnames)}")
        if order is not None and len(order) != nB:
            raise ValueError(f"one ordinal per molecule: {len(order)} for {nB} molecules")
        if self._gathered:
            raise RuntimeError("step() after gather(): call init_storage() first")
        gd, n1 = g.nodes["g"].data, g.nodes["n1"].data
        is_dummy = gd["is_dummy"].float().contiguous() if "is_dummy" in gd else None
        be = get_backend()
        rows, tensors = self._moments(be, plan, gd, n1, self.suffix, self.suffix_ref, is_dummy)
        self._rows.append(rows[:nB])
        if self._classical:
            self._rows_cl.append(self._moments(be, plan, gd, n1, self.suffix_classical, self.suffix_classical_ref, is_dummy)[0][:nB])
        base = len(self._names)
        self._names += [str(n) for n in dsnames]
        self._ordinals += [int(o) for o in order] if order is not None else list(range(base, base + nB))
        if self.keep_data:
            self._keep(plan, nB, dsnames, is_dummy, *tensors)

    def _keep(self, plan, nB, dsnames, is_dummy, e, er, g, gr):
        """evaluation.py:216-238 per molecule: centred energies of the real conformations (n_confs,), gradients (n_atoms * n_confs, 3)"""
        ptr = plan.atom_molptr.cpu().tolist()
        real = (is_dummy == 0).cpu() if is_dummy is not None else torch.ones(e.shape, dtype=torch.bool)
        for b in range(nB):
            m = real[b].to(e.device)
            kept = self._kept.setdefault(str(dsnames[b]), {"energies": [], "gradients": [], "reference_energies": [], "reference_gradients": []})
            for key, t in (("energies", e), ("reference_energies", er)):
                v = t[b][m]
                kept[key].append(v - v.mean())
            for key, t in (("gradients", g), ("reference_gradients", gr)):
                kept[key].append(t[ptr[b]:ptr[b + 1]][:, m].flatten(0, 1))

    def collect(self, bootstrap_seed: Optional[int] = None):
        """keep_data=True: the concatenated tensors of every dataset (evaluation.py:264-311), resampled like the reference's when a seed is given"""
        if not self.keep_data:
            raise RuntimeError("collect() needs Evaluator(keep_data=True): by default only the moment rows are kept")
        names = list(self._kept)
        if bootstrap_seed is not None:
            np.random.seed(bootstrap_seed)              # (the reference's own call, with its effect on numpy's global state)
            sel = {d: np.random.choice(len(self._kept[d]["energies"]), size=len(self._kept[d]["energies"]), replace=True).tolist() for d in names}
        else:
            sel = {d: range(len(self._kept[d]["energies"])) for d in names}
        self.n_mols = {d: len(self._kept[d]["energies"]) for d in names}
        for key in ("energies", "gradients", "reference_energies", "reference_gradients"):
            setattr(self, f"all_{key}", {d: torch.cat([self._kept[d][key][i] for i in sel[d]], dim=0) for d in names})

    # ------------------------------------------------------------------------------------------------------------------
    def gather(self) -> None:
        """data parallel (torch.distributed, more than one rank): all-gather the moment rows, their dataset names and ordinals, so that every
        rank holds the whole table; `pool` sorts it by ordinal, hence pools the same rows in the same order as a single rank would -- the
        same bits.  Collective: every rank calls it (a rank without molecules too)."""
        import torch.distributed as tdist
        if self._gathered or not (tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1):
            return
        world = tdist.get_world_size()
        meta = [None] * world
        tdist.all_gather_object(meta, (self._names, self._ordinals))
        counts = [len(m[0]) for m in meta]
        dev = self._rows[0].device if self._rows else torch.device("cuda" if tdist.get_backend() == "nccl" else "cpu")

        def gathered(parts):
            mine = torch.cat(parts) if parts else torch.zeros((0, _lib.EVAL_NMOM), dtype=torch.float64, device=dev)
            pad = torch.zeros((max(counts), _lib.EVAL_NMOM), dtype=torch.float64, device=dev)
            pad[:mine.shape[0]] = mine
            bufs = [torch.empty_like(pad) for _ in range(world)]
            tdist.all_gather(bufs, pad)
            return [torch.cat([b[:c] for b, c in zip(bufs, counts)])]

        self._rows = gathered(self._rows)
        if self._classical:
            self._rows_cl = gathered(self._rows_cl)
        self._names = [n for m in meta for n in m[0]]
        self._ordinals = [o for m in meta for o in m[1]]
        self._gathered = True

    def _table(self):
        """-> dataset names in the order of their first molecule, molecules per dataset, the moment tables with their rows grouped by dataset
        and, within a dataset, in the order of the molecules' ordinals"""
        by_ordinal = sorted(range(len(self._names)), key=lambda i: self._ordinals[i])
        ds_of: Dict[str, int] = {}
        for i in by_ordinal:
            ds_of.setdefault(self._names[i], len(ds_of))
        perm = sorted(by_ordinal, key=lambda i: ds_of[self._names[i]])          # (stable: the ordinals' order within a dataset)
        counts = [0] * len(ds_of)
        for n in self._names:
            counts[ds_of[n]] += 1
        dev = self._rows[0].device
        sel = torch.tensor(perm, dtype=torch.int64).to(dev, non_blocking=True)
        tables = [torch.cat(r).index_select(0, sel).contiguous() for r in ((self._rows, self._rows_cl) if self._classical else (self._rows,))]
        return list(ds_of), counts, tables

    @torch.no_grad()
    def pool(self, n_bootstrap: int = 0, seed: int = 0) -> dict:
        """n_bootstrap == 0: {dataset: {'n_confs', 'n_mols', metric: value}} (the reference's get_metrics).
        n_bootstrap > 0: {dataset: {metric: {'mean', 'std'}, 'n_confs', 'n_mols'}} over n_bootstrap replicates: replicate 0 is the full
        dataset, the others resample its molecules with replacement; std is np.std over the replicates (evaluation.py:314-355).
        The resamples are drawn on the host with numpy's global generator, seeded as the reference seeds it (`bootstrap_indices`); the
        caller's generator state is saved before and restored after, so pooling does not move anybody else's random numbers.  The index
        table is uploaded in replicate chunks of at most 64 MiB; everything is read back in one copy."""
        self.gather()
        if not self._names:
            return {}
        names, counts, tables = self._table()
        n_rep, n_ds, M = max(int(n_bootstrap), 1), len(names), len(self._names)
        nmet = len(_lib.EVAL_METRICS)
        dev = tables[0].device
        be = get_backend()
        idx = bootstrap_indices(counts, n_rep, seed)
        ds_ptr_dev = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(dev)
        out = torch.zeros((len(tables), n_rep + 2, n_ds, nmet), dtype=torch.float64, device=dev)       # per table: replicates, mean, std
        per_chunk = max(1, min(INDEX_CHUNK_BYTES // (4 * M), 65535))
        for r0 in range(0, n_rep, per_chunk):
            r1 = min(r0 + per_chunk, n_rep)
            chunk = torch.from_numpy(idx[r0:r1])
            if dev.type == "cuda":
                chunk = chunk.pin_memory().to(dev, non_blocking=True)          # one upload per chunk, read by every table's launch
            for t, table in enumerate(tables):
                be.eval_bootstrap(table, ds_ptr_dev, chunk, n_rep, r0, r1, out[t, :n_rep], out[t, n_rep], out[t, n_rep + 1])
        # n_confs of the full datasets: column 0 of the rows, added per dataset on the device (integers in double: exact in any order)
        seg = torch.repeat_interleave(torch.arange(n_ds, device=dev), ds_ptr_dev[1:].long() - ds_ptr_dev[:-1].long(), output_size=M)
        n_confs = torch.zeros(n_ds, dtype=torch.float64, device=dev).index_add_(0, seg, tables[0][:, 0])
        host = torch.cat([out[:, 0].reshape(-1), out[:, n_rep:].reshape(-1), n_confs]).cpu().numpy()          # THE read-back
        k = len(tables) * n_ds * nmet
        full = host[:k].reshape(len(tables), n_ds, nmet)
        spread = host[k:3 * k].reshape(len(tables), 2, n_ds, nmet)
        n_confs = host[3 * k:]
        cl = {"rmse_classical_energies_from_ref": 2, "rmse_classical_gradients_from_ref": 4, "crmse_classical_gradients_from_ref": 5}
        metrics = {}
        for d, name in enumerate(names):
            counts_d = {"n_confs": int(n_confs[d]), "n_mols": counts[d]}
            cols = [(m, 0, j) for j, m in enumerate(_lib.EVAL_METRICS)] + ([(m, 1, j) for m, j in cl.items()] if len(tables) > 1 else [])
            if n_bootstrap > 0:
                metrics[name] = {m: {"mean": float(spread[t, 0, d, j]), "std": float(spread[t, 1, d, j])} for m, t, j in cols}
                metrics[name].update(counts_d)
            else:
                metrics[name] = dict(counts_d)
                metrics[name].update({m: float(full[t, d, j]) for m, t, j in cols})
        return metrics

    def get_metrics(self) -> dict:
        """the plain metrics of the full datasets (evaluation.py:358-386)"""
        return self.pool(0)


def eval_model(model, datasets: Dict[str, "DeviceDataset"], n_bootstrap: int = 1000, seed: int = 0, forces_per_batch: float = 2e3,  # noqa: F821
               batch_size: Optional[int] = None) -> dict:
    """the test metrics of a trained model (training/eval_model.py): every dataset resident on the device, batches with all conformations
    (`conf_strategy='all'`), model + Energy without gradients, one `Evaluator` over all of them -> {'test': {dataset: metrics}}.
    batch_size=None: int(forces_per_batch / max_confs / max_atoms) molecules, at least 1, per dataset (eval_model.py:175-185; the reference
    keeps the first dataset's value for the later ones, which only changes how the same per-molecule sums are batched)."""
    from .energy import Energy
    was_training = model.training
    model.eval()
    energy = Energy()
    ev = Evaluator()
    try:
        with torch.no_grad():
            for ds in datasets.values():
                if batch_size is None:
                    bs = max(int(forces_per_batch / max(int(ds.n_confs[:len(ds)].max()), 1) / max(int(ds.count["n1"][:len(ds)].max()), 1)), 1)
                else:
                    bs = int(max(1, batch_size))
                for i in range(0, len(ds), bs):
                    g, names = ds.collate(list(range(i, min(i + bs, len(ds)))), "all")
                    ev.step(energy(model(g)), list(names))
            return {"test": ev.pool(n_bootstrap=n_bootstrap, seed=seed)}
    finally:
        model.train(was_training)
