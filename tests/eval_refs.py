"""Test-only backend for the bootstrapped Evaluator: the oracle's `RefBackend` plus float64 torch restatements of the two entry points
`grappa_eval_moments_f32` / `grappa_eval_bootstrap_f64` (include/grappa_hip.h), so that the host logic of `grappa_amd.evaluation.Evaluator`
runs on a machine without a GPU, and the kernels have something to be compared with.  Written from the header's text: plain sums and
means, no attempt to mirror the kernels' order of summation."""
import numpy as np
import torch

from oracle.ops_ref import RefBackend

NMOM, NMET = 10, 7
D64 = torch.float64


class EvalRefBackend(RefBackend):
    def eval_moments(self, plan, energy, energy_ref, is_dummy, grad, grad_ref, out):
        B = plan.B
        n_real = getattr(plan, "n_real_mols", None)
        nB = B if n_real is None else int(n_real)                     # rows of a trailing padding molecule stay as the caller made them
        real = torch.ones(energy.shape, dtype=torch.bool) if is_dummy is None else (is_dummy.cpu() == 0)
        ptr = plan.atom_molptr.cpu().long().tolist()
        e64, er64 = energy.cpu().to(D64), energy_ref.cpu().to(D64)
        for b in range(nB):
            m = real[b]
            e, r = e64[b][m], er64[b][m]
            r = r - r.mean()
            d = (e - e.mean()) - r
            row = [float(m.sum()), float((d * d).sum()), float(d.abs().sum()), float(r.sum()), float((r * r).sum()), 0.0, 0.0, 0.0, 0.0, 0.0]
            if grad is not None:
                gr = grad_ref.cpu().to(D64)[ptr[b]:ptr[b + 1]][:, m]
                dg = grad.cpu().to(D64)[ptr[b]:ptr[b + 1]][:, m] - gr
                sq = (dg * dg).sum(-1)
                row[5:] = [float(sq.numel()), float(sq.sum()), float(sq.sqrt().sum()), float(gr.sum()), float((gr * gr).sum())]
            out[b] = torch.tensor(row, dtype=D64)

    def eval_bootstrap(self, mom, ds_ptr, idx, n_rep, rep0, rep1, rep_metrics, mean, std):
        M = mom.shape[0]
        p = ds_ptr.cpu().long().tolist()
        n_ds = len(p) - 1
        if n_rep < 1 or not (0 <= rep0 < rep1 <= n_rep) or idx.numel() != (rep1 - rep0) * M:
            raise ValueError("GRAPPA_ERR_ARG")
        sel = idx.cpu().long().reshape(rep1 - rep0, M)
        rm = rep_metrics.view(n_rep, n_ds, NMET)
        nan = float("nan")
        for i in range(rep1 - rep0):
            for d in range(n_ds):
                n = p[d + 1] - p[d]
                k = sel[i, p[d]:p[d + 1]]
                if n and (int(k.min()) < 0 or int(k.max()) >= n):
                    raise ValueError("GRAPPA_ERR_ARG")
                s = mom.cpu()[p[d] + k].sum(0).tolist() if n else [0.0] * NMOM
                nE, nV, nC = s[0], s[5], 3.0 * s[5]
                with np.errstate(all="ignore"):
                    f = np.float64
                    var_e = (f(s[4]) - f(s[3]) * f(s[3]) / f(nE)) / f(nE - 1.0)
                    var_g = (f(s[9]) - f(s[8]) * f(s[8]) / f(nC)) / f(nC - 1.0)
                    row = [np.sqrt(max(var_e, 0.0) if var_e == var_e else nan), np.sqrt(max(var_g, 0.0) if var_g == var_g else nan) * np.sqrt(3.0),
                           np.sqrt(f(s[1]) / f(nE)), f(s[2]) / f(nE), np.sqrt(f(s[6]) / f(nV)), np.sqrt(f(s[6]) / f(nC)), f(s[7]) / f(nV)]
                rm[rep0 + i, d] = torch.tensor([float(v) for v in row], dtype=D64)
        if rep1 == n_rep:
            x = rm.cpu().numpy()
            y = x - x[0:1]                                 # relative to replicate 0: equal replicates give exactly that value and a std of 0
            mu = y.mean(0)
            mean.view(n_ds, NMET).copy_(torch.from_numpy(x[0] + mu))
            std.view(n_ds, NMET).copy_(torch.from_numpy(np.sqrt(((y - mu) ** 2).mean(0))))
