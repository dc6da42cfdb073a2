"""The inputs and the restated trajectories of the stepwise dynamics with X-H constraints (grappa_md_steps_*_cons_f32), for
tests/test_host_md_steps_cons.py (CPU) and tests/test_gpu_md_steps_cons.py.  Never imported by the product.  The molecules are
relax_refs.gen_molecule's with leaves attached by md_cons_refs.attach_leaves; the truth is md_cons_refs.gbaoab_ref in float64, the
yardstick md_cons_refs.fp32_realisations; under a cutoff both run inside md_cut_refs.cut_force.

Cases, the smallest shapes at which a cluster that crosses the 64-atom blocks of the stepwise decomposition can go wrong:
    span64        60 heavy atoms, 3 conformations; 3 leaves on the odd-indexed end atoms, 2 on the even-indexed ones, 1 on every atom
                  with two bonds whose index is a multiple of 3: all centres in block 0, the leaves (60 ..) in blocks 0 and 1
    scattered130  90 heavy atoms, 3 conformations; 2 leaves on even-indexed end atoms, 1 on even-indexed atoms with two bonds; all atoms
                  permuted: three blocks, centres above and below their leaves
    k300          300 heavy atoms with one leaf each, 1 conformation: 600 atoms in ten blocks and 300 clusters -- above both limits of the
                  fused kernel -- and far longer than the cutoff, so that tiles are really skipped
    mixed         xh (2 atoms), a plain molecule of 7 atoms, a molecule without atoms, 50 heavy atoms with one leaf on the odd-indexed
                  atoms of at most two bonds, and xh4; 3 conformations: batch independence
md_cons_refs' own mix, edge256 and ethane64 are read through the same functions."""
import functools

import numpy as np
import torch

import md_cons_refs as mc
import md_cut_refs as mcut
import md_steps_refs as ms
import nb_cut_refs as nc
import relax_refs as rr

OWN = ("span64", "scattered130", "k300", "mixed")
TRAJ_CASES = list(OWN) + ["mix"]
CUT_CASES = ["span64", "k300"]
TRAJ_STEPS = mc.TRAJ_STEPS          # 1, 5, 40
TRAJ_DT = mc.TRAJ_DT                # 2 fs
NOMINAL = 9.0
BLOCK = 64                          # GRAPPA_NB_IBLOCK


def _degrees(mol):
    return np.bincount(mol["idx"][0].reshape(-1), minlength=mol["n"])


def _build(name):
    rng = np.random.default_rng(sum(map(ord, name)) * 7919 + 11)
    if name == "span64":
        mol = rr.gen_molecule(60, 3, rng)
        deg = _degrees(mol)
        leaves = {a: (3 if a % 2 else 2) for a in range(60) if deg[a] == 1}
        leaves.update({a: 1 for a in range(60) if deg[a] == 2 and a % 3 == 0})
        return [mc.attach_leaves(mol, leaves, rng)]
    if name == "scattered130":
        mol = rr.gen_molecule(90, 3, rng)
        deg = _degrees(mol)
        leaves = {a: 2 for a in range(0, 90, 2) if deg[a] == 1}
        leaves.update({a: 1 for a in range(0, 90, 2) if deg[a] == 2})
        n = 90 + sum(leaves.values())
        return [mc.attach_leaves(mol, leaves, rng, np.random.default_rng(5).permutation(n))]
    if name == "k300":
        return [mc.attach_leaves(rr.gen_molecule(300, 1, rng), {a: 1 for a in range(300)}, rng)]
    if name == "mixed":
        xh = mc.attach_leaves(rr.gen_molecule(1, 3, rng), {0: 1}, rng)
        plain, empty = mc._plain(7, 3, rng), mc._plain(0, 3, rng)
        mol = rr.gen_molecule(50, 3, rng)
        deg = _degrees(mol)
        chain = mc.attach_leaves(mol, {a: 1 for a in range(1, 50, 2) if deg[a] <= 2}, rng)
        return [xh, plain, empty, chain, mc.attach_leaves(rr.gen_molecule(1, 3, rng), {0: 4}, rng)]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (relax_refs.Batch, [Constraints or None per molecule], masses (N,) float32, keys (B,) uint64); computed once, read-only"""
    if name not in OWN:
        return mc.case(name)
    from grappa_amd.dynamics import mol_keys
    parts = _build(name)
    batch = rr.Batch([p[0] for p in parts])
    return batch, [p[1] for p in parts], np.concatenate([p[2] for p in parts]), mol_keys(sum(map(ord, name)), batch.B)


@functools.lru_cache(maxsize=None)
def tables(name) -> mc.Tables:
    batch, cons, _, _ = case(name)
    return mc.Tables(batch, cons)


@functools.lru_cache(maxsize=None)
def thermal_velocities(name, temperature=300.0) -> torch.Tensor:
    """md_cons_refs.thermal_velocities' recipe on this module's cases"""
    if name not in OWN:
        return mc.thermal_velocities(name, temperature)
    batch, _, m, _ = case(name)
    rng = np.random.default_rng(sum(map(ord, name)) * 15485863 + 3)
    s = np.sqrt(mc.ACC * mc.KB * temperature / m.astype(np.float64))
    return torch.from_numpy((s[:, None, None] * rng.standard_normal((batch.N, batch.xyz.shape[1], 3))).astype(np.float32))


@functools.lru_cache(maxsize=None)
def cutoff(name, prune=True) -> nc.Cutoff:
    """the nominal 9 A placed in the largest gap of the case's pair distances, switch from 0.8 rc, reaction field of water"""
    b = case(name)[0]
    rc, _ = nc.place_cutoff(b.params, b.xyz.numpy(), NOMINAL)
    return nc.Cutoff(rc, 0.8 * rc, 78.3, prune)


class _NoCut:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def force_of(name, cut):
    """the context in which the restatements of a case run: its cutoff's force, or all pairs"""
    return mcut.cut_force(cutoff(name)) if cut else _NoCut()


def restate(name, cut=False, dtype=torch.float64, **kw):
    """md_cons_refs.gbaoab_ref of the case (under its cutoff if cut)"""
    batch, cons, m, _ = case(name)
    with force_of(name, cut):
        return mc.gbaoab_ref(batch, m, cons, dtype, **kw)


def realisations(name, cut=False, **kw):
    batch, cons, m, _ = case(name)
    with force_of(name, cut):
        return mc.fp32_realisations(batch, m, cons, TRAJ_STEPS, **kw)


@functools.lru_cache(maxsize=None)
def verlet(name, cut=False):
    """friction 0, 2 fs, from the case coordinates with thermal_velocities, snapshots after TRAJ_STEPS: the float64 restatement (with
    its statuses, step counts and the most Newton updates any S took)"""
    return restate(name, cut, velocities=thermal_velocities(name), snapshots=TRAJ_STEPS, n_steps=max(TRAJ_STEPS), dt=TRAJ_DT)


@functools.lru_cache(maxsize=None)
def verlet32(name, cut=False):
    return realisations(name, cut, velocities=thermal_velocities(name), n_steps=max(TRAJ_STEPS), dt=TRAJ_DT)


def steady_counts(name, cut=False):
    """-> {"x": (non-steady, pairs), "v": ...} over the (item, step count) pairs of the case, in md_steps_refs.steady's sense"""
    b = case(name)[0]
    out = {"x": [0, 0], "v": [0, 0]}
    for k in TRAJ_STEPS:
        r32s = [r[k] for r in verlet32(name, cut)]
        for label, idx in (("x", 0), ("v", 1)):
            s = ms.steady(b, r32s, idx)
            out[label][0] += int((~s).sum())
            out[label][1] += s.numel()
    return out


def blocks_of(name):
    """per cluster of the case's FIRST clustered molecule: (block of the centre, blocks of its leaves), blocks counted within the molecule"""
    batch, cons, _, _ = case(name)
    b = next(i for i, c in enumerate(cons) if c is not None and c.n_clusters)
    return [(int(row[0]) // BLOCK, [int(a) // BLOCK for a in row[1:] if a >= 0]) for row in cons[b].clusters]
