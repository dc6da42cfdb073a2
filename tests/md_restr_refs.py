"""The restatements of the stepwise dynamics with restraints (grappa_md_steps_*_restr_f32), for tests/test_host_md_restr.py (CPU) and
tests/test_gpu_md_restr.py.  Never imported by the product.

`restr_force` is a context manager in the style of md_cut_refs.cut_force: inside it, what relax_refs.forces returns has the restraint
gradient added to G -- autograd of relax_restr_refs.restraint_terms, the tethers' reference taken from the batch's own xyz (plus an
offset) unless one is given, so that md_refs.fp32_realisations' rotated siblings carry a rotated reference -- E unchanged, and Er and
phi beside it.  With that md_refs.baoab_ref, md_refs.fp32_realisations, md_cons_refs.gbaoab_ref and test_gpu_md._gate_state serve
unchanged, and it composes with md_cut_refs.cut_force, md_gb_refs.gb_force and md_gb_cut_refs.gb_cut_force (those replace
nonbonded_refs.nb_ref, which relax_refs.forces looks up when it is called).  With empty tables it returns the unpatched tensors exactly.

Cases, on molecules of relax_steps_refs (masses, keys and 300 K velocities those of md_steps_refs); frozen atoms are masses of 0:
    s9_65_C17            two conformation chunks: one dihedral on the 9 atoms, two dihedrals and tethers on the 65
    s65_C3               a dihedral that names atom 64, the first atom of the second block, and atoms of the first (the issue's atoms 62
                         to 65 counted from 1 lie at 61 to 64: a proper of the molecule that holds atom 64 is taken), tethers on every
                         third atom, three frozen atoms
    s129_C3              three blocks: four dihedrals whose atoms lie in all three
    s1_2_17_130_5_64_C3  16 dihedrals on the 17 atoms, tethers with a DISPLACED reference on the single atom (no force-field force: a
                         pure oscillator), None for the molecules of 2 and 5 atoms, dihedrals and tethers on the 130, tethers on the 64
    s513_C1              two dihedrals and tethers, at 1 and 5 steps only
Targets differ per conformation, 0.3 to 1.5 rad from the start; pos_k 5 to 50 kcal/mol/A^2; dih_k 100 to 239 kcal/mol."""
import contextlib
import functools

import numpy as np
import torch

import md_refs as md
import md_steps_refs as ms
import relax_refs as rr
import relax_restr_refs as rs
from grappa_amd.restraints import MAX_DIHEDRALS, RestraintBatch, Restraints

TRAJ_STEPS = ms.TRAJ_STEPS
MIXED = ms.MIXED
CASES = ["s9_65_C17", "s65_C3", "s129_C3", MIXED, "s513_C1"]
SHORT = {"s513_C1": (1, 5)}          # step counts of a case that does not run all of TRAJ_STEPS
TRAJ = [(n, s) for n in CASES for s in SHORT.get(n, TRAJ_STEPS)]
BLOCK = 64
SALT = {}          # case -> seed offset: seeds with which the restatements alone stay inside the steady limit (tests/test_host_md_restr.py)


@contextlib.contextmanager
def restr_force(rb, reference=None, offset=None):
    """inside: relax_refs.forces (what md_refs.baoab_ref evaluates) adds the restraint gradient of `rb` to G; E stays the force field's;
    Er (B,C), phi (R,C) and abs_er beside them.  reference (N,C,3): the tethers'; None: the batch's own xyz (+ offset (N,C,3) float32,
    added in float32, as the caller of the library forms it)"""
    plain = rr.forces

    def with_restraints(batch, x, dtype=torch.float64, nonbonded=True):
        f = plain(batch, x, dtype, nonbonded)
        if rb is None or rb.empty:
            return f
        start = reference_of(batch, reference, offset)
        r = rs.restraint_terms(batch, rs.Tables(batch, rb), x, start, dtype)
        return {**f, "G": f["G"] + r["G"], "abs_f": f["abs_f"] + r["abs_g"], "Er": r["E"], "phi": r["phi"], "abs_er": r["abs_e"]}

    rr.forces = with_restraints
    try:
        yield
    finally:
        rr.forces = plain


def reference_of(batch, reference=None, offset=None):
    """the tethers' reference (N,C,3) float32 of a batch"""
    if reference is not None:
        return reference
    return batch.xyz if offset is None else batch.xyz + offset


def energy_at(batch, rb, x, reference=None, offset=None, dtype=torch.float64):
    """E_r (B,C) and phi (R,C) at x (N,C,3)"""
    r = rs.restraint_terms(batch, rs.Tables(batch, rb), x, reference_of(batch, reference, offset), dtype)
    return r["E"], r["phi"]


# ------------------------------------------------------------------------------------------------------------------------- cases
def _targets(mol, rows, C, rng):
    phi0 = rs.dihedral_t(torch.from_numpy(mol["xyz"]).double(), torch.from_numpy(rows).long()).numpy()
    tg = phi0 + rng.choice([-1.0, 1.0], size=(len(rows), C)) * rng.uniform(0.3, 1.5, size=(len(rows), C))
    return np.mod(tg + np.pi, 2 * np.pi) - np.pi


def _with_rows(mol, rows, C, rng, tether_every=0, frozen=None):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    n = mol["n"]
    pk = np.where(np.arange(n) % tether_every == 1, rng.uniform(5, 50, n), 0.0) if tether_every else None
    fz = None
    if frozen is not None:
        fz = np.zeros(n, dtype=bool)
        fz[list(frozen)] = True
    return Restraints(frozen=fz, position_k=pk, dihedrals=rows if len(rows) else None, dihedral_k=rng.uniform(100, 239, len(rows)) if len(rows) else None,
                      dihedral_targets=_targets(mol, rows, C, rng) if len(rows) else None)


def _proper_with(mol, want, also=None):
    """the first proper of the molecule that names atom `want` (and, with also = (lo, hi), an atom in [lo, hi))"""
    for row in mol["idx"][2]:
        if want in row and (also is None or any(also[0] <= a < also[1] for a in row if a != want)):
            return row
    raise AssertionError(f"no proper names atom {want}")


def _proper_within(mol, lo, hi):
    for row in mol["idx"][2]:
        if lo <= row.min() and row.max() < hi:
            return row
    raise AssertionError(f"no proper inside [{lo}, {hi})")


def _build(name, batch, C, rng):
    """-> ([Restraints or None per molecule], offset (N,C,3) float32 or None)"""
    mols = batch.mols
    if name == "s9_65_C17":
        return [rs._restraints_of(mols[0], C, rng, 1), rs._restraints_of(mols[1], C, rng, 2, 0, 4)], None
    if name == "s65_C3":
        row = _proper_with(mols[0], 64, (0, 64))
        return [_with_rows(mols[0], [row], C, rng, tether_every=3, frozen=(5, 63, 64))], None
    if name == "s129_C3":
        rows = [_proper_within(mols[0], 0, 64), _proper_with(mols[0], 64, (0, 64)), _proper_within(mols[0], 64, 128), _proper_with(mols[0], 128)]
        assert {int(a) // BLOCK for r in rows for a in r} == {0, 1, 2} and len({tuple(r) for r in rows}) == 4
        return [_with_rows(mols[0], rows, C, rng, tether_every=7)], None
    if name == MIXED:
        assert batch.counts == [1, 2, 17, 130, 5, 64]
        single = Restraints(position_k=rng.uniform(5, 50, 1))
        items = [single, None, rs._restraints_of(mols[2], C, rng, MAX_DIHEDRALS), rs._restraints_of(mols[3], C, rng, 2, 0, 5), None,
                 rs._restraints_of(mols[5], C, rng, 0, 0, 3)]
        offset = np.zeros((batch.N, C, 3), dtype=np.float32)
        offset[0] = rng.uniform(0.2, 0.5, size=(C, 3)) * rng.choice([-1.0, 1.0], size=(C, 3))
        return items, torch.from_numpy(offset)
    if name == "s513_C1":
        return [rs._restraints_of(mols[0], C, rng, 2, 0, 5)], None
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: batch, rb (the RestraintBatch WITHOUT frozen: what goes down), rb_frozen (with it: what the front end is given), masses
    (frozen atoms 0), masses_in (as the front end is given them), keys, vel, offset, frozen (atom indices).  Computed once, read-only"""
    batch = ms.case(name)
    C = batch.xyz.shape[1]
    rng = np.random.default_rng(sum(map(ord, name)) * 104729 + C + 1000003 * SALT.get(name, 0) + 7)
    items, offset = _build(name, batch, C, rng)
    full = RestraintBatch(items, C, atom_counts=batch.counts)
    m_in = ms.masses(name)
    frozen = np.zeros(batch.N, dtype=bool) if full.frozen is None else full.frozen.numpy() != 0
    m = np.where(frozen, np.float32(0.0), m_in).astype(np.float32)
    down = RestraintBatch([None if r is None else Restraints(position_k=r.position_k, dihedrals=r.dihedrals if r.n_dihedrals else None,
                                                            dihedral_k=r.dihedral_k if r.n_dihedrals else None,
                                                            dihedral_targets=r.dihedral_targets if r.n_dihedrals else None) for r in items],
                          C, atom_counts=batch.counts)
    return dict(batch=batch, rb=down, rb_frozen=full, masses=m, masses_in=m_in, keys=ms.keys(name), vel=ms.thermal_velocities(name), offset=offset,
                frozen=np.flatnonzero(frozen))


def zero_strength(rb: RestraintBatch, batch) -> RestraintBatch:
    """the same rows with dih_k = 0 and pos_k = 0 (R > 0 stays)"""
    out = rb.to("cpu")
    out.dih_k = torch.zeros_like(rb.dih_k)
    out.pos_k = torch.zeros(batch.N, dtype=torch.float32)
    return out


@functools.lru_cache(maxsize=None)
def verlet32(name, steps=None):
    """friction 0, 1 fs, from the case coordinates with thermal velocities: md_refs.fp32_realisations after the case's step counts"""
    c = case(name)
    snaps = SHORT.get(name, TRAJ_STEPS)
    with restr_force(c["rb"], offset=c["offset"]):
        return md.fp32_realisations(c["batch"], c["masses"], snaps, velocities=c["vel"], n_steps=max(snaps) if steps is None else steps)


def verlet(name):
    return {k: pair[1] for k, pair in verlet32(name)[0].items()}


def steady_counts(names=CASES):
    """-> {"x": [non-steady, pairs], "v": ...} over all (item, step count) pairs, in md_steps_refs.steady's sense"""
    out = {"x": [0, 0], "v": [0, 0]}
    for name in names:
        b = case(name)["batch"]
        for k in SHORT.get(name, TRAJ_STEPS):
            r32s = [r[k] for r in verlet32(name)]
            for label, idx in (("x", 0), ("v", 1)):
                s = ms.steady(b, r32s, idx)
                out[label][0] += int((~s).sum())
                out[label][1] += s.numel()
    return out


# ------------------------------------------------------------------------------------------------------------------------- conservation
@functools.lru_cache(maxsize=None)
def nve_case():
    """md_steps_refs.nve_batch (s2_130_9_C3 at its relaxed coordinates) with tethers on every fourth atom of the 130 and two dihedrals
    on it, one dihedral on the 9: -> (batch, RestraintBatch)"""
    b = ms.nve_batch()
    C = b.xyz.shape[1]
    rng = np.random.default_rng(20240607)
    items = [None, rs._restraints_of(b.mols[1], C, rng, 2, 0, 4), rs._restraints_of(b.mols[2], C, rng, 1)]
    return b, RestraintBatch(items, C, atom_counts=b.counts)


@functools.lru_cache(maxsize=None)
def nve_drift(dtype):
    """D = max over frames and items of |E_tot - E_tot at step 0| with E_tot = epot + E_r + ekin, of the restatement in `dtype`"""
    b, rb = nve_case()
    m, v = ms.masses(ms.NVE_CASE), ms.thermal_velocities(ms.NVE_CASE)
    with restr_force(rb):
        start = md.baoab_ref(b, m, dtype, velocities=v, n_steps=0)
        r = md.baoab_ref(b, m, dtype, velocities=v, **ms.NVE)
    assert not r["status"].any()
    er0 = energy_at(b, rb, start["xyz"], dtype=dtype)[0].double()
    er = torch.stack([energy_at(b, rb, x, dtype=dtype)[0].double() for x in r["frame_xyz"]])
    return md.drift(start["epot"] + er0 + start["ekin"], r["frame_epot"] + er + r["frame_ekin"])
