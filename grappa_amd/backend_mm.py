"""The molecular-mechanics part of `HipBackend` (backend.py inherits it): bonded energy, gradient and backward, nonbonded terms, the
two FIRE minimisers and the two Langevin dynamics.  Every method reads as checks, descriptor, call; what several of them check the same way
is a helper here.  It uses `self.lib`, `self._stream()` and `self._workspace()` of the backend."""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from ._marshal import _chk, _flat, _ptr

_F32, _I32, _I64 = torch.float32, torch.int32, torch.int64
_NB_INT = ("atom_molptr", "exc_ptr", "exc_atom")
_NB_F32 = ("charge", "sigma", "epsilon", "exc_qq", "exc_sigma", "exc_eps")


def _xyz3(xyz, who):
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 3 or xyz.shape[2] != 3:
        raise ValueError(f"{who}: xyz must be an (N, C, 3) tensor, got {tuple(xyz.shape) if isinstance(xyz, torch.Tensor) else type(xyz)}")


def _tensors(dev, specs, optional=(), where=None):
    """every (tensor, name, dtype) of specs is a contiguous tensor of that type on dev; the ones named in `optional` may be None"""
    where = f" on {dev}" if where is None else where
    for t, n, dt in specs:
        if t is None and n in optional:
            continue
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{n}: expected a contiguous {dt} tensor{where}")
        _flat(t, n, dev, dt)


def _opts_struct(cls, opts, who):
    """the ctypes options struct `cls` from a dict that holds exactly its fields"""
    names = [f[0] for f in cls._fields_]
    if sorted(opts) != sorted(names):
        raise ValueError(f"{who}: opts must hold exactly {names}, got {sorted(opts)}")
    o = cls()
    for k, ct in cls._fields_:
        setattr(o, k, float(opts[k]) if ct is C.c_float else int(opts[k]))
    return o


def _cut_struct(cutoff, who):
    """grappa_nb_cut from a `grappa_amd.nonbonded.Cutoff` (or a plain distance)"""
    from .nonbonded import as_cutoff
    return _opts_struct(_lib.NbCut, as_cutoff(cutoff).as_opts(), who)


def _atom_counts(atom_counts_host, N, B, who, limit=None):
    """atoms per molecule as the caller knows them on the host; limit: the size a molecule may have (None: any, none negative)"""
    counts = [int(c) for c in atom_counts_host]
    if len(counts) != B or sum(counts) != N or (limit is None and counts and min(counts) < 0):
        raise ValueError(f"{who}: atom_counts_host names {len(counts)} molecules / {sum(counts)} atoms, the batch has {B} / {N}")
    if limit is not None and counts and max(counts) > limit:
        raise ValueError(f"{who}: a molecule of {max(counts)} atoms is above the limit of {limit} atoms per molecule")
    return counts


def _relax_outputs(who, xyz, B, xyz_out, energy, gmax, steps, status, term_energy, grad):
    """the outputs the two minimisers share"""
    _tensors(xyz.device, ((xyz_out, "xyz_out", _F32), (energy, "energy", _F32), (gmax, "gmax", _F32), (steps, "steps", _I32),
                          (status, "status", _I32), (term_energy, "term_energy", _F32), (grad, "grad", _F32)), ("term_energy", "grad"))
    BC = B * xyz.shape[1]
    if xyz_out.shape != xyz.shape or (grad is not None and grad.shape != xyz.shape) or any(t.numel() != BC for t in (energy, gmax, steps, status)) \
            or (term_energy is not None and term_energy.numel() != 6 * BC):
        raise ValueError(f"{who}: expected xyz_out / grad (N,C,3), energy / gmax / steps / status (B,C), term_energy (6,B,C)")


def _nb_desc(N, Cc, B, xyz, tables):
    d = _lib.NbDesc()
    d.N, d.C, d.B, d.xyz = N, Cc, B, _ptr(xyz)
    for n in _NB_INT + _NB_F32:
        setattr(d, n, tables[n].data_ptr())
    return d


def _nb_tables_desc(nb, N, Cc, B, dev, who):
    """grappa_nb_desc of the device tables of a NonbondedBatch (atom_molptr, charge, sigma, epsilon, exc_ptr, exc_atom, exc_qq, exc_sigma,
    exc_eps) for the kernels that take their coordinates from the MM descriptor (xyz = NULL); None for nb = None"""
    if nb is None:
        return None
    t = {n: getattr(nb, n) for n in _NB_INT + _NB_F32}
    _tensors(dev, [(t[n], "nb." + n, _I32) for n in _NB_INT] + [(t[n], "nb." + n, _F32) for n in _NB_F32])
    if nb.atom_molptr.numel() != B + 1 or nb.exc_ptr.numel() != N + 1 or any(t[n].numel() != N for n in ("charge", "sigma", "epsilon")):
        raise ValueError(f"{who}: the nonbonded tables do not describe the batch's {B} molecules / {N} atoms")
    if not (nb.exc_atom.numel() == nb.exc_qq.numel() == nb.exc_sigma.numel() == nb.exc_eps.numel() >= 1):
        raise ValueError(f"{who}: exc_atom / exc_qq / exc_sigma / exc_eps must share one length >= 1")
    return _nb_desc(N, Cc, B, None, t)


class MMBackend:
    # ------------------------------------------------------------------ MM energy
    def _mm_desc(self, plan, xyz, ks, eqs, n_per, offset_torsion):
        from .constants import TUPLE_LEVELS
        dev = xyz.device
        _flat(xyz, "xyz", dev)
        N, Cc = xyz.shape[0], xyz.shape[1]
        if N != plan.N or xyz.shape[2] != 3 or plan.indptr.device != dev:
            raise ValueError("mm: xyz does not match the batch plan")
        d = _lib.MMDesc()
        d.N, d.C, d.B = N, Cc, plan.B
        d.xyz = xyz.data_ptr()
        for l, lvl in enumerate(TUPLE_LEVELS):
            T = plan.T[lvl]
            d.T[l] = T
            d.idx[l] = plan.idx32[lvl].data_ptr()
            d.mol_ptr[l] = plan.mol_ptr[lvl].data_ptr()
            k = ks[l]
            _flat(k, f"k[{lvl}]", dev)
            if l < 2:
                if k.numel() != T:
                    raise ValueError(f"mm: k[{lvl}] length")
                _flat(eqs[l], f"eq[{lvl}]", dev)
                if eqs[l].numel() != T:
                    raise ValueError(f"mm: eq[{lvl}] length")
                d.eq[l] = eqs[l].data_ptr()
                d.n_per[l] = 0
            else:
                if k.numel() != T * n_per[l]:
                    raise ValueError(f"mm: k[{lvl}] must be (T,{n_per[l]})")
                d.n_per[l] = n_per[l]
            d.k[l] = k.data_ptr()
        d.offset_torsion = int(offset_torsion)
        d.inc_ptr, d.inc_code, d.atom_molptr = plan.inc_ptr.data_ptr(), plan.inc_code.data_ptr(), plan.atom_molptr.data_ptr()
        return d

    def mm_energy_fwd(self, plan, xyz, ks, eqs, n_per, offset_torsion, energy, term_energy, tuple_e=None, tuple_x=None) -> None:
        d = self._mm_desc(plan, xyz, ks, eqs, n_per, offset_torsion)
        te = _lib.VP4(*[_ptr(t) for t in (tuple_e or [None] * 4)])
        tx = _lib.VP4(*[_ptr(t) for t in (tuple_x or [None] * 4)])
        _chk(self.lib.grappa_mm_energy_fwd_f32(self._stream(), C.byref(d), energy.data_ptr(), _ptr(term_energy), C.byref(te), C.byref(tx)),
             "grappa_mm_energy_fwd_f32")

    def mm_gradient_fwd(self, plan, xyz, ks, eqs, n_per, grad) -> None:
        d = self._mm_desc(plan, xyz, ks, eqs, n_per, False)
        _flat(grad, "grad", xyz.device)
        if grad.shape != xyz.shape:
            raise ValueError("mm_gradient_fwd: grad shape")
        _chk(self.lib.grappa_mm_gradient_fwd_f32(self._stream(), C.byref(d), grad.data_ptr()), "grappa_mm_gradient_fwd_f32")

    def mm_bwd(self, plan, xyz, ks, eqs, n_per, offset_torsion, gE, gG, gks, geqs) -> None:
        d = self._mm_desc(plan, xyz, ks, eqs, n_per, offset_torsion)
        for t, n in ((gE, "gE"), (gG, "gG")):
            if t is not None:
                _flat(t, n, xyz.device)
        a = _lib.VP4(*[_ptr(t) for t in gks])
        b = _lib.VP4(*[_ptr(t) for t in geqs])
        _chk(self.lib.grappa_mm_bwd_f32(self._stream(), C.byref(d), _ptr(gE), _ptr(gG), C.byref(a), C.byref(b)), "grappa_mm_bwd_f32")

    # ------------------------------------------------------------------ nonbonded
    def nonbonded_plan(self, atom_molptr_host, N: int, n_confs: int, device) -> "tuple":
        """the work-item list of the nonbonded kernel for C = n_confs, built on the host from a HOST atom_molptr (int32, (B+1,)) and
        uploaded: (table on the device, n_items, n_blocks, C) for `nonbonded(..., plan=)` (include/grappa_hip.h grappa_nonbonded_plan)"""
        _flat(atom_molptr_host, "atom_molptr_host", torch.device("cpu"), torch.int32)
        B = atom_molptr_host.numel() - 1
        if B < 1 or n_confs < 1:
            return (None, 0, 0, int(n_confs))
        need = self.lib.grappa_nonbonded_plan(int(N), int(n_confs), B, atom_molptr_host.data_ptr(), None, 0)
        if need < 0:
            _chk(int(need), "grappa_nonbonded_plan")
        table = torch.empty(int(need), dtype=torch.int32)
        rc = self.lib.grappa_nonbonded_plan(int(N), int(n_confs), B, atom_molptr_host.data_ptr(), table.data_ptr(), table.numel())
        if rc < 0:
            _chk(int(rc), "grappa_nonbonded_plan")
        return (table.to(device), int(table[0]), int(table[1]), int(n_confs))

    def nonbonded(self, xyz, atom_molptr, charge, sigma, epsilon, exc_ptr, exc_atom, exc_qq, exc_sigma, exc_eps, energy, term_energy=None, grad=None,
                  plan=None, cutoff=None, tiles=None) -> None:
        """Lennard-Jones + Coulomb energy and gradient over all pairs of every molecule (include/grappa_hip.h grappa_nonbonded_fwd_f32):
        xyz (N,C,3), atom_molptr (B+1,) int32, charge / sigma / epsilon (N,), the symmetric CSR exception table exc_ptr (N+1,) int32,
        exc_atom int32, exc_qq / exc_sigma / exc_eps (at least one element each) -> energy (B,C), term_energy (2,B,C) or None,
        grad (N,C,3) or None.  Angstrom, kcal/mol, elementary charges; the gradient is +dE/dxyz.
        plan: what `nonbonded_plan` returned for this atom_molptr and C (the work-item list built once on the host: one launch less and
        an exact grid); None: the list is built on the device by every call.  Same bits either way.
        cutoff: a `grappa_amd.nonbonded.Cutoff` or a distance (None: all pairs, the calls above) -- grappa_nonbonded_fwd_cut_f32: a
        reaction field and a switch below the cutoff, exceptions uncut, far tiles skipped; it needs `plan`.  tiles: an int32 tensor of
        n_items or None -> the tiles each work item evaluated.
        Out of scope: gradients with respect to charge, sigma or epsilon (no autograd wrapper: the term has no learnable input);
        periodic boxes, PME, a long-range Lennard-Jones correction."""
        _xyz3(xyz, "nonbonded")
        if tiles is not None and cutoff is None:
            raise ValueError("nonbonded: tiles needs a cutoff")
        dev = xyz.device
        tb = dict(atom_molptr=atom_molptr, exc_ptr=exc_ptr, exc_atom=exc_atom, charge=charge, sigma=sigma, epsilon=epsilon, exc_qq=exc_qq,
                 exc_sigma=exc_sigma, exc_eps=exc_eps)
        _tensors(dev, [(xyz, "xyz", _F32)] + [(tb[n], n, _I32) for n in _NB_INT] + [(tb[n], n, _F32) for n in _NB_F32] +
                 [(energy, "energy", _F32), (term_energy, "term_energy", _F32), (grad, "grad", _F32)], ("term_energy", "grad"))
        N, Cc, B = xyz.shape[0], xyz.shape[1], atom_molptr.numel() - 1
        if B < 0 or exc_ptr.numel() != N + 1 or any(t.numel() != N for t in (charge, sigma, epsilon)):
            raise ValueError("nonbonded: atom_molptr must be (B+1,), exc_ptr (N+1,), charge / sigma / epsilon (N,)")
        if not (exc_atom.numel() == exc_qq.numel() == exc_sigma.numel() == exc_eps.numel() >= 1):
            raise ValueError("nonbonded: exc_atom / exc_qq / exc_sigma / exc_eps must share one length >= 1")
        if energy.numel() != B * Cc or (term_energy is not None and term_energy.numel() != 2 * B * Cc) or (grad is not None and grad.shape != xyz.shape):
            raise ValueError("nonbonded: expected energy (B,C), term_energy (2,B,C), grad (N,C,3)")
        d = _nb_desc(N, Cc, B, xyz, tb)
        if cutoff is not None and (plan is None or plan[0] is None) and N and Cc and B:
            raise ValueError("nonbonded: a cutoff needs the plan of `nonbonded_plan` (the planned form is the only one with a cutoff)")
        if plan is not None and plan[0] is not None:
            table, n_items, n_blocks, plan_c = plan
            if plan_c != Cc or table.device != dev or table.dtype != torch.int32 or table.numel() < 4 + B + 1 + 4 * n_items:
                raise ValueError(f"nonbonded: the plan was made for C = {plan_c} on {table.device}, the call has C = {Cc} on {dev}")
            if cutoff is not None:
                cut = _cut_struct(cutoff, "nonbonded")
                if tiles is not None:
                    _tensors(dev, ((tiles, "tiles", _I32),))
                    if tiles.numel() != n_items:
                        raise ValueError(f"nonbonded: tiles must hold one int32 per work item ({n_items})")
                ws = self._workspace(int(self.lib.grappa_nonbonded_cut_workspace_bytes(Cc, n_blocks)), dev)
                _chk(self.lib.grappa_nonbonded_fwd_cut_f32(self._stream(), C.byref(d), C.byref(cut), table.data_ptr(), n_items, n_blocks,
                                                           energy.data_ptr(), _ptr(term_energy), _ptr(grad), _ptr(tiles), ws.data_ptr(), ws.numel()),
                     "grappa_nonbonded_fwd_cut_f32")
                return
            ws = self._workspace(16 * n_blocks * Cc, dev)
            _chk(self.lib.grappa_nonbonded_fwd_planned_f32(self._stream(), C.byref(d), table.data_ptr(), n_items, n_blocks, energy.data_ptr(),
                                                           _ptr(term_energy), _ptr(grad), ws.data_ptr(), ws.numel()), "grappa_nonbonded_fwd_planned_f32")
            return
        ws = self._workspace(self.lib.grappa_nonbonded_workspace_bytes(N, Cc, B), dev)
        _chk(self.lib.grappa_nonbonded_fwd_f32(self._stream(), C.byref(d), energy.data_ptr(), _ptr(term_energy), _ptr(grad), ws.data_ptr(), ws.numel()),
             "grappa_nonbonded_fwd_f32")

    # ------------------------------------------------------------------ implicit solvent
    def gb_obc(self, xyz, atom_molptr, charge, radius, scale, opts, energy, term_energy=None, grad=None, born=None, plan=None, cut=None,
               tiles=None) -> None:
        """GB/SA implicit solvent in the Onufriev-Bashford-Case form (include/grappa_hip.h grappa_gb_obc_fwd_f32 states the energy):
        xyz (N,C,3), atom_molptr (B+1,) int32, charge / radius / scale (N,) float32; opts: the eight options of grappa_gb_desc by name
        (`ImplicitSolvent.as_opts()`); plan (required): what `nonbonded_plan` returned for this atom_molptr and C.
        -> energy (B,C), term_energy (2,B,C: polar, surface area) or None, grad (N,C,3) = +dE/dxyz or None, born (N,C) = the Born radii
        or None.  Angstrom, kcal/mol, elementary charges.  4 launches, 3 without grad.  radius <= offset or scale <= 0 make the
        molecule's results NaN (`GBParameters.validate` refuses them on the host).
        cut: None (all pairs, the call above) or the two options of grappa_gb_cut by name (`ImplicitSolvent.cut_opts()`) --
        grappa_gb_obc_fwd_cut_f32: every pair sum over j != i keeps the pairs with r < cutoff only, far tiles are skipped (prune); one
        launch more.  tiles: an int32 tensor of n_items or None -> the tiles each work item evaluated.
        Out of scope: HCT / GBn, a salt term."""
        _xyz3(xyz, "gb_obc")
        if tiles is not None and cut is None:
            raise ValueError("gb_obc: tiles needs a cutoff")
        gc = None if cut is None else _opts_struct(_lib.GbCut, cut, "gb_obc: cut")
        dev = xyz.device
        _tensors(dev, [(xyz, "xyz", _F32), (atom_molptr, "atom_molptr", _I32), (charge, "charge", _F32), (radius, "radius", _F32),
                       (scale, "scale", _F32), (energy, "energy", _F32), (term_energy, "term_energy", _F32), (grad, "grad", _F32),
                       (born, "born", _F32)], ("term_energy", "grad", "born"))
        N, Cc, B = xyz.shape[0], xyz.shape[1], atom_molptr.numel() - 1
        if B < 0 or any(t.numel() != N for t in (charge, radius, scale)):
            raise ValueError("gb_obc: atom_molptr must be (B+1,), charge / radius / scale (N,)")
        if energy.numel() != B * Cc or (term_energy is not None and term_energy.numel() != 2 * B * Cc) or (grad is not None and grad.shape != xyz.shape) \
                or (born is not None and born.numel() != N * Cc):
            raise ValueError("gb_obc: expected energy (B,C), term_energy (2,B,C), grad (N,C,3), born (N,C)")
        names = [f[0] for f in _lib.GbDesc._fields_ if f[0] not in ("radius", "scale")]
        if sorted(opts) != sorted(names):
            raise ValueError(f"gb_obc: opts must hold exactly {names}, got {sorted(opts)}")
        if N == 0 or Cc == 0 or B == 0:
            return
        if plan is None or plan[0] is None:
            raise ValueError("gb_obc: the plan of `nonbonded_plan` is required (the planned form is the only one)")
        table, n_items, n_blocks, plan_c = plan
        if plan_c != Cc or table.device != dev or table.dtype != torch.int32 or table.numel() < 4 + B + 1 + 4 * n_items:
            raise ValueError(f"gb_obc: the plan was made for C = {plan_c} on {table.device}, the call has C = {Cc} on {dev}")
        d = _lib.NbDesc()
        d.N, d.C, d.B, d.xyz, d.atom_molptr, d.charge = N, Cc, B, xyz.data_ptr(), atom_molptr.data_ptr(), charge.data_ptr()
        g = _lib.GbDesc(radius=radius.data_ptr(), scale=scale.data_ptr(), **{k: float(opts[k]) for k in names})
        if gc is not None:
            if tiles is not None:
                _tensors(dev, ((tiles, "tiles", _I32),))
                if tiles.numel() != n_items:
                    raise ValueError(f"gb_obc: tiles must hold one int32 per work item ({n_items})")
            ws = self._workspace(int(self.lib.grappa_gb_obc_cut_workspace_bytes(N, Cc, n_blocks)), dev)
            _chk(self.lib.grappa_gb_obc_fwd_cut_f32(self._stream(), C.byref(d), C.byref(g), C.byref(gc), table.data_ptr(), n_items, n_blocks,
                                                    energy.data_ptr(), _ptr(term_energy), _ptr(grad), _ptr(born), _ptr(tiles), ws.data_ptr(),
                                                    ws.numel()), "grappa_gb_obc_fwd_cut_f32")
            return
        ws = self._workspace(int(self.lib.grappa_gb_obc_workspace_bytes(N, Cc, n_blocks)), dev)
        _chk(self.lib.grappa_gb_obc_fwd_f32(self._stream(), C.byref(d), C.byref(g), table.data_ptr(), n_items, n_blocks, energy.data_ptr(),
                                            _ptr(term_energy), _ptr(grad), _ptr(born), ws.data_ptr(), ws.numel()), "grappa_gb_obc_fwd_f32")

    # ------------------------------------------------------------------ relaxation
    def relax_max_atoms(self) -> int:
        return int(self.lib.grappa_relax_max_atoms())

    def relax_fire(self, plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, xyz_out, energy, gmax, steps, status, term_energy=None, grad=None,
                   atom_counts_host=None, restraints=None, restraint_energy=None, dihedral_out=None) -> None:
        """the fused FIRE minimiser (include/grappa_hip.h grappa_relax_fire_f32): one launch relaxes every (molecule, conformation) of
        the batch under the bonded terms (plan, ks, eqs, n_per, offset_torsion as for mm_energy_fwd; xyz (N,C,3) is the start) plus,
        if nb is not None, Lennard-Jones + Coulomb (nb: the device tables of a NonbondedBatch: atom_molptr, charge, sigma, epsilon,
        exc_ptr, exc_atom, exc_qq, exc_sigma, exc_eps).  opts: the ten fields of grappa_relax_opts by name, all of them.
        -> xyz_out (N,C,3), energy / gmax (B,C) float32, steps / status (B,C) int32; term_energy (6,B,C) and grad (N,C,3) or None.
        status: 0 = max_steps reached, 1 = converged, 2 = non-finite gradient, 3 = above relax_max_atoms() (nothing else written).
        atom_counts_host: atoms per molecule as the caller knows them on the host; with it a molecule above the limit raises here,
        before the launch and without a device sync (without it such a molecule comes back with status 3).
        restraints: a `grappa_amd.restraints.RestraintBatch` on xyz's device (None: the call above, unchanged) -- the frozen atoms,
        tethers and dihedral restraints of grappa_relax_fire_restr_f32, which minimises E + E_r, keeps energy / term_energy the force
        field's, writes restraint_energy (B,C) float32 (required with restraints) = E_r at xyz_out and dihedral_out (R,C) float32 or
        None = the restrained dihedrals there, and adds status 5 = the item's restraint tables are refused, nothing else written."""
        r = restraints
        if r is not None:
            from .restraints import RestraintBatch
            if not isinstance(r, RestraintBatch):
                raise TypeError(f"relax_fire: restraints must be a RestraintBatch or None, got {type(r).__name__}")
        elif restraint_energy is not None or dihedral_out is not None:
            raise ValueError("relax_fire: restraint_energy and dihedral_out need restraints")
        _xyz3(xyz, "relax_fire")
        dev = xyz.device
        d = self._mm_desc(plan, xyz, ks, eqs, n_per, offset_torsion)
        _relax_outputs("relax_fire", xyz, d.B, xyz_out, energy, gmax, steps, status, term_energy, grad)
        if xyz_out.data_ptr() == xyz.data_ptr() and xyz.numel():
            raise ValueError("relax_fire: xyz_out must not be the start coordinates")
        if atom_counts_host is not None:
            _atom_counts(atom_counts_host, d.N, d.B, "relax_fire", self.relax_max_atoms())
        if r is not None:
            R = int(r.dih_atoms.shape[0])
            _tensors(dev, ((r.dih_molptr, "dih_molptr", _I32), (r.dih_atoms, "dih_atoms", _I32), (r.dih_k, "dih_k", _F32), (r.dih_target, "dih_target", _F32),
                           (r.frozen, "frozen", _I32), (r.pos_k, "pos_k", _F32), (restraint_energy, "restraint_energy", _F32),
                           (dihedral_out, "dihedral_out", _F32)), ("frozen", "pos_k", "dihedral_out"))
            if r.dih_molptr.numel() != d.B + 1 or r.dih_atoms.shape != (R, 4) or r.dih_k.numel() != R or r.dih_target.numel() != R * d.C \
                    or any(t is not None and t.numel() != d.N for t in (r.frozen, r.pos_k)):
                raise ValueError(f"relax_fire: expected dih_molptr ({d.B + 1},), dih_atoms (R,4), dih_k (R,), dih_target (R,{d.C}), frozen / pos_k ({d.N},)")
            if restraint_energy.numel() != d.B * d.C or (dihedral_out is not None and dihedral_out.numel() != R * d.C):
                raise ValueError(f"relax_fire: expected restraint_energy (B,C), dihedral_out ({R},{d.C})")
        nd = _nb_tables_desc(nb, d.N, d.C, d.B, dev, "relax_fire")
        o = _opts_struct(_lib.RelaxOpts, opts, "relax_fire")
        head = (self._stream(), C.byref(d), C.byref(nd) if nd is not None else None, C.byref(o))
        outs = (xyz_out.data_ptr(), energy.data_ptr(), _ptr(term_energy), _ptr(grad), gmax.data_ptr(), steps.data_ptr(), status.data_ptr())
        if r is None:
            _chk(self.lib.grappa_relax_fire_f32(*head, *outs), "grappa_relax_fire_f32")
            return
        rr = _lib.RelaxRestr(frozen=_ptr(r.frozen), pos_k=_ptr(r.pos_k), dih_molptr=r.dih_molptr.data_ptr() if R else None,
                             dih_atoms=r.dih_atoms.data_ptr() if R else None, dih_k=r.dih_k.data_ptr() if R else None,
                             dih_target=r.dih_target.data_ptr() if R else None, R=R)
        _chk(self.lib.grappa_relax_fire_restr_f32(*head, C.byref(rr), *outs, restraint_energy.data_ptr(), _ptr(dihedral_out)),
             "grappa_relax_fire_restr_f32")

    def _item_table(self, nb, counts, N, Cc, dev):
        """the work-item table of the stepwise paths: the nonbonded plan of these molecules for this C (it is about atoms: it also serves
        nb = None), reused from nb's cache of plans where nb keeps one"""
        cache = getattr(nb, "_plans", None) if nb is not None else None
        table = cache.get(Cc) if isinstance(cache, dict) else None
        if table is None or table[0] is None or table[0].device != dev:
            molptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(counts, dtype=torch.int64).cumsum(0)]).to(torch.int32)
            table = self.nonbonded_plan(molptr, N, Cc, dev)
            if isinstance(cache, dict) and nb.charge.device == dev:
                cache[Cc] = table
        return table

    def relax_steps(self, plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, xyz_out, energy, gmax, steps, status, term_energy=None, grad=None,
                    atom_counts_host=None, check_every: int = 32, workspace=None, cutoff=None) -> None:
        """the stepwise FIRE minimiser for molecules of any size (include/grappa_hip.h grappa_relax_steps_*_f32): the loop, the
        arguments and the outputs of `relax_fire`, but a molecule spans many workgroups, the state lives in device memory and a step
        is four launches.  atom_counts_host (required): atoms per molecule on the host; the work-item table is the nonbonded plan
        built from it (reused from nb's cache of plans where nb keeps one).  check_every: steps enqueued between two looks at the
        device's count of running items.  The host SYNCS with the device once per chunk (one `.item()`), never per step; the loop
        ends when no item runs or max_steps steps are enqueued.  Status 3 does not occur.  workspace: a uint8 tensor of at least
        `grappa_relax_steps_workspace_bytes` to use instead of the backend's own.
        cutoff: a `grappa_amd.nonbonded.Cutoff` or a distance (None: all pairs, the calls above, unchanged) -- the nonbonded force and
        energy of grappa_relax_steps_*_cut_f32: `nonbonded(..., cutoff=)`'s; it needs nb; the workspace is then
        `grappa_relax_steps_cut_workspace_bytes`; a step stays four launches."""
        self._relax_steps("relax_steps", plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, xyz_out, energy, gmax, steps, status, term_energy, grad,
                          atom_counts_host, check_every, workspace, cutoff)

    def relax_steps_gb(self, plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, xyz_out, energy, gmax, steps, status, term_energy=None, grad=None,
                       atom_counts_host=None, check_every: int = 32, workspace=None, gb=None, solvent="obc2", esolv=None) -> None:
        """`relax_steps` in GB/SA implicit solvent (include/grappa_hip.h grappa_relax_steps_*_gb_f32): its arguments without the cutoff
        (GB under a cutoff is not implemented) plus gb, a `grappa_amd.solvent.GBBatch` on xyz's device holding the batch's molecules in
        order, and solvent, a model name or an `ImplicitSolvent`.  nb is required: it carries the charges.  The loop minimises the
        energy with the solvent term: energy includes it, esolv (B,C) float32 or None -> the solvent term alone, term_energy is then
        (8,B,C) with the polar and the surface-area term in rows 6 and 7, and grad is the total gradient.  A step is seven launches;
        the workspace is `grappa_relax_steps_gb_workspace_bytes`.  The same chunked loop: one `.item()` per check_every steps."""
        from .solvent import GBBatch, as_implicit_solvent
        sv = as_implicit_solvent(solvent)
        if sv is None or not isinstance(gb, GBBatch):
            raise TypeError(f"relax_steps_gb: gb must be a GBBatch and solvent a model, got {type(gb).__name__}, {solvent!r}")
        if sv.cutoff is not None:
            raise ValueError("relax_steps_gb: the implicit solvent's cutoff serves the energy entry and the stepwise dynamics: the minimiser does not run under it")
        if nb is None:
            raise ValueError("relax_steps_gb: the implicit solvent needs the nonbonded tables (nb): they carry the charges")
        gb.check_offset(sv.offset)
        self._relax_steps("relax_steps_gb", plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, xyz_out, energy, gmax, steps, status, term_energy,
                          grad, atom_counts_host, check_every, workspace, None, gb=gb, solvent=sv, esolv=esolv)

    def _relax_steps(self, who, plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, xyz_out, energy, gmax, steps, status, term_energy, grad,
                     atom_counts_host, check_every, workspace, cutoff, gb=None, solvent=None, esolv=None):
        """init, the run calls and finish of one stepwise minimisation: the plain calls, the _cut_ calls with a cutoff, the _gb_ calls
        with an implicit solvent"""
        _xyz3(xyz, who)
        if isinstance(check_every, bool) or int(check_every) != check_every or check_every < 1:
            raise ValueError(f"{who}: check_every must be an integer >= 1, got {check_every}")
        check_every = int(check_every)
        dev = xyz.device
        d = self._mm_desc(plan, xyz, ks, eqs, n_per, offset_torsion)
        N, Cc, B = d.N, d.C, d.B
        if gb is not None and term_energy is not None:          # (rows 6 and 7: the solvent's terms)
            _tensors(dev, ((term_energy, "term_energy", _F32),))
            if term_energy.numel() != 8 * B * Cc:
                raise ValueError(f"{who}: expected term_energy (8,B,C)")
            _relax_outputs(who, xyz, B, xyz_out, energy, gmax, steps, status, term_energy.reshape(-1)[:6 * B * Cc], grad)
        else:
            _relax_outputs(who, xyz, B, xyz_out, energy, gmax, steps, status, term_energy, grad)
        if atom_counts_host is None:
            raise ValueError(f"{who}: atom_counts_host is required (the work-item table is built from it)")
        counts = _atom_counts(atom_counts_host, N, B, who)
        nd = _nb_tables_desc(nb, N, Cc, B, dev, who)
        o = _opts_struct(_lib.RelaxOpts, opts, who)
        cut = None
        if cutoff is not None:
            if nb is None:
                raise ValueError(f"{who}: a cutoff needs the nonbonded tables (nb)")
            cut = _cut_struct(cutoff, who)
        gbd = None
        if gb is not None:
            _tensors(dev, ((gb.radius, "gb.radius", _F32), (gb.scale, "gb.scale", _F32), (esolv, "esolv", _F32)), ("esolv",))
            if gb.radius.numel() != N or gb.scale.numel() != N or (esolv is not None and esolv.numel() != B * Cc):
                raise ValueError(f"{who}: expected gb.radius / gb.scale ({N},), esolv (B,C)")
            gbd = _lib.GbDesc(radius=gb.radius.data_ptr(), scale=gb.scale.data_ptr(), **solvent.as_opts())
        if N == 0 or Cc == 0 or B == 0:
            return
        table = self._item_table(nb, counts, N, Cc, dev)
        table_dev, n_items, n_blocks, _ = table
        if gbd is not None:
            need = int(self.lib.grappa_relax_steps_gb_workspace_bytes(N, Cc, B, n_blocks))
        else:
            need = int((self.lib.grappa_relax_steps_workspace_bytes if cut is None else self.lib.grappa_relax_steps_cut_workspace_bytes)(N, Cc, B, n_blocks))
        if workspace is None:
            workspace = self._workspace(need, dev, who)
        else:
            _flat(workspace, "workspace", dev, torch.uint8)
        n_running = torch.zeros(1, dtype=torch.int32, device=dev)
        st, ndp = self._stream(), (C.byref(nd) if nd is not None else None)
        if gbd is not None:
            head, sfx = (st, C.byref(d), ndp, None, C.byref(gbd), C.byref(o)), "_gb_f32"
        elif cut is None:
            head, sfx = (st, C.byref(d), ndp, C.byref(o)), "_f32"
        else:
            head, sfx = (st, C.byref(d), ndp, C.byref(cut), C.byref(o)), "_cut_f32"
        init, run, finish = (getattr(self.lib, f"grappa_relax_steps_{n}{sfx}") for n in ("init", "run", "finish"))
        common = (*head, table_dev.data_ptr(), n_items, n_blocks, workspace.data_ptr(), workspace.numel())
        _chk(init(*common, n_running.data_ptr()), f"grappa_relax_steps_init{sfx}")
        left = o.max_steps
        while left > 0:
            n = min(check_every, left)
            _chk(run(*common, n, n_running.data_ptr()), f"grappa_relax_steps_run{sfx}")
            left -= n
            if int(n_running.item()) <= 0:          # the one host sync per chunk
                break
        _chk(finish(*common, xyz_out.data_ptr(), energy.data_ptr(), _ptr(term_energy), _ptr(grad), gmax.data_ptr(), steps.data_ptr(),
                    status.data_ptr(), *((_ptr(esolv),) if gbd is not None else ())), f"grappa_relax_steps_finish{sfx}")

    # ------------------------------------------------------------------ dynamics
    def _md_call(self, who, plan, xyz, ks, eqs, n_per, offset_torsion, opts, mass, mol_key, vel_in, xyz_out, vel_out, epot, ekin, steps, status,
                 frames_xyz, frames_epot, frames_ekin):
        """the checks the two dynamics seams share -> (grappa_mm_desc, grappa_md_opts)"""
        _xyz3(xyz, who)
        dev = xyz.device
        d = self._mm_desc(plan, xyz, ks, eqs, n_per, offset_torsion)
        N, Cc, B = d.N, d.C, d.B
        o = _opts_struct(_lib.MdOpts, opts, who)
        F = o.n_steps // o.save_every if o.save_every > 0 and o.n_steps > 0 else 0
        _tensors(dev, ((mass, "mass", _F32), (mol_key, "mol_key", _I64), (vel_in, "vel_in", _F32), (xyz_out, "xyz_out", _F32),
                       (vel_out, "vel_out", _F32), (epot, "epot", _F32), (ekin, "ekin", _F32), (steps, "steps", _I32), (status, "status", _I32),
                       (frames_xyz, "frames_xyz", _F32), (frames_epot, "frames_epot", _F32), (frames_ekin, "frames_ekin", _F32)),
                 ("vel_in", "frames_xyz", "frames_epot", "frames_ekin"))
        if mass.numel() != N or mol_key.numel() != B or any(t is not None and t.shape != xyz.shape for t in (vel_in, xyz_out, vel_out)) \
                or any(t.numel() != B * Cc for t in (epot, ekin, steps, status)) \
                or (frames_xyz is not None and frames_xyz.numel() != F * N * Cc * 3) \
                or any(t is not None and t.numel() != F * B * Cc for t in (frames_epot, frames_ekin)):
            raise ValueError(f"{who}: expected mass (N,), mol_key (B,), vel_in / xyz_out / vel_out (N,C,3), epot / ekin / steps / status "
                             f"(B,C), frames_xyz ({F},N,C,3), frames_epot / frames_ekin ({F},B,C)")
        if xyz.numel() and (xyz_out.data_ptr() == xyz.data_ptr() or (vel_in is not None and vel_out.data_ptr() == vel_in.data_ptr())):
            raise ValueError(f"{who}: xyz_out / vel_out must not be the start coordinates / velocities")
        return d, o

    @staticmethod
    def _md_cons(constraints, B, dev, constrain_start, who="md_langevin"):
        """grappa_md_cons from a ConstraintBatch on `dev`"""
        from .constraints import MAX_LEAVES, ConstraintBatch
        if not isinstance(constraints, ConstraintBatch):
            raise TypeError(f"{who}: constraints must be a ConstraintBatch or None, got {type(constraints).__name__}")
        ptr, atoms, dd = constraints.cluster_molptr, constraints.cluster_atoms, constraints.cluster_d
        _tensors(dev, ((ptr, "cluster_molptr", _I32), (atoms, "cluster_atoms", _I32), (dd, "cluster_d", _F32)))
        K = int(atoms.shape[0])
        if ptr.numel() != B + 1 or atoms.shape != (K, MAX_LEAVES + 1) or dd.shape != (K, MAX_LEAVES):
            raise ValueError(f"{who}: expected cluster_molptr ({B + 1},), cluster_atoms (K,{MAX_LEAVES + 1}), cluster_d (K,{MAX_LEAVES})")
        return _lib.MdCons(cluster_molptr=ptr.data_ptr(), cluster_atoms=atoms.data_ptr() if K else None, cluster_d=dd.data_ptr() if K else None,
                           K=K, tolerance=float(constraints.tolerance), constrain_start=int(bool(constrain_start)))

    def md_langevin(self, plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, mass, mol_key, vel_in, xyz_out, vel_out, epot, ekin, steps, status,
                    frames_xyz=None, frames_epot=None, frames_ekin=None, atom_counts_host=None, constraints=None, constrain_start=True) -> None:
        """fused Langevin dynamics (include/grappa_hip.h grappa_md_langevin_f32): one launch runs opts["n_steps"] BAOAB steps of every
        (molecule, conformation) of the batch.  plan, xyz (N,C,3: the start), ks, eqs, n_per, offset_torsion, nb and atom_counts_host
        as for `relax_fire`.  opts: the seven fields of grappa_md_opts by name, all of them.  mass (N,) float32 in amu (0: a frozen
        atom); mol_key (B,) int64 holding the molecules' 64-bit keys bit for bit; vel_in (N,C,3) or None (velocities drawn at
        init_temperature).  -> xyz_out, vel_out (N,C,3), epot / ekin (B,C) float32, steps / status (B,C) int32 (status 0 = ran
        n_steps steps, 2 = non-finite gradient, 3 = above relax_max_atoms(), nothing else written); frames_xyz (F,N,C,3), frames_epot /
        frames_ekin (F,B,C) with F = n_steps // save_every, or None.
        constraints: a `grappa_amd.constraints.ConstraintBatch` on xyz's device (None: the call above, unchanged) -- the X-H bond
        constraints of grappa_md_langevin_cons_f32, which adds status 4 = a position constraint did not converge and 5 = the item's
        constraint tables are refused, nothing else written; constrain_start: True constrains the input first, False continues a run."""
        d, o = self._md_call("md_langevin", plan, xyz, ks, eqs, n_per, offset_torsion, opts, mass, mol_key, vel_in, xyz_out, vel_out, epot, ekin,
                             steps, status, frames_xyz, frames_epot, frames_ekin)
        dev, N, Cc, B = xyz.device, d.N, d.C, d.B
        if atom_counts_host is not None:
            _atom_counts(atom_counts_host, N, B, "md_langevin", self.relax_max_atoms())
        nd = _nb_tables_desc(nb, N, Cc, B, dev, "md_langevin")
        head = (self._stream(), C.byref(d), C.byref(nd) if nd is not None else None, C.byref(o))
        tail = (mass.data_ptr(), mol_key.data_ptr(), _ptr(vel_in), xyz_out.data_ptr(), vel_out.data_ptr(), epot.data_ptr(), ekin.data_ptr(),
                steps.data_ptr(), status.data_ptr(), _ptr(frames_xyz), _ptr(frames_epot), _ptr(frames_ekin))
        if constraints is not None:
            cons = self._md_cons(constraints, B, dev, constrain_start)
            _chk(self.lib.grappa_md_langevin_cons_f32(*head, C.byref(cons), *tail), "grappa_md_langevin_cons_f32")
            return
        _chk(self.lib.grappa_md_langevin_f32(*head, *tail), "grappa_md_langevin_f32")

    def md_steps(self, plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, mass, mol_key, vel_in, xyz_out, vel_out, epot, ekin, steps, status,
                 frames_xyz=None, frames_epot=None, frames_ekin=None, atom_counts_host=None, steps_per_call: int = 1000, workspace=None,
                 cutoff=None) -> None:
        """stepwise Langevin dynamics for molecules of any size (include/grappa_hip.h grappa_md_steps_*_f32): the loop, the arguments
        and the outputs of `md_langevin`, but a molecule spans many workgroups, the state lives in device memory and a step is two
        launches.  opts: the whole run's (n_steps its total).  atom_counts_host (required): atoms per molecule on the host; the
        work-item table is the nonbonded plan built from it (reused from nb's cache of plans where nb keeps one).  steps_per_call:
        steps enqueued per run call at most (rounded down to a multiple of save_every when frames are written); the result does not
        depend on it.  There is NO device sync anywhere in it: init, the run calls and finish are only enqueued.  Status 3 does not
        occur.  workspace: a uint8 tensor of at least `grappa_md_steps_workspace_bytes` to use instead of the backend's own.
        cutoff: a `grappa_amd.nonbonded.Cutoff` or a distance (None: all pairs, the calls above, unchanged) -- the nonbonded force and
        energies of grappa_md_steps_*_cut_f32: `nonbonded(..., cutoff=)`'s; it needs nb; the workspace is then
        `grappa_md_steps_cut_workspace_bytes`; a step stays two launches."""
        self._md_steps("md_steps", plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, mass, mol_key, vel_in, xyz_out, vel_out, epot, ekin, steps,
                       status, frames_xyz, frames_epot, frames_ekin, atom_counts_host, steps_per_call, workspace, cutoff, None, True)

    def md_steps_cons(self, plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, mass, mol_key, vel_in, xyz_out, vel_out, epot, ekin, steps, status,
                      frames_xyz=None, frames_epot=None, frames_ekin=None, atom_counts_host=None, steps_per_call: int = 1000, workspace=None,
                      cutoff=None, constraints=None, constrain_start=True) -> None:
        """`md_steps` with X-H bond constraints (include/grappa_hip.h grappa_md_steps_*_cons_f32): its arguments plus constraints, a
        `grappa_amd.constraints.ConstraintBatch` on xyz's device with any number of clusters per molecule (None: `md_steps` itself), and
        constrain_start (True constrains the input first, False continues a run; init alone reads it).  The loop is `md_langevin`'s with
        constraints, with its statuses 4 and 5; a step is three launches, four under a cutoff; the workspace is
        `grappa_md_steps_cons_workspace_bytes`.  Like `md_steps` it has NO device sync."""
        self._md_steps("md_steps_cons", plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, mass, mol_key, vel_in, xyz_out, vel_out, epot, ekin,
                       steps, status, frames_xyz, frames_epot, frames_ekin, atom_counts_host, steps_per_call, workspace, cutoff, constraints,
                       constrain_start)

    def md_steps_gb(self, plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, mass, mol_key, vel_in, xyz_out, vel_out, epot, ekin, steps, status,
                    frames_xyz=None, frames_epot=None, frames_ekin=None, atom_counts_host=None, steps_per_call: int = 1000, workspace=None,
                    constraints=None, constrain_start=True, gb=None, solvent="obc2", esolv=None, frames_esolv=None, cutoff=None) -> None:
        """`md_steps_cons` in GB/SA implicit solvent (include/grappa_hip.h grappa_md_steps_*_gb_f32): its arguments (the cutoff last, see
        below) plus gb, a `grappa_amd.solvent.GBBatch` on xyz's device holding the batch's molecules in
        order, and solvent, a model name or an `ImplicitSolvent`.  nb is required: it carries the charges.  constraints may be None.
        epot then includes the solvent term; esolv (B,C) and frames_esolv (F,B,C) float32 or None -> the solvent term alone.  A step is
        five launches, six with constraints; the workspace is `grappa_md_steps_gb_workspace_bytes`.  Like `md_steps` it has NO device
        sync.
        A solvent with a cutoff of its own (`ImplicitSolvent(cutoff=)`, `solvent.cut_opts()`) runs the grappa_md_steps_*_gbcut_f32
        calls: the three passes under that cutoff, far tiles skipped.  cutoff: the NONBONDED cutoff (a `Cutoff` or a distance), taken
        only beside a solvent that has a cutoff; one set of boxes serves both."""
        from .solvent import GBBatch, as_implicit_solvent
        sv = as_implicit_solvent(solvent)
        if sv is None or not isinstance(gb, GBBatch):
            raise TypeError(f"md_steps_gb: gb must be a GBBatch and solvent a model, got {type(gb).__name__}, {solvent!r}")
        if cutoff is not None and sv.cutoff is None:
            raise ValueError("md_steps_gb: a nonbonded cutoff beside the implicit solvent needs a solvent with a cutoff of its own "
                             "(ImplicitSolvent(cutoff=))")
        if nb is None:
            raise ValueError("md_steps_gb: the implicit solvent needs the nonbonded tables (nb): they carry the charges")
        gb.check_offset(sv.offset)
        self._md_steps("md_steps_gb", plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, mass, mol_key, vel_in, xyz_out, vel_out, epot, ekin,
                       steps, status, frames_xyz, frames_epot, frames_ekin, atom_counts_host, steps_per_call, workspace, cutoff, constraints,
                       constrain_start, gb=gb, solvent=sv, esolv=esolv, frames_esolv=frames_esolv)

    def md_steps_restr(self, plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, mass, mol_key, vel_in, xyz_out, vel_out, epot, ekin, steps,
                       status, frames_xyz=None, frames_epot=None, frames_ekin=None, atom_counts_host=None, steps_per_call: int = 1000,
                       workspace=None, constraints=None, constrain_start=True, gb=None, solvent=None, esolv=None, frames_esolv=None, cutoff=None,
                       restraints=None, restraint_reference=None, restraint_energy=None, dihedral_out=None, frames_restraint_energy=None,
                       frames_dihedrals=None) -> None:
        """the stepwise dynamics with restraints (include/grappa_hip.h grappa_md_steps_*_restr_f32): `md_steps_gb`'s arguments with gb /
        solvent optional (None: vacuum; constraints and cutoff as `md_steps_cons` takes them), plus restraints, a
        `grappa_amd.restraints.RestraintBatch` on xyz's device (tethers and dihedral restraints; `frozen` must be None: the caller folds
        frozen atoms into the masses), restraint_reference (N,C,3) float32 or None (the tethers' reference; None: xyz -- a continued run
        must pass the original reference), restraint_energy (B,C) float32 (required) -> E_r at xyz_out, dihedral_out (R,C) or None -> the
        restrained dihedrals there, frames_restraint_energy (F,B,C) / frames_dihedrals (F,R,C) or None -> the same per frame.  epot stays
        the force field's (plus the solvent's).  Status 5: the item's restraint (or constraint) tables were refused.  A step has the
        launches of the same call without restraints.  Like `md_steps` it has NO device sync."""
        from .restraints import RestraintBatch
        from .solvent import GBBatch, as_implicit_solvent
        who = "md_steps_restr"
        if not isinstance(restraints, RestraintBatch):
            raise TypeError(f"{who}: restraints must be a RestraintBatch, got {type(restraints).__name__}")
        if restraints.frozen is not None:
            raise ValueError(f"{who}: frozen atoms are not sent down: fold them into the masses (mass 0) and pass restraints without `frozen`")
        if restraint_energy is None:
            raise ValueError(f"{who}: restraint_energy (B,C) is required")
        sv = as_implicit_solvent(solvent) if gb is not None or solvent is not None else None
        if (sv is None) != (gb is None) or (gb is not None and not isinstance(gb, GBBatch)):
            raise TypeError(f"{who}: gb (a GBBatch) and solvent (a model) go together, got {type(gb).__name__}, {solvent!r}")
        if sv is not None:
            if cutoff is not None and sv.cutoff is None:
                raise ValueError(f"{who}: a nonbonded cutoff beside the implicit solvent needs a solvent with a cutoff of its own "
                                 "(ImplicitSolvent(cutoff=))")
            if nb is None:
                raise ValueError(f"{who}: the implicit solvent needs the nonbonded tables (nb): they carry the charges")
            gb.check_offset(sv.offset)
        self._md_steps(who, plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, mass, mol_key, vel_in, xyz_out, vel_out, epot, ekin, steps,
                       status, frames_xyz, frames_epot, frames_ekin, atom_counts_host, steps_per_call, workspace, cutoff, constraints,
                       constrain_start, gb=gb, solvent=sv, esolv=esolv, frames_esolv=frames_esolv,
                       restr=(restraints, restraint_reference, restraint_energy, dihedral_out, frames_restraint_energy, frames_dihedrals))

    def md_steps_remd(self, plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, mass, mol_key, vel_in, xyz_out, vel_out, epot, ekin, steps,
                      status, frames_xyz=None, frames_epot=None, frames_ekin=None, atom_counts_host=None, steps_per_call: int = 1000,
                      workspace=None, constraints=None, constrain_start=True, gb=None, solvent=None, esolv=None, frames_esolv=None, cutoff=None,
                      restraints=None, restraint_reference=None, restraint_energy=None, dihedral_out=None, frames_restraint_energy=None,
                      frames_dihedrals=None, temperatures=None, slots=None, exchange_every: int = 0, init_at_ladder: bool = True,
                      slots_out=None, exchange_slots=None, exchange_epot=None, exchange_erestr=None) -> None:
        """the stepwise dynamics on a temperature ladder, with or without replica exchange (include/grappa_hip.h grappa_md_remd_*_f32):
        `md_steps_restr`'s arguments with restraints optional too, plus temperatures (C,) float32 on xyz's device (kelvin; slot s of the
        ladder), slots (B,C) int32 or None (the slot every replica starts in, a permutation per molecule; None: slot c), exchange_every
        (K; 0: a ladder without exchanges), init_at_ladder (velocities that are drawn: at the replica's slot temperature, else at
        init_temperature), slots_out (B,C) int32 (required) -> the slots at the end, and the logs of the run's X = n_steps // K attempts,
        each (X,B,C) or None: exchange_slots int32 (the slots after the attempt), exchange_epot / exchange_erestr float32 (the energies the
        decision read).  With K > 0 and a log, opts["first_step"] must be a multiple of K.  temperatures None: no ladder, the _restr_ family's
        calls through the ladder's entries (slots_out is then c).  Status 5: also a slots row that is no permutation or a
        temperature the ladder refuses.  run calls are cut at multiples of both save_every and K.  NO device sync."""
        from .restraints import RestraintBatch
        from .solvent import GBBatch, as_implicit_solvent
        who = "md_steps_remd"
        restr = None
        if restraints is not None:
            if not isinstance(restraints, RestraintBatch):
                raise TypeError(f"{who}: restraints must be a RestraintBatch or None, got {type(restraints).__name__}")
            if restraints.frozen is not None:
                raise ValueError(f"{who}: frozen atoms are not sent down: fold them into the masses (mass 0) and pass restraints without `frozen`")
            if restraint_energy is None:
                raise ValueError(f"{who}: restraint_energy (B,C) is required with restraints")
            restr = (restraints, restraint_reference, restraint_energy, dihedral_out, frames_restraint_energy, frames_dihedrals)
        sv = as_implicit_solvent(solvent) if gb is not None or solvent is not None else None
        if (sv is None) != (gb is None) or (gb is not None and not isinstance(gb, GBBatch)):
            raise TypeError(f"{who}: gb (a GBBatch) and solvent (a model) go together, got {type(gb).__name__}, {solvent!r}")
        if sv is not None:
            if cutoff is not None and sv.cutoff is None:
                raise ValueError(f"{who}: a nonbonded cutoff beside the implicit solvent needs a solvent with a cutoff of its own "
                                 "(ImplicitSolvent(cutoff=))")
            if nb is None:
                raise ValueError(f"{who}: the implicit solvent needs the nonbonded tables (nb): they carry the charges")
            gb.check_offset(sv.offset)
        if isinstance(exchange_every, bool) or int(exchange_every) != exchange_every or exchange_every < 0:
            raise ValueError(f"{who}: exchange_every must be an integer >= 0, got {exchange_every!r}")
        self._md_steps(who, plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, mass, mol_key, vel_in, xyz_out, vel_out, epot, ekin, steps,
                       status, frames_xyz, frames_epot, frames_ekin, atom_counts_host, steps_per_call, workspace, cutoff, constraints,
                       constrain_start, gb=gb, solvent=sv, esolv=esolv, frames_esolv=frames_esolv, restr=restr,
                       remd=(temperatures, slots, int(exchange_every), bool(init_at_ladder), slots_out, exchange_slots, exchange_epot,
                             exchange_erestr))

    # The seven families of entries, narrowest first.  A family takes the optional structs of the one before it plus one
    # (a family IS the widest call with the others NULL), so a row says only which: the structs of its head behind (stream, mm, nb), the
    # arguments of its workspace_bytes behind n_blocks, and how many of the optional outputs -- (frames_)esolv, (frames_)erestr, phi --
    # its run and finish take behind the required ones.
    _MD_STEPS_FAMILIES = {
        "":       (("o",), (), 0),
        "_cut":   (("cut", "o"), (), 0),
        "_cons":  (("cut", "o", "cons"), ("K", "with_cut"), 0),
        "_gb":    (("cut", "o", "cons", "gb"), ("K",), 1),
        "_gbcut": (("cut", "o", "cons", "gb", "gbcut"), ("K",), 1),
        "_restr": (("cut", "o", "cons", "gb", "gbcut", "restr"), ("K", "with_cut", "with_gb", "with_gbcut"), 3),
        # (the ladder's entries are named grappa_md_remd_*, not grappa_md_steps_*_remd_*: `_md_steps_entry`; behind the optional outputs
        # its run takes the three logs and its finish slots_out)
        "_remd":  (("cut", "o", "cons", "gb", "gbcut", "restr", "remd"), ("K", "with_cut", "with_gb", "with_gbcut", "with_restr"), 3),
    }

    def _md_steps_entry(self, fam, which):
        """the entry `which` (workspace_bytes, init, run, finish) of a family -> (function, name)"""
        if fam == "_remd":
            name = f"grappa_md_remd_{which}" + ("" if which == "workspace_bytes" else "_f32")
        else:
            name = f"grappa_md_steps{fam}_workspace_bytes" if which == "workspace_bytes" else f"grappa_md_steps_{which}{fam}_f32"
        return getattr(self.lib, name), name

    def _md_steps(self, who, plan, xyz, ks, eqs, n_per, offset_torsion, nb, opts, mass, mol_key, vel_in, xyz_out, vel_out, epot, ekin, steps, status,
                  frames_xyz, frames_epot, frames_ekin, atom_counts_host, steps_per_call, workspace, cutoff, constraints, constrain_start,
                  gb=None, solvent=None, esolv=None, frames_esolv=None, restr=None, remd=None):
        """init, the run calls and finish of one stepwise run, through the narrowest family of entries that expresses it: the widest
        option the run has (a ladder, restraints, the solvent's cutoff, the solvent, constraints, the nonbonded cutoff, none) names the family,
        and `_MD_STEPS_FAMILIES` says what that family's calls take; every option the run lacks goes down as NULL"""
        if isinstance(steps_per_call, bool) or int(steps_per_call) != steps_per_call or steps_per_call < 1:
            raise ValueError(f"{who}: steps_per_call must be an integer >= 1, got {steps_per_call}")
        d, o = self._md_call(who, plan, xyz, ks, eqs, n_per, offset_torsion, opts, mass, mol_key, vel_in, xyz_out, vel_out, epot, ekin,
                             steps, status, frames_xyz, frames_epot, frames_ekin)
        dev, N, Cc, B = xyz.device, d.N, d.C, d.B
        if atom_counts_host is None:
            raise ValueError(f"{who}: atom_counts_host is required (the work-item table is built from it)")
        counts = _atom_counts(atom_counts_host, N, B, who)
        nd = _nb_tables_desc(nb, N, Cc, B, dev, who)
        cut = None
        if cutoff is not None:
            if nb is None:
                raise ValueError(f"{who}: a cutoff needs the nonbonded tables (nb)")
            cut = _cut_struct(cutoff, who)
        cons = self._md_cons(constraints, B, dev, constrain_start, who) if constraints is not None else None
        F = o.n_steps // o.save_every if o.save_every > 0 and o.n_steps > 0 else 0          # frames of the run
        gbd = gbc = None
        if gb is not None:
            _tensors(dev, ((gb.radius, "gb.radius", _F32), (gb.scale, "gb.scale", _F32), (esolv, "esolv", _F32), (frames_esolv, "frames_esolv", _F32)),
                     ("esolv", "frames_esolv"))
            if gb.radius.numel() != N or gb.scale.numel() != N or (esolv is not None and esolv.numel() != B * Cc) \
                    or (frames_esolv is not None and frames_esolv.numel() != F * B * Cc):
                raise ValueError(f"{who}: expected gb.radius / gb.scale ({N},), esolv (B,C), frames_esolv ({F},B,C)")
            gbd = _lib.GbDesc(radius=gb.radius.data_ptr(), scale=gb.scale.data_ptr(), **solvent.as_opts())
            gco = solvent.cut_opts()
            gbc = None if gco is None else _opts_struct(_lib.GbCut, gco, f"{who}: the solvent's cutoff")
        rr = er = phi = fer = fphi = None
        if restr is not None:
            r, ref, er, phi, fer, fphi = restr
            R = int(r.dih_atoms.shape[0])
            _tensors(dev, ((r.dih_molptr, "dih_molptr", _I32), (r.dih_atoms, "dih_atoms", _I32), (r.dih_k, "dih_k", _F32), (r.dih_target, "dih_target", _F32),
                           (r.pos_k, "pos_k", _F32), (ref, "restraint_reference", _F32), (er, "restraint_energy", _F32), (phi, "dihedral_out", _F32),
                           (fer, "frames_restraint_energy", _F32), (fphi, "frames_dihedrals", _F32)),
                     ("pos_k", "restraint_reference", "dihedral_out", "frames_restraint_energy", "frames_dihedrals"))
            if r.dih_molptr.numel() != B + 1 or r.dih_atoms.shape != (R, 4) or r.dih_k.numel() != R or r.dih_target.numel() != R * Cc \
                    or (r.pos_k is not None and r.pos_k.numel() != N) or (ref is not None and ref.shape != xyz.shape):
                raise ValueError(f"{who}: expected dih_molptr ({B + 1},), dih_atoms (R,4), dih_k (R,), dih_target (R,{Cc}), pos_k ({N},), "
                                 f"restraint_reference {tuple(xyz.shape)}")
            if er.numel() != B * Cc or (phi is not None and phi.numel() != R * Cc) or (fer is not None and fer.numel() != F * B * Cc) \
                    or (fphi is not None and fphi.numel() != F * R * Cc):
                raise ValueError(f"{who}: expected restraint_energy (B,C), dihedral_out ({R},{Cc}), frames_restraint_energy ({F},B,C), "
                                 f"frames_dihedrals ({F},{R},{Cc})")
            if R * Cc >= 2 ** 31:
                raise ValueError(f"{who}: R * C must stay below 2^31, got {R} * {Cc}")
            if ref is not None and r.pos_k is None:
                ref = None          # (no tether reads it)
            rr = _lib.MdRestr(pos_k=_ptr(r.pos_k), pos_ref=_ptr(ref), dih_molptr=r.dih_molptr.data_ptr() if R else None,
                              dih_atoms=r.dih_atoms.data_ptr() if R else None, dih_k=r.dih_k.data_ptr() if R else None,
                              dih_target=r.dih_target.data_ptr() if R else None, R=R)
        xr, K, slots_out, logs = None, 0, None, (None, None, None)
        if remd is not None:
            temps, slots_in, K, at_ladder, slots_out, *logs = remd
            X = o.n_steps // K if K > 0 else 0          # attempts of the run
            _tensors(dev, ((temps, "temperatures", _F32), (slots_in, "slots", _I32), (slots_out, "slots_out", _I32), (logs[0], "exchange_slots", _I32),
                           (logs[1], "exchange_epot", _F32), (logs[2], "exchange_erestr", _F32)),
                     ("temperatures", "slots", "exchange_slots", "exchange_epot", "exchange_erestr"))
            if temps is None and (slots_in is not None or K != 0):
                raise ValueError(f"{who}: slots and exchange_every need temperatures")
            if (temps is not None and temps.numel() != Cc) or (slots_in is not None and slots_in.numel() != B * Cc) or slots_out.numel() != B * Cc \
                    or any(t is not None and t.numel() != X * B * Cc for t in logs):
                raise ValueError(f"{who}: expected temperatures ({Cc},), slots / slots_out (B,C), the exchange logs ({X},B,C)")
            if X == 0:
                logs = (None, None, None)
            if temps is not None:          # (None: no ladder -- the entries then make the _restr_ family's calls and write slots_out as c)
                xr = _lib.MdRemd(temperatures=temps.data_ptr(), slots_in=_ptr(slots_in), exchange_every=K, init_at_ladder=int(at_ladder))
            if er is None:          # (the finish owes its caller erestr whatever the plan holds)
                er = torch.empty(B * Cc, dtype=_F32, device=dev)
        if N == 0 or Cc == 0 or B == 0:
            return
        table_dev, n_items, n_blocks, _ = self._item_table(nb, counts, N, Cc, dev)
        have = {"cut": cut, "o": o, "cons": cons, "gb": gbd, "gbcut": gbc, "restr": rr, "remd": xr}
        fam = "_remd" if remd is not None else next((f"_{k}" for k in ("restr", "gbcut", "gb", "cons", "cut") if have[k] is not None), "")
        head_names, size_names, n_opt = self._MD_STEPS_FAMILIES[fam]
        sizes = {"K": cons.K if cons is not None else 0, "with_cut": int(cut is not None), "with_gb": int(gbd is not None),
                 "with_gbcut": int(gbc is not None), "with_restr": int(rr is not None)}
        need = int(self._md_steps_entry(fam, "workspace_bytes")[0](N, Cc, B, n_blocks, *(sizes[k] for k in size_names)))
        if workspace is None:
            workspace = self._workspace(need, dev, who)
        else:
            _flat(workspace, "workspace", dev, torch.uint8)
        (init, init_name), (run, run_name), (finish, finish_name) = (self._md_steps_entry(fam, n) for n in ("init", "run", "finish"))
        head = (self._stream(), C.byref(d), C.byref(nd) if nd is not None else None,
                *(C.byref(have[k]) if have[k] is not None else None for k in head_names))
        tail = (table_dev.data_ptr(), n_items, n_blocks, workspace.data_ptr(), workspace.numel())
        _chk(init(*head, mass.data_ptr(), mol_key.data_ptr(), _ptr(vel_in), *tail), init_name)
        frame_outs = (frames_xyz, frames_epot, frames_ekin, frames_esolv, fer, fphi)
        every = o.save_every if F > 0 and any(t is not None for t in frame_outs) else 0
        chunk = int(steps_per_call)
        align = math.lcm(every if every > 0 else 1, K if K > 0 else 1)          # a run call is cut where frames and attempts both allow
        if align > 1:
            chunk = max(chunk // align, 1) * align
        done = 0
        while done < o.n_steps:
            n = min(chunk, o.n_steps - done)
            f0 = done // every if every > 0 else 0
            fr = [None if t is None or every == 0 else t.data_ptr() + f0 * (t.numel() // F) * t.element_size() for t in frame_outs[:3 + n_opt]]
            if remd is not None:          # the rows of the logs of this call's attempts
                fr += [None if t is None else t.data_ptr() + (done // K) * B * Cc * t.element_size() for t in logs]
            _chk(run(*head, mass.data_ptr(), mol_key.data_ptr(), *tail, done, n, *fr), run_name)
            done += n
        _chk(finish(*head, *tail, xyz_out.data_ptr(), vel_out.data_ptr(), epot.data_ptr(), ekin.data_ptr(), steps.data_ptr(), status.data_ptr(),
                    *(_ptr(t) for t in (esolv, er, phi)[:n_opt]), *((slots_out.data_ptr(),) if remd is not None else ())), finish_name)

    def md_noise(self, mol_key, atom_molptr, C_, step: int, purpose: int, out) -> None:
        """the normal deviates `md_langevin` draws for one step (include/grappa_hip.h grappa_md_noise_f32): mol_key (B,) int64,
        atom_molptr (B+1,) int32, C_ conformations, step = the global step index, purpose 0 (thermostat) or 1 (start velocities)
        -> out (N, C_, 3) float32"""
        _tensors(out.device, ((mol_key, "mol_key", _I64), (atom_molptr, "atom_molptr", _I32), (out, "out", _F32)), where="")
        B = mol_key.numel()
        if atom_molptr.numel() != B + 1 or out.dim() != 3 or out.shape[1] != C_ or out.shape[2] != 3:
            raise ValueError("md_noise: expected mol_key (B,), atom_molptr (B+1,), out (N,C,3)")
        if not (0 <= int(step) < 2 ** 32 and 0 <= int(purpose) < 2 ** 32):
            raise ValueError(f"md_noise: step and purpose must lie in [0, 2^32), got {step}, {purpose}")
        _chk(self.lib.grappa_md_noise_f32(self._stream(), mol_key.data_ptr(), atom_molptr.data_ptr(), out.shape[0], int(C_), B, int(step),
                                          int(purpose), out.data_ptr()), "grappa_md_noise_f32")
