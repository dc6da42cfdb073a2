"""The inputs and restatements of the temperature-ladder tests (tests/test_host_md_remd.py on the CPU, tests/test_gpu_md_remd.py): the
decision and the swap of an exchange attempt in numpy float64 (`exchange_ref`, `attempt_ref`), Philox from md_refs.philox, and the
ladder run composed from md_refs.baoab_ref (`ladder_ref`): one call per conformation at its slot temperature, selecting that
conformation, segments chained through velocities=, first_step= and the swap applied on the host.

The cases are those of tests/md_steps_refs.py.  The ladders are a few tens of kelvin apart around 300 K: with the energies these
molecules hold, D = (beta_s - beta_{s+1}) (U_lo - U_hi) then lies within a few units of 0, so that a run decides both ways."""
import functools

import numpy as np
import torch

import md_refs as md
import md_steps_refs as ms

KB = md.KB
RUNNING = 0          # `status` of exchange_ref: 0 runs, anything else has stopped


def ladder(C, t0=280.0, step=25.0) -> np.ndarray:
    """(C,) float32 kelvin: t0, t0 + step, .."""
    return (t0 + step * np.arange(C)).astype(np.float32)


# the exchange cases: name -> (ladder, friction, seeds are the case's own).  EXCHANGE_K: the K each runs with, over EXCHANGE_STEPS steps
EXCHANGE_STEPS = 40
EXCHANGE_K = (1, 4)
EXCHANGE_CASES = {"s65_C3": ladder(3, 250.0, 60.0), "s9_65_C17": ladder(17, 240.0, 12.0), ms.MIXED: ladder(3, 250.0, 60.0), "s17_C2": ladder(2, 270.0, 60.0)}
FRICTION = 20.0


def beta(T):
    return 1.0 / (KB * np.float64(np.float32(T)))


def uniform(key, s, g, philox=None):
    """u of the pair whose lower slot is s, behind global step g: ((double)w0 + 0.5) 2^-32, w0 = word 0 of Philox(key, (s, 0, g, 2));
    philox(key, c0, c1, c2, c3) -> the four words (default: md_refs.philox; the GPU test passes the library's own generator)"""
    w0 = md.philox(np.uint64(key), s, 0, g, 2)[..., 0] if philox is None else philox(int(key), int(s), 0, int(g), 2)[0]
    return (np.float64(w0) + 0.5) * 2.0 ** -32


def exchange_ref(slots, who, T, U, key, g, K, status, philox=None):
    """One molecule's attempt behind global step g (g % K == 0; the attempt's number is g // K) in float64.  slots (C,): the slot of each
    replica; who (C,): its inverse; T (C,) kelvin; U (C,): epot + erestr per replica; status (C,): RUNNING or stopped.
    -> (slots, who) after the attempt (new arrays) and the decisions [(s, lo, hi, D, u, attempted, accepted)]"""
    slots, who = np.array(slots, dtype=np.int64), np.array(who, dtype=np.int64)
    C, a = len(slots), g // K
    assert g % K == 0 and sorted(slots) == list(range(C)) and all(slots[who[s]] == s for s in range(C))
    out = []
    for s in range(a % 2, C - 1, 2):
        lo, hi = int(who[s]), int(who[s + 1])
        ok = status[lo] == RUNNING and status[hi] == RUNNING and np.isfinite(U[lo]) and np.isfinite(U[hi])
        D, u, acc = np.nan, np.nan, False
        if ok:
            D = (beta(T[s]) - beta(T[s + 1])) * (np.float64(U[lo]) - np.float64(U[hi]))
            u = float(uniform(key, s, g, philox))
            acc = bool(D >= 0 or u < np.exp(D))
        if acc:
            slots[lo], slots[hi] = s + 1, s
            who[s], who[s + 1] = hi, lo
        out.append((s, lo, hi, float(D), u, bool(ok), acc))
    return slots, who, out


def inverse(slots):
    who = np.empty_like(np.asarray(slots))
    who[np.asarray(slots)] = np.arange(len(slots))
    return who


def attempt_ref(slots, T, U, keys, g, K, status):
    """exchange_ref over a batch: slots, U, status (B, C) -> slots after (B, C), decisions per molecule"""
    new, dec = [], []
    for b in range(len(slots)):
        s, _, d = exchange_ref(slots[b], inverse(slots[b]), T, U[b], keys[b], g, K, status[b])
        new.append(s), dec.append(d)
    return np.stack(new), dec


def scale_of(T_new, T_old):
    """the factor of a swapped replica's velocities, as the library forms it"""
    return np.float32(np.sqrt(np.float64(np.float32(T_new)) / np.float64(np.float32(T_old))))


def ladder_ref(batch, masses, keys, T, K, n_steps, velocities, slots=None, first_step=0, friction=FRICTION, dt=0.001, erestr_at=None,
               dtype=torch.float64):
    """The ladder run in `dtype`, composed from md_refs.baoab_ref.  Segments of K steps (K == 0: one segment); in a segment, one
    baoab_ref call per slot temperature, of which the (molecule, conformation)s that hold that slot are selected.
    erestr_at(x) -> (B, C) float64: E_r at x (None: 0); inside md_restr_refs.restr_force the force already holds the restraints.
    -> dict: xyz, vel (N, C, 3), slots (B, C), status (B, C), log [dict(g, slots (B, C) after, U (B, C), decisions per molecule)]"""
    B, C = batch.B, batch.xyz.shape[1]
    T = np.asarray(T, dtype=np.float32)
    slots = np.tile(np.arange(C), (B, 1)) if slots is None else np.array(slots, dtype=np.int64).reshape(B, C)
    x, v = batch.xyz.to(dtype).clone(), velocities.to(dtype).clone()
    status = np.zeros((B, C), dtype=np.int64)
    am = batch.atom_mol.numpy()
    log, done = [], 0
    seg = K if K > 0 else n_steps
    assert first_step % max(K, 1) == 0
    while done < n_steps:
        n = min(seg, n_steps - done)
        xn, vn, E = x.clone(), v.clone(), torch.zeros(B, C, dtype=torch.float64)
        for s in sorted(set(slots.reshape(-1).tolist())):
            confs = sorted(set(np.nonzero(slots == s)[1].tolist()))
            r = _segment(batch, x, masses, keys, v, float(T[s]), friction, dt, n, first_step + done, dtype)
            for c in confs:
                mols = torch.from_numpy(slots[:, c] == s)
                rows = mols[torch.from_numpy(am)]
                xn[rows, c], vn[rows, c] = r["xyz"][rows, c], r["vel"][rows, c]
                E[mols, c] = r["epot"][mols, c]
                status[mols.numpy(), c] = np.where(status[mols.numpy(), c] != 0, status[mols.numpy(), c], r["status"][mols, c].numpy())
        x, v, done = xn, vn, done + n
        if K > 0 and done % K == 0:
            g = first_step + done
            U = E.numpy().copy()
            if erestr_at is not None:
                U = U + erestr_at(x).numpy()
            before = slots.copy()
            slots, dec = attempt_ref(slots, T, U, keys, g, K, status)
            for b in range(B):
                p0, p1 = int(batch.ptr[b]), int(batch.ptr[b + 1])
                for c in range(C):
                    if slots[b, c] != before[b, c]:
                        v[p0:p1, c] = (v[p0:p1, c].to(dtype) * torch.tensor(float(scale_of(T[slots[b, c]], T[before[b, c]])), dtype=dtype))
            log.append(dict(g=g, slots=slots.copy(), U=U, decisions=dec))
    return dict(xyz=x, vel=v, slots=slots, status=status, log=log)


def _segment(batch, x, masses, keys, v, temperature, friction, dt, n, first_step, dtype):
    """n steps of md_refs.baoab_ref from (x, v) at one temperature: the batch's tables with x, held in `dtype`, as its coordinates"""
    import relax_refs as rr
    b = rr.Batch.from_tables(batch.counts, batch.idx, batch.mol_ptr, batch.ks, batch.eqs, batch.n_per, batch.params, x)
    return md.baoab_ref(b, masses, dtype, velocities=v, keys=keys, temperature=temperature, init_temperature=temperature, friction=friction, dt=dt,
                        n_steps=n, first_step=first_step)


@functools.lru_cache(maxsize=None)
def exchange_run(name, K):
    """the float64 ladder run of an exchange case: computed once and shared, read-only"""
    b = ms.case(name)
    return ladder_ref(b, ms.masses(name), ms.keys(name), EXCHANGE_CASES[name], K, EXCHANGE_STEPS, ms.thermal_velocities(name))


def decisive(run, margin=0.5):
    """-> (accepted, rejected): the decisions of a run with |ln u - D| >= margin (D >= 0 accepts whatever u is: it counts as decisive
    when D >= margin or ln u <= -margin)"""
    acc = rej = 0
    for row in run["log"]:
        for dec in row["decisions"]:
            for s, lo, hi, D, u, ok, a in dec:
                if not ok:
                    continue
                if a and (D >= margin or abs(np.log(u) - D) >= margin):
                    acc += 1
                if not a and abs(np.log(u) - D) >= margin:
                    rej += 1
    return acc, rej
