"""Temperature ladders and replica exchange (parallel tempering) on the stepwise dynamics (`simulate(..., replicas=)`,
include/grappa_hip.h grappa_md_remd_*_f32).  The C conformations of a call are C replicas; `temperatures` (C,) in kelvin is the ladder.
Replica c keeps its coordinates, its noise stream and its index; what moves is the SLOT of the ladder it holds.  With
`exchange_every = K > 0`, behind every K-th step the replicas in neighbouring slots (s, s + 1), s of the attempt's parity, swap their
slots with the Metropolis probability min(1, exp((beta_s - beta_{s+1}) (U_lo - U_hi))) and their velocities are rescaled to the new
temperature; K = 0 is a ladder without exchanges (simulated-annealing starts, high-temperature conformer search followed by `relax`).
Every molecule of a batch has its own independent ladder state over the same temperatures.  A continued run passes
`ReplicaExchange(..., slots=result.slots)` with `velocities=` and `first_step=`.  Not here: Hamiltonian exchange between umbrella
windows, coordinate exchange, non-neighbour pairs, per-replica friction or time step, annealing schedules."""
import numpy as np


class ReplicaExchange:
    """temperatures: (C,) kelvin, slot s of the ladder; finite and >= 0, with exchanges > 0.  exchange_every: K >= 0 (0: no exchanges).
    slots: None (replica c starts in slot c), (C,) or (B, C) integers: the slot every replica starts in, a permutation of 0 .. C-1 per
    molecule.  What is checked here on the host is what the device vets (status 5)."""

    def __init__(self, temperatures, exchange_every: int = 0, slots=None):
        t = np.asarray(temperatures, dtype=np.float64)
        if t.ndim != 1 or t.shape[0] < 1:
            raise ValueError(f"temperatures must be a non-empty 1-D sequence, got shape {t.shape}")
        if isinstance(exchange_every, bool) or not isinstance(exchange_every, (int, np.integer)) or exchange_every < 0:
            raise ValueError(f"exchange_every must be an integer >= 0, got {exchange_every!r}")
        with np.errstate(over="ignore"):
            finite = np.isfinite(t).all() and np.isfinite(t.astype(np.float32)).all()          # (the library reads them as fp32)
        if not finite:
            raise ValueError("temperatures must be finite")
        if exchange_every > 0 and not (t > 0).all():
            raise ValueError("temperatures must be positive when replicas exchange")
        if not (t >= 0).all():
            raise ValueError("temperatures must be >= 0")
        self.temperatures = t.astype(np.float32)
        self.exchange_every = int(exchange_every)
        self.slots = None
        if slots is not None:
            # (a tensor first: `MDResult.slots` of `simulate_graph` lies on the graph's device, which np.asarray does not take)
            s = slots.detach().cpu().numpy() if hasattr(slots, "detach") else np.asarray(slots)
            if s.dtype.kind not in "iu" or s.ndim not in (1, 2) or s.shape[-1] != t.shape[0]:
                raise ValueError(f"slots must be integers of shape (C,) or (B, C) with C = {t.shape[0]}, got {s.dtype} {s.shape}")
            rows = s.reshape(-1, t.shape[0])
            if not (np.sort(rows, axis=1) == np.arange(t.shape[0])[None]).all():
                raise ValueError("slots must be a permutation of 0 .. C-1 for every molecule")
            self.slots = s.astype(np.int32)

    @property
    def C(self) -> int:
        return int(self.temperatures.shape[0])

    def slots_for(self, B: int):
        """(B, C) int32 or None: the start slots of a batch of B molecules ((C,) is every molecule's row)"""
        if self.slots is None:
            return None
        if self.slots.ndim == 1:
            return np.tile(self.slots[None], (B, 1))
        if self.slots.shape[0] != B:
            raise ValueError(f"slots describe {self.slots.shape[0]} molecules, the batch has {B}")
        return self.slots


def acceptance(exchange_slots, slots0, first_attempt: int = 1):
    """accepted / attempted per neighbouring pair of slots, on the host: exchange_slots (X, B, C), the slots after each attempt
    (`MDResult.exchange_slots`); slots0 (B, C) or (C,), the slots the run started in; first_attempt: the number of the attempt of row 0
    (first_step / exchange_every + 1).  -> (B, C-1) float64; attempt a counts as an attempt of the pairs (s, s + 1) with s = a (mod 2)
    (a pair that was not attempted because a replica had stopped counts as rejected); NaN for a pair that no attempt names."""
    to_np = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)      # noqa: E731
    xs = to_np(exchange_slots)
    if xs.ndim != 3:
        raise ValueError(f"exchange_slots must be (X, B, C), got {xs.shape}")
    X, B, C = xs.shape
    prev = np.broadcast_to(to_np(slots0).reshape(-1, C), (B, C)).copy()
    acc, att = np.zeros((B, max(C - 1, 0))), np.zeros((B, max(C - 1, 0)))
    for i in range(X):
        a = int(first_attempt) + i
        for s in range(a % 2, C - 1, 2):
            att[:, s] += 1
            for b in range(B):
                lo = np.nonzero(prev[b] == s)[0]
                if lo.size == 1 and xs[i, b, lo[0]] == s + 1:
                    acc[b, s] += 1
        prev = xs[i].copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(att > 0, acc / att, np.nan)
