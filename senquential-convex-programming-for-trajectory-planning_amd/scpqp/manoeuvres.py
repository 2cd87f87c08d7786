"""Obstacle manoeuvres: braking, accelerating and turning obstacles the controller does not
know of (include/scpqp_manoeuvres.h; csrc/manoeuvres.hip).

A manoeuvre schedule is a float64 tensor ``[B, nObst, 4, 3]`` of pieces ``(dur, accel,
dyaw)`` on top of the obstacle rows of ``scpqp.obstacles``: the pieces follow each other from
t = 0 (a piece of duration 0 is skipped); during a piece the obstacle accelerates by
``accel`` and turns at the row's yaw rate plus ``dyaw``; after the last piece it keeps the
speed it has reached and the row's yaw rate.  An obstacle that brakes to a stop stands, with
its heading, until a piece with ``accel > 0`` starts it again.  The world follows the schedule
(``PathMetrics.accumulate(..., manoeuvres=)``, ``ClosedLoopBatch.reset(..., manoeuvres=)``);
the controller measures the true pose and speed at each step and knows nothing else.

``off``            an all-off schedule: the rows' own motion
``is_off``         host-side check: no lane has a piece that does anything
``rows``           a schedule from scalars or arrays per (piece, field)
``brake``          composer: coast until t0, then brake at ``decel`` for ``duration``
``turn``           composer: coast until t0, then turn at ``dyaw`` more for ``duration``
``lane_change``    composer: coast until t0, then +dyaw and -dyaw for ``duration`` each
``ManoeuvreDist``  a distribution per (piece, field), sampled on the device from one seed
``from_table``     schedules gathered from a table of K candidates
``validate``       host-side check of a schedule (and its rows) before a rollout
``state``          the snapshot row [B, nObst, 7] of every lane at a time t
``pose``           x, y, heading of every lane over a range of global ticks
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as LB

NSEG = LB.MAN_NSEG
NF = LB.MAN_NF
FIELDS = LB.MAN_FIELDS


def _need_obstacles(nO):
    if not 1 <= nO <= LB.MAX_OBST:
        raise ValueError(f"a manoeuvre schedule needs 1..{LB.MAX_OBST} obstacles, got {nO}")


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, float)


def _field_index(field):
    if isinstance(field, str):
        if field not in FIELDS:
            raise ValueError(f"unknown manoeuvre field {field!r}: one of {FIELDS}")
        return FIELDS.index(field)
    f = int(field)
    if not 0 <= f < NF:
        raise ValueError(f"manoeuvre field index {f} out of range")
    return f


def _seg_index(seg):
    i = int(seg)
    if not 0 <= i < NSEG:
        raise ValueError(f"manoeuvre piece {i} out of range: 0..{NSEG - 1}")
    return i


def off(B, n_obst, device=None):
    """[B, nObst, 4, 3] of zeros: every lane moves by its row alone."""
    _need_obstacles(int(n_obst))
    return torch.zeros((int(B), int(n_obst), NSEG, NF), dtype=torch.float64,
                       device=torch.device(device or "cuda"))


def off_lanes(man):
    """[B, nObst] bool on the host: the lanes whose every piece has dur == 0 or
    (accel == 0 and dyaw == 0)."""
    t = _host(man)
    return ((t[..., LB.MAN_DUR] == 0.0)
            | ((t[..., LB.MAN_ACCEL] == 0.0) & (t[..., LB.MAN_DYAW] == 0.0))).all(axis=-1)


def is_off(man):
    """True when every lane is off and no field is bad (host side)."""
    t = _host(man)
    return bool(np.isfinite(t).all() and (t[..., LB.MAN_DUR] >= 0.0).all() and off_lanes(t).all())


def rows(B, n_obst, pieces, device=None):
    """[B, nObst, 4, 3] from up to four pieces ``(dur, accel, dyaw)``; each value a scalar or
    an array that broadcasts to [B, nObst] (``[B, 1]``: one schedule per realisation).  The
    pieces not given are zero.  Validated."""
    B, n_obst = int(B), int(n_obst)
    _need_obstacles(n_obst)
    pieces = list(pieces)
    if len(pieces) > NSEG:
        raise ValueError(f"a schedule holds at most {NSEG} pieces, got {len(pieces)}")
    out = np.zeros((B, n_obst, NSEG, NF))
    for i, piece in enumerate(pieces):
        piece = tuple(piece)
        if len(piece) != NF:
            raise ValueError(f"piece {i} must be (dur, accel, dyaw)")
        for f, val in enumerate(piece):
            try:
                out[:, :, i, f] = np.broadcast_to(np.asarray(_host(val), float), (B, n_obst))
            except ValueError:
                raise ValueError(f"piece {i} {FIELDS[f]} does not broadcast to [B, nObst] = "
                                 f"[{B}, {n_obst}]") from None
    validate(out)
    return torch.as_tensor(out, dtype=torch.float64, device=torch.device(device or "cuda"))


def brake(t0, decel, duration):
    """Pieces: coast for ``t0``, then an acceleration of ``-decel`` for ``duration`` (an
    obstacle that stops before the end stands for the rest)."""
    return [(t0, 0.0, 0.0), (duration, -np.asarray(_host(decel), float), 0.0)]


def turn(t0, dyaw, duration):
    """Pieces: coast for ``t0``, then the row's turn rate plus ``dyaw`` for ``duration``."""
    return [(t0, 0.0, 0.0), (duration, 0.0, dyaw)]


def lane_change(t0, dyaw, duration):
    """Pieces: coast for ``t0``, then ``+dyaw`` and ``-dyaw`` for ``duration`` each: the
    heading returns to what it would have been, the obstacle is displaced sideways."""
    return [(t0, 0.0, 0.0), (duration, 0.0, dyaw), (duration, 0.0, -np.asarray(_host(dyaw), float))]


class ManoeuvreDist:
    """A distribution of schedules, the same for every obstacle.  Every (piece, field) starts
    FIXED at 0 (an off schedule); ``uniform`` / ``normal`` / ``fixed`` set one.  ``sample(B)``
    draws on the device: field f of piece i of realisation b, obstacle o, comes from one Philox
    call of counter (3 i + f, 0, (8 << 24) | o, b_offset + b), so a batch split over calls or
    ranks (``b_offset`` = global index of the call's first realisation) samples what one call
    would.  A duration that could come out negative is refused."""

    def __init__(self, n_obst, seed, b_offset=0):
        self.n_obst = int(n_obst)
        _need_obstacles(self.n_obst)
        self.seed, self.b_offset = int(seed), int(b_offset)
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("seed must be in [0, 2**64)")
        if not 0 <= self.b_offset < 2 ** 32:
            raise ValueError("b_offset must be in [0, 2**32)")
        self.mean = np.zeros((NSEG, NF))
        self.kind = np.full((NSEG, NF), LB.TRUTH_FIXED, int)
        self.spread = np.zeros((NSEG, NF))
        self.lo = np.full((NSEG, NF), -math.inf)
        self.hi = np.full((NSEG, NF), math.inf)

    def _set(self, seg, field, kind, mean, spread, lo, hi):
        i, f = _seg_index(seg), _field_index(field)
        name = f"manoeuvre piece {i} field {FIELDS[f]}"
        mean, spread = float(mean), float(spread)
        if not math.isfinite(mean):
            raise ValueError(f"{name}: the mean must be finite")
        if not (0.0 <= spread < math.inf):
            raise ValueError(f"{name}: spread must be finite and >= 0")
        lo = -math.inf if lo is None else float(lo)
        hi = math.inf if hi is None else float(hi)
        if not lo <= hi:
            raise ValueError(f"{name}: lo must be <= hi")
        if f == LB.MAN_DUR and not lo >= 0.0:
            raise ValueError(f"{name}: lo must be >= 0 (a drawn duration is never negative)")
        self.kind[i, f], self.mean[i, f], self.spread[i, f] = kind, mean, spread
        self.lo[i, f], self.hi[i, f] = lo, hi
        return self

    def uniform(self, seg, field, mean, spread, lo=None, hi=None):
        """mean + spread * xi, xi uniform in [-1, 1), clamped to [lo, hi]."""
        return self._set(seg, field, LB.TRUTH_UNIFORM, mean, spread, lo, hi)

    def normal(self, seg, field, mean, spread, lo=None, hi=None):
        """mean + spread * z, z standard normal, clamped to [lo, hi]."""
        return self._set(seg, field, LB.TRUTH_NORMAL, mean, spread, lo, hi)

    def fixed(self, seg, field, value):
        """The same value for every lane."""
        i, f = _seg_index(seg), _field_index(field)
        value = float(value)
        name = f"manoeuvre piece {i} field {FIELDS[f]}"
        if not math.isfinite(value):
            raise ValueError(f"{name}: a fixed value must be finite")
        if f == LB.MAN_DUR and value < 0.0:
            raise ValueError(f"{name}: a fixed duration must be >= 0")
        self.kind[i, f], self.mean[i, f], self.spread[i, f] = LB.TRUTH_FIXED, value, 0.0
        self.lo[i, f], self.hi[i, f] = -math.inf, math.inf
        return self

    def with_offset(self, b_offset):
        """The same distribution for the shard whose first realisation is ``b_offset``."""
        d = ManoeuvreDist.__new__(ManoeuvreDist)
        d.__dict__.update(self.__dict__)
        for k in ("mean", "kind", "spread", "lo", "hi"):
            setattr(d, k, getattr(self, k).copy())
        d.b_offset = int(b_offset)
        if not 0 <= d.b_offset < 2 ** 32:
            raise ValueError("b_offset must be in [0, 2**32)")
        return d

    def c_struct(self):
        d = LB.ManoeuvreDist()
        d.n_obst = self.n_obst
        d.seed, d.b_offset = self.seed, self.b_offset
        for i in range(NSEG):
            for f in range(NF):
                d.mean[i][f] = float(self.mean[i, f])
                d.field[i][f].kind = int(self.kind[i, f])
                d.field[i][f].spread = float(self.spread[i, f])
                d.field[i][f].lo = float(self.lo[i, f])
                d.field[i][f].hi = float(self.hi[i, f])
        return d

    def sample(self, B, device=None):
        """[B, nObst, 4, 3] on the device (scpqp_manoeuvres_sample)."""
        from .plant import _ptr, _stream
        device = torch.device(device or "cuda")
        lib = LB.load()
        out = torch.empty((int(B), self.n_obst, NSEG, NF), dtype=torch.float64, device=device)
        d = self.c_struct()
        LB.check(lib.scpqp_manoeuvres_sample(C.byref(d), int(B), _ptr(out), _stream(device)), lib)
        return out


def from_table(table, index, device=None):
    """table [K, nObst, 4, 3], index [B] -> the schedule [B, nObst, 4, 3] with realisation b
    holding table[index[b]] (a discrete study: K candidate manoeuvres)."""
    device = torch.device(device or (table.device if isinstance(table, torch.Tensor) else "cuda"))
    table = torch.as_tensor(table, dtype=torch.float64, device=device)
    if table.dim() != 4 or tuple(table.shape[2:]) != (NSEG, NF):
        raise ValueError("table must be [K, nObst, 4, 3]")
    idx = torch.as_tensor(index, device=device).reshape(-1).long()
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= table.shape[0]):
        raise ValueError("index outside the table")
    return table[idx].contiguous()


def validate(man, rows=None):
    """ValueError on a schedule the device would treat as bad (include/scpqp_manoeuvres.h): a
    non-finite field or a negative duration and, with the obstacle ``rows`` [B, nObst, 7], a
    lane that is not off on a row with a negative speed.  The message names ``man[b, o, seg]``
    and the field.  Host side: one copy of the array."""
    t = _host(man)
    if t.ndim != 4 or tuple(t.shape[2:]) != (NSEG, NF):
        raise ValueError("man must be [B, nObst, 4, 3]")
    bad = np.argwhere(~np.isfinite(t))
    if len(bad):
        b, o, i, f = bad[0]
        raise ValueError(f"man[{b}, {o}, {i}]: {FIELDS[f]} is not finite")
    bad = np.argwhere(t[..., LB.MAN_DUR] < 0.0)
    if len(bad):
        b, o, i = bad[0]
        raise ValueError(f"man[{b}, {o}, {i}]: dur must be >= 0")
    if rows is not None:
        r = _host(rows)
        if r.ndim != 3 or r.shape[2] != LB.OBST_NP or r.shape[:2] != t.shape[:2]:
            raise ValueError(f"rows must be [B, nObst, 7] = [{t.shape[0]}, {t.shape[1]}, 7]")
        bad = np.argwhere(~off_lanes(t) & (r[..., LB.OBST_SPEED] < 0.0))
        if len(bad):
            b, o = bad[0]
            raise ValueError(f"man[{b}, {o}]: a manoeuvre needs a row with speed >= 0")


def _man_arg(man, B, nO):
    if man is None:
        return None
    if not isinstance(man, torch.Tensor) or man.dtype != torch.float64 or not man.is_cuda \
            or tuple(man.shape) != (B, nO, NSEG, NF):
        raise ValueError(f"man must be a float64 [B, nObst, 4, 3] = [{B}, {nO}, 4, 3] tensor on "
                         f"the GPU")
    return man.contiguous()


def state(rows, man, t):
    """rows [B, nObst, 7], man [B, nObst, 4, 3] (None: every lane off) -> the snapshot rows
    [B, nObst, 7] at time ``t`` >= 0: position, heading and speed there, the footprint, and the
    turn rate in effect (scpqp_manoeuvres_state).  ``obstacles.predict(state, 0, ...)`` is the
    controller's prediction from the true pose and speed at ``t``.  A bad lane's block is
    NaN."""
    from .obstacles import _rows_arg
    from .plant import _ptr, _stream
    rows = _rows_arg(rows)
    B, nO = int(rows.shape[0]), int(rows.shape[1])
    man = _man_arg(man, B, nO)
    lib = LB.load()
    out = torch.empty((B, nO, LB.OBST_NP), dtype=torch.float64, device=rows.device)
    LB.check(lib.scpqp_manoeuvres_state(B, nO, _ptr(rows), _ptr(man), float(t), _ptr(out),
                                        _stream(rows.device)), lib)
    return out


def pose(rows, man, tick_length, tick0, n_ticks):
    """rows [B, nObst, 7], man [B, nObst, 4, 3] (None: every lane off) ->
    [B, nObst, n_ticks + 1, 3]: x, y, heading at the global ticks tick0 .. tick0 + n_ticks
    (scpqp_manoeuvres_pose).  An off lane is bitwise ``obstacles.pose``; a bad lane's block is
    NaN."""
    from .obstacles import _rows_arg
    from .plant import _ptr, _stream
    rows = _rows_arg(rows)
    B, nO = int(rows.shape[0]), int(rows.shape[1])
    man = _man_arg(man, B, nO)
    if int(n_ticks) < 0:
        raise ValueError("n_ticks must be >= 0")
    lib = LB.load()
    out = torch.empty((B, nO, int(n_ticks) + 1, 3), dtype=torch.float64, device=rows.device)
    LB.check(lib.scpqp_manoeuvres_pose(B, nO, _ptr(rows), _ptr(man), float(tick_length),
                                       int(tick0), int(n_ticks), _ptr(out),
                                       _stream(rows.device)), lib)
    return out
