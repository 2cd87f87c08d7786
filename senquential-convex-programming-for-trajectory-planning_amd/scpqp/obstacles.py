"""Obstacle truth: per-(realisation, obstacle) motion the controller does not know
(include/scpqp_obstacles.h).

An obstacle truth is a float64 tensor ``[B, nObst, 7]`` of rows ``(x, y, heading, speed,
length, width, yaw_rate)``: the pose at t = 0, the constant speed, the footprint and the
constant turn rate of the obstacle the realised path is measured against
(``PathMetrics.accumulate(..., obstacles=)``, ``ClosedLoopBatch.reset(..., obstacles=)``).
The controller measures the true pose and extrapolates it on a straight line
(MPC_Iter.py:45-51); it never sees the turn rate.

``nominal``       the rows of the scenario's own obstacles (turn rate 0)
``ObstacleDist``  a distribution per field, sampled on the device from one seed
                  (sharding-invariant through ``b_offset``)
``from_table``    rows gathered from a table of K candidates, for discrete studies
``validate``      host-side check of the rows before a rollout
``predict``       the controller's prediction [B, nObst, 2, Hp] of one MPC step
``pose``          x, y, heading of every row over a range of global ticks

``scpqp.sensing.predict_sensed`` is ``predict`` from a noisy measurement of the pose and speed
(include/scpqp_sensing.h).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as LB

NP = LB.OBST_NP
FIELDS = LB.OBSTACLE_FIELDS


def _field_index(field):
    if isinstance(field, str):
        if field not in FIELDS:
            raise ValueError(f"unknown obstacle field {field!r}: one of {FIELDS}")
        return FIELDS.index(field)
    f = int(field)
    if not 0 <= f < NP:
        raise ValueError(f"obstacle field index {f} out of range")
    return f


def nominal_rows(scenario):
    """The nominal rows [nObst, 7] on the host: scenario.obstacles[o][0:6] and turn rate 0."""
    nO = int(scenario.nObst)
    rows = np.zeros((nO, NP))
    if nO:
        rows[:, :6] = np.asarray(scenario.obstacles, float).reshape(nO, -1)[:, :6]
    return rows


def _need_obstacles(nO):
    if not 1 <= nO <= LB.MAX_OBST:
        raise ValueError(f"an obstacle truth needs 1..{LB.MAX_OBST} obstacles, the scenario has {nO}")


def _rows_arg(rows):
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float64 or rows.dim() != 3 \
            or rows.shape[2] != NP or not rows.is_cuda:
        raise ValueError("rows must be a float64 [B, nObst, 7] tensor on the GPU")
    _need_obstacles(int(rows.shape[1]))
    return rows.contiguous()


def nominal(scenario, B, device=None):
    """[B, nObst, 7]: the truth under which every obstacle does what the controller predicts
    (scpqp_obstacles_fill_nominal)."""
    from .plant import _ptr, _stream
    host = np.ascontiguousarray(nominal_rows(scenario)[:, :6])
    nO = host.shape[0]
    _need_obstacles(nO)
    device = torch.device(device or "cuda")
    lib = LB.load()
    out = torch.empty((int(B), nO, NP), dtype=torch.float64, device=device)
    LB.check(lib.scpqp_obstacles_fill_nominal(nO, host.ctypes.data_as(C.POINTER(C.c_double)), int(B),
                                              _ptr(out), _stream(device)), lib)
    return out


class ObstacleDist:
    """A distribution of obstacle rows around the scenario's own obstacles.  Every field
    starts FIXED at its nominal value (turn rate 0); ``uniform`` / ``normal`` / ``fixed`` set
    one field.  ``sample(B)`` draws on the device: field f of realisation b, obstacle o, comes
    from one Philox call of counter (f, 0, (4 << 24) | o, b_offset + b), so a batch split over
    calls or ranks (``b_offset`` = global index of the call's first realisation) samples what
    one call would."""

    def __init__(self, scenario, seed, b_offset=0):
        self.mean = nominal_rows(scenario).T.copy()          # [7, nObst]
        self.n_obst = self.mean.shape[1]
        _need_obstacles(self.n_obst)
        self.seed, self.b_offset = int(seed), int(b_offset)
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("seed must be in [0, 2**64)")
        if not 0 <= self.b_offset < 2 ** 32:
            raise ValueError("b_offset must be in [0, 2**32)")
        self.kind = [LB.TRUTH_FIXED] * NP
        self.spread = [0.0] * NP
        self.lo = [-math.inf] * NP
        self.hi = [math.inf] * NP

    def _set(self, field, kind, spread, lo, hi):
        f = _field_index(field)
        spread = float(spread)
        if not (0.0 <= spread < math.inf):
            raise ValueError(f"obstacle field {FIELDS[f]}: spread must be finite and >= 0")
        lo = -math.inf if lo is None else float(lo)
        hi = math.inf if hi is None else float(hi)
        if not lo <= hi:
            raise ValueError(f"obstacle field {FIELDS[f]}: lo must be <= hi")
        if f in (LB.OBST_LENGTH, LB.OBST_WIDTH) and not lo >= 0.0:
            raise ValueError(f"obstacle field {FIELDS[f]}: lo must be >= 0 (a drawn footprint "
                             f"is never negative)")
        self.kind[f], self.spread[f], self.lo[f], self.hi[f] = kind, spread, lo, hi
        return self

    def uniform(self, field, spread, lo=None, hi=None):
        """mean + spread * xi, xi uniform in [-1, 1), clamped to [lo, hi]."""
        return self._set(field, LB.TRUTH_UNIFORM, spread, lo, hi)

    def normal(self, field, spread, lo=None, hi=None):
        """mean + spread * z, z standard normal, clamped to [lo, hi]."""
        return self._set(field, LB.TRUTH_NORMAL, spread, lo, hi)

    def fixed(self, field, value):
        """The same value for every realisation (a scalar, or one per obstacle)."""
        f = _field_index(field)
        value = np.broadcast_to(np.asarray(value, float), (self.n_obst,))
        if not np.isfinite(value).all():
            raise ValueError(f"obstacle field {FIELDS[f]}: a fixed value must be finite")
        if f in (LB.OBST_LENGTH, LB.OBST_WIDTH) and (value < 0.0).any():
            raise ValueError(f"obstacle field {FIELDS[f]}: a fixed value must be >= 0")
        self.mean[f, :] = value
        self.kind[f], self.spread[f], self.lo[f], self.hi[f] = LB.TRUTH_FIXED, 0.0, -math.inf, math.inf
        return self

    def with_offset(self, b_offset):
        """The same distribution for the shard whose first realisation is ``b_offset``."""
        d = ObstacleDist.__new__(ObstacleDist)
        d.__dict__.update(self.__dict__)
        d.mean = self.mean.copy()
        d.kind, d.spread, d.lo, d.hi = list(self.kind), list(self.spread), list(self.lo), list(self.hi)
        d.b_offset = int(b_offset)
        if not 0 <= d.b_offset < 2 ** 32:
            raise ValueError("b_offset must be in [0, 2**32)")
        return d

    def c_struct(self):
        d = LB.ObstacleDist()
        d.n_obst = self.n_obst
        d.seed, d.b_offset = self.seed, self.b_offset
        for f in range(NP):
            for o in range(self.n_obst):
                d.mean[f][o] = float(self.mean[f, o])
            d.field[f].kind = self.kind[f]
            d.field[f].spread = self.spread[f]
            d.field[f].lo = self.lo[f]
            d.field[f].hi = self.hi[f]
        return d

    def sample(self, B, device=None):
        """[B, nObst, 7] on the device (scpqp_obstacles_sample)."""
        from .plant import _ptr, _stream
        device = torch.device(device or "cuda")
        lib = LB.load()
        out = torch.empty((int(B), self.n_obst, NP), dtype=torch.float64, device=device)
        d = self.c_struct()
        LB.check(lib.scpqp_obstacles_sample(C.byref(d), int(B), _ptr(out), _stream(device)), lib)
        return out


def from_table(rows, index, device=None):
    """rows [K, nObst, 7], index [B] -> the truth [B, nObst, 7] with realisation b holding
    rows[index[b]] (a discrete study: K candidate obstacle sets)."""
    device = torch.device(device or (rows.device if isinstance(rows, torch.Tensor) else "cuda"))
    rows = torch.as_tensor(rows, dtype=torch.float64, device=device)
    if rows.dim() != 3 or rows.shape[2] != NP:
        raise ValueError("rows must be [K, nObst, 7]")
    idx = torch.as_tensor(index, device=device).reshape(-1).long()
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= rows.shape[0]):
        raise ValueError("index outside the table")
    return rows[idx].contiguous()


def validate(rows):
    """ValueError on rows the device would treat as bad (include/scpqp_obstacles.h): a
    non-finite field, or a negative length or width.  Host side: one copy of the array."""
    t = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows, float)
    if t.ndim != 3 or t.shape[2] != NP:
        raise ValueError("rows must be [B, nObst, 7]")
    if not np.isfinite(t).all():
        b, o, f = np.argwhere(~np.isfinite(t))[0]
        raise ValueError(f"rows[{b}, {o}]: {FIELDS[f]} is not finite")
    for f in (LB.OBST_LENGTH, LB.OBST_WIDTH):
        bad = np.argwhere(t[..., f] < 0.0)
        if len(bad):
            raise ValueError(f"rows[{bad[0][0]}, {bad[0][1]}]: {FIELDS[f]} must be >= 0")


def predict(rows, t_meas, lead, dt, hp):
    """rows [B, nObst, 7] -> the controller's prediction [B, nObst, 2, hp] from the true pose
    at ``t_meas``: a straight line at the measured heading and the row's speed, sampled at
    (k + 1) dt + lead (scpqp_obstacles_predict).  A bad row's block is NaN."""
    from .plant import _ptr, _stream
    rows = _rows_arg(rows)
    B, nO = int(rows.shape[0]), int(rows.shape[1])
    lib = LB.load()
    out = torch.empty((B, nO, 2, int(hp)), dtype=torch.float64, device=rows.device)
    LB.check(lib.scpqp_obstacles_predict(B, nO, int(hp), _ptr(rows), float(t_meas), float(lead),
                                         float(dt), _ptr(out), _stream(rows.device)), lib)
    return out


def pose(rows, tick_length, tick0, n_ticks):
    """rows [B, nObst, 7] -> [B, nObst, n_ticks + 1, 3]: x, y, heading at the global ticks
    tick0 .. tick0 + n_ticks (scpqp_obstacles_pose).  A bad row's block is NaN."""
    from .plant import _ptr, _stream
    rows = _rows_arg(rows)
    B, nO = int(rows.shape[0]), int(rows.shape[1])
    lib = LB.load()
    if int(n_ticks) < 0:
        raise ValueError("n_ticks must be >= 0")
    out = torch.empty((B, nO, int(n_ticks) + 1, 3), dtype=torch.float64, device=rows.device)
    LB.check(lib.scpqp_obstacles_pose(B, nO, _ptr(rows), float(tick_length), int(tick0),
                                      int(n_ticks), _ptr(out), _stream(rows.device)), lib)
    return out
