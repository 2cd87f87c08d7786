"""Sensing truth: per-(realisation, vehicle) sensors the controller does not know
(include/scpqp_sensing.h).

A sensing truth is a float64 tensor ``[B, nVeh, 8]`` of rows ``(sig_pos, sig_heading,
sig_speed, sig_steer, bias_heading, scale_speed, p_drop, lag)``: the noise on the measured
position, heading, speed and steering angle, a compass offset, an odometer scale, the
probability that a step's measurement is lost and an extra latency in ticks
(``ClosedLoopBatch.reset(..., sensing=)``).  The controller takes the measurement as the
state; it does not know that it is noisy, stale or held.  An obstacle sensing is a float64
tensor ``[B, nObst, 3]`` of rows ``(sig_pos, sig_heading, sig_speed)``: the noise on the
obstacle pose and speed the controller extrapolates (``reset(..., obstacle_sensing=)``).

``nominal``         the rows of the exact sensor: today's measurement, bitwise
``SenseDist``       a distribution per field, sampled on the device from one seed
                    (sharding-invariant through ``b_offset``)
``from_table``      rows gathered from a table of K candidates, for discrete studies
``validate``        host-side check of the rows before a rollout
``measure``         the measurement [B, nVeh, 6] of one MPC step
``predict_sensed``  the controller's obstacle prediction [B, nObst, 2, Hp] of one MPC step
                    from a noisy pose and speed
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as LB

NP = LB.SENSE_NP
FIELDS = LB.SENSE_FIELDS
ONP = LB.OSENSE_NP
OFIELDS = LB.OSENSE_FIELDS
NOMINAL_ROW = (0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0)
_SIGMAS = (LB.SENSE_SIG_POS, LB.SENSE_SIG_HEADING, LB.SENSE_SIG_SPEED, LB.SENSE_SIG_STEER)


def _field_index(field):
    if isinstance(field, str):
        if field not in FIELDS:
            raise ValueError(f"unknown sensing field {field!r}: one of {FIELDS}")
        return FIELDS.index(field)
    f = int(field)
    if not 0 <= f < NP:
        raise ValueError(f"sensing field index {f} out of range")
    return f


def _need_vehicles(nV):
    if not 1 <= nV <= LB.MAX_VEH:
        raise ValueError(f"a sensing truth needs 1..{LB.MAX_VEH} vehicles, got {nV}")


def nominal_rows(n_veh):
    """The nominal rows [nVeh, 8] on the host: (0, 0, 0, 0, 0, 1, 0, 0)."""
    return np.tile(np.array(NOMINAL_ROW), (int(n_veh), 1))


def is_nominal(rows):
    """True when every row is exactly the nominal one (host side)."""
    t = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows, float)
    return bool((t == np.array(NOMINAL_ROW)).all())


def nominal(B, n_veh, device=None):
    """[B, nVeh, 8]: the exact sensor (scpqp_sense_fill_nominal)."""
    from .plant import _ptr, _stream
    _need_vehicles(int(n_veh))
    device = torch.device(device or "cuda")
    lib = LB.load()
    out = torch.empty((int(B), int(n_veh), NP), dtype=torch.float64, device=device)
    LB.check(lib.scpqp_sense_fill_nominal(int(B), int(n_veh), _ptr(out), _stream(device)), lib)
    return out


def _check_floor(f, kind, lo, hi, mean):
    """The sampler's refusals (scpqp_sense_sample): a distribution that could emit a bad row."""
    name = FIELDS[f]
    if f in (LB.SENSE_BIAS_HEADING, LB.SENSE_SCALE_SPEED):
        return
    floor = float(np.min(mean)) if kind == LB.TRUTH_FIXED else lo
    top = float(np.max(mean)) if kind == LB.TRUTH_FIXED else hi
    if not floor >= 0.0:
        raise ValueError(f"sensing field {name}: the smallest value must be >= 0")
    if f == LB.SENSE_P_DROP and not (floor <= 1.0 and top <= 1.0):
        raise ValueError(f"sensing field {name}: the smallest and the largest value must be in [0, 1]")


class SenseDist:
    """A distribution of sensing rows around the exact sensor.  Every field starts FIXED at
    its nominal value; ``uniform`` / ``normal`` / ``fixed`` set one field.  ``sample(B)`` draws
    on the device: field f of realisation b, vehicle v, comes from one Philox call of counter
    (f, 0, (5 << 24) | v, b_offset + b), so a batch split over calls or ranks (``b_offset`` =
    global index of the call's first realisation) samples what one call would.  ``lag`` is
    rounded to a whole number of ticks after clamping."""

    def __init__(self, n_veh, seed, b_offset=0):
        n_veh = int(getattr(n_veh, "nVeh", n_veh))       # a scenario, or the number itself
        _need_vehicles(n_veh)
        self.mean = nominal_rows(n_veh).T.copy()             # [8, nVeh]
        self.n_veh = n_veh
        self.seed, self.b_offset = int(seed), int(b_offset)
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("seed must be in [0, 2**64)")
        if not 0 <= self.b_offset < 2 ** 32:
            raise ValueError("b_offset must be in [0, 2**32)")
        self.kind = [LB.TRUTH_FIXED] * NP
        self.spread = [0.0] * NP
        self.lo = [-math.inf] * NP
        self.hi = [math.inf] * NP

    def _set(self, field, kind, mean, spread, lo, hi):
        f = _field_index(field)
        spread = float(spread)
        if not (0.0 <= spread < math.inf):
            raise ValueError(f"sensing field {FIELDS[f]}: spread must be finite and >= 0")
        lo = -math.inf if lo is None else float(lo)
        hi = math.inf if hi is None else float(hi)
        if not lo <= hi:
            raise ValueError(f"sensing field {FIELDS[f]}: lo must be <= hi")
        m = self.mean[f] if mean is None else np.broadcast_to(np.asarray(mean, float), (self.n_veh,))
        if not np.isfinite(m).all():
            raise ValueError(f"sensing field {FIELDS[f]}: every mean must be finite")
        _check_floor(f, kind, lo, hi, m)
        self.mean[f, :] = m
        self.kind[f], self.spread[f], self.lo[f], self.hi[f] = kind, spread, lo, hi
        return self

    def uniform(self, field, spread, lo=None, hi=None, mean=None):
        """mean + spread * xi, xi uniform in [-1, 1), clamped to [lo, hi]."""
        return self._set(field, LB.TRUTH_UNIFORM, mean, spread, lo, hi)

    def normal(self, field, spread, lo=None, hi=None, mean=None):
        """mean + spread * z, z standard normal, clamped to [lo, hi]."""
        return self._set(field, LB.TRUTH_NORMAL, mean, spread, lo, hi)

    def fixed(self, field, value):
        """The same value for every realisation (a scalar, or one per vehicle)."""
        f = _field_index(field)
        value = np.broadcast_to(np.asarray(value, float), (self.n_veh,))
        if not np.isfinite(value).all():
            raise ValueError(f"sensing field {FIELDS[f]}: a fixed value must be finite")
        _check_floor(f, LB.TRUTH_FIXED, -math.inf, math.inf, value)
        self.mean[f, :] = value
        self.kind[f], self.spread[f], self.lo[f], self.hi[f] = LB.TRUTH_FIXED, 0.0, -math.inf, math.inf
        return self

    def with_offset(self, b_offset):
        """The same distribution for the shard whose first realisation is ``b_offset``."""
        d = SenseDist.__new__(SenseDist)
        d.__dict__.update(self.__dict__)
        d.mean = self.mean.copy()
        d.kind, d.spread, d.lo, d.hi = list(self.kind), list(self.spread), list(self.lo), list(self.hi)
        d.b_offset = int(b_offset)
        if not 0 <= d.b_offset < 2 ** 32:
            raise ValueError("b_offset must be in [0, 2**32)")
        return d

    def c_struct(self):
        d = LB.SenseDist()
        d.n_veh = self.n_veh
        d.seed, d.b_offset = self.seed, self.b_offset
        for f in range(NP):
            for v in range(self.n_veh):
                d.mean[f][v] = float(self.mean[f, v])
            d.field[f].kind = self.kind[f]
            d.field[f].spread = self.spread[f]
            d.field[f].lo = self.lo[f]
            d.field[f].hi = self.hi[f]
        return d

    def sample(self, B, device=None):
        """[B, nVeh, 8] on the device (scpqp_sense_sample)."""
        from .plant import _ptr, _stream
        device = torch.device(device or "cuda")
        lib = LB.load()
        out = torch.empty((int(B), self.n_veh, NP), dtype=torch.float64, device=device)
        d = self.c_struct()
        LB.check(lib.scpqp_sense_sample(C.byref(d), int(B), _ptr(out), _stream(device)), lib)
        return out


def from_table(rows, index, device=None):
    """rows [K, nVeh, 8], index [B] -> the sensing truth [B, nVeh, 8] with realisation b
    holding rows[index[b]] (a discrete study: K candidate sensor sets)."""
    device = torch.device(device or (rows.device if isinstance(rows, torch.Tensor) else "cuda"))
    rows = torch.as_tensor(rows, dtype=torch.float64, device=device)
    if rows.dim() != 3 or rows.shape[2] != NP:
        raise ValueError("rows must be [K, nVeh, 8]")
    idx = torch.as_tensor(index, device=device).reshape(-1).long()
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= rows.shape[0]):
        raise ValueError("index outside the table")
    return rows[idx].contiguous()


def validate(rows, max_lag=None):
    """ValueError on rows the device would treat as bad (include/scpqp_sensing.h): a
    non-finite field, a negative sigma, p_drop outside [0, 1], a lag that is negative or not a
    whole number; with ``max_lag`` also a lag above it (a rollout can look back only into the
    previous step's path).  Host side: one copy of the array."""
    t = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows, float)
    if t.ndim != 3 or t.shape[2] != NP:
        raise ValueError("rows must be [B, nVeh, 8]")

    if not np.isfinite(t).all():
        b, v, f = np.argwhere(~np.isfinite(t))[0]
        raise ValueError(f"rows[{b}, {v}]: {FIELDS[f]} is not finite")

    def refuse(mask, what):
        bad = np.argwhere(mask)                              # mask [B, nVeh]
        if len(bad):
            raise ValueError(f"rows[{bad[0][0]}, {bad[0][1]}]: {what}")

    for f in _SIGMAS:
        refuse(t[..., f] < 0.0, f"{FIELDS[f]} must be >= 0")
    p, lag = t[..., LB.SENSE_P_DROP], t[..., LB.SENSE_LAG]
    refuse((p < 0.0) | (p > 1.0), "p_drop must be in [0, 1]")
    refuse(lag < 0.0, "lag must be >= 0")
    refuse(lag != np.rint(lag), "lag must be a whole number of ticks")
    if max_lag is not None:
        refuse(lag > float(max_lag), f"lag must be <= {int(max_lag)} ticks (the measured tick lies "
                                     f"in the previous step's path)")


def validate_obstacle_sensing(osense):
    """ValueError on obstacle sensing rows [B, nObst, 3] with a non-finite or negative field."""
    t = osense.detach().cpu().numpy() if isinstance(osense, torch.Tensor) \
        else np.asarray(osense, float)
    if t.ndim != 3 or t.shape[2] != ONP:
        raise ValueError("obstacle sensing rows must be [B, nObst, 3]")
    bad = np.argwhere(~np.isfinite(t))
    if len(bad):
        b, o, f = bad[0]
        raise ValueError(f"obstacle_sensing[{b}, {o}]: {OFIELDS[f]} is not finite")
    bad = np.argwhere(t < 0.0)
    if len(bad):
        b, o, f = bad[0]
        raise ValueError(f"obstacle_sensing[{b}, {o}]: {OFIELDS[f]} must be >= 0")


def _stream_struct(seed, epoch, b_offset):
    seed, epoch, b_offset = int(seed), int(epoch), int(b_offset)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be in [0, 2**64)")
    if not 0 <= epoch < 2 ** 32:
        raise ValueError("epoch must be in [0, 2**32)")
    if not 0 <= b_offset < 2 ** 32:
        raise ValueError("b_offset must be in [0, 2**32)")
    return LB.SenseStream(seed=seed, epoch=epoch, b_offset=b_offset)


def _gpu_f64(t, what, last):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_cuda \
            or t.shape[-1] != last:
        raise ValueError(f"{what} must be a float64 [..., {last}] tensor on the GPU")
    return t.contiguous()


def measure(x_path, k_meas, rows, seed, epoch, b_offset, x_held, delivered=None):
    """x_path [B, nVeh, n_ticks + 1, 6] (or a state [B, nVeh, 6]: n_ticks = 0) -> the
    measurement [B, nVeh, 6] of MPC step ``epoch`` taken at entry ``k_meas``
    (scpqp_sense_measure).  ``x_held`` [B, nVeh, 6] is updated in place: the last delivered
    measurement (NaN before the first step).  ``delivered`` (int32 [B, nVeh], optional)
    receives 1 where this step's measurement arrived.  A bad row's lane is NaN."""
    from .plant import _ptr, _stream
    rows = _gpu_f64(rows, "rows", NP)
    x_path = _gpu_f64(x_path, "x_path", 6)
    if x_path.dim() == 3:
        x_path = x_path[:, :, None, :]
    if rows.dim() != 3 or x_path.dim() != 4 or tuple(x_path.shape[:2]) != tuple(rows.shape[:2]):
        raise ValueError("x_path must be [B, nVeh, n_ticks + 1, 6] and rows [B, nVeh, 8]")
    B, nV, K = int(x_path.shape[0]), int(x_path.shape[1]), int(x_path.shape[2])
    _need_vehicles(nV)
    if K < 1 or not 0 <= int(k_meas) < K:
        raise ValueError(f"k_meas must be in 0..{K - 1}")
    if not isinstance(x_held, torch.Tensor) or x_held.dtype != torch.float64 or not x_held.is_cuda \
            or tuple(x_held.shape) != (B, nV, 6) or not x_held.is_contiguous():
        raise ValueError("x_held must be a contiguous float64 [B, nVeh, 6] tensor on the GPU")
    if delivered is not None and (not isinstance(delivered, torch.Tensor)
                                  or delivered.dtype != torch.int32 or not delivered.is_cuda
                                  or tuple(delivered.shape) != (B, nV)
                                  or not delivered.is_contiguous()):
        raise ValueError("delivered must be a contiguous int32 [B, nVeh] tensor on the GPU")
    st = _stream_struct(seed, epoch, b_offset)
    lib = LB.load()
    out = torch.empty((B, nV, 6), dtype=torch.float64, device=rows.device)
    LB.check(lib.scpqp_sense_measure(B, nV, K - 1, int(k_meas), _ptr(x_path), _ptr(rows),
                                     C.byref(st), _ptr(x_held), _ptr(delivered), _ptr(out),
                                     _stream(rows.device)), lib)
    return out


def predict_sensed(rows, osense, seed, epoch, b_offset, t_meas, lead, dt, hp):
    """``obstacles.predict`` from the measured pose and speed: rows [B, nObst, 7] (the
    obstacle truth), osense [B, nObst, 3] -> [B, nObst, 2, hp]
    (scpqp_obstacles_predict_sensed).  An all-zero osense row gives ``obstacles.predict``
    bitwise; a bad row of either kind gives a NaN block."""
    from .obstacles import _rows_arg
    from .plant import _ptr, _stream
    rows = _rows_arg(rows)
    osense = _gpu_f64(osense, "osense", ONP)
    B, nO = int(rows.shape[0]), int(rows.shape[1])
    if tuple(osense.shape) != (B, nO, ONP):
        raise ValueError("osense must be [B, nObst, 3]")
    st = _stream_struct(seed, epoch, b_offset)
    lib = LB.load()
    out = torch.empty((B, nO, 2, int(hp)), dtype=torch.float64, device=rows.device)
    LB.check(lib.scpqp_obstacles_predict_sensed(B, nO, int(hp), _ptr(rows), _ptr(osense),
                                                C.byref(st), float(t_meas), float(lead),
                                                float(dt), _ptr(out), _stream(rows.device)), lib)
    return out
