"""Drive truth: a longitudinal actuator per (realisation, vehicle) between the governor's
command and the plant (include/scpqp_drive.h).

A drive is a float64 tensor ``[B, nVeh, 6]`` of rows ``(tau_a, gain_a, bias_a, a_max, b_max,
hold)``: the lag of the realised acceleration, the gain and offset of the command, the largest
realisable acceleration and deceleration, and whether the brakes hold the vehicle at rest
(``plant_step(..., drive=, a_cmd=)``, ``ClosedLoopBatch.reset(..., drive=)``).  The controller
and the governor keep assuming the ideal drive.

``ideal``       the rows under which the plant realises the command exactly, at once
``rows``        rows from keywords, scalars or one value per vehicle
``DriveDist``   a distribution per field, sampled on the device from one seed
                (sharding-invariant through ``b_offset``, as the plant truth is)
``from_table``  rows gathered from a table of K candidates, for discrete studies
``validate``    host-side check of a drive before a rollout
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as LB

NP = LB.DRIVE_NP
FIELDS = LB.DRIVE_FIELDS
IDEAL_ROW = (0.0, 1.0, 0.0, math.inf, math.inf, 0.0)
MIN_TAU_STEPS = 8      # validate: 0 < tau_a < 8 h_max is refused (include/scpqp_drive.h, Accuracy)


def _field_index(field):
    if isinstance(field, str):
        if field not in FIELDS:
            raise ValueError(f"unknown drive field {field!r}: one of {FIELDS}")
        return FIELDS.index(field)
    f = int(field)
    if not 0 <= f < NP:
        raise ValueError(f"drive field index {f} out of range")
    return f


def _host(drive):
    return drive.detach().cpu().numpy() if isinstance(drive, torch.Tensor) \
        else np.asarray(drive, float)


def ideal_rows(n_veh):
    """The ideal rows [nVeh, 6] on the host: (0, 1, 0, +inf, +inf, 0)."""
    return np.broadcast_to(np.array(IDEAL_ROW), (int(n_veh), NP)).copy()


def ideal(B, n_veh, device=None):
    """[B, nVeh, 6]: the drive under which the plant realises the command exactly
    (scpqp_drive_fill_ideal)."""
    from .plant import _ptr, _stream
    device = torch.device(device or "cuda")
    lib = LB.load()
    out = torch.empty((int(B), int(n_veh), NP), dtype=torch.float64, device=device)
    LB.check(lib.scpqp_drive_fill_ideal(int(n_veh), int(B), _ptr(out), _stream(device)), lib)
    return out


def is_ideal(drive):
    """True when every row is the ideal row: the rollout then allocates and launches nothing."""
    return bool((_host(drive) == np.array(IDEAL_ROW)).all())


def rows(B, n_veh, tau=0.0, gain=1.0, bias=0.0, a_max=math.inf, b_max=math.inf, hold=0,
         device=None):
    """[B, nVeh, 6] with every realisation holding the same rows; each keyword is a scalar or
    one value per vehicle."""
    r = np.empty((int(n_veh), NP))
    for f, val in enumerate((tau, gain, bias, a_max, b_max, hold)):
        r[:, f] = np.broadcast_to(np.asarray(val, float), (int(n_veh),))
    out = np.broadcast_to(r[None], (int(B), int(n_veh), NP)).copy()
    return torch.as_tensor(out, dtype=torch.float64, device=torch.device(device or "cuda"))


class DriveDist:
    """A distribution of drive rows.  Every field starts FIXED at its ideal value; ``uniform``
    / ``normal`` / ``fixed`` set one field.  ``sample(B)`` draws on the device: field f of
    realisation b, vehicle v, comes from one Philox call of counter
    (f, 0, (9 << 24) | v, b_offset + b), so a batch split over calls or ranks (``b_offset`` =
    global index of the call's first realisation) samples what one call would.  ``hold`` stays
    FIXED at 0 or 1, and a drawn field needs a finite mean: fix it first
    (``d.fixed("b_max", 3.0).uniform("b_max", 1.0, lo=1.5)``)."""

    def __init__(self, n_veh, seed, b_offset=0):
        self.n_veh = int(n_veh)
        if not 1 <= self.n_veh <= LB.MAX_VEH:
            raise ValueError("need 1..16 vehicles")
        self.mean = ideal_rows(self.n_veh).T.copy()          # [6, nVeh]
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
        name = FIELDS[f]
        if f == LB.DRIVE_HOLD:
            raise ValueError("drive field hold: must be fixed at 0 or 1")
        spread = float(spread)
        if not (0.0 <= spread < math.inf):
            raise ValueError(f"drive field {name}: spread must be finite and >= 0")
        lo = -math.inf if lo is None else float(lo)
        hi = math.inf if hi is None else float(hi)
        if not lo <= hi:
            raise ValueError(f"drive field {name}: lo must be <= hi")
        if not np.isfinite(self.mean[f]).all():
            raise ValueError(f"drive field {name}: a drawn field needs a finite mean "
                             f"(fixed({name!r}, value) first)")
        if f in (LB.DRIVE_TAU_A, LB.DRIVE_A_MAX, LB.DRIVE_B_MAX) and not lo >= 0.0:
            raise ValueError(f"drive field {name}: the smallest value must be >= 0 (lo=)")
        if f in (LB.DRIVE_GAIN_A, LB.DRIVE_BIAS_A) and (lo == math.inf or hi == -math.inf):
            raise ValueError(f"drive field {name}: must stay finite")
        self.kind[f], self.spread[f], self.lo[f], self.hi[f] = kind, spread, lo, hi
        return self

    def uniform(self, field, spread, lo=None, hi=None):
        """mean + spread * xi, xi uniform in [-1, 1), clamped to [lo, hi]."""
        return self._set(field, LB.TRUTH_UNIFORM, spread, lo, hi)

    def normal(self, field, spread, lo=None, hi=None):
        """mean + spread * z, z standard normal, clamped to [lo, hi]."""
        return self._set(field, LB.TRUTH_NORMAL, spread, lo, hi)

    def fixed(self, field, value):
        """The same value for every realisation (a scalar, or one per vehicle)."""
        f = _field_index(field)
        val = np.broadcast_to(np.asarray(value, float), (self.n_veh,))
        probe = ideal_rows(self.n_veh)[None]
        probe[0, :, f] = val
        _check_rows(probe, "fixed")
        self.mean[f, :] = val
        self.kind[f], self.spread[f], self.lo[f], self.hi[f] = LB.TRUTH_FIXED, 0.0, -math.inf, math.inf
        return self

    def with_offset(self, b_offset):
        """The same distribution for the shard whose first realisation is ``b_offset``."""
        d = DriveDist.__new__(DriveDist)
        d.__dict__.update(self.__dict__)
        d.mean = self.mean.copy()
        d.kind, d.spread, d.lo, d.hi = list(self.kind), list(self.spread), list(self.lo), list(self.hi)
        d.b_offset = int(b_offset)
        if not 0 <= d.b_offset < 2 ** 32:
            raise ValueError("b_offset must be in [0, 2**32)")
        return d

    def c_struct(self):
        d = LB.DriveDist()
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
        """[B, nVeh, 6] on the device (scpqp_drive_sample)."""
        from .plant import _ptr, _stream
        device = torch.device(device or "cuda")
        lib = LB.load()
        out = torch.empty((int(B), self.n_veh, NP), dtype=torch.float64, device=device)
        d = self.c_struct()
        LB.check(lib.scpqp_drive_sample(C.byref(d), int(B), _ptr(out), _stream(device)), lib)
        return out


def from_table(rows, index, device=None):
    """rows [K, nVeh, 6], index [B] -> the drive [B, nVeh, 6] with realisation b holding
    rows[index[b]] (a discrete study: K candidate drives)."""
    device = torch.device(device or (rows.device if isinstance(rows, torch.Tensor) else "cuda"))
    rows = torch.as_tensor(rows, dtype=torch.float64, device=device)
    if rows.dim() != 3 or rows.shape[2] != NP:
        raise ValueError("rows must be [K, nVeh, 6]")
    idx = torch.as_tensor(index, device=device).reshape(-1).long()
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= rows.shape[0]):
        raise ValueError("index outside the table")
    return rows[idx].contiguous()


def _check_rows(t, what="drive"):
    """The row part of the header's bad rule, as a ValueError naming the first bad row."""
    def first(mask):
        bad = np.argwhere(mask)
        return None if not len(bad) else tuple(int(i) for i in bad[0])

    for f, name in ((LB.DRIVE_TAU_A, "tau_a"), (LB.DRIVE_A_MAX, "a_max"), (LB.DRIVE_B_MAX, "b_max")):
        at = first(~(t[..., f] >= 0.0))
        if at is not None:
            raise ValueError(f"{what}[{at[0]}, {at[1]}]: {name} must be >= 0")
    for f, name in ((LB.DRIVE_GAIN_A, "gain_a"), (LB.DRIVE_BIAS_A, "bias_a")):
        at = first(~np.isfinite(t[..., f]))
        if at is not None:
            raise ValueError(f"{what}[{at[0]}, {at[1]}]: {name} is not finite")
    at = first(~((t[..., LB.DRIVE_HOLD] == 0.0) | (t[..., LB.DRIVE_HOLD] == 1.0)))
    if at is not None:
        raise ValueError(f"{what}[{at[0]}, {at[1]}]: hold must be 0 or 1")


def validate(drive, h_max):
    """ValueError on a drive the plant would turn into NaN, or integrate too coarsely: a bad
    row of include/scpqp_drive.h (tau_a, a_max or b_max not >= 0, a non-finite gain_a or
    bias_a, hold neither 0 nor 1), a tau_a that is not finite, or 0 < tau_a < 8 h_max (the
    fixed-step RK4's error grows with h_max / tau_a).  Host side: one copy of the array."""
    t = _host(drive)
    if t.ndim != 3 or t.shape[2] != NP:
        raise ValueError("drive must be [B, nVeh, 6]")
    _check_rows(t)
    tau = t[..., LB.DRIVE_TAU_A]
    bad = np.argwhere(~np.isfinite(tau))
    if len(bad):
        raise ValueError(f"drive[{bad[0][0]}, {bad[0][1]}]: tau_a is not finite")
    bad = np.argwhere((tau > 0.0) & (tau < MIN_TAU_STEPS * float(h_max)))
    if len(bad):
        raise ValueError(f"drive[{bad[0][0]}, {bad[0][1]}]: tau_a = {tau[bad[0][0], bad[0][1]]:g} "
                         f"is below 8 * h_max = {MIN_TAU_STEPS * float(h_max):g}: lower h_max")
