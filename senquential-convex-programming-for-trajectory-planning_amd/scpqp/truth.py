"""Plant truth: per-(realisation, vehicle) plant parameters the controller does not know
(include/scpqp_truth.h).

A truth is a float64 tensor ``[B, nVeh, 5]`` of rows ``(lf, lr, tau, gain, bias)``: the
axle distances, the steering lag and the steering gain and offset of the vehicle that
realises the path (``plant_step(..., truth=)``, ``ClosedLoopBatch.reset(..., truth=)``).
The controller keeps the scenario's nominal model (main.py:121-123).

``nominal``     the rows that reproduce the nominal plant bitwise
``TruthDist``   a distribution per field, sampled on the device from one seed
                (sharding-invariant through ``b_offset``, as the model noise is)
``from_table``  rows gathered from a table of K candidates, for discrete studies
``validate``    host-side check of a truth before a rollout
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as LB

NP = LB.TRUTH_NP
FIELDS = LB.TRUTH_FIELDS
TAU_NOMINAL = LB.TRUTH_TAU_NOMINAL
MIN_TAU_STEPS = 8      # validate: tau >= 8 h_max keeps the fixed-step RK4 within ~5e-8


def _params_of(scenario_or_params):
    if isinstance(scenario_or_params, LB.PlantParams):
        return scenario_or_params
    from .plant import plant_params
    return plant_params(scenario_or_params.Lf, scenario_or_params.Lr)


def _field_index(field):
    if isinstance(field, str):
        if field not in FIELDS:
            raise ValueError(f"unknown truth field {field!r}: one of {FIELDS}")
        return FIELDS.index(field)
    f = int(field)
    if not 0 <= f < NP:
        raise ValueError(f"truth field index {f} out of range")
    return f


def nominal_rows(scenario_or_params):
    """The nominal rows [nVeh, 5] on the host: (Lf[v], Lr[v], 0.1, 1, 0)."""
    p = _params_of(scenario_or_params)
    rows = np.zeros((p.n_veh, NP))
    rows[:, LB.TRUTH_LF] = [p.lf[v] for v in range(p.n_veh)]
    rows[:, LB.TRUTH_LR] = [p.lr[v] for v in range(p.n_veh)]
    rows[:, LB.TRUTH_TAU] = TAU_NOMINAL
    rows[:, LB.TRUTH_GAIN] = 1.0
    return rows


def nominal(scenario_or_params, B, device=None):
    """[B, nVeh, 5]: the truth under which the plant is the controller's own model
    (scpqp_truth_fill_nominal)."""
    from .plant import _ptr, _stream
    p = _params_of(scenario_or_params)
    device = torch.device(device or "cuda")
    lib = LB.load()
    out = torch.empty((int(B), p.n_veh, NP), dtype=torch.float64, device=device)
    LB.check(lib.scpqp_truth_fill_nominal(C.byref(p), int(B), _ptr(out), _stream(device)), lib)
    return out


class TruthDist:
    """A distribution of truth rows around the scenario's nominal model.  Every field
    starts FIXED at its nominal value; ``uniform`` / ``normal`` / ``fixed`` set one field,
    ``relative`` the usual robustness study.  ``sample(B)`` draws on the device: field f of
    realisation b, vehicle v, comes from one Philox call of counter
    (f, 0, (3 << 24) | v, b_offset + b), so a batch split over calls or ranks
    (``b_offset`` = global index of the call's first realisation) samples what one call
    would."""

    def __init__(self, scenario, seed, b_offset=0):
        self.mean = nominal_rows(scenario).T.copy()          # [5, nVeh]
        self.n_veh = self.mean.shape[1]
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
            raise ValueError(f"truth field {FIELDS[f]}: spread must be finite and >= 0")
        lo = -math.inf if lo is None else float(lo)
        hi = math.inf if hi is None else float(hi)
        if not lo <= hi:
            raise ValueError(f"truth field {FIELDS[f]}: lo must be <= hi")
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
        self.mean[f, :] = np.broadcast_to(np.asarray(value, float), (self.n_veh,))
        self.kind[f], self.spread[f], self.lo[f], self.hi[f] = LB.TRUTH_FIXED, 0.0, -math.inf, math.inf
        return self

    def relative(self, pct):
        """Uniform +-pct % of nominal on lf, lr, tau and gain, clamped to that range.  lf
        and lr are per vehicle, so their spread and clamp are those of the vehicle with the
        largest nominal value; with equal vehicles every one gets exactly +-pct %."""
        r = float(pct) / 100.0
        if not 0.0 <= r < 1.0:
            raise ValueError("pct must be in [0, 100)")
        for name in ("lf", "lr", "tau", "gain"):
            m = self.mean[FIELDS.index(name)]
            self.uniform(name, r * float(m.max()), float(m.min()) * (1.0 - r),
                         float(m.max()) * (1.0 + r))
        return self

    def with_offset(self, b_offset):
        """The same distribution for the shard whose first realisation is ``b_offset``."""
        d = TruthDist.__new__(TruthDist)
        d.__dict__.update(self.__dict__)
        d.mean = self.mean.copy()
        d.kind, d.spread, d.lo, d.hi = list(self.kind), list(self.spread), list(self.lo), list(self.hi)
        d.b_offset = int(b_offset)
        return d

    def c_struct(self):
        d = LB.TruthDist()
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
        """[B, nVeh, 5] on the device (scpqp_truth_sample)."""
        from .plant import _ptr, _stream
        device = torch.device(device or "cuda")
        lib = LB.load()
        out = torch.empty((int(B), self.n_veh, NP), dtype=torch.float64, device=device)
        d = self.c_struct()
        LB.check(lib.scpqp_truth_sample(C.byref(d), int(B), _ptr(out), _stream(device)), lib)
        return out


def from_table(rows, index, device=None):
    """rows [K, nVeh, 5], index [B] -> the truth [B, nVeh, 5] with realisation b holding
    rows[index[b]] (a discrete study: K candidate vehicles)."""
    device = torch.device(device or (rows.device if isinstance(rows, torch.Tensor) else "cuda"))
    rows = torch.as_tensor(rows, dtype=torch.float64, device=device)
    if rows.dim() != 3 or rows.shape[2] != NP:
        raise ValueError("rows must be [K, nVeh, 5]")
    idx = torch.as_tensor(index, device=device).reshape(-1).long()
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= rows.shape[0]):
        raise ValueError("index outside the table")
    return rows[idx].contiguous()


def validate(truth, h_max):
    """ValueError on a truth the plant would turn into NaN, or integrate too coarsely: a
    non-finite entry, lf + lr <= 0, tau <= 0, or tau < 8 h_max (the fixed-step RK4's error
    grows with h_max / tau: DESIGN §7, "Plant truth").  Host side: one copy of the array."""
    t = truth.detach().cpu().numpy() if isinstance(truth, torch.Tensor) else np.asarray(truth, float)
    if t.ndim != 3 or t.shape[2] != NP:
        raise ValueError("truth must be [B, nVeh, 5]")
    if not np.isfinite(t).all():
        b, v, f = np.argwhere(~np.isfinite(t))[0]
        raise ValueError(f"truth[{b}, {v}]: {FIELDS[f]} is not finite")
    bad = np.argwhere(~(t[..., LB.TRUTH_LF] + t[..., LB.TRUTH_LR] > 0.0))
    if len(bad):
        raise ValueError(f"truth[{bad[0][0]}, {bad[0][1]}]: lf + lr must be > 0")
    bad = np.argwhere(~(t[..., LB.TRUTH_TAU] > 0.0))
    if len(bad):
        raise ValueError(f"truth[{bad[0][0]}, {bad[0][1]}]: tau must be > 0")
    bad = np.argwhere(t[..., LB.TRUTH_TAU] < MIN_TAU_STEPS * float(h_max))
    if len(bad):
        raise ValueError(f"truth[{bad[0][0]}, {bad[0][1]}]: tau = {t[bad[0][0], bad[0][1], 2]:g} "
                         f"is below 8 * h_max = {MIN_TAU_STEPS * float(h_max):g}: lower h_max")
