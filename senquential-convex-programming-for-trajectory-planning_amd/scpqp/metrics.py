"""Realised-path metrics of closed-loop rollouts, accumulated on the GPU step by step
(csrc/metrics.hip, include/scpqp_metrics.h).

``PathMetrics``  the footprint gap between vehicles and to the obstacles (the rectangles
                 the reference draws: plotOnline.py:91-101, :120-132), collisions, the
                 margin to the planner's ``dsafe`` and the cross-track error to the
                 reference polylines, along the path the plant really drove at tick
                 resolution.  It holds O(B * nVeh) state for a whole run: no kept paths.
``summarize_by_variant``  the same per scenario variant of a sweep.
``summarize``    batch summary of one or several result dicts as plain Python numbers
                 (collision rate with its Wilson 95 % interval, clearance quantiles,
                 cross-track RMS and maximum).

There is no CPU path: without the HIP library or a GPU ``PathMetrics`` raises.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as LB

_INT_FIELDS = ("argmin_gap_veh", "argmin_gap_obs", "first_collision_tick", "n_collision_ticks",
               "n_ticks_seen")
QUANTILES = (0.01, 0.05, 0.5)
WILSON_Z = 1.959963984540054      # the 97.5 % point of the normal distribution


def pack_params(scenario):
    """``scpqp_metrics_params`` of a scenario and the arrays its pointers refer to (keep
    them alive until create has copied them).  The polylines are packed as
    ``ScpQpSolver`` packs them for ``scpqp_params``."""
    nV, nO = int(scenario.nVeh), int(scenario.nObst)
    keep = []

    def arr(x, shape=None, dtype=np.float64):
        a = np.ascontiguousarray(np.asarray(x, dtype=dtype).reshape(shape if shape else -1))
        keep.append(a)
        return a

    def dptr(a):
        return a.ctypes.data_as(C.POINTER(C.c_double))

    length, width = arr(scenario.Length), arr(scenario.Width)
    if len(length) != nV or len(width) != nV:
        raise ValueError("scenario.Length and scenario.Width need one entry per vehicle")
    dv = arr(scenario.dsafeVehicles, (nV * nV,))
    do = arr(scenario.dsafeObstacles, (nV * nO,)) if nO else None
    ob = arr(np.asarray(scenario.obstacles, float).reshape(nO, -1)[:, :6], (nO * 6,)) if nO else None
    refs = [np.asarray(t, float).reshape(-1, 2) for t in scenario.referenceTrajectories]
    mp = max(2, max(len(t) for t in refs))
    if mp > LB.MAX_REFPTS:
        raise ValueError("reference polyline has too many points")
    poly = np.zeros((nV, mp, 2))
    npts = np.zeros(nV, np.int32)
    for v, t in enumerate(refs):
        poly[v, :len(t)] = t
        npts[v] = len(t)
    poly = arr(poly)
    npts = arr(npts, dtype=np.int32)
    P = LB.MetricsParams(n_veh=nV, n_obst=nO, ref_max_pts=mp, pad0=0,
                         tick_length=float(scenario.tick_length), length=dptr(length),
                         width=dptr(width), dsafe_veh=dptr(dv),
                         dsafe_obs=dptr(do) if nO else None, obstacles=dptr(ob) if nO else None,
                         ref_polyline=dptr(poly),
                         ref_npts=npts.ctypes.data_as(C.POINTER(C.c_int32)))
    return P, keep


class PathMetrics:
    """Scenario-bound accumulator of realised-path metrics for up to ``max_batch``
    realisations on one GPU."""

    def __init__(self, scenario, max_batch, device=None, variants=None):
        if not torch.cuda.is_available():
            raise RuntimeError("scpqp: no GPU visible; the HIP path has no CPU fallback")
        self.lib = LB.load()
        self.device = torch.device(device or "cuda")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.nV, self.nO = int(scenario.nVeh), int(scenario.nObst)
        self.n_pair = self.nV * (self.nV - 1) // 2
        self.tick_length = float(scenario.tick_length)
        self.max_batch = int(max_batch)
        if self.max_batch < 1:
            raise ValueError("max_batch must be >= 1")
        P, keep = pack_params(scenario)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            LB.check(self.lib.scpqp_metrics_create(C.byref(P), self.device.index, C.byref(h)),
                     self.lib)
        del keep
        self.h = h
        M, f, i = self.max_batch, torch.float64, torch.int32
        shapes = dict(min_gap_veh=(M,), min_gap_obs=(M,), min_margin_veh=(M,), min_margin_obs=(M,),
                      argmin_gap_veh=(M, 3), argmin_gap_obs=(M, 3), first_collision_tick=(M,),
                      n_collision_ticks=(M,), n_ticks_seen=(M,), max_xtrack=(M, self.nV),
                      sum_sq_xtrack=(M, self.nV))
        self.acc = {k: torch.empty(s, dtype=i if k in _INT_FIELDS else f, device=self.device)
                    for k, s in shapes.items()}
        self._acc = LB.MetricsAcc(**{k: self.acc[k].data_ptr() for k in LB.METRICS_ACC_FIELDS})
        self.B = 0
        self.n_variants = 1
        if variants is not None:
            self.set_variants(variants)

    def set_variants(self, scenarios):
        """Install the scenarios as the handle's table of constants
        (``scpqp_metrics_set_variants``): realisation b of ``accumulate(..., variant=)`` is
        measured against ``scenarios[variant[b]]``.  Footprints, dsafe tables, obstacles and
        polylines may differ; nVeh, nObst and tick_length are the handle's."""
        scenarios = list(scenarios)
        if not scenarios:
            raise ValueError("set_variants needs at least one scenario")
        packed = [pack_params(sc) for sc in scenarios]
        table = (LB.MetricsParams * len(packed))(*[P for P, _ in packed])
        with torch.cuda.device(self.device):
            LB.check(self.lib.scpqp_metrics_set_variants(self.h, len(packed), table), self.lib)
        del packed
        self.n_variants = len(scenarios)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def reset(self, B=None):
        """Reset the accumulator of the first ``B`` realisations (default max_batch)."""
        B = self.max_batch if B is None else int(B)
        if not 0 <= B <= self.max_batch:
            raise ValueError("B must be in 0..max_batch")
        self.B = B
        LB.check(self.lib.scpqp_metrics_reset(self.h, B, C.byref(self._acc), self._stream()),
                 self.lib)

    def accumulate(self, x_path, tick0, k_first, dense=False, variant=None, obstacles=None,
                   manoeuvres=None, check_off=True):
        """Merge one step's path ``x_path`` [B, nVeh, K, 6] (a float64 device tensor, the
        output of ``plant.plant_step``; entry k is global tick ``tick0 + k``) over its
        entries ``k_first..K-1``.  ``dense=True`` also returns this call's ``gap_veh``
        [B, K, n_pair], ``gap_obs`` [B, K, nVeh, nObst] and ``xtrack`` [B, K, nVeh], over
        every entry; ``dense="only"`` returns them and leaves the accumulator alone.
        ``variant`` [B] int: realisation b is measured against entry ``variant[b]`` of the
        table of ``set_variants`` (None: entry 0); with an index outside the table the
        realisation's accumulator and dense rows are left as they are.
        ``obstacles`` [B, nObst, 7] (scpqp/obstacles.py; include/scpqp_obstacles.h): obstacle
        o of realisation b moves and is sized by its own row instead of the scenario's
        constant obstacle; a realisation with a bad row is left as it is.
        ``manoeuvres`` [B, nObst, 4, 3] (scpqp/manoeuvres.py; include/scpqp_manoeuvres.h), with
        ``obstacles=``: the obstacles follow their schedules.  Their poses at the call's ticks
        are computed first (``manoeuvres.pose``) and the gaps are measured against them
        (scpqp_metrics_accumulate_posed); a realisation with a bad lane is left as it is.
        ``check_off`` (default True): the schedule is first checked on the host
        (``manoeuvres.is_off``: one device-to-host copy and a synchronisation), and one in which
        no piece does anything takes the ``obstacles=`` path.  ``check_off=False`` skips the
        check and sends the schedule through the posed entry as it is: for a caller that has
        already made the check (the rollout makes it once, at reset)."""
        if x_path.dtype != torch.float64 or x_path.device != self.device or x_path.dim() != 4:
            raise ValueError("x_path must be a float64 [B, nVeh, K, 6] tensor on the metrics' device")
        B, V, K, nx = (int(s) for s in x_path.shape)
        if V != self.nV or nx != 6 or K < 1:
            raise ValueError("x_path must be [B, nVeh, K, 6]")
        if dense != "only" and B != self.B:
            raise ValueError(f"x_path holds {B} realisations, reset() was called for {self.B}")
        x = x_path.contiguous()
        var = None
        if variant is not None:
            var = torch.as_tensor(variant, device=self.device).to(torch.int32).contiguous()
            if var.numel() != B:
                raise ValueError(f"variant [B]: expected {B} elements, got {var.numel()}")
        out, D = None, None
        if dense:
            f = dict(dtype=torch.float64, device=self.device)
            out = dict(gap_veh=torch.empty((B, K, self.n_pair), **f),
                       gap_obs=torch.empty((B, K, V, self.nO), **f),
                       xtrack=torch.empty((B, K, V), **f))
            D = LB.MetricsDense(gap_veh=out["gap_veh"].data_ptr() if self.n_pair else None,
                                gap_obs=out["gap_obs"].data_ptr() if self.nO else None,
                                xtrack=out["xtrack"].data_ptr())
        acc = None if dense == "only" else C.byref(self._acc)
        if manoeuvres is not None and obstacles is None:
            raise ValueError("manoeuvres needs obstacles= rows")
        posed = None
        if manoeuvres is not None:
            from . import manoeuvres as MAN
            if not isinstance(manoeuvres, torch.Tensor) or manoeuvres.dtype != torch.float64 \
                    or manoeuvres.device != self.device \
                    or tuple(manoeuvres.shape) != (B, self.nO, MAN.NSEG, MAN.NF):
                raise ValueError(f"manoeuvres must be a float64 [B, nObst, 4, 3] = [{B}, {self.nO}, "
                                 f"4, 3] tensor on the metrics' device")
            if not check_off or not MAN.is_off(manoeuvres):
                posed = manoeuvres.contiguous()
        if obstacles is not None:
            rows = obstacles
            if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float64 \
                    or rows.device != self.device:
                raise ValueError("obstacles must be a float64 tensor on the metrics' device")
            if not self.nO:
                raise ValueError("obstacles given, but the scenario has no obstacles")
            if tuple(rows.shape) != (B, self.nO, LB.OBST_NP):
                raise ValueError(f"obstacles must be [B, nObst, 7] = [{B}, {self.nO}, 7], got "
                                 f"{list(rows.shape)}")
            rows = rows.contiguous()
            if posed is not None:
                p = MAN.pose(rows, posed, self.tick_length, int(tick0), K - 1)
                LB.check(self.lib.scpqp_metrics_accumulate_posed(
                    self.h, B, K - 1, int(tick0), int(k_first), C.c_void_p(x.data_ptr()), acc,
                    None if D is None else C.byref(D),
                    None if var is None else C.c_void_p(var.data_ptr()),
                    C.c_void_p(rows.data_ptr()), C.c_void_p(p.data_ptr()), self._stream()),
                    self.lib)
                self._last_variant, self._last_rows, self._last_pose = var, rows, p
                return out
            LB.check(self.lib.scpqp_metrics_accumulate_obstacles(
                self.h, B, K - 1, int(tick0), int(k_first), C.c_void_p(x.data_ptr()), acc,
                None if D is None else C.byref(D),
                None if var is None else C.c_void_p(var.data_ptr()),
                C.c_void_p(rows.data_ptr()), self._stream()), self.lib)
            self._last_variant, self._last_rows = var, rows   # alive until the stream has read them
        elif var is None:
            LB.check(self.lib.scpqp_metrics_accumulate(
                self.h, B, K - 1, int(tick0), int(k_first), C.c_void_p(x.data_ptr()), acc,
                None if D is None else C.byref(D), self._stream()), self.lib)
        else:
            LB.check(self.lib.scpqp_metrics_accumulate_variants(
                self.h, B, K - 1, int(tick0), int(k_first), C.c_void_p(x.data_ptr()), acc,
                None if D is None else C.byref(D), C.c_void_p(var.data_ptr()), self._stream()),
                self.lib)
            self._last_variant = var   # alive until the stream has consumed it
        return out

    def result(self):
        """The accumulator of the realisations of the last ``reset``: a dict of device
        tensors (copies; see include/scpqp_metrics.h for the fields)."""
        return {k: t[:self.B].clone() for k, t in self.acc.items()}

    def close(self):
        if getattr(self, "h", None):
            self.lib.scpqp_metrics_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def wilson_interval(k, n, z=WILSON_Z):
    """Wilson score interval of a proportion k / n (Wilson 1927)."""
    if n <= 0:
        return (0.0, 1.0)
    p = k / n
    den = 1.0 + z * z / n
    mid = (p + z * z / (2 * n)) / den
    half = z * math.sqrt(p * (1 - p) / n + z * z / (4.0 * n * n)) / den
    return (max(0.0, mid - half), min(1.0, mid + half))


def _quantiles(x):
    out = {"min": float(x.min())}
    for q in QUANTILES:
        out["q%02d" % round(q * 100)] = float(np.quantile(x, q))
    return out


def summarize(results):
    """Batch summary of one result dict (``PathMetrics.result()``) or a list of them (one
    per rank; they are concatenated), as plain Python numbers."""
    if isinstance(results, dict):
        results = [results]
    if not results:
        raise ValueError("no results")

    def cat(k):
        return np.concatenate([np.asarray(r[k].cpu() if hasattr(r[k], "cpu") else r[k])
                               for r in results], axis=0)

    first = cat("first_collision_tick")
    n = int(first.shape[0])
    if n == 0:
        raise ValueError("no realisations")
    n_coll = int((first >= 0).sum())
    lo, hi = wilson_interval(n_coll, n)
    gap_veh, margin_veh = cat("min_gap_veh"), cat("min_margin_veh")
    gap_obs, margin_obs = cat("min_gap_obs"), cat("min_margin_obs")
    # a single vehicle has no pair, a scenario without obstacles no obstacle gap: None
    have_veh, have_obs = bool(np.isfinite(gap_veh).any()), bool(np.isfinite(gap_obs).any())
    seen = cat("n_ticks_seen").astype(np.float64)
    ssq, xmax = cat("sum_sq_xtrack"), cat("max_xtrack")
    ticks = float(seen.sum()) * ssq.shape[1]
    out = {
        "n_realisations": n,
        "n_collisions": n_coll,
        "collision_rate": n_coll / n,
        "collision_rate_wilson95": [lo, hi],
        "min_gap_veh": _quantiles(gap_veh) if have_veh else None,
        "min_gap_obs": _quantiles(gap_obs) if have_obs else None,
        "frac_margin_veh_below_0": float((margin_veh < 0).mean()) if have_veh else None,
        "frac_margin_obs_below_0": float((margin_obs < 0).mean()) if have_obs else None,
        "xtrack_rms": math.sqrt(float(ssq.sum()) / ticks) if ticks > 0 else 0.0,
        "xtrack_max": float(xmax.max()),
    }
    return out


def summarize_by_variant(results, variant_of):
    """``{variant: summarize(...)}`` over the realisations of each variant.  ``results``: one
    result dict or a list of them (concatenated, as ``summarize`` does); ``variant_of``: the
    variant index of every realisation, in the same order."""
    if isinstance(results, dict):
        results = [results]
    if not results:
        raise ValueError("no results")
    var = np.asarray(variant_of.cpu() if hasattr(variant_of, "cpu") else variant_of).reshape(-1)
    merged = {k: np.concatenate([np.asarray(r[k].cpu() if hasattr(r[k], "cpu") else r[k])
                                 for r in results], axis=0) for k in results[0]}
    n = int(merged["first_collision_tick"].shape[0])
    if var.shape[0] != n:
        raise ValueError(f"variant_of holds {var.shape[0]} entries for {n} realisations")
    return {int(k): summarize({f: a[var == k] for f, a in merged.items()})
            for k in np.unique(var)}
