"""Chance-constrained obstacle margins: the trackers' covariances, pushed through the horizon
the planner is told, as a safety margin per (realisation, obstacle, horizon step)
(include/scpqp_margin.h; csrc/margin.hip).

The margin is ``min(kappa * sqrt(lam), m_max)`` with ``lam`` the larger eigenvalue of the
second moment of the obstacle's predicted position about the told point: twelve sigma states
per mode through the mode's own horizon, plus ``tau Q_POS^2``, plus the spread between the
modes' points.  ``Solver.solve(..., obst_margin=)`` adds it to the obstacle safety distance;
``ClosedLoopBatch.reset(..., margin=(kappa, m_max))`` runs it after every tracker step.

``kappa_for``  the kappa of a miss probability: ``sqrt(-2 ln p_miss)``
``alloc``      the output arrays of ``step``
``validate``   host-side check of ``kappa`` and ``m_max``
``step``       the margins of every lane (scpqp_obstacles_margin)
"""
from __future__ import annotations

import math

import torch

from . import _lib as LB
from . import tracker_accel as TRKA

NP = LB.TRKA_NP
NS = LB.TRKA_NS
MAX_MODES = LB.IMM_MAX_MODES

_gpu = TRKA._gpu


def kappa_for(p_miss):
    """The kappa at which a two-dimensional Gaussian lies farther than ``kappa`` sigmas of its
    larger principal axis from its mean with probability at most ``p_miss``."""
    p = float(p_miss)
    if not 0.0 < p <= 1.0:
        raise ValueError("p_miss must lie in (0, 1]")
    return math.sqrt(-2.0 * math.log(p))


def validate(kappa, m_max):
    """ValueError unless ``kappa`` and ``m_max`` are finite and >= 0; returns them as floats."""
    kappa, m_max = float(kappa), float(m_max)
    if not (math.isfinite(kappa) and kappa >= 0.0):
        raise ValueError("kappa must be finite and >= 0")
    if not (math.isfinite(m_max) and m_max >= 0.0):
        raise ValueError("m_max must be finite and >= 0")
    return kappa, m_max


def alloc(B, n_obst, hp, device=None):
    """(margin [B, nObst, hp], sigma [B, nObst, hp, 3]) of zeros."""
    TRKA._need_obstacles(int(n_obst))
    f = dict(dtype=torch.float64, device=torch.device(device or "cuda"))
    return (torch.zeros((int(B), int(n_obst), int(hp)), **f),
            torch.zeros((int(B), int(n_obst), int(hp), 3), **f))


def step(trk, x, cov, mu, lead, dt, hp, kappa, m_max, sigma=False, out=None):
    """The margins of every lane (scpqp_obstacles_margin), after the tracker step of the same
    MPC step and with its ``lead``, ``dt`` and ``hp``.  Either the arrays of
    ``tracker_accel.step`` (``trk`` [B, nObst, 14], ``x`` [B, nObst, 6], ``cov``
    [B, nObst, 6, 6], ``mu`` None) or those of ``imm.step`` (``trk`` [B, nObst, M, 14], ``x``
    [B, nObst, M, 6], ``cov`` [B, nObst, M, 6, 6], ``mu`` [B, nObst, M]; ``mu`` None needs
    M = 1).  Nothing of the state is written.  Returns ``margin`` [B, nObst, hp], or
    ``(margin, Sigma [B, nObst, hp, 3] = Sxx, Sxy, Syy)`` with ``sigma=True``; ``out``: the
    margin tensor to write into.  Device tensors."""
    from .plant import _ptr, _stream
    kappa, m_max = validate(kappa, m_max)
    if not isinstance(trk, torch.Tensor) or trk.dim() not in (3, 4):
        raise ValueError("trk must be a [B, nObst, 14] or [B, nObst, M, 14] tensor")
    B, nO = int(trk.shape[0]), int(trk.shape[1])
    M = int(trk.shape[2]) if trk.dim() == 4 else 1
    TRKA._need_obstacles(nO)
    if not 1 <= M <= MAX_MODES:
        raise ValueError(f"a bank holds 1..{MAX_MODES} modes, got {M}")
    lead4 = (B, nO, M) if trk.dim() == 4 else (B, nO)
    trk = _gpu(trk, "trk", lead4 + (NP,))
    x = _gpu(x, "x", lead4 + (NS,))
    cov = _gpu(cov, "cov", lead4 + (NS, NS))
    if mu is not None:
        mu = _gpu(mu, "mu", (B, nO, M))
    elif M != 1:
        raise ValueError("mu may be None only with one mode")
    hp = int(hp)
    f = dict(dtype=torch.float64, device=trk.device)
    margin = torch.empty((B, nO, hp), **f) if out is None else _gpu(out, "out", (B, nO, hp))
    sig = torch.empty((B, nO, hp, 3), **f) if sigma else None
    lib = LB.load()
    LB.check(lib.scpqp_obstacles_margin(B, nO, hp, M, _ptr(trk), _ptr(x), _ptr(cov), _ptr(mu),
                                        float(lead), float(dt), kappa, m_max, _ptr(margin),
                                        _ptr(sig), _stream(trk.device)), lib)
    return (margin, sig) if sigma else margin
