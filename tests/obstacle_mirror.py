"""CPU mirror of the obstacle truth (include/scpqp_obstacles.h), for the obstacle tests: the
pose of a row at time t, the controller's prediction, the sampler on the mirror's Philox
(tests/noise_mirror.py) and the metrics mirror's constants with the obstacles posed by a
realisation's rows (a subclass of ``metrics_mirror.Constants``).  Plain fp64, one rounding
per operation; written from the header's description, not from the device code."""
import math

import numpy as np

import metrics_mirror as MM
import noise_mirror as NM

NP = 7
X, Y, HEADING, SPEED, LENGTH, WIDTH, YAW_RATE = range(NP)
FIXED, UNIFORM, NORMAL = 0, 1, 2
SITE_OBSTACLE = 4
SINC_SWITCH = 1e-4


def nominal_rows(sc):
    rows = np.zeros((sc.nObst, NP))
    for o, ob in enumerate(sc.obstacles):
        rows[o, :6] = np.asarray(ob, float)[:6]
    return rows


def bad_row(row):
    row = np.asarray(row, float)
    return bool((~np.isfinite(row)).any() or row[LENGTH] < 0.0 or row[WIDTH] < 0.0)


def sinc(a):
    return 1.0 - a * a / 6.0 if abs(a) < SINC_SWITCH else math.sin(a) / a


def pose(row, t):
    """(x, y, heading) of the row at time t."""
    x, y, h, s, w = (float(row[i]) for i in (X, Y, HEADING, SPEED, YAW_RATE))
    t = float(t)
    if w == 0.0:
        return (t * s * math.cos(h) + x, t * s * math.sin(h) + y, h)
    a = 0.5 * w * t
    chord = (s * t) * sinc(a)
    return (x + chord * math.cos(h + a), y + chord * math.sin(h + a), h + w * t)


def poses(rows, tick_length, tick0, n_ticks):
    """rows [B, nO, 7] -> [B, nO, n_ticks + 1, 3] at the global ticks tick0 .. tick0 + n_ticks;
    a bad row's block is NaN."""
    rows = np.asarray(rows, float)
    B, nO = rows.shape[:2]
    out = np.full((B, nO, n_ticks + 1, 3), np.nan)
    for b in range(B):
        for o in range(nO):
            if bad_row(rows[b, o]):
                continue
            for j in range(n_ticks + 1):
                out[b, o, j] = pose(rows[b, o], float(tick0 + j) * tick_length)
    return out


def predict(rows, t_meas, lead, dt, hp):
    """rows [B, nO, 7] -> [B, nO, 2, hp]: the straight line from the true pose at t_meas.
    ``lead``: the number the entry point takes, or the reference's terms (delay_x, dt,
    delay_u), which MPC_Iter.py:47 adds to (k + 1) dt one by one, left to right: the sum
    formed first can differ from that by an ulp of the step."""
    rows = np.asarray(rows, float)
    B, nO = rows.shape[:2]
    out = np.full((B, nO, 2, hp), np.nan)
    terms = tuple(float(x) for x in lead) if isinstance(lead, (tuple, list)) else (float(lead),)
    for b in range(B):
        for o in range(nO):
            if bad_row(rows[b, o]):
                continue
            x, y, h = pose(rows[b, o], t_meas)
            for k in range(hp):
                ahead = (k + 1) * dt
                for term in terms:
                    ahead = ahead + term
                step = ahead * float(rows[b, o, SPEED])
                out[b, o, 0, k] = step * math.cos(h) + x
                out[b, o, 1, k] = step * math.sin(h) + y
    return out


class Dist:
    """The fields of scpqp_obstacles_dist."""

    def __init__(self, mean, seed, b_offset=0):
        self.mean = np.array(mean, float)                   # [7, nObst]
        self.n_obst = self.mean.shape[1]
        self.seed, self.b_offset = seed, b_offset
        self.kind = [FIXED] * NP
        self.spread = [0.0] * NP
        self.lo = [-np.inf] * NP
        self.hi = [np.inf] * NP

    def set(self, f, kind, spread, lo=-np.inf, hi=np.inf):
        self.kind[f], self.spread[f], self.lo[f], self.hi[f] = kind, spread, lo, hi
        return self


def xi(dist, B):
    """[B, nO, 7] the unit draws (0 for a FIXED field) of realisations b_offset .. + B."""
    b, o, f = np.meshgrid(np.arange(B), np.arange(dist.n_obst), np.arange(NP), indexing="ij")
    seed = dist.seed
    w = NM.philox4x32_10((f, 0, (SITE_OBSTACLE << 24) | o, (dist.b_offset + b) & NM.MASK),
                         (seed & NM.MASK, (seed >> 32) & NM.MASK))
    u1, u2 = NM.uniforms(w)
    uni = 2.0 * u2 - 1.0
    nor = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    kind = np.array(dist.kind)[None, None, :]
    return np.where(kind == UNIFORM, uni, np.where(kind == NORMAL, nor, 0.0))


def sample(dist, B):
    """[B, nO, 7]: fmin(fmax(mean + spread * xi, lo), hi); a FIXED field is its mean."""
    x = xi(dist, B)
    mean = dist.mean.T[None]                                # [1, nO, 7]
    val = mean + np.array(dist.spread)[None, None, :] * x
    val = np.minimum(np.maximum(val, np.array(dist.lo)[None, None, :]),
                     np.array(dist.hi)[None, None, :])
    fixed = (np.array(dist.kind) == FIXED)[None, None, :]
    return np.where(fixed, np.broadcast_to(mean, val.shape), val)


class RowConstants(MM.Constants):
    """``metrics_mirror.Constants`` of one realisation whose obstacles are its rows [nO, 7]:
    the rectangle of obstacle o at a tick is centred at the row's pose, rotated by its
    heading there, and sized by the row."""

    def __init__(self, base, rows):
        self.__dict__.update(base.__dict__)
        self.rows = np.asarray(rows, float).reshape(-1, NP)
        assert len(self.rows) == self.nO

    def obstacle_rect(self, o, tick):
        r = self.rows[o]
        x, y, h = pose(r, float(tick) * self.tick_length)
        return (x, y, math.cos(h), math.sin(h), r[LENGTH] / 2, r[WIDTH] / 2)


def run(base, rows, calls, B):
    """``metrics_mirror.run`` with realisation b measured against rows[b]; a realisation with
    a bad row keeps its reset values.  Returns the accumulators with a leading B."""
    rows = np.asarray(rows, float)
    accs = [MM.new_acc(base.nV) for _ in range(B)]
    for x_path, tick0, k_first in calls:
        x = np.asarray(x_path, float)
        for b in range(B):
            if any(bad_row(r) for r in rows[b]):
                continue
            MM.accumulate(RowConstants(base, rows[b]), accs[b], x[b], tick0, k_first)
    out = {}
    for k in accs[0]:
        a = np.array([acc[k] for acc in accs])
        out[k] = a.astype(np.int32) if k.startswith(("argmin", "first", "n_")) else a.astype(float)
    return out
