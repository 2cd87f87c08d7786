"""CPU mirror of the obstacle manoeuvres (include/scpqp_manoeuvres.h), for the manoeuvre
tests: p and r (both branches), one piece, the state and the pose of a lane, the off and bad
rules, the sampler on the mirror's Philox (tests/noise_mirror.py) and the metrics mirror's
constants with the obstacles posed by it (a subclass of ``metrics_mirror.Constants``).  Plain
fp64, one rounding per operation; written from the header's description, not from the device
code.  An off lane is ``obstacle_mirror.pose`` and nothing else."""
import math

import numpy as np

import metrics_mirror as MM
import noise_mirror as NM
import obstacle_mirror as OM

NSEG, NF = 4, 3
DUR, ACCEL, DYAW = range(NF)
PR_SWITCH = 0.1
SITE_MANOEUVRE = 8
FIXED, UNIFORM, NORMAL = 0, 1, 2

P_COEF = (1.0 / 2.0, 1.0 / 8.0, 1.0 / 144.0, 1.0 / 5760.0, 1.0 / 403200.0, 1.0 / 43545600.0)
R_COEF = (1.0 / 3.0, 1.0 / 30.0, 1.0 / 840.0, 1.0 / 45360.0, 1.0 / 3991680.0, 1.0 / 518918400.0)


def _horner(coef, t2):
    acc = coef[-1]
    for c in coef[-2::-1]:
        acc = c - t2 * acc
    return acc


def p_series(th):
    return _horner(P_COEF, th * th)


def r_series(th):
    return th * _horner(R_COEF, th * th)


def p_closed(th):
    return (math.cos(th) + th * math.sin(th) - 1.0) / (th * th)


def r_closed(th):
    return (math.sin(th) - th * math.cos(th)) / (th * th)


def p_of(th):
    return p_series(th) if abs(th) < PR_SWITCH else p_closed(th)


def r_of(th):
    return r_series(th) if abs(th) < PR_SWITCH else r_closed(th)


def piece(q, a, w, tau):
    """(x, y, h, s) after a piece of acceleration a and turn rate w over tau >= 0; returns
    (x, y, h, s, w_in_effect)."""
    x, y, h, s = q
    if a < 0.0:
        stop = s / -a
    elif a == 0.0 and s == 0.0:
        stop = 0.0
    else:
        stop = math.inf
    stops = tau >= stop
    T = stop if stops else tau
    th = w * T
    A = 0.5 * th
    chord = (s * T) * OM.sinc(A)
    dx, dy = chord * math.cos(h + A), chord * math.sin(h + A)
    if a != 0.0:
        p, r, aT2 = p_of(th), r_of(th), a * (T * T)
        dx = dx + aT2 * (p * math.cos(h) - r * math.sin(h))
        dy = dy + aT2 * (p * math.sin(h) + r * math.cos(h))
    s1 = 0.0 if stops else max(s + a * T, 0.0)
    return (x + dx, y + dy, h + th, s1, 0.0 if (s1 == 0.0 and a <= 0.0) else w)


def bad_schedule(m):
    m = np.asarray(m, float).reshape(NSEG, NF)
    return bool((~np.isfinite(m)).any() or (m[:, DUR] < 0.0).any())


def off_schedule(m):
    m = np.asarray(m, float).reshape(NSEG, NF)
    return bool(((m[:, DUR] == 0.0) | ((m[:, ACCEL] == 0.0) & (m[:, DYAW] == 0.0))).all())


def lane_class(row, m):
    """0: a schedule to walk, 1: off, 2: bad."""
    if OM.bad_row(row):
        return 2
    if m is None:
        return 1
    if bad_schedule(m):
        return 2
    if off_schedule(m):
        return 1
    return 2 if float(row[OM.SPEED]) < 0.0 else 0


def walk(row, m, t):
    """(x, y, h, s, w) at t >= 0 of a row under a schedule that is neither off nor bad."""
    m = np.asarray(m, float).reshape(NSEG, NF)
    w0 = float(row[OM.YAW_RATE])
    q = (float(row[OM.X]), float(row[OM.Y]), float(row[OM.HEADING]), float(row[OM.SPEED]), w0)
    ti = 0.0
    for i in range(NSEG):
        dur = float(m[i, DUR])
        if dur == 0.0:
            continue
        if t < ti:
            return q
        q = piece(q[:4], float(m[i, ACCEL]), w0 + float(m[i, DYAW]), min(t - ti, dur))
        ti = ti + dur
    if t >= ti:
        q = piece(q[:4], 0.0, w0, t - ti)
    return q


def state_lane(row, m, t):
    """The snapshot row [7] of one lane at t; NaN for a bad lane."""
    row = np.asarray(row, float)
    cls = lane_class(row, m)
    if cls == 2:
        return np.full(OM.NP, np.nan)
    out = row.copy()
    if cls == 1:
        out[OM.X], out[OM.Y], out[OM.HEADING] = OM.pose(row, t)
        return out
    out[OM.X], out[OM.Y], out[OM.HEADING], out[OM.SPEED], out[OM.YAW_RATE] = walk(row, m, t)
    return out


def state(rows, man, t):
    """rows [B, nO, 7], man [B, nO, 4, 3] or None -> [B, nO, 7]."""
    rows = np.asarray(rows, float)
    B, nO = rows.shape[:2]
    out = np.empty((B, nO, OM.NP))
    for b in range(B):
        for o in range(nO):
            out[b, o] = state_lane(rows[b, o], None if man is None else man[b, o], float(t))
    return out


def poses(rows, man, tick_length, tick0, n_ticks):
    """-> [B, nO, n_ticks + 1, 3] at the global ticks tick0 .. tick0 + n_ticks; a bad lane's
    block is NaN, an off lane's is ``obstacle_mirror.poses``'."""
    rows = np.asarray(rows, float)
    B, nO = rows.shape[:2]
    out = OM.poses(rows, tick_length, tick0, n_ticks)
    if man is None:
        return out
    for b in range(B):
        for o in range(nO):
            cls = lane_class(rows[b, o], man[b, o])
            if cls == 1:
                continue
            for j in range(n_ticks + 1):
                out[b, o, j] = np.nan if cls == 2 else \
                    walk(rows[b, o], man[b, o], float(tick0 + j) * tick_length)[:3]
    return out


class Dist:
    """The fields of scpqp_manoeuvres_dist."""

    def __init__(self, n_obst, seed, b_offset=0):
        self.n_obst, self.seed, self.b_offset = n_obst, seed, b_offset
        self.mean = np.zeros((NSEG, NF))
        self.kind = np.full((NSEG, NF), FIXED)
        self.spread = np.zeros((NSEG, NF))
        self.lo = np.full((NSEG, NF), -np.inf)
        self.hi = np.full((NSEG, NF), np.inf)

    def set(self, i, f, kind, mean, spread=0.0, lo=-np.inf, hi=np.inf):
        self.kind[i, f], self.mean[i, f], self.spread[i, f] = kind, mean, spread
        self.lo[i, f], self.hi[i, f] = lo, hi
        return self


def sample(dist, B):
    """[B, nO, 4, 3]: fmin(fmax(mean + spread * xi, lo), hi); a FIXED field is its mean."""
    b, o, i, f = np.meshgrid(np.arange(B), np.arange(dist.n_obst), np.arange(NSEG), np.arange(NF),
                             indexing="ij")
    seed = dist.seed
    w = NM.philox4x32_10((NF * i + f, 0, (SITE_MANOEUVRE << 24) | o, (dist.b_offset + b) & NM.MASK),
                         (seed & NM.MASK, (seed >> 32) & NM.MASK))
    u1, u2 = NM.uniforms(w)
    uni = 2.0 * u2 - 1.0
    nor = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    kind = dist.kind[None, None]
    xi = np.where(kind == UNIFORM, uni, np.where(kind == NORMAL, nor, 0.0))
    val = dist.mean[None, None] + dist.spread[None, None] * xi
    val = np.minimum(np.maximum(val, dist.lo[None, None]), dist.hi[None, None])
    return np.where(kind == FIXED, np.broadcast_to(dist.mean[None, None], val.shape), val)


class PosedConstants(MM.Constants):
    """``metrics_mirror.Constants`` of one realisation whose obstacles are at given poses
    [nO, K, 3] from global tick ``tick0`` on, sized by its rows [nO, 7]."""

    def __init__(self, base, rows, pose, tick0):
        self.__dict__.update(base.__dict__)
        self.rows = np.asarray(rows, float).reshape(-1, OM.NP)
        self.pose, self.tick0 = np.asarray(pose, float), tick0
        assert len(self.rows) == self.nO == len(self.pose)

    def obstacle_rect(self, o, tick):
        x, y, h = self.pose[o, tick - self.tick0]
        r = self.rows[o]
        return (x, y, math.cos(h), math.sin(h), r[OM.LENGTH] / 2, r[OM.WIDTH] / 2)


def run(base, rows, man, calls, B):
    """``metrics_mirror.run`` with realisation b measured against its manoeuvring obstacles; a
    realisation with a bad lane keeps its reset values.  Returns the accumulators with a
    leading B."""
    rows = np.asarray(rows, float)
    accs = [MM.new_acc(base.nV) for _ in range(B)]
    for x_path, tick0, k_first in calls:
        x = np.asarray(x_path, float)
        pose = poses(rows, man, base.tick_length, tick0, x.shape[2] - 1)
        for b in range(B):
            if not np.isfinite(pose[b]).all() or any(OM.bad_row(r) for r in rows[b]):
                continue
            MM.accumulate(PosedConstants(base, rows[b], pose[b], tick0), accs[b], x[b], tick0,
                          k_first)
    out = {}
    for k in accs[0]:
        a = np.array([acc[k] for acc in accs])
        out[k] = a.astype(np.int32) if k.startswith(("argmin", "first", "n_")) else a.astype(float)
    return out
