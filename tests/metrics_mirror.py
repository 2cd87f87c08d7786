"""Plain fp64 restatement of the realised-path metrics (include/scpqp_metrics.h), the
same formulas in the same order as csrc/metrics.hip, one item at a time.

A rectangle is (cx, cy, heading, length, width).  ``accumulate`` runs the accumulator of
one realisation over one call; ``run`` over a batch and a list of calls.
"""
import math

import numpy as np

INF = float("inf")


def _rect(cx, cy, h, length, width):
    return (cx, cy, math.cos(h), math.sin(h), length / 2, width / 2)


def _radius(r, nx, ny):
    return r[4] * abs(nx * r[2] + ny * r[3]) + r[5] * abs(ny * r[2] - nx * r[3])


def separation_margins(a, b):
    """|n.d| - (rA(n) + rB(n)) on the four axes a1, a2, b1, b2 (separated when > 0)."""
    dx, dy = b[0] - a[0], b[1] - a[1]
    out = []
    for nx, ny in ((a[2], a[3]), (-a[3], a[2]), (b[2], b[3]), (-b[3], b[2])):
        out.append(abs(nx * dx + ny * dy) - (_radius(a, nx, ny) + _radius(b, nx, ny)))
    return out


def _separated(a, b):
    dx, dy = b[0] - a[0], b[1] - a[1]
    for nx, ny in ((a[2], a[3]), (-a[3], a[2]), (b[2], b[3]), (-b[3], b[2])):
        if abs(nx * dx + ny * dy) > _radius(a, nx, ny) + _radius(b, nx, ny):
            return True
    return False


def _corners_to(a, b):
    best = INF
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            qx = a[0] + sx * a[4] * a[2] - sy * a[5] * a[3]
            qy = a[1] + sx * a[4] * a[3] + sy * a[5] * a[2]
            rx, ry = qx - b[0], qy - b[1]
            px, py = rx * b[2] + ry * b[3], ry * b[2] - rx * b[3]
            best = min(best, math.hypot(max(abs(px) - b[4], 0.0), max(abs(py) - b[5], 0.0)))
    return best


def _gap(a, b):
    if not _separated(a, b):
        return 0.0
    return min(_corners_to(a, b), _corners_to(b, a))


def footprint_gap(rect_a, rect_b):
    """Gap of two rectangles (cx, cy, heading, length, width); 0.0 exactly on overlap."""
    return _gap(_rect(*rect_a), _rect(*rect_b))


def overlap(rect_a, rect_b):
    return not _separated(_rect(*rect_a), _rect(*rect_b))


def cross_track(poly, px, py):
    """Distance of (px, py) to the polyline [n][2], the end segments extended as lines."""
    n = len(poly)
    best = INF
    for j in range(n - 1):
        ax, ay = float(poly[j][0]), float(poly[j][1])
        ex, ey = float(poly[j + 1][0]) - ax, float(poly[j + 1][1]) - ay
        l2 = ex * ex + ey * ey
        t = ((px - ax) * ex + (py - ay) * ey) / l2 if l2 > 0.0 else 0.0
        if j > 0:
            t = max(t, 0.0)
        if j + 2 < n:
            t = min(t, 1.0)
        best = min(best, math.hypot(px - (ax + t * ex), py - (ay + t * ey)))
    return best


class Constants:
    """The scenario constants of scpqp_metrics_params as plain arrays."""

    def __init__(self, length, width, dsafe_veh, dsafe_obs, obstacles, polylines, tick_length):
        self.length = [float(x) for x in length]
        self.width = [float(x) for x in width]
        self.nV = len(self.length)
        self.obstacles = np.asarray(obstacles, float).reshape(-1, 6) if len(obstacles) else \
            np.zeros((0, 6))
        self.nO = len(self.obstacles)
        self.dsafe_veh = np.asarray(dsafe_veh, float).reshape(self.nV, self.nV)
        self.dsafe_obs = np.asarray(dsafe_obs, float).reshape(self.nV, self.nO) if self.nO else \
            np.zeros((self.nV, 0))
        self.polylines = [np.asarray(p, float).reshape(-1, 2) for p in polylines]
        self.tick_length = float(tick_length)
        self.pairs = [(v, w) for v in range(self.nV) for w in range(v + 1, self.nV)]

    @classmethod
    def of_scenario(cls, sc):
        return cls(sc.Length, sc.Width, sc.dsafeVehicles, sc.dsafeObstacles if sc.nObst else [],
                   [np.asarray(o, float)[:6] for o in sc.obstacles], sc.referenceTrajectories,
                   sc.tick_length)

    def obstacle_rect(self, o, tick):
        ob = self.obstacles[o]
        t = float(tick) * self.tick_length
        c, s = math.cos(ob[2]), math.sin(ob[2])
        return (t * ob[3] * c + ob[0], t * ob[3] * s + ob[1], c, s, ob[4] / 2, ob[5] / 2)


def new_acc(nV):
    return dict(min_gap_veh=INF, min_gap_obs=INF, min_margin_veh=INF, min_margin_obs=INF,
                argmin_gap_veh=[-1, -1, -1], argmin_gap_obs=[-1, -1, -1], first_collision_tick=-1,
                n_collision_ticks=0, n_ticks_seen=0, max_xtrack=[0.0] * nV,
                sum_sq_xtrack=[0.0] * nV)


def dense(C, x_path, tick0):
    """One realisation's x_path [nV][K][6] -> gap_veh [K][n_pair], gap_obs [K][nV][nO],
    xtrack [K][nV], margin_veh [K][n_pair], margin_obs [K][nV][nO]."""
    x = np.asarray(x_path, float)
    nV, K = x.shape[0], x.shape[1]
    gv = np.zeros((K, len(C.pairs)))
    mv = np.zeros((K, len(C.pairs)))
    go = np.zeros((K, nV, C.nO))
    mo = np.zeros((K, nV, C.nO))
    xt = np.zeros((K, nV))
    for k in range(K):
        rects = [_rect(float(x[v, k, 0]), float(x[v, k, 1]), float(x[v, k, 2]), C.length[v],
                       C.width[v]) for v in range(nV)]
        for v in range(nV):
            xt[k, v] = cross_track(C.polylines[v], rects[v][0], rects[v][1])
        for p, (v, w) in enumerate(C.pairs):
            a, b = rects[v], rects[w]
            gv[k, p] = _gap(a, b)
            mv[k, p] = math.hypot(b[0] - a[0], b[1] - a[1]) - C.dsafe_veh[v, w]
        for o in range(C.nO):
            ob = C.obstacle_rect(o, tick0 + k)
            for v in range(nV):
                a = rects[v]
                go[k, v, o] = _gap(a, ob)
                mo[k, v, o] = math.hypot(ob[0] - a[0], ob[1] - a[1]) - C.dsafe_obs[v, o]
    return dict(gap_veh=gv, gap_obs=go, xtrack=xt, margin_veh=mv, margin_obs=mo)


def accumulate(C, acc, x_path, tick0, k_first):
    """Merge the entries k_first..K-1 of one realisation's x_path [nV][K][6] into acc."""
    d = dense(C, x_path, tick0)
    K, nV = d["xtrack"].shape
    best_v, best_o = (INF, None), (INF, None)
    for k in range(k_first, K):
        tick = tick0 + k
        hit = False
        for p, (v, w) in enumerate(C.pairs):
            g = d["gap_veh"][k, p]
            if g < best_v[0]:                  # items in lexicographic order: the first stays
                best_v = (g, (tick, v, w))
            hit |= g == 0.0
            acc["min_margin_veh"] = min(acc["min_margin_veh"], d["margin_veh"][k, p])
        for v in range(nV):
            for o in range(C.nO):
                g = d["gap_obs"][k, v, o]
                if g < best_o[0]:
                    best_o = (g, (tick, v, o))
                hit |= g == 0.0
                acc["min_margin_obs"] = min(acc["min_margin_obs"], d["margin_obs"][k, v, o])
        if hit:
            acc["n_collision_ticks"] += 1
            if acc["first_collision_tick"] < 0 or tick < acc["first_collision_tick"]:
                acc["first_collision_tick"] = tick
        for v in range(nV):
            e = float(d["xtrack"][k, v])
            acc["max_xtrack"][v] = max(acc["max_xtrack"][v], e)
            acc["sum_sq_xtrack"][v] = acc["sum_sq_xtrack"][v] + e * e
        acc["n_ticks_seen"] += 1
    if best_v[0] < acc["min_gap_veh"]:         # across calls only a strictly smaller gap
        acc["min_gap_veh"], acc["argmin_gap_veh"] = float(best_v[0]), list(best_v[1])
    if best_o[0] < acc["min_gap_obs"]:
        acc["min_gap_obs"], acc["argmin_gap_obs"] = float(best_o[0]), list(best_o[1])
    return d


def run(C, calls, B):
    """calls: list of (x_path [B][nV][K][6], tick0, k_first).  Returns the accumulators as
    arrays with a leading B, like PathMetrics.result()."""
    accs = [new_acc(C.nV) for _ in range(B)]
    for x_path, tick0, k_first in calls:
        x = np.asarray(x_path, float)
        for b in range(B):
            accumulate(C, accs[b], x[b], tick0, k_first)
    out = {}
    for k in accs[0]:
        a = np.array([acc[k] for acc in accs])
        out[k] = a.astype(np.int32) if k.startswith(("argmin", "first", "n_")) else a.astype(float)
    return out
