"""CPU mirror of the speed governor step (include/scpqp_governor.h), for its tests: numpy,
generic in the number format (``F64``, ``F80``), written from the header's steps 1 to 6, not
from the device code.  The arrays are those of ``scpqp_governor_step``: per problem a slot with
the problem's own horizon as the packed prefix."""
import math

import numpy as np

NP = 7
V_REF, A_ACC, A_BRAKE, K_V, J_MAX, LOOK, BAND = range(NP)
MAX_HP = 64
K_NONE, K_BAD = -1, -2


class Format:
    def __init__(self, dtype):
        self.dtype = dtype

    def num(self, v):
        return self.dtype(v)

    def array(self, a):
        return np.asarray(a, dtype=self.dtype)


F64 = Format(np.float64)
F80 = Format(np.longdouble)


def is_off_row(row):
    return bool((np.asarray(row, float) == 0.0).all())


def is_bad_row(row):
    """The row part of the header's bad-lane rule."""
    row = np.asarray(row, float)
    for f in range(NP):
        if row[f] < 0.0:
            return True
        if not math.isfinite(row[f]) and not (f == J_MAX and row[f] == math.inf):
            return True
    return row[LOOK] != math.floor(row[LOOK]) or row[LOOK] > MAX_HP


def clearances(v, K, hb, traj, obst, margin, dreq_obs, dreq_veh, band, fm=F64):
    """Every examined clearance of vehicle v over its first K steps as a list of
    (k, c, which, scale), scale = distance + |required| + |band|, the absolute terms of c:
    traj [hb][2][nV], obst [nO][2][hb] or None, margin [nO][hb] or None, dreq_obs [nO],
    dreq_veh [nV]; which = ('o', o) or ('v', w).  A non-finite input, or a c that is not a
    number, gives c = -inf."""
    nV = traj.shape[2]
    nO = 0 if obst is None else obst.shape[0]
    out = []
    ninf = fm.num(-np.inf)
    with np.errstate(all="ignore"):
        for k in range(K):
            px, py = fm.num(traj[k, 0, v]), fm.num(traj[k, 1, v])
            for o in range(nO):
                qx, qy = fm.num(obst[o, 0, k]), fm.num(obst[o, 1, k])
                m = fm.num(0.0) if margin is None else fm.num(margin[o, k])
                need = fm.num(dreq_obs[o]) + m
                out.append((k,) + _clear(px, py, qx, qy, need, band, fm, ninf, ("o", o)))
            for w in range(nV):
                if w == v:
                    continue
                qx, qy = fm.num(traj[k, 0, w]), fm.num(traj[k, 1, w])
                out.append((k,) + _clear(px, py, qx, qy, fm.num(dreq_veh[w]), band, fm, ninf,
                                         ("v", w)))
    return out


def _clear(px, py, qx, qy, need, band, fm, ninf, which):
    if not all(np.isfinite(t) for t in (px, py, qx, qy, need)):
        return ninf, which, fm.num(1.0)
    dx, dy = px - qx, py - qy
    dist = np.sqrt(dx * dx + dy * dy)
    c = dist - (need + fm.num(band))
    if np.isnan(c):
        return ninf, which, fm.num(1.0)
    return c, which, dist + abs(need) + abs(fm.num(band))


def command(row, s, a_now, conflict, t_hold, t_back, fm=F64, detail=None):
    """Steps 2 to 4.  ``detail`` (a dict) receives the clamp arguments that decide a branch."""
    r = fm.array(row)
    s, a_now, th, tb = fm.num(s), fm.num(a_now), fm.num(t_hold), fm.num(t_back)
    wish = r[K_V] * (r[V_REF] - s)
    a = -r[A_BRAKE] if conflict else min(max(wish, -r[A_BRAKE]), r[A_ACC])
    a_des = a
    lo = hi = None
    if math.isfinite(float(row[J_MAX])):
        d = r[J_MAX] * th
        lo, hi = a_now - d, a_now + d
        a = min(max(a, lo), hi)
    a_slew = a
    s_raw = s - a_now * tb
    s_app = max(s_raw, fm.num(0.0))
    floor = -s_app / th
    a = max(a, floor)
    if detail is not None:
        detail.update(wish=wish, a_des=a_des, lo=lo, hi=hi, a_slew=a_slew, s_raw=s_raw,
                      s_app=s_app, floor=floor, conflict=conflict)
    return a


def lane(row, x0, v, hb, traj, obst, margin, dreq_obs, dreq_veh, t_hold, t_back, fm=F64,
         detail=None):
    """One lane (b, v) -> (a_cmd, k_conf, clear).  x0 [6] of the vehicle; the arrays are the
    problem's own (``clearances``); hb is the problem's horizon, None when it lies outside its
    slot."""
    nan = fm.num(np.nan)
    if is_off_row(row):
        return fm.num(x0[4]), K_NONE, nan
    if is_bad_row(row) or hb is None or not (math.isfinite(x0[3]) and math.isfinite(x0[4])):
        return nan, K_BAD, nan
    K = min(int(row[LOOK]), hb)
    cs = clearances(v, K, hb, traj, obst, margin, dreq_obs, dreq_veh, row[BAND], fm)
    clear = min((e[1] for e in cs), default=fm.num(np.inf))
    hit = [e[0] for e in cs if e[1] < 0]
    k_conf = min(hit) if hit else K_NONE
    if detail is not None:
        detail["clearances"] = cs
    a = command(row, x0[3], x0[4], k_conf >= 0, t_hold, t_back, fm, detail)
    return a, k_conf, clear


def unpack(b, nV, nO, hp_max, hb, traj, obst, margin):
    """The arrays of problem b out of the batch's slots: traj [B, hp_max * 2 * nV] -> [hb, 2, nV],
    obst [B, nO * 2 * hp_max] -> [nO, 2, hb], margin [B, nO * hp_max] -> [nO, hb]."""
    t = np.asarray(traj).reshape(len(traj), -1)[b, :hb * 2 * nV].reshape(hb, 2, nV)
    o = m = None
    if nO:
        o = np.asarray(obst).reshape(len(obst), -1)[b, :nO * 2 * hb].reshape(nO, 2, hb)
        if margin is not None:
            m = np.asarray(margin).reshape(len(margin), -1)[b, :nO * hb].reshape(nO, hb)
    return t, o, m


def step(rows, x0, traj, obst, margin, hp, dreq_obs, dreq_veh, t_hold, t_back, hp_max, fm=F64,
         details=None):
    """The mirror of scpqp_governor_step: rows [B, nV, 7], x0 [B, nV, 6], traj / obst / margin
    in slots of hp_max (any shape with B leading), hp [B] or None, dreq_obs [B, nV, nO],
    dreq_veh [B, nV, nV].  Returns (a_cmd [B, nV], k_conf int32 [B, nV], clear [B, nV]);
    ``details`` (a dict) receives per (b, v) the examined clearances and clamp arguments."""
    rows = np.asarray(rows, float)
    B, nV = rows.shape[:2]
    nO = 0 if obst is None else np.asarray(dreq_obs).shape[2]
    a = np.empty((B, nV), dtype=fm.dtype)
    kc = np.empty((B, nV), dtype=np.int32)
    cl = np.empty((B, nV), dtype=fm.dtype)
    for b in range(B):
        hb = hp_max if hp is None else int(hp[b])
        ok = 1 <= hb <= hp_max
        t, o, m = unpack(b, nV, nO, hp_max, hb, traj, obst, margin) if ok else (None,) * 3
        for v in range(nV):
            d = None if details is None else details.setdefault((b, v), {})
            a[b, v], kc[b, v], cl[b, v] = lane(
                rows[b, v], np.asarray(x0)[b, v], v, hb if ok else None, t, o, m,
                None if not nO else np.asarray(dreq_obs)[b, v], np.asarray(dreq_veh)[b, v],
                t_hold, t_back, fm, d)
    return a, kc, cl
