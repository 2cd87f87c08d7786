"""CPU mirror of the right-of-way step (include/scpqp_yield.h), for its tests: numpy, generic
in the number format (``F64``, ``F80``), written from the header's steps 1 to 5, not from the
device code.  The clearances and the slew and stop rules are ``governor_mirror``'s, as the
header takes them from the governor's.  The arrays are those of ``scpqp_yield_step``: per
problem a slot with the problem's own horizon as the packed prefix."""
import math

import numpy as np

import governor_mirror as GM
from governor_mirror import F64, F80, MAX_HP, unpack  # noqa: F401

NP = 10
V_REF, A_ACC, A_BRAKE, K_V, J_MAX, LOOK, BAND, PRIO, A_EASE, S_STAND = range(NP)
PRIO_MAX = 2 ** 20
K_NONE, K_BAD = -1, -2


def is_off_row(row):
    return bool((np.asarray(row, float) == 0.0).all())


def is_bad_row(row):
    """The row part of the header's bad-lane rule (the fields alone); an off row is not bad."""
    row = np.asarray(row, float)
    if is_off_row(row):
        return False
    if GM.is_bad_row(row[:GM.NP]):
        return True
    for f in (PRIO, A_EASE, S_STAND):
        if not math.isfinite(row[f]) or row[f] < 0.0:
            return True
    if row[PRIO] != math.floor(row[PRIO]) or row[PRIO] > PRIO_MAX:
        return True
    return row[A_EASE] > row[A_BRAKE]


def counts(rows_b, x0_b, v, w):
    """Rule 2: does vehicle w count for vehicle v (rows_b [nV, 10], x0_b [nV, 6])?"""
    rv, rw = np.asarray(rows_b[v], float), np.asarray(rows_b[w], float)
    governed = not is_off_row(rw) and not is_bad_row(rw)
    standing = rv[S_STAND] > 0.0 and not (x0_b[w][3] > rv[S_STAND])
    return not (governed and rv[PRIO] > rw[PRIO] and not standing)


def stop_length(x0, v, k_conf, traj, fm=F64):
    """sum_{j < k_conf} |p_v(j) - p_v(j-1)| in ascending order, p_v(-1) = x0[0:2]; (the sum,
    the sum of the absolute terms)."""
    d = fm.num(0.0)
    ax, ay = fm.num(x0[0]), fm.num(x0[1])
    with np.errstate(all="ignore"):
        for j in range(k_conf):
            px, py = fm.num(traj[j, 0, v]), fm.num(traj[j, 1, v])
            ex, ey = px - ax, py - ay
            d = d + np.sqrt(ex * ex + ey * ey)
            ax, ay = px, py
    return d


def command(row, s, a_now, conflict, d_stop, t_hold, t_back, fm=F64, detail=None):
    """Steps 4 and 5.  ``detail`` (a dict) receives the arguments that decide a branch."""
    r = fm.array(row)
    s_, a_now_, th, tb = fm.num(s), fm.num(a_now), fm.num(t_hold), fm.num(t_back)
    wish = r[K_V] * (r[V_REF] - s_)
    a_need = None
    if conflict:
        sp = max(s_, fm.num(0.0))
        with np.errstate(all="ignore"):
            ok = bool(np.isfinite(d_stop)) and d_stop > 0
            a_need = sp * sp / (fm.num(2.0) * d_stop) if ok else fm.num(np.inf)
        a = -min(r[A_BRAKE], max(r[A_EASE], a_need))
    else:
        a = min(max(wish, -r[A_BRAKE]), r[A_ACC])
    a_des = a
    lo = hi = None
    if math.isfinite(float(row[J_MAX])):
        d = r[J_MAX] * th
        lo, hi = a_now_ - d, a_now_ + d
        a = min(max(a, lo), hi)
    a_slew = a
    s_raw = s_ - a_now_ * tb
    s_app = max(s_raw, fm.num(0.0))
    floor = -s_app / th
    a = max(a, floor)
    if detail is not None:
        detail.update(wish=wish, a_des=a_des, lo=lo, hi=hi, a_slew=a_slew, s_raw=s_raw,
                      s_app=s_app, floor=floor, conflict=conflict, a_need=a_need)
    return a


def lane(rows_b, x0_b, v, hb, traj, obst, margin, dreq_obs, dreq_veh, t_hold, t_back, fm=F64,
         detail=None):
    """One lane (b, v) -> (a_cmd, k_conf, clear, k_any, who, d_stop).  rows_b [nV, 10] and x0_b
    [nV, 6] of the realisation; the arrays are the problem's own (``governor_mirror.
    clearances``); hb is the problem's horizon, None when it lies outside its slot."""
    nan = fm.num(np.nan)
    row, x0 = np.asarray(rows_b[v], float), np.asarray(x0_b[v], float)
    if is_off_row(row):
        return fm.num(x0[4]), K_NONE, nan, K_NONE, K_NONE, nan
    if is_bad_row(row) or hb is None or not (math.isfinite(x0[3]) and math.isfinite(x0[4])):
        return nan, K_BAD, nan, K_BAD, K_BAD, nan
    nV = len(rows_b)
    nO = 0 if obst is None else obst.shape[0]
    K = min(int(row[LOOK]), hb)
    cs = GM.clearances(v, K, hb, traj, obst, margin, dreq_obs, dreq_veh, row[BAND], fm)
    cnt = [w != v and counts(rows_b, x0_b, v, w) for w in range(nV)]
    clear = min((e[1] for e in cs), default=fm.num(np.inf))
    hit_any = [e[0] for e in cs if e[1] < 0]
    k_any = min(hit_any) if hit_any else K_NONE
    keys = []
    for k, c, (kind, i), _ in cs:
        if c < 0 and (kind == "o" or cnt[i] or c == -np.inf):
            # c = -inf: a non-finite examined entry (or a c that is not a number) counts
            # whatever the ranks; a finite expression cannot give -inf
            keys.append(k * (nO + nV) + (i if kind == "o" else nO + i))
    if keys:
        k_conf, who = divmod(min(keys), nO + nV)
        d_stop = stop_length(x0, v, k_conf, traj, fm)
    else:
        k_conf, who, d_stop = K_NONE, K_NONE, fm.num(np.inf)
    if detail is not None:
        detail["clearances"] = cs
        detail["counts"] = cnt
    a = command(row, x0[3], x0[4], k_conf >= 0, d_stop, t_hold, t_back, fm, detail)
    return a, k_conf, clear, k_any, who, d_stop


def step(rows, x0, traj, obst, margin, hp, dreq_obs, dreq_veh, t_hold, t_back, hp_max, fm=F64,
         details=None):
    """The mirror of scpqp_yield_step: rows [B, nV, 10], the other arrays as in
    ``governor_mirror.step``.  Returns (a_cmd, k_conf int32, clear, k_any int32, who int32,
    d_stop), each [B, nV]; ``details`` (a dict) receives per (b, v) the examined clearances,
    the counts and the branch arguments."""
    rows = np.asarray(rows, float)
    x0 = np.asarray(x0, float)
    B, nV = rows.shape[:2]
    nO = 0 if obst is None else np.asarray(dreq_obs).shape[2]
    fl = lambda: np.empty((B, nV), dtype=fm.dtype)
    il = lambda: np.empty((B, nV), dtype=np.int32)
    a, kc, cl, ka, wh, ds = fl(), il(), fl(), il(), il(), fl()
    for b in range(B):
        hb = hp_max if hp is None else int(hp[b])
        ok = 1 <= hb <= hp_max
        t, o, m = unpack(b, nV, nO, hp_max, hb, traj, obst, margin) if ok else (None,) * 3
        for v in range(nV):
            d = None if details is None else details.setdefault((b, v), {})
            a[b, v], kc[b, v], cl[b, v], ka[b, v], wh[b, v], ds[b, v] = lane(
                rows[b], x0[b], v, hb if ok else None, t, o, m,
                None if not nO else np.asarray(dreq_obs)[b, v], np.asarray(dreq_veh)[b, v],
                t_hold, t_back, fm, d)
    return a, kc, cl, ka, wh, ds
