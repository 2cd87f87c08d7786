"""The case table of the problem-setup tests (tests/test_setup_host.py on the CPU,
tests/test_gpu_setup.py on the GPU): shapes, per-vehicle states off the nominal start, and a
reference polyline with a placement for every vehicle of every problem, all generated on the
host without random numbers.

Shapes (SHAPES): the smallest that run each layout of the setup scratch (``plan_query``): frog's
1 x 10 with its obstacles, c2's compiled 4 x 20, c5's 4 x 30 with a horizon array of
(30, 10, 1), c3's compiled 8 x 30, a run-time 6 x 10 (its second round has two idle waves),
13 x 5 (four rounds, one live wave in the last) and 1 x 64.

States.  Slot i of the table (vehicles counted through all problems of all shapes) takes
speed SPEEDS[i % 10], steering STEER[i % 7], heading HEAD[i % 9], acceleration ACC[i % 3],
u0 U0[i % 11] and model noise NOISE[i % 4], NOISE[(i + 1) % 4]: the periods are coprime, so
the 70 speed-steering pairs all occur.  PINNED overrides the speeds of a few problems so that
one round of four waves sees four different squaring counts and a later round a larger count
than the first.  Lf and Lr differ per vehicle and per problem.

Polylines and placements.  Problem b of a shape has its own scenario variant b (variant 0 is
the constructor's scenario): a polyline of 3 to 8 points per vehicle, rotated, scaled so that
every segment is longer than the vehicle's step |v| dt, and the vehicle placed on it by
KINDS:

  wedge     3 points; before the normal through the corner on segment 1 and behind it on
            segment 2: the one region where the reference does not raise (every problem
            with b % 4 == 0 is made of these, so that it has a clear status flag)
  inside    beside the inside of a segment
  corner    outside the corner of an axis-parallel line of integer coordinates, step exactly
            1 m (speed 2.5 m/s): the nearest point is the vertex itself, so the walk starts
            with no length left and alternates about the vertex on a tie, remaining length
            against step, that only exact arithmetic decides alike everywhere
  before    before the start
  past      past the end (the B.1 alternation from the first step)
  short     the first segment shorter than the step (the reference's assert)
  repeat    the last point repeated; the vehicle beside segment 1, so the walk stays off it
  vertex    exactly on point 1 of an axis-parallel line of integer coordinates
  endpoint  exactly on the last point of such a line, step exactly 1 m (speed 2.5 m/s)
  endpoint2 the same on a line of two points: the index past the end
  short2    a line of two points shorter than the step: the assert alone (speed 8 m/s)

corner, vertex, endpoint and endpoint2 are the exact cases: their coordinates and products
are integers, so the decisions on lambda, the distances and (corner, endpoint) the remaining
length are exact in float64 and equal on every IEEE machine; EXACT names the decision kinds
left out of their separation (a repeated point at speed 0 adds the assert's 0 > 0).  Speeds
0 and below give ``step = 0`` and ``step < 0`` with every placement.

FAR is one more state, steering 1.56 rad at 4 m/s (the argument's norm is 2.4e4: 13
squarings), to be a vehicle of the table only if the float64 restatement keeps the table's
bounds on it (tests/test_setup_host.py holds FAR_KEPT to that).  It does not: with Lf 0.34
and Lr 0.30 its worst ratios are Ad 54, Bd 88 and Ed 0.6 against the table's Bd of 6.9 (bound
27.4); states of 12 squarings reached through the speed (2e4 m/s at 0.05 rad, 1.2e4 m/s at
0.3 rad) or 64 m/s at 1.5 rad give 52 on Bd alike.  So FAR_KEPT is False and no case runs
it; the largest count of the table is 6.

BOUNDS.  MEASURED holds, per output, the worst ratio |x_f64 - x_80| / (u yardstick) of the
float64 restatement of the device's algorithm (setup_mirror: expm="pade") against the 80-bit
mirror over the whole table, as tests/test_setup_host.py::test_bound_of_the_float64_restatement
prints it; BOUND is four times that: the margin for the device's own tan, sin, cos and atan
against the host's and another order of summation.  No device run went into them."""
import functools
import math

import numpy as np

import setup_mirror as SM

DT = 0.4
U_LIM = math.pi / 180 * 3

# id, scenario, V, hp_max, horizons (None: no horizon array), problems
SHAPES = (
    ("frog_1x10", "frog", 1, 10, None, 16),
    ("c2_4x20", "circle", 4, 20, None, 8),
    ("c5_4x30_mixed", "circle", 4, 30, (30, 10, 1), 9),
    ("c3_8x30", "circle", 8, 30, None, 4),
    ("rt_6x10", "circle", 6, 10, None, 4),
    ("rt_13x5", "circle", 13, 5, None, 3),
    ("rt_1x64", "circle", 1, 64, None, 8),
)
SHAPE_IDS = tuple(s[0] for s in SHAPES)
# the solve-kernel instantiation (HG, VG, RM, OCC, SH) each shape runs: its scratch layout
KERNELS = {"frog_1x10": (0, 0, 1, 3, 0), "c2_4x20": (0, 1, 2, 3, 1), "c5_4x30_mixed": (0, 1, 2, 2, 2),
           "c3_8x30": (1, 1, 4, 2, 3), "rt_6x10": (0, 1, 1, 3, 0), "rt_13x5": (0, 1, 2, 2, 0),
           "rt_1x64": (0, 0, 2, 3, 0)}

SPEEDS = (0.0, 4.0, 16.0, 64.0, 0.01, 8.0, 32.0, -1.0, -0.01, 1.0)
STEER = (0.0, 0.05, -0.3, 0.6, -0.05, 0.3, -0.6)
HEAD = (0.4, 2.0, -2.5, -0.9, 3.5, -4.0, 7.0, math.pi / 2, -math.pi)
ACC = (0.0, 2.0, -2.0)
U0 = (0.0, 0.5 * U_LIM, -0.5 * U_LIM, U_LIM, -U_LIM, 2 * U_LIM, -2 * U_LIM, 0.3, -0.3, 0.6, -0.6)
NOISE = (0.0, 1e-3, -1e-3, 5e-4)
# (shape, problem) -> speeds: four counts in one round; a larger count in a later round
PINNED = {("c3_8x30", 1): (1.0, 4.0, 16.0, 64.0, 0.01, 8.0, 32.0, 64.0),
          ("c3_8x30", 2): (0.0, 1.0, -1.0, 0.01, 64.0, 32.0, 16.0, 8.0),
          ("rt_6x10", 1): (64.0, 1.0, 16.0, 4.0, 32.0, 0.0),
          ("rt_13x5", 1): (1.0,) * 12 + (64.0,)}
KINDS = ("inside", "corner", "before", "past", "inside", "short", "repeat", "vertex", "endpoint")
EXACT = {"vertex": ("lam", "sd"), "endpoint": ("lam", "sd", "rem"), "endpoint2": ("lam", "sd", "rem"),
         "corner": ("rem",)}
# (shape, problem) -> the kinds on a line of two points (one vehicle each)
TWO_POINT = {("frog_1x10", 13): "endpoint2", ("frog_1x10", 14): "short2", ("rt_1x64", 5): "short2"}
FAR = dict(v=4.0, delta=1.56)
FAR_AT = ("frog_1x10", 15, 0)      # shape, problem, vehicle
FAR_KEPT = False
SEPARATION = 1e-9                  # metres, or units of lambda

# turns (degrees) and segment lengths (units) of the polylines of 3 .. 8 points
TURNS = {3: (75,), 4: (40, -70), 5: (30, 30, -50, 60), 6: (-35, 50, 45, -60, 25),
         7: (20, -45, 60, 30, -70, 40), 8: (-30, -30, 55, 50, -65, 35, 20)}
LENS = (10.0, 12.0, 11.0, 13.0, 10.5, 12.5, 11.5)

# ---------------------------------------------------------------------------------------
# bounds: measured on the CPU by test_setup_host.py::test_bound_of_the_float64_restatement
# ---------------------------------------------------------------------------------------
# that run printed (x86-64, glibc's libm, numpy longdouble = 80-bit extended):
#   Ad 68.57 (rt_6x10 problem 0 vehicle 0: 32 m/s, -0.05 rad)   Bd 6.844 (the same vehicle)
#   Ed 2.540 (c5_4x30_mixed 5/1: 1 m/s, -0.6 rad)
#   g 13160 (frog_1x10 8/0: -0.01 m/s, 0.05 rad)
#   const_term 91.14, psi0 68.41 (c5_4x30_mixed 3/3: 64 m/s, 0 rad)
# The constants are those figures rounded up in the third digit.  g's is large because the
# position rows of Ad and Bd cancel at a crawl (their yardstick S, with e^(+10 dt) for the
# steering lag, is far above their magnitude, and g's yardstick is built on the magnitudes);
# it is still 6e-12 of the yardstick.
MEASURED = {"Ad": 68.6, "Bd": 6.85, "Ed": 2.55, "g": 13200.0, "const_term": 91.2, "psi0": 68.5}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
# expm8 alone on EXPM_MATRICES: |X_f64 - X_80| / (u expm(|A|))
EXPM_MEASURED = 2.99          # the run printed 2.986
EXPM_BOUND = 4.0 * EXPM_MEASURED
REF_TOL = 1e-12                    # metres: the device's sampler against the oracle's


class Case:
    """One shape's problems.  x0 [B, V, 6], u0 [B, V], ec [B, V, 2], hp [B], Lf / Lr / Q / Qf
    [B, V], poly[b][v] the polyline [n, 2], kind[b][v], hp_arg (the horizon array or None)."""


def _rot(a):
    return np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])


def polyline(npts, origin, angle, scale):
    pts = [np.zeros(2)]
    h = 0.0
    for j in range(npts - 1):
        if j:
            h += math.radians(TURNS[npts][j - 1])
        pts.append(pts[-1] + LENS[j] * np.array([math.cos(h), math.sin(h)]))
    return np.asarray(origin) + scale * (np.array(pts) @ _rot(angle).T)


def _unit(d):
    return d / math.hypot(d[0], d[1])


def _place(kind, b, v, step):
    """(polyline, position) of placement ``kind`` for a vehicle of step ``step``."""
    a = abs(step)
    slot = 3 * b + 5 * v
    angle = 0.37 + 0.83 * slot
    origin = (3.0 * ((slot % 7) - 3), 2.0 * ((slot % 5) - 2))
    scale = max(1.0, 1.3 * a / 10.0) * (1 + 0.1 * (v % 3))
    if kind in ("vertex", "endpoint", "endpoint2", "corner"):
        S = 9.0 * 2 ** max(0, math.ceil(math.log2(max(1.3 * a / 9.0, 1.0))))
        if kind == "endpoint2":
            P = np.array([[0.0, 0.0], [S, 0.0]])
            return P, P[1].copy()
        P = np.array([[0.0, 0.0], [S, 0.0], [S, S]])
        if kind == "corner":
            return P, P[1] + np.array([1.0, -1.0])
        return P, P[1 if kind == "vertex" else 2].copy()
    if kind == "short2":
        d = np.array([math.cos(angle), math.sin(angle)])
        P = np.array([origin, np.asarray(origin) + 0.8 * a * d])
        return P, P[0] + 0.3 * (P[1] - P[0]) + 0.4 * a * np.array([-d[1], d[0]])
    if kind == "wedge":
        P = polyline(3, origin, angle, scale)
        din, dout = _unit(P[1] - P[0]), _unit(P[2] - P[1])
        return P, P[1] + scale * ((-3.0 - 0.2 * (v % 4)) * din + (4.0 + 0.3 * (b % 3)) * dout)
    npts = 3 + (b + 2 * v) % 6
    if kind == "short":
        P = polyline(npts, origin, angle, 1.0)
        # the first segment 0.8 steps long, the others four times as long as that or more
        P = P[0] + (P - P[0]) * (0.8 * a / LENS[0])
        P[1:] = P[1] + (P[1:] - P[1]) * 5.0
        return P, P[0] + 0.3 * (P[1] - P[0]) + 0.4 * a * _unit((P[1] - P[0])[::-1] * (1, -1))
    if kind == "repeat":
        P = polyline(max(npts - 1, 3), origin, angle, scale)
        P = np.concatenate([P, P[-1:]])
        d = _unit(P[1] - P[0])
        return P, P[0] + 0.37 * (P[1] - P[0]) + 0.8 * np.array([-d[1], d[0]])
    P = polyline(npts, origin, angle, scale)
    n = len(P)
    if kind == "inside":
        j = 1 + (b + v) % (n - 1)
        d = _unit(P[j] - P[j - 1])
        side = 1.0 if (b + v) % 2 else -1.0
        return P, P[j - 1] + 0.37 * (P[j] - P[j - 1]) + 0.8 * side * np.array([-d[1], d[0]])
    if kind == "before":
        d = _unit(P[1] - P[0])
        return P, P[0] - 2.3 * d + 0.6 * np.array([-d[1], d[0]])
    if kind == "past":
        d = _unit(P[-1] - P[-2])
        return P, P[-1] + 1.7 * d + 0.5 * np.array([-d[1], d[0]])
    raise ValueError(kind)


def _slot_base(sid):
    base = 0
    for s in SHAPES:
        if s[0] == sid:
            return base
        base += s[2] * s[5]
    raise KeyError(sid)


@functools.lru_cache(maxsize=None)
def case(sid):
    _, scen, V, Hm, hps, B = next(s for s in SHAPES if s[0] == sid)
    c = Case()
    c.id, c.scenario, c.V, c.hp_max, c.B = sid, scen, V, Hm, B
    c.hp = np.array([hps[b % len(hps)] if hps else Hm for b in range(B)], dtype=np.int32)
    c.hp_arg = c.hp if hps else None
    c.x0 = np.zeros((B, V, 6))
    c.u0 = np.zeros((B, V))
    c.ec = np.zeros((B, V, 2))
    c.Lf, c.Lr = np.zeros((B, V)), np.zeros((B, V))
    c.Q, c.Qf = np.zeros((B, V)), np.zeros((B, V))
    c.poly = [[None] * V for _ in range(B)]
    c.kind = [[None] * V for _ in range(B)]
    i0 = _slot_base(sid)
    for b in range(B):
        for v in range(V):
            i = i0 + b * V + v
            speed = SPEEDS[i % 10]
            if (sid, b) in PINNED:
                speed = PINNED[(sid, b)][v]
            delta = STEER[i % 7]
            kind = "wedge" if b % 4 == 0 else KINDS[(3 * b + v) % len(KINDS)]
            if (sid, b) in TWO_POINT:
                kind = TWO_POINT[(sid, b)]
            if (sid, b, v) == FAR_AT and FAR_KEPT:
                speed, delta, kind = FAR["v"], FAR["delta"], "inside"
            if kind in ("endpoint", "endpoint2", "corner"):
                speed = 2.5
            if kind == "short2":
                speed = 8.0
            if kind == "short" and speed < 1.0:
                kind = "inside"
            P, pos = _place(kind, b, v, speed * DT)
            c.x0[b, v] = (pos[0], pos[1], HEAD[i % 9], speed, ACC[i % 3], delta)
            c.u0[b, v] = U0[i % 11]
            c.ec[b, v] = (NOISE[i % 4], NOISE[(i + 1) % 4])
            c.Lf[b, v] = 0.34 + 0.03 * ((v + b) % 4)
            c.Lr[b, v] = 0.34 - 0.02 * ((v + 2 * b) % 5)
            c.Q[b, v] = 1.0 + 0.125 * ((v + b) % 3)
            c.Qf[b, v] = 20.0 - 2.5 * ((v + 2 * b) % 4)
            c.poly[b][v], c.kind[b][v] = P, kind
    return c


def scenarios(c):
    """The scenario variants of a case, one per problem; entry 0 is the constructor's."""
    import copy

    from oracle import scp_reference as R
    base = R.frog_scenario(Hp=c.hp_max) if c.scenario == "frog" else R.circle_scenario(c.V, Hp=c.hp_max)
    out = []
    for b in range(c.B):
        sc = copy.deepcopy(base)
        sc.Lf, sc.Lr = list(c.Lf[b]), list(c.Lr[b])
        sc.Q, sc.Q_final = list(c.Q[b]), list(c.Qf[b])
        sc.referenceTrajectories = [np.array(p) for p in c.poly[b]]
        out.append(sc)
    return out


def samples(c, b, v, ft=SM.F64, seed=None):
    """The mirror's sampler on vehicle v of problem b at its own horizon."""
    x = c.x0[b, v]
    return SM.sample(int(c.hp[b]), c.poly[b][v], x[0], x[1], x[3] * DT, ft, seed)


def exact_kinds(c, b, v):
    if c.kind[b][v] == "repeat" and c.x0[b, v, 3] == 0.0:
        return ("assert",)          # the repeated point's length 0 against the step 0
    return EXACT.get(c.kind[b][v], ())


def separated(c, b, v):
    return SM.separation(samples(c, b, v), exact_kinds(c, b, v)) >= SEPARATION


def would_raise(c, b):
    """Whether the reference would raise on problem b: on any of its vehicles."""
    return any(bool(samples(c, b, v).raises) for v in range(c.V))


@functools.lru_cache(maxsize=None)
def reference_points(sid):
    """[B][hp_b, 2, V] float64: the mirror's sampler (it is the oracle's wherever the oracle
    returns; tests/test_setup_host.py)."""
    c = case(sid)
    out = []
    for b in range(c.B):
        r = np.zeros((int(c.hp[b]), 2, c.V))
        for v in range(c.V):
            r[:, :, v] = np.asarray(samples(c, b, v).points, dtype=np.float64)
        out.append(r)
    return out


def evaluate(c, ft, expm="taylor", seed=None, refs=None):
    """{(b, v): {output: (value, yardstick)}} of a case in number format ``ft``.  refs:
    [B][hp_b, 2, V] reference points (default: reference_points).  The seeded mistakes of
    setup_mirror.SEEDS are passed on; "qf_hpmax" puts Qf on step hp_max - 1."""
    refs = reference_points(c.id) if refs is None else refs
    out = {}
    for b in range(c.B):
        Hb = int(c.hp[b])
        for v in range(c.V):
            r = SM.vehicle(c.x0[b, v], c.u0[b, v], c.Lf[b, v], c.Lr[b, v], c.ec[b, v], DT, Hb, ft,
                           expm, seed)
            last = c.hp_max - 1 if seed == "qf_hpmax" else None
            o = SM.outputs(r, refs[b][:, :, v], c.Q[b, v], c.Qf[b, v], ft, last)
            o["_vehicle"] = r
            out[(b, v)] = o
    return out


@functools.lru_cache(maxsize=None)
def reference(sid):
    """The 80-bit mirror of a case on the mirror's own reference points (computed once)."""
    return evaluate(case(sid), SM.F80)


# ---------------------------------------------------------------------------------------
# expm8 alone (tests/setup_harness.py): launches of four 8x8 matrices and a wave mask
# ---------------------------------------------------------------------------------------
def _expm_matrices():
    rng_free = np.arange(64, dtype=np.float64).reshape(8, 8)
    dense = np.cos(1.7 * rng_free + 0.3) * 0.9                 # V - U needs row swaps
    lower = np.tril(np.sin(0.9 * rng_free + 1.1), -1) * 2.0    # lower triangular: swaps
    # a tie in the first pivot column: rows 0 and 3 of V - U agree there in magnitude.  A
    # permutation-like generator: exp(t J) with J the cyclic shift keeps circulant structure
    J = np.roll(np.eye(8), 1, axis=1)
    tie = 1.5 * (J - J.T)
    nil = np.triu(np.ones((8, 8)), 1) * 0.75                   # nilpotent
    zero = np.zeros((8, 8))

    def at_norm(A, nrm):
        return A * (nrm / SM.norm1(A))
    below = at_norm(dense, SM.THETA13 * (1 - 2.0 ** -20))
    above = at_norm(dense, SM.THETA13 * (1 + 2.0 ** -20))
    big = at_norm(lower, 40.0)                                 # three squarings
    return {"dense": dense, "lower": lower, "tie": tie, "nil": nil, "zero": zero,
            "below": below, "above": above, "big": big}


EXPM_MATRICES = _expm_matrices()
# (names of the four waves' matrices, wave mask)
EXPM_LAUNCHES = ((("dense", "lower", "tie", "nil"), 15), (("zero", "below", "above", "big"), 15),
                 (("big", "dense", "zero", "above"), 0b1011), (("nil", "big", "lower", "tie"), 0b0110))
