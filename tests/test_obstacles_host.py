"""Obstacle truth, the parts that need no GPU: the C-ABI of include/scpqp_obstacles.h
(exports, ctypes layout by a gcc probe of the header, argument validation without touching
a device), the CPU mirror (tests/obstacle_mirror.py) pinned by the oracle and by the
geometry of a circle, and scpqp.obstacles' host side."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import obstacle_mirror as OM
from oracle import plant_reference as PR
from oracle import scp_reference as R
from scpqp import _lib as LB
from scpqp import obstacles as OB
from scpqp.build import LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scpqp_obstacles.h")
E_ARG, E_SIZE = -1, -4
U, N, F = LB.TRUTH_UNIFORM, LB.TRUTH_NORMAL, LB.TRUTH_FIXED


def header_functions():
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"^int\s+(scpqp_\w+)\(", txt, re.M)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        pytest.fail("libscpqp.so not built: run __graft_entry__.build()")
    return LB.load()


# ---------------------------------------------------------------------------
# 1. exports and layout
# ---------------------------------------------------------------------------
def test_obstacles_header_declares_the_boundary():
    assert header_functions() == sorted(LB.OBSTACLE_EXPORTS)
    others = (set(LB.EXPORTS) | set(LB.NOISE_EXPORTS) | set(LB.METRICS_EXPORTS)
              | set(LB.VARIANT_EXPORTS) | set(LB.TRUTH_EXPORTS))
    assert not set(LB.OBSTACLE_EXPORTS) & others


def test_library_exports_every_obstacle_symbol(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\sT\s(scpqp_\w+)", out))
    assert set(header_functions()) <= exported
    for name in LB.OBSTACLE_EXPORTS:
        assert hasattr(lib, name)


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "scpqp_obstacles.h"
int main(void) {
  printf("size %zu\n", sizeof(scpqp_obstacles_dist));
  printf("n_obst %zu\n", offsetof(scpqp_obstacles_dist, n_obst));
  printf("mean %zu\n", offsetof(scpqp_obstacles_dist, mean));
  printf("field %zu\n", offsetof(scpqp_obstacles_dist, field));
  printf("seed %zu\n", offsetof(scpqp_obstacles_dist, seed));
  printf("b_offset %zu\n", offsetof(scpqp_obstacles_dist, b_offset));
  printf("fsize %zu\n", sizeof(scpqp_truth_field));
  printf("np %d\n", SCPQP_OBST_NP);
  printf("idx %d%d%d%d%d%d%d\n", SCPQP_OBST_X, SCPQP_OBST_Y, SCPQP_OBST_HEADING, SCPQP_OBST_SPEED,
         SCPQP_OBST_LENGTH, SCPQP_OBST_WIDTH, SCPQP_OBST_YAW_RATE);
  printf("site %d\n", SCPQP_NOISE_SITE_OBSTACLE);
  printf("maxobst %d\n", SCPQP_MAX_OBST);
  printf("maxhp %d\n", SCPQP_MAX_HP);
  return 0;
}
"""


def test_obstacles_ctypes_layout_matches_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", f"-I{os.path.dirname(HEADER)}", str(src), "-o", str(exe)],
                   check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(LB.ObstacleDist)
    for f in ("n_obst", "mean", "field", "seed", "b_offset"):
        assert int(got[f]) == getattr(LB.ObstacleDist, f).offset, f
    assert int(got["fsize"]) == C.sizeof(LB.TruthField)
    assert int(got["np"]) == LB.OBST_NP == OM.NP == OB.NP == 7
    assert got["idx"] == "0123456"
    assert (LB.OBST_X, LB.OBST_Y, LB.OBST_HEADING, LB.OBST_SPEED, LB.OBST_LENGTH, LB.OBST_WIDTH,
            LB.OBST_YAW_RATE) == tuple(range(7)) == (OM.X, OM.Y, OM.HEADING, OM.SPEED, OM.LENGTH,
                                                    OM.WIDTH, OM.YAW_RATE)
    assert len(LB.OBSTACLE_FIELDS) == 7
    assert int(got["site"]) == LB.NOISE_SITE_OBSTACLE == OM.SITE_OBSTACLE == 4
    assert LB.NOISE_SITE_OBSTACLE not in (LB.NOISE_SITE_DELAY, LB.NOISE_SITE_PLANT,
                                          LB.NOISE_SITE_LINEARIZE, LB.NOISE_SITE_TRUTH)
    assert int(got["maxobst"]) == LB.MAX_OBST and int(got["maxhp"]) == LB.MAX_HP


# ---------------------------------------------------------------------------
# 2. argument validation without a GPU
# ---------------------------------------------------------------------------
def _dummy():
    buf = (C.c_double * 256)()
    return buf, C.cast(buf, C.c_void_p)


def test_predict_and_pose_argument_validation_without_gpu(lib):
    _keep, D = _dummy()

    def err():
        return lib.scpqp_last_error()

    def predict(B=0, n_obst=3, hp=10, rows=None, t=0.4, lead=0.43, dt=0.4, out=None):
        return lib.scpqp_obstacles_predict(B, n_obst, hp, rows, t, lead, dt, out, None)

    assert predict() == 0                                   # B = 0: a no-op, NULL arrays
    assert predict(B=-1) == E_ARG and b"batch" in err()
    for n in (0, -1, LB.MAX_OBST + 1):
        assert predict(n_obst=n) == E_ARG and b"n_obst" in err()
    assert predict(n_obst=LB.MAX_OBST) == 0
    for hp in (0, -3, LB.MAX_HP + 1):
        assert predict(hp=hp) == E_ARG and b"hp" in err()
    assert predict(hp=LB.MAX_HP) == 0
    for kw in (dict(t=math.nan), dict(lead=math.inf), dict(dt=-math.inf)):
        assert predict(**kw) == E_ARG and b"finite" in err()
    assert predict(B=3, out=D) == E_ARG and b"rows" in err()          # a NULL rows pointer
    assert predict(B=3, rows=D) == E_ARG and b"output" in err()
    assert predict(B=1 << 22, n_obst=32, hp=64, rows=D, out=D) == E_SIZE and b"too large" in err()
    assert predict(B=1 << 22, n_obst=32, hp=64) == E_SIZE            # sizes before the pointers

    def pose(B=0, n_obst=3, rows=None, tl=0.01, tick0=0, n_ticks=40, out=None):
        return lib.scpqp_obstacles_pose(B, n_obst, rows, tl, tick0, n_ticks, out, None)

    assert pose() == 0
    assert pose(B=-1) == E_ARG
    for n in (0, LB.MAX_OBST + 1):
        assert pose(n_obst=n) == E_ARG and b"n_obst" in err()
    for tl in (0.0, -0.01, math.inf, math.nan):
        assert pose(tl=tl) == E_ARG and b"tick_length" in err()
    assert pose(tick0=-1) == E_ARG and b"tick0" in err()
    assert pose(n_ticks=-1) == E_ARG and b"n_ticks" in err()
    assert pose(tick0=2 ** 31 - 1, n_ticks=1) == E_SIZE
    assert pose(B=3, out=D) == E_ARG and b"rows" in err()
    assert pose(B=3, rows=D) == E_ARG and b"output" in err()
    assert pose(B=1 << 16, n_obst=32, n_ticks=2000, rows=D, out=D) == E_SIZE and b"too large" in err()
    assert pose(B=1, n_obst=32, n_ticks=2 ** 31 - 2) == E_SIZE


def _dist(n_obst=2):
    d = LB.ObstacleDist()
    d.n_obst = n_obst
    for o in range(LB.MAX_OBST):
        d.mean[LB.OBST_X][o], d.mean[LB.OBST_Y][o] = 7.0, -3.0
        d.mean[LB.OBST_HEADING][o], d.mean[LB.OBST_SPEED][o] = 1.5, 2.0
        d.mean[LB.OBST_LENGTH][o], d.mean[LB.OBST_WIDTH][o] = 4.0, 2.0
    d.seed = 5
    return d


def _field(d, f, kind, spread=0.0, lo=-math.inf, hi=math.inf):
    d.field[f].kind, d.field[f].spread, d.field[f].lo, d.field[f].hi = kind, spread, lo, hi
    return d


def test_sample_and_fill_argument_validation_without_gpu(lib):
    _keep, D = _dummy()

    def sample(d, B=0, out=None):
        return lib.scpqp_obstacles_sample(None if d is None else C.byref(d), B, out, None)

    def err():
        return lib.scpqp_last_error()

    assert sample(None) == E_ARG and b"null" in err()
    assert sample(_dist()) == 0                           # all FIXED at nominal, B = 0, NULL array
    for n in (0, -1, LB.MAX_OBST + 1):
        assert sample(_dist(n)) == E_ARG and b"n_obst" in err()
    for f, name in enumerate(LB.OBSTACLE_FIELDS):
        nm = name.encode()
        for kind in (-1, 3):
            assert sample(_field(_dist(), f, kind)) == E_ARG and nm in err() and b"kind" in err()
        for kind in (U, N):
            for s in (-1e-3, math.inf, math.nan):
                assert sample(_field(_dist(), f, kind, s, 0.01, 1.0)) == E_ARG
                assert nm in err() and b"spread" in err()
            assert sample(_field(_dist(), f, kind, 0.01, 1.0, 0.5)) == E_ARG
            assert nm in err() and b"lo" in err()
            assert sample(_field(_dist(), f, kind, 0.01, math.nan, 0.5)) == E_ARG
            assert sample(_field(_dist(), f, kind, 0.01, 0.05, 1.0)) == 0
        # a FIXED field ignores spread, lo and hi
        assert sample(_field(_dist(), f, F, -1.0, 2.0, 1.0)) == 0
        # a non-finite mean, fixed or not, inside n_obst only
        for bad in (math.nan, math.inf):
            d = _dist()
            d.mean[f][1] = bad
            assert sample(d) == E_ARG and nm in err() and b"mean" in err()
            assert sample(_field(d, f, U, 0.1, 0.0, 1.0)) == E_ARG and nm in err()
            d.n_obst = 1                                  # obstacle 1 is outside: not looked at
            assert sample(d) == 0
    # a distribution that could emit a bad row: the footprint's floor below 0
    for f in (LB.OBST_LENGTH, LB.OBST_WIDTH):
        nm = LB.OBSTACLE_FIELDS[f].encode()
        assert sample(_field(_dist(), f, U, 0.5)) == E_ARG and nm in err()          # lo = -inf
        assert sample(_field(_dist(), f, N, 0.5, -1e-9, 5.0)) == E_ARG and nm in err()
        assert sample(_field(_dist(), f, U, 0.5, 0.0, 5.0)) == 0
        d = _dist()
        d.mean[f][0] = -0.5                               # FIXED: its floor is the mean
        assert sample(d) == E_ARG and nm in err() and b">= 0" in err()
    # the other fields need no floor
    assert sample(_field(_dist(), LB.OBST_YAW_RATE, U, 0.3)) == 0
    assert sample(_field(_dist(), LB.OBST_SPEED, N, 0.3)) == 0
    # sizes and arrays
    assert sample(_dist(), B=-1) == E_ARG
    assert sample(_dist(), B=3) == E_ARG and b"rows" in err()
    assert sample(_dist(32), B=1 << 30, out=D) == E_SIZE

    host = (C.c_double * (6 * LB.MAX_OBST))(*([7.0, 1.0, 0.5, 2.0, 4.0, 2.0] * LB.MAX_OBST))

    def fill(n_obst=2, ob=host, B=0, out=None):
        return lib.scpqp_obstacles_fill_nominal(n_obst, ob, B, out, None)

    assert fill() == 0
    assert fill(ob=None) == E_ARG and b"null" in err()
    for n in (0, LB.MAX_OBST + 1):
        assert fill(n_obst=n) == E_ARG and b"n_obst" in err()
    assert fill(B=-1) == E_ARG
    assert fill(B=3) == E_ARG and b"rows" in err()
    assert fill(n_obst=32, B=1 << 30, out=D) == E_SIZE
    bad = (C.c_double * 12)(*([7.0, 1.0, 0.5, 2.0, 4.0, 2.0] * 2))
    bad[11] = -1.0
    assert fill(ob=bad) == E_ARG and b"width" in err()
    assert fill(n_obst=1, ob=bad) == 0
    bad[11], bad[3] = 2.0, math.nan
    assert fill(ob=bad) == E_ARG and b"speed" in err()


def test_metrics_accumulate_obstacles_argument_validation_without_gpu(lib):
    """The handle is never dereferenced before the arguments that need none of it are
    checked; a NULL handle is refused (creating one needs a device)."""
    _keep, D = _dummy()
    acc = LB.MetricsAcc(**{k: D.value for k in LB.METRICS_ACC_FIELDS})

    def call(m=None, B=1, n_ticks=40, tick0=0, k_first=0, x=D, a=C.byref(acc), var=None, rows=D):
        return lib.scpqp_metrics_accumulate_obstacles(m, B, n_ticks, tick0, k_first, x, a, None,
                                                      var, rows, None)

    def err():
        return lib.scpqp_last_error()

    assert call(B=-1) == E_ARG
    assert call(n_ticks=-1) == E_ARG
    assert call(tick0=-1) == E_ARG and b"tick0" in err()
    assert call(k_first=2) == E_ARG and b"k_first" in err()
    assert call(tick0=2 ** 31 - 1, n_ticks=1) == E_SIZE
    assert call() == E_ARG and b"handle" in err()
    assert call(B=0, rows=None) == E_ARG and b"handle" in err()


# ---------------------------------------------------------------------------
# 3. the mirror is pinned by the oracle and by closed forms
# ---------------------------------------------------------------------------
def test_mirror_straight_rows_are_the_oracle_bitwise():
    """YAW_RATE == 0: the mirror's pose is oracle.plant_reference.obstacle_state and its
    prediction obstacle_prediction, bit for bit (frog: 22 moving obstacles)."""
    sc = R.frog_scenario(Hp=10)
    rows = OM.nominal_rows(sc)[None]
    assert rows.shape == (1, 22, 7) and np.all(rows[..., OM.YAW_RATE] == 0.0)
    lead = sc.delay_x + sc.dt + sc.delay_u
    for tick in (0, 1, 40, 77, 1999):
        want = PR.obstacle_state(sc, tick)
        got = OM.poses(rows, sc.tick_length, tick, 0)[0, :, 0]
        assert np.array_equal(got[:, 0:2], want)
        assert np.array_equal(got[:, 2], rows[0, :, OM.HEADING])
        # the reference adds delay_x, dt and delay_u to (k + 1) dt one by one
        pred = OM.predict(rows, tick * sc.tick_length, (sc.delay_x, sc.dt, sc.delay_u), sc.dt,
                          sc.Hp)[0]
        want = PR.obstacle_prediction(sc, tick)
        assert np.array_equal(pred, want)
        # the entry point takes their sum: a few ulp of the coordinates (< 128 m) at the most
        summed = OM.predict(rows, tick * sc.tick_length, lead, sc.dt, sc.Hp)[0]
        assert np.abs(summed - want).max() <= 4 * 2.0 ** -46


ARCS = [  # x, y, heading, speed, length, width, yaw rate
    np.array([7.0, -15.0, math.pi / 2, 2.0, 4.0, 2.0, 0.3]),
    np.array([-20.0, 33.0, -2.5, 5.0, 1.0, 1.0, -1.1]),
    np.array([60.0, 60.0, 0.1, 0.7, 2.0, 3.0, 0.05]),
]


@pytest.mark.parametrize("row", ARCS)
def test_mirror_turning_rows_run_a_circle(row):
    """w != 0: the obstacle stays at distance s / |w| from the centre
    (x - s / w sin h, y + s / w cos h) and is back at its start after t = 2 pi / |w|.

    Tolerance.  The pose is  x + chord * cos(h + a)  with chord = 2 (s / w) sin a up to a
    few roundings: its error is a few ulp of the radius rho = s / |w| from the roundings of
    a, h + a, sinc and the products (each relative 2^-53, the argument errors of cos
    enter as rho * (|h| + |a|) * 2^-53 with |h| + |a| <= 2 pi here), plus half an ulp of the
    coordinate from the final sum.  The scale is m = max(|x|, |y|) + 2 rho, and 32 ulp of
    it covers  (2 pi + 6) rho 2^-53 + 2^-53 m  with room for the centre's own rounding."""
    x, y, h, s, w = row[OM.X], row[OM.Y], row[OM.HEADING], row[OM.SPEED], row[OM.YAW_RATE]
    rho = s / abs(w)
    cx, cy = x - s / w * math.sin(h), y + s / w * math.cos(h)
    tol = 32 * 2.0 ** -53 * (max(abs(x), abs(y)) + 2 * rho)
    period = 2 * math.pi / abs(w)
    worst = 0.0
    for t in np.linspace(0.0, period, 97):
        px, py, ph = OM.pose(row, t)
        worst = max(worst, abs(math.hypot(px - cx, py - cy) - rho))
        assert ph == h + w * t
    px, py, _ = OM.pose(row, period)
    back = math.hypot(px - x, py - y)
    print(f"radius error {worst:.2e}, return error {back:.2e}, tolerance {tol:.2e}")
    assert worst <= tol and back <= tol
    # a quarter turn is where the closed form says
    px, py, _ = OM.pose(row, period / 4)
    sg = math.copysign(1.0, w)
    assert abs(px - (cx + rho * math.sin(h + sg * math.pi / 2) * sg)) <= tol
    assert abs(py - (cy - rho * math.cos(h + sg * math.pi / 2) * sg)) <= tol


def test_mirror_is_continuous_across_the_sinc_switch():
    """At |a| = 1e-4 the series and sin(a) / a agree to an ulp (a^4 / 120 = 8e-19), so the
    pose does not jump where the branch changes; and a turn rate going to 0 approaches the
    straight line."""
    a0 = OM.SINC_SWITCH
    lo, hi = np.nextafter(a0, 0.0), a0
    assert abs(lo) < a0 <= abs(hi)
    assert abs(OM.sinc(lo) - OM.sinc(hi)) <= 2.0 ** -52
    assert abs(OM.sinc(-lo) - OM.sinc(-hi)) <= 2.0 ** -52
    assert abs((1.0 - a0 * a0 / 6.0) - math.sin(a0) / a0) <= 2.0 ** -52
    row = np.array([3.0, -4.0, 0.7, 2.0, 4.0, 2.0, 0.0])
    t = 10.0
    for w in (2 * lo / t, 2 * hi / t, -2 * lo / t, -2 * hi / t):
        r = row.copy()
        r[OM.YAW_RATE] = w
        p, q = OM.pose(r, t), OM.pose(r, np.nextafter(t, 100.0))
        assert math.hypot(p[0] - q[0], p[1] - q[1]) <= 1e-13
    prev = None
    for w in (1e-3, 1e-5, 1e-7, 1e-9):
        r = row.copy()
        r[OM.YAW_RATE] = w
        p, s = OM.pose(r, t), OM.pose(row, t)
        d = math.hypot(p[0] - s[0], p[1] - s[1])
        assert d <= 0.5 * row[OM.SPEED] * t * (w * t) + 1e-14      # the arc leaves by s t a
        assert prev is None or d < prev
        prev = d


def test_mirror_prediction_extrapolates_the_measured_pose_straight():
    row = ARCS[0]
    rows = row[None, None]
    t_meas, lead, dt = 1.6, 0.43, 0.4
    x, y, h = OM.pose(row, t_meas)
    pred = OM.predict(rows, t_meas, lead, dt, 5)[0, 0]
    for k in range(5):
        d = ((k + 1) * dt + lead) * row[OM.SPEED]
        assert pred[0, k] == d * math.cos(h) + x and pred[1, k] == d * math.sin(h) + y
    bad = np.stack([row, row])[None].copy()
    bad[0, 1, OM.WIDTH] = -1.0
    p = OM.predict(bad, t_meas, lead, dt, 5)
    assert np.isnan(p[0, 1]).all() and np.array_equal(p[0, 0], pred)
    assert np.isnan(OM.poses(bad, 0.01, 0, 3)[0, 1]).all()


def test_mirror_sampler():
    mean = OM.nominal_rows(R.parallel_scenario(5, Hp=10)).T
    d = OM.Dist(mean, 11)
    s = OM.sample(d, 5)
    assert s.shape == (5, 4, 7)
    assert np.array_equal(s, np.broadcast_to(mean.T[None], s.shape))     # FIXED: exactly the mean
    d.set(OM.YAW_RATE, OM.UNIFORM, 0.3).set(OM.LENGTH, OM.NORMAL, 1.0, 1.0, 5.0)
    s = OM.sample(d, 400)
    assert np.all(np.abs(s[..., OM.YAW_RATE]) <= 0.3) and s[..., OM.YAW_RATE].min() < -0.25
    assert np.all(s[..., OM.LENGTH] >= 1.0) and (s[..., OM.LENGTH] == 1.0).any()
    assert (s[..., OM.LENGTH] == 5.0).any()
    x = OM.xi(d, 8)
    assert not np.any(x[:, 0, OM.YAW_RATE] == x[:, 1, OM.YAW_RATE])     # obstacles: own counters
    assert np.all(x[..., OM.X] == 0.0)                                   # a FIXED field draws nothing
    whole = OM.sample(d, 6)
    d2 = OM.Dist(mean, 11, 3).set(OM.YAW_RATE, OM.UNIFORM, 0.3).set(OM.LENGTH, OM.NORMAL, 1.0, 1.0, 5.0)
    assert np.array_equal(whole, np.concatenate([OM.sample(d, 3), OM.sample(d2, 3)]))
    # site 4: no counter shared with the truth sampler's site 3 at the same seed
    import truth_mirror as TM
    td = TM.Dist(np.ones((5, 4)), 11).set(TM.LF, TM.UNIFORM, 1.0)
    od = OM.Dist(mean, 11).set(OM.X, OM.UNIFORM, 1.0)
    assert not np.any(TM.xi(td, 8)[..., TM.LF] == OM.xi(od, 8)[..., OM.X])


def test_row_constants_with_nominal_rows_are_the_constant_obstacles():
    import metrics_mirror as MM
    sc = R.frog_scenario(Hp=10)
    base = MM.Constants.of_scenario(sc)
    rc = OM.RowConstants(base, OM.nominal_rows(sc))
    for o in (0, 7, 21):
        for tick in (0, 41, 1999):
            assert rc.obstacle_rect(o, tick) == base.obstacle_rect(o, tick)
    rows = OM.nominal_rows(sc)
    rows[3, OM.YAW_RATE] = 0.4
    rows[3, OM.LENGTH] = 1.0
    r = OM.RowConstants(base, rows).obstacle_rect(3, 100)
    h = rows[3, OM.HEADING] + 0.4 * 1.0
    assert r[2:] == (math.cos(h), math.sin(h), 0.5, rows[3, OM.WIDTH] / 2)


# ---------------------------------------------------------------------------
# 4. scpqp.obstacles on the host
# ---------------------------------------------------------------------------
def test_nominal_rows_and_validate():
    sc = R.frog_scenario(Hp=10)
    rows = OB.nominal_rows(sc)
    assert rows.shape == (22, 7) and np.array_equal(rows, OM.nominal_rows(sc))
    assert np.array_equal(rows[:, :6], np.asarray(sc.obstacles)) and np.all(rows[:, 6] == 0.0)
    assert OB.nominal_rows(R.circle_scenario(2)).shape == (0, 7)
    good = np.broadcast_to(rows[None], (3, 22, 7)).copy()
    OB.validate(good)
    for f, name in enumerate(OB.FIELDS):
        for bad in (math.nan, math.inf, -math.inf):
            t = good.copy()
            t[2, 21, f] = bad
            with pytest.raises(ValueError, match=rf"rows\[2, 21\]: {name} is not finite"):
                OB.validate(t)
    for f, name in ((4, "length"), (5, "width")):
        t = good.copy()
        t[1, 3, f] = -1e-9
        with pytest.raises(ValueError, match=rf"rows\[1, 3\]: {name} must be >= 0"):
            OB.validate(t)
        t[1, 3, f] = 0.0
        OB.validate(t)
    with pytest.raises(ValueError, match=r"\[B, nObst, 7\]"):
        OB.validate(good[..., :6])
    with pytest.raises(ValueError, match=r"\[B, nObst, 7\]"):
        OB.validate(good[0])


def test_obstacle_dist_object():
    sc = R.parallel_scenario(5, Hp=10)
    d = OB.ObstacleDist(sc, seed=9, b_offset=4)
    c = d.c_struct()
    assert (c.n_obst, c.seed, c.b_offset) == (4, 9, 4)
    assert [c.field[f].kind for f in range(7)] == [F] * 7
    assert [c.mean[f][1] for f in range(7)] == [-2.0, -7.0, 0.0, 0.0, 4.0, 2.0, 0.0]
    d.uniform("yaw_rate", 0.3).normal("speed", 0.5, 0.0, 3.0).fixed("length", [1, 2, 3, 4])
    c = d.c_struct()
    assert (c.field[6].kind, c.field[6].spread, c.field[6].lo, c.field[6].hi) == (U, 0.3, -math.inf,
                                                                                 math.inf)
    assert (c.field[3].kind, c.field[3].spread, c.field[3].lo, c.field[3].hi) == (N, 0.5, 0.0, 3.0)
    assert c.field[4].kind == F and [c.mean[4][o] for o in range(4)] == [1.0, 2.0, 3.0, 4.0]
    e = d.with_offset(100)
    assert (e.b_offset, d.b_offset, e.seed) == (100, 4, 9) and e.kind == d.kind
    e.fixed("x", 0.0)
    assert d.mean[0, 0] == -15.0                           # with_offset copies
    for bad, what in ((lambda: d.uniform("mass", 0.1), "unknown obstacle field"),
                      (lambda: d.uniform("x", -0.1), "x: spread"),
                      (lambda: d.uniform("heading", math.nan), "heading: spread"),
                      (lambda: d.normal("speed", 0.1, 1.0, 0.5), "speed: lo must be <= hi"),
                      (lambda: d.uniform("width", 0.5), "width: lo must be >= 0"),
                      (lambda: d.normal("length", 0.5, -0.1, 3.0), "length: lo must be >= 0"),
                      (lambda: d.fixed("width", -1.0), "width: a fixed value must be >= 0"),
                      (lambda: d.fixed("y", math.nan), "y: a fixed value must be finite"),
                      (lambda: d.uniform(7, 0.1), "out of range"),
                      (lambda: OB.ObstacleDist(sc, seed=-1), "seed"),
                      (lambda: OB.ObstacleDist(sc, seed=1, b_offset=2 ** 32), "b_offset"),
                      (lambda: OB.ObstacleDist(R.circle_scenario(2), seed=1), "obstacles")):
        with pytest.raises(ValueError, match=what):
            bad()


def test_from_table_gathers_rows():
    import torch
    rows = np.arange(3 * 2 * 7, dtype=float).reshape(3, 2, 7)
    t = OB.from_table(rows, [2, 0, 0, 1], device="cpu")
    assert t.dtype == torch.float64 and tuple(t.shape) == (4, 2, 7) and t.is_contiguous()
    assert np.array_equal(t.numpy(), rows[[2, 0, 0, 1]])
    with pytest.raises(ValueError):
        OB.from_table(rows, [3], device="cpu")
    with pytest.raises(ValueError):
        OB.from_table(rows[..., :6], [0], device="cpu")


def test_the_wrappers_refuse_host_rows():
    import torch
    rows = torch.zeros((2, 3, 7), dtype=torch.float64)
    for call in (lambda: OB.predict(rows, 0.0, 0.43, 0.4, 10), lambda: OB.pose(rows, 0.01, 0, 4),
                 lambda: OB.predict(np.zeros((2, 3, 7)), 0.0, 0.43, 0.4, 10)):
        with pytest.raises(ValueError, match="on the GPU"):
            call()
