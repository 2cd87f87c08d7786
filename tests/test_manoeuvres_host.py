"""Obstacle manoeuvres, the parts that need no GPU: the C-ABI of include/scpqp_manoeuvres.h
(exports, constants and the dist layout by a gcc probe of the header, argument validation
without touching a device), the CPU mirror's anchors (tests/manoeuvre_mirror.py) and
scpqp.manoeuvres' host side.

Bounds.  p and r against an 80-bit evaluation, asserted at twice the figures
include/scpqp_manoeuvres.h states: the series 8e-16 relative on (1e-6, 0.1), the closed forms
1e-13 relative on [0.1, 0.5] and 2.2e-14 absolute up to 12, the two branches 8e-14 apart at
0.999, 1 and 1.001 times the switch.  One piece against a 40-point Gauss-Legendre quadrature
of (s + a tau)(cos, sin)(h + w tau): 8.6e-14 m over 2000 pieces with s <= 15, a in [-4, 3],
T <= 3 and |w| <= 0.6.  The pose against a classical Runge-Kutta integration of the ODE, cut
at the piece boundaries and at the stop, 400 steps per cut: the local error h^5 |w|^4 s / 2880
sums to below 1e-10 m with h <= 0.0075 s, |w| <= 0.9 rad/s and s <= 15 m/s; asserted at 1e-9 m.
A coast split in two against the unsplit arc: 1e-13 relative to max(1, |value|), three
roundings of coordinates below 64 m."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import manoeuvre_mirror as MNM
import obstacle_mirror as OM
from scpqp import _lib as LB
from scpqp import manoeuvres as MAN
from scpqp.build import LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scpqp_manoeuvres.h")
E_ARG, E_SIZE = -1, -4
LD = np.longdouble


def header_functions(path=HEADER):
    txt = open(path).read()
    return sorted(set(re.findall(r"^(?:int|const char\*)\s+(scpqp_\w+)\(", txt, re.M)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        pytest.fail("libscpqp.so not built: run __graft_entry__.build()")
    return LB.load()


# ---------------------------------------------------------------------------
# 1. boundary
# ---------------------------------------------------------------------------
def test_manoeuvres_header_declares_the_boundary():
    assert header_functions() == sorted(LB.MAN_EXPORTS) == [
        "scpqp_manoeuvres_pose", "scpqp_manoeuvres_sample", "scpqp_manoeuvres_state",
        "scpqp_metrics_accumulate_posed"]
    others = (set(LB.EXPORTS) | set(LB.NOISE_EXPORTS) | set(LB.METRICS_EXPORTS)
              | set(LB.VARIANT_EXPORTS) | set(LB.TRUTH_EXPORTS) | set(LB.OBSTACLE_EXPORTS)
              | set(LB.SENSE_EXPORTS) | set(LB.EST_EXPORTS) | set(LB.TRK_EXPORTS))
    assert not set(LB.MAN_EXPORTS) & others
    txt = open(HEADER).read()
    for word in ("Off lane", "Bad lane", "Snapshot row", "Stopped obstacles", "tau_stop",
                 "SCPQP_MAN_PR_SWITCH", "Site 8"):
        assert word in txt, word


def test_scpqp_h_function_list_is_unchanged():
    got = header_functions(os.path.join(ROOT, "include", "scpqp.h"))
    assert got == sorted(LB.EXPORTS)
    assert not any("manoeuvre" in name for name in got)


def test_library_exports_the_manoeuvre_symbols(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\sT\s(scpqp_\w+)", out))
    assert set(header_functions()) <= exported
    for name in LB.MAN_EXPORTS:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "scpqp_manoeuvres.h"
int main(void) {
  printf("nseg %d\n", SCPQP_MAN_NSEG);
  printf("nf %d\n", SCPQP_MAN_NF);
  printf("idx %d%d%d\n", SCPQP_MAN_DUR, SCPQP_MAN_ACCEL, SCPQP_MAN_DYAW);
  printf("switch %.17g\n", SCPQP_MAN_PR_SWITCH);
  printf("site %d\n", SCPQP_NOISE_SITE_MANOEUVRE);
  printf("size %zu\n", sizeof(scpqp_manoeuvres_dist));
  printf("mean %zu\n", offsetof(scpqp_manoeuvres_dist, mean));
  printf("field %zu\n", offsetof(scpqp_manoeuvres_dist, field));
  printf("seed %zu\n", offsetof(scpqp_manoeuvres_dist, seed));
  printf("b_offset %zu\n", offsetof(scpqp_manoeuvres_dist, b_offset));
  printf("fsize %zu\n", sizeof(scpqp_truth_field));
  return 0;
}
"""


def test_manoeuvre_ctypes_layout_matches_header(tmp_path, lib):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", f"-I{os.path.dirname(HEADER)}", str(src), "-o", str(exe)],
                   check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["nseg"]) == LB.MAN_NSEG == MNM.NSEG == MAN.NSEG == 4
    assert int(got["nf"]) == LB.MAN_NF == MNM.NF == MAN.NF == 3
    assert got["idx"] == "012"
    assert (LB.MAN_DUR, LB.MAN_ACCEL, LB.MAN_DYAW) == (0, 1, 2) == (MNM.DUR, MNM.ACCEL, MNM.DYAW)
    assert float(got["switch"]) == LB.MAN_PR_SWITCH == MNM.PR_SWITCH == 0.1
    assert int(got["site"]) == LB.NOISE_SITE_MANOEUVRE == MNM.SITE_MANOEUVRE == 8
    sites = {LB.NOISE_SITE_DELAY, LB.NOISE_SITE_PLANT, LB.NOISE_SITE_LINEARIZE, LB.NOISE_SITE_TRUTH,
             LB.NOISE_SITE_OBSTACLE, LB.NOISE_SITE_SENSE, LB.NOISE_SITE_SENSE_DRAW,
             LB.NOISE_SITE_SENSE_OBST}
    assert sites == set(range(8))
    D = LB.ManoeuvreDist
    assert int(got["size"]) == C.sizeof(D)
    for name in ("mean", "field", "seed", "b_offset"):
        assert int(got[name]) == getattr(D, name).offset, name
    assert int(got["fsize"]) == C.sizeof(LB.TruthField)
    # the declared argument lists, in the header's order
    txt = open(HEADER).read()
    for fn in LB.MAN_EXPORTS:
        proto = re.search(rf"int {fn}\((.*?)\);", txt, re.S).group(1)
        args = [a.strip() for a in proto.replace("\n", " ").split(",")]
        types = getattr(lib, fn).argtypes
        assert len(args) == len(types), fn
        for a, t in zip(args, types):
            if a.startswith("double "):
                assert t is C.c_double, (fn, a)
            elif a.startswith("int32_t "):
                assert t is C.c_int32, (fn, a)
            else:
                assert "*" in a and t is not C.c_double and t is not C.c_int32, (fn, a)


def test_argument_validation_without_gpu(lib):
    buf = (C.c_double * 256)()
    D = C.cast(buf, C.c_void_p)

    def err():
        return lib.scpqp_last_error()

    def state(B=0, n_obst=3, rows=None, man=None, t=0.5, out=None):
        return lib.scpqp_manoeuvres_state(B, n_obst, rows, man, t, out, None)

    def pose(B=0, n_obst=3, rows=None, man=None, tick=0.01, tick0=0, n_ticks=4, out=None):
        return lib.scpqp_manoeuvres_pose(B, n_obst, rows, man, tick, tick0, n_ticks, out, None)

    assert state() == 0 and pose() == 0                      # B = 0: a no-op, NULL arrays
    assert state(t=0.0) == 0
    for fn in (state, pose):
        assert fn(B=-1) == E_ARG and b"batch" in err()
        for n in (0, -1, LB.MAX_OBST + 1):
            assert fn(n_obst=n) == E_ARG and b"n_obst" in err()
        assert fn(B=1 << 27, n_obst=2, rows=D, man=D, out=D) == E_SIZE and b"12" in err()
        assert fn(B=2, man=D, out=D) == E_ARG and b"rows" in err()
        assert fn(B=2, rows=D, man=D) == E_ARG and b"output" in err()
    for t in (-1e-9, math.nan, math.inf):
        assert state(t=t) == E_ARG and b"t must be" in err()
    for tick in (0.0, -0.01, math.nan, math.inf):
        assert pose(tick=tick) == E_ARG and b"tick_length" in err()
    assert pose(tick0=-1) == E_ARG and b"tick0" in err()
    assert pose(n_ticks=-1) == E_ARG and b"n_ticks" in err()
    assert pose(B=1 << 15, n_obst=8, n_ticks=1 << 12, rows=D, man=D, out=D) == E_SIZE
    assert b"n_ticks + 1" in err()

    # the sampler
    def dist():
        d = LB.ManoeuvreDist()
        d.n_obst = 3
        d.seed = 5
        return d

    assert lib.scpqp_manoeuvres_sample(C.byref(dist()), 0, None, None) == 0
    assert lib.scpqp_manoeuvres_sample(None, 0, None, None) == E_ARG and b"distribution" in err()
    assert lib.scpqp_manoeuvres_sample(C.byref(dist()), -1, None, None) == E_ARG and b"batch" in err()
    assert lib.scpqp_manoeuvres_sample(C.byref(dist()), 2, None, None) == E_ARG and b"output" in err()
    assert lib.scpqp_manoeuvres_sample(C.byref(dist()), 1 << 27, D, None) == E_SIZE
    d = dist()
    d.n_obst = 0
    assert lib.scpqp_manoeuvres_sample(C.byref(d), 0, None, None) == E_ARG and b"n_obst" in err()
    for (i, f), setup, word in (
            ((1, 0), dict(kind=LB.TRUTH_UNIFORM, spread=1.0, lo=-0.1, hi=2.0), b"piece 1 field dur: lo"),
            ((2, 0), dict(kind=LB.TRUTH_NORMAL, spread=1.0, lo=-math.inf, hi=2.0), b"piece 2 field dur: lo"),
            ((3, 0), dict(kind=LB.TRUTH_FIXED, mean=-0.5), b"piece 3 field dur: a fixed duration"),
            ((0, 1), dict(kind=3), b"piece 0 field accel: kind"),
            ((0, 2), dict(kind=LB.TRUTH_NORMAL, spread=-1.0, lo=0.0, hi=1.0), b"piece 0 field dyaw: spread"),
            ((1, 1), dict(kind=LB.TRUTH_UNIFORM, spread=1.0, lo=2.0, hi=1.0), b"piece 1 field accel: lo"),
            ((1, 2), dict(kind=LB.TRUTH_FIXED, mean=math.nan), b"piece 1 field dyaw: the mean")):
        d = dist()
        for k, v in setup.items():
            if k == "mean":
                d.mean[i][f] = v
            else:
                setattr(d.field[i][f], k, v)
        assert lib.scpqp_manoeuvres_sample(C.byref(d), 0, None, None) == E_ARG, word
        assert word in err(), (word, err())
    ok = dist()                                              # a negative acceleration is legal
    ok.field[1][1].kind, ok.field[1][1].spread = LB.TRUTH_UNIFORM, 1.0
    ok.field[1][1].lo, ok.field[1][1].hi, ok.mean[1][1] = -4.0, 0.0, -2.0
    assert lib.scpqp_manoeuvres_sample(C.byref(ok), 0, None, None) == 0

    # the posed metrics: everything that can be refused without a handle
    acc = LB.MetricsAcc()

    def posed(B=0, n_ticks=4, tick0=0, k_first=0, m=None):
        return lib.scpqp_metrics_accumulate_posed(m, B, n_ticks, tick0, k_first, D, C.byref(acc),
                                                  None, None, D, D, None)

    assert posed(B=-1) == E_ARG and b"batch" in err()
    assert posed(n_ticks=-1) == E_ARG
    assert posed(tick0=-1) == E_ARG and b"tick0" in err()
    assert posed(k_first=2) == E_ARG and b"k_first" in err()
    assert posed() == E_ARG and b"handle" in err()


# ---------------------------------------------------------------------------
# 2. mirror anchors: p, r, one piece
# ---------------------------------------------------------------------------
def _need_long_double():
    if np.finfo(LD).eps > 1e-18:
        pytest.fail("numpy's long double is not an 80-bit type on this machine")


def _p_ld(th):
    th = LD(th)
    if abs(th) < 0.3:       # the 80-bit closed form cancels below: a series to its rounding
        t2, term, acc, k = th * th, LD(1) / 2, LD(0), 0
        while abs(term) > LD(1e-30):
            acc += term
            k += 1
            term = -term * t2 * LD(2 * k + 1) / (LD(2 * k - 1) * LD(2 * k + 1) * LD(2 * k + 2))
        return acc
    return (np.cos(th) + th * np.sin(th) - 1) / (th * th)


def _r_ld(th):
    th = LD(th)
    if abs(th) < 0.3:
        t2, term, acc, k = th * th, th / 3, LD(0), 0
        while abs(term) > LD(1e-30):
            acc += term
            k += 1
            term = -term * t2 * LD(2 * k + 2) / (LD(2 * k) * LD(2 * k + 2) * LD(2 * k + 3))
        return acc
    return (np.sin(th) - th * np.cos(th)) / (th * th)


def test_the_long_double_references_agree_with_their_closed_forms():
    _need_long_double()
    for th in (0.29, 0.2, 0.1):
        t = LD(th)
        assert abs(float(_p_ld(th) - (np.cos(t) + t * np.sin(t) - 1) / (t * t))) < 1e-16
        assert abs(float(_r_ld(th) - (np.sin(t) - t * np.cos(t)) / (t * t))) < 1e-16
    assert float(_p_ld(1e-9)) == 0.5 and abs(float(_r_ld(3e-9)) - 1e-9) < 1e-24


def test_p_and_r_series_against_long_double():
    _need_long_double()
    worst = 0.0
    for th in np.concatenate([np.logspace(-6, -1, 400, endpoint=False), [0.0999, 0.999 * 0.1]]):
        for sign in (1.0, -1.0):
            t = sign * float(th)
            worst = max(worst, abs(float((LD(MNM.p_series(t)) - _p_ld(t)) / _p_ld(t))),
                        abs(float((LD(MNM.r_series(t)) - _r_ld(t)) / _r_ld(t))))
    print(f"series: largest relative error {worst:.2e}")
    assert worst <= 2 * 4e-16
    assert MNM.p_of(0.0) == 0.5 and MNM.r_of(0.0) == 0.0


def test_p_and_r_closed_forms_against_long_double():
    _need_long_double()
    rel = ab = 0.0
    for th in np.concatenate([np.linspace(0.1, 0.5, 200), np.logspace(-1, math.log10(12.0), 300)]):
        for sign in (1.0, -1.0):
            t = sign * float(th)
            dp = abs(float(LD(MNM.p_closed(t)) - _p_ld(t)))
            dr = abs(float(LD(MNM.r_closed(t)) - _r_ld(t)))
            ab = max(ab, dp, dr)
            if th <= 0.5:
                rel = max(rel, dp / abs(float(_p_ld(t))), dr / abs(float(_r_ld(t))))
    print(f"closed forms: largest relative error on [0.1, 0.5] {rel:.2e}, absolute to 12 {ab:.2e}")
    assert rel <= 2 * 5e-14 and ab <= 2 * 1.1e-14


@pytest.mark.parametrize("factor", [0.999, 1.0, 1.001])
def test_both_branches_at_the_switch(factor):
    _need_long_double()
    for sign in (1.0, -1.0):
        t = sign * factor * MNM.PR_SWITCH
        assert abs(MNM.p_series(t) - MNM.p_closed(t)) < 2 * 4e-14
        assert abs(MNM.r_series(t) - MNM.r_closed(t)) < 2 * 4e-14
        for got, want in ((MNM.p_of(t), _p_ld(t)), (MNM.r_of(t), _r_ld(t))):
            assert abs(float(LD(got) - want)) < 2 * 4e-14
    assert MNM.p_of(0.999 * 0.1) == MNM.p_series(0.999 * 0.1)
    assert MNM.p_of(0.1) == MNM.p_closed(0.1) and MNM.r_of(-0.1) == MNM.r_closed(-0.1)


def test_one_piece_against_quadrature():
    rng = np.random.default_rng(5)
    xg, wg = np.polynomial.legendre.leggauss(40)
    worst = 0.0
    for n in range(2000):
        s, a = rng.uniform(0.0, 15.0), rng.uniform(-4.0, 3.0)
        T = rng.uniform(0.0, 3.0)
        if a < 0.0:
            T = min(T, 0.999 * s / -a)          # the quadrature knows no stop
        w = (0.0, rng.uniform(-0.6, 0.6), rng.uniform(-0.03, 0.03) / max(T, 1e-3))[n % 3]
        h = rng.uniform(-3.0, 3.0)
        x1, y1, h1, s1, w1 = MNM.piece((0.0, 0.0, h, s), a, w, T)
        tau = 0.5 * T * (xg + 1.0)
        qx = 0.5 * T * float(np.sum(wg * (s + a * tau) * np.cos(h + w * tau)))
        qy = 0.5 * T * float(np.sum(wg * (s + a * tau) * np.sin(h + w * tau)))
        worst = max(worst, abs(x1 - qx), abs(y1 - qy))
        assert h1 == h + w * T and abs(s1 - (s + a * T)) <= 1e-15 * 16
    print(f"piece against quadrature: largest difference {worst:.2e} m")
    assert worst <= 2 * 4.3e-14


# ---------------------------------------------------------------------------
# 3. state and pose of the mirror
# ---------------------------------------------------------------------------
ROW = np.array([1.0, -2.0, 0.3, 6.0, 4.0, 2.0, 0.2])


def _rk4(row, man, t_end, n=400):
    """Classical Runge-Kutta of x' = s cos h, y' = s sin h, h' = w, s' = a, cut at the piece
    boundaries and at the stop; a standing obstacle keeps its pose."""
    x, y, h, s = (float(row[i]) for i in (0, 1, 2, 3))
    w0 = float(row[6])
    cuts = [(float(d), float(a), w0 + float(dw)) for d, a, dw in np.asarray(man).reshape(4, 3) if d > 0.0]
    cuts.append((math.inf, 0.0, w0))
    t = 0.0
    for dur, a, w in cuts:
        span = min(dur, t_end - t)
        if span <= 0.0:
            break
        t += span
        if a < 0.0:
            span = min(span, s / -a)
        elif a == 0.0 and s == 0.0:
            span = 0.0
        if span > 0.0:
            hh = span / n

            def f(u, tt):
                return np.array([(s + a * tt) * math.cos(u[2]), (s + a * tt) * math.sin(u[2]), w])
            u = np.array([x, y, h])
            for k in range(n):
                tt = k * hh
                k1 = f(u, tt)
                k2 = f(u + 0.5 * hh * k1, tt + 0.5 * hh)
                k3 = f(u + 0.5 * hh * k2, tt + 0.5 * hh)
                k4 = f(u + hh * k3, tt + hh)
                u = u + hh / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
            x, y, h = (float(v) for v in u)
            s = max(s + a * span, 0.0)
            if a < 0.0 and abs(s) < 1e-12:
                s = 0.0
    return x, y, h, s


SCHEDULES = {
    "brake to a stop, wait, start again": [(1.0, 0.0, 0.0), (3.0, -3.0, 0.1), (0.5, 0.0, 0.4), (2.0, 1.5, -0.3)],
    "lane change": [(0.7, 0.0, 0.0), (1.5, 0.0, 0.3), (1.5, 0.0, -0.3), (0.0, 0.0, 0.0)],
    "accelerate in a turn": [(0.0, 5.0, 5.0), (2.5, 2.0, 0.5), (0.0, -1.0, 0.0), (1.0, -1.0, -0.7)],
}


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_pose_against_runge_kutta(name):
    man = np.array(SCHEDULES[name])
    worst = 0.0
    for t in (0.0, 0.35, 1.0, 2.2, 3.0, 3.7, 4.5, 5.1, 6.5, 9.0):
        got = MNM.walk(ROW, man, t)
        want = _rk4(ROW, man, t)
        worst = max(worst, max(abs(g - w) for g, w in zip(got[:4], want)))
    print(f"{name}: largest |mirror - RK4| {worst:.2e}")
    assert worst <= 1e-9


def test_an_off_lane_is_the_obstacle_mirror_bitwise():
    rows = np.array([[ROW, ROW * np.array([1, 1, -1, 0.5, 1, 1, 0])]])
    off = np.zeros((1, 2, 4, 3))
    off[0, 0] = [(0.0, -3.0, 0.2), (1.5, 0.0, 0.0), (0.0, 0.0, 0.0), (2.0, -0.0, 0.0)]   # off, not zero
    assert MNM.lane_class(rows[0, 0], off[0, 0]) == 1 and MAN.is_off(off)
    for man in (off, None):
        assert np.array_equal(MNM.poses(rows, man, 0.01, 37, 9), OM.poses(rows, 0.01, 37, 9))
        st = MNM.state(rows, man, 1.234)
        for o in range(2):
            assert tuple(st[0, o, :3]) == OM.pose(rows[0, o], 1.234)
            assert np.array_equal(st[0, o, 3:], rows[0, o, 3:])


def test_a_coast_split_in_two_is_the_unsplit_arc():
    for w in (0.0, 0.2, -1.1):
        row = ROW.copy()
        row[6] = w
        split = np.array([(0.8, 0.0, 0.0), (1.3, 0.0, 1e-300), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)])
        assert MNM.lane_class(row, split) == 0
        for t in (0.5, 0.8, 1.7, 2.1, 5.0):
            got = np.array(MNM.walk(row, split, t)[:3])
            want = np.array(OM.pose(row, t))
            assert (np.abs(got - want) <= 1e-13 * np.maximum(1.0, np.abs(want))).all(), (w, t)


def test_braking_to_a_stop_freezes_the_obstacle_and_a_later_piece_restarts_it():
    man = np.array(SCHEDULES["brake to a stop, wait, start again"])
    # 6 m/s at -3 m/s^2 from t = 1: stands at t = 3, for the rest of the piece and the next
    stop = MNM.walk(ROW, man, 3.0)
    assert stop[3] == 0.0 and stop[4] == 0.0
    for t in (3.0, 3.5, 4.0, 4.2, 4.5):
        q = MNM.walk(ROW, man, t)
        assert q[:4] == stop[:4], t
    assert MNM.walk(ROW, man, 4.49)[4] == 0.0
    assert MNM.walk(ROW, man, 4.5)[4] == ROW[6] - 0.3       # on the boundary: the later piece's
    moving = MNM.walk(ROW, man, 5.5)
    assert moving[3] == 1.5 and moving[:2] != stop[:2] and moving[2] != stop[2]
    after = MNM.walk(ROW, man, 8.0)
    assert after[3] == 3.0 and after[4] == ROW[6]           # the speed reached, the row's turn rate
    # an obstacle that stands from the start under a schedule keeps its pose
    still = ROW.copy()
    still[3] = 0.0
    q = MNM.walk(still, np.array([(1.0, 0.0, 0.5)] + [(0.0, 0.0, 0.0)] * 3), 0.7)
    assert q[:4] == (1.0, -2.0, 0.3, 0.0) and q[4] == 0.0


def test_continuity_boundaries_and_times_beyond_the_schedule():
    for man in map(np.array, SCHEDULES.values()):
        bounds = np.cumsum([d for d, _, _ in man if d > 0.0])
        for tb in bounds:
            lo, at, hi = (np.array(MNM.walk(ROW, man, t)[:4]) for t in (tb * (1 - 1e-12), tb, tb * (1 + 1e-12)))
            assert np.abs(at - lo).max() < 1e-9 and np.abs(hi - at).max() < 1e-9
        end = float(bounds[-1])
        q_end = MNM.walk(ROW, man, end)
        assert q_end[4] == ROW[6] or q_end[3] == 0.0         # at the end: the row's turn rate
        far = MNM.walk(ROW, man, end + 100.0)
        assert far[3] == q_end[3]
        r_end = np.array([q_end[0], q_end[1], q_end[2], q_end[3], 4.0, 2.0, q_end[4]])
        want = np.array(OM.pose(r_end, 100.0))
        got = MNM.walk(ROW, man, end + 100.0)[:3]
        assert (np.abs(np.array(got) - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all()
    # t exactly on a boundary: the turn rate in effect is the later piece's
    man = np.array(SCHEDULES["lane change"])
    assert MNM.walk(ROW, man, 0.7)[4] == ROW[6] + 0.3
    assert MNM.walk(ROW, man, 0.7 + 1.5)[4] == ROW[6] - 0.3
    assert MNM.walk(ROW, man, 0.0)[4] == ROW[6]
    assert MNM.walk(ROW, man, 0.0)[:4] == tuple(ROW[:4])
    # the snapshot measured at its own t = 0 is the pose at t
    snap = MNM.state_lane(ROW, man, 1.9)
    assert OM.pose(snap, 0.0) == tuple(snap[:3]) and tuple(snap[4:6]) == (4.0, 2.0)


def test_bad_lanes_of_the_mirror():
    man = np.array(SCHEDULES["lane change"])
    rows, mans = np.array([[ROW, ROW]]), np.array([[man, man]])
    for where, val in (((0, 1, 2, 1), math.nan), ((0, 1, 0, 2), math.inf), ((0, 1, 1, 0), -0.5)):
        bad = mans.copy()
        bad[where] = val
        st, ps = MNM.state(rows, bad, 1.0), MNM.poses(rows, bad, 0.01, 0, 3)
        assert np.isnan(st[0, 1]).all() and np.isnan(ps[0, 1]).all()
        assert np.isfinite(st[0, 0]).all() and np.isfinite(ps[0, 0]).all()
    back = rows.copy()
    back[0, 1, 3] = -1.0                                     # a reversing row cannot manoeuvre
    assert np.isnan(MNM.state(back, mans, 1.0)[0, 1]).all()
    assert np.isfinite(MNM.state(back, np.zeros_like(mans), 1.0)).all()     # ... but is a legal row
    neg_len = rows.copy()
    neg_len[0, 0, 4] = -1.0
    assert np.isnan(MNM.state(neg_len, None, 1.0)[0, 0]).all()


# ---------------------------------------------------------------------------
# 4. scpqp.manoeuvres' host side
# ---------------------------------------------------------------------------
def test_validate_names_the_lane_the_piece_and_the_field():
    good = MAN.rows(3, 2, MAN.brake(1.0, 3.0, 2.0), device="cpu").numpy()
    MAN.validate(good)
    MAN.validate(np.zeros((3, 2, 4, 3)))
    assert MAN.is_off(np.zeros((3, 2, 4, 3))) and not MAN.is_off(good)
    assert MAN.is_off(MAN.off(3, 2, device="cpu"))
    for (b, o, i, f), val, what in (((2, 1, 1, 1), math.nan, "accel is not finite"),
                                    ((0, 1, 3, 2), math.inf, "dyaw is not finite"),
                                    ((1, 0, 0, 0), -1e-9, "dur must be >= 0")):
        bad = good.copy()
        bad[b, o, i, f] = val
        with pytest.raises(ValueError, match=rf"man\[{b}, {o}, {i}\]: {what}"):
            MAN.validate(bad)
        with pytest.raises(ValueError):
            MAN.validate(torch.as_tensor(bad))
        assert not MAN.is_off(bad)
        assert MNM.bad_schedule(bad[b, o])
    rows = np.broadcast_to(ROW, (3, 2, 7)).copy()
    MAN.validate(good, rows)
    rows[1, 1, 3] = -0.5
    with pytest.raises(ValueError, match=r"man\[1, 1\]: a manoeuvre needs a row with speed >= 0"):
        MAN.validate(good, rows)
    MAN.validate(np.zeros((3, 2, 4, 3)), rows)
    for shape in ((3, 2, 4, 2), (3, 2, 12), (3, 2, 3, 3)):
        with pytest.raises(ValueError, match="man must be"):
            MAN.validate(np.zeros(shape))


def test_rows_composers_and_from_table():
    m = MAN.rows(4, 3, MAN.brake(np.array([[0.5], [1.0], [1.5], [2.0]]), 3.0, 10.0), device="cpu")
    assert tuple(m.shape) == (4, 3, 4, 3) and m.dtype == torch.float64
    assert m[:, 0, 0, 0].tolist() == [0.5, 1.0, 1.5, 2.0] and (m[:, :, 0, 1:] == 0).all()
    assert (m[:, :, 1] == torch.tensor([10.0, -3.0, 0.0], dtype=torch.float64)).all()
    assert (m[:, :, 2:] == 0).all()
    t = MAN.rows(2, 1, MAN.turn(1.0, 0.25, 2.0), device="cpu").numpy()
    assert t[0, 0].tolist() == [[1.0, 0, 0], [2.0, 0, 0.25], [0, 0, 0], [0, 0, 0]]
    lc = MAN.rows(2, 1, MAN.lane_change(1.0, 0.3, 1.5), device="cpu").numpy()
    assert lc[1, 0].tolist() == [[1.0, 0, 0], [1.5, 0, 0.3], [1.5, 0, -0.3], [0, 0, 0]]
    # a lane change returns the heading to what it would have been
    row = ROW.copy()
    q = MNM.walk(row, lc[0, 0], 4.0)
    assert abs(q[2] - (row[2] + row[6] * 4.0)) < 1e-15 * 8
    with pytest.raises(ValueError, match="piece 1 accel does not broadcast"):
        MAN.rows(4, 3, [(1.0, 0.0, 0.0), (1.0, np.ones(5), 0.0)], device="cpu")
    with pytest.raises(ValueError, match="at most 4 pieces"):
        MAN.rows(4, 3, [(1.0, 0.0, 0.0)] * 5, device="cpu")
    with pytest.raises(ValueError, match=r"man\[0, 0, 1\]: dur must be >= 0"):
        MAN.rows(4, 3, MAN.brake(1.0, 3.0, -1.0), device="cpu")
    table = torch.stack([MAN.rows(1, 3, MAN.brake(1.0, d, 5.0), device="cpu")[0] for d in (2.0, 4.0)])
    got = MAN.from_table(table, [1, 0, 1], device="cpu")
    assert got[:, 0, 1, 1].tolist() == [-4.0, -2.0, -4.0]
    with pytest.raises(ValueError, match="outside the table"):
        MAN.from_table(table, [2], device="cpu")


def test_dist_refuses_a_duration_that_could_be_negative():
    d = MAN.ManoeuvreDist(3, seed=9)
    d.uniform(0, "dur", 2.0, 2.0, lo=0.0).fixed(1, "dur", 3.0).uniform(1, "accel", -3.0, 1.0, hi=0.0)
    with pytest.raises(ValueError, match="piece 0 field dur: lo must be >= 0"):
        d.uniform(0, "dur", 2.0, 2.0)
    with pytest.raises(ValueError, match="piece 2 field dur: lo must be >= 0"):
        d.normal(2, 0, 2.0, 0.5, lo=-1.0)
    with pytest.raises(ValueError, match="piece 3 field dur: a fixed duration must be >= 0"):
        d.fixed(3, "dur", -1.0)
    with pytest.raises(ValueError, match="unknown manoeuvre field"):
        d.fixed(0, "jerk", 1.0)
    with pytest.raises(ValueError, match="piece 4 out of range"):
        d.fixed(4, "dur", 1.0)
    c = d.c_struct()
    assert c.n_obst == 3 and c.seed == 9 and c.field[0][0].kind == LB.TRUTH_UNIFORM
    assert c.field[0][0].lo == 0.0 and c.mean[1][0] == 3.0 and c.field[1][1].hi == 0.0
    e = d.with_offset(7)
    assert e.b_offset == 7 and d.b_offset == 0 and e.mean is not d.mean
    # the mirror's sampler: a FIXED field is its mean, a drawn duration stays in its clamp
    md = MNM.Dist(3, 9).set(0, 0, MNM.UNIFORM, 2.0, 2.0, lo=0.0).set(1, 0, MNM.FIXED, 3.0) \
        .set(1, 1, MNM.UNIFORM, -3.0, 1.0, hi=0.0)
    s = MNM.sample(md, 6)
    assert s.shape == (6, 3, 4, 3) and (s[..., 1, 0] == 3.0).all() and (s[..., 0, 0] >= 0).all()
    assert (s[..., 2:, :] == 0).all() and len(np.unique(s[..., 0, 0])) == 18
    whole = MNM.sample(md, 6)
    md.b_offset = 4
    assert np.array_equal(MNM.sample(md, 2), whole[4:])


def test_state_and_pose_refuse_host_tensors():
    rows = torch.zeros((2, 3, 7), dtype=torch.float64)
    with pytest.raises(ValueError, match="rows must be .* on the GPU"):
        MAN.state(rows, None, 0.0)
    with pytest.raises(ValueError, match="rows must be .* on the GPU"):
        MAN.pose(rows, None, 0.01, 0, 3)
