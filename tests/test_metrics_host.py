"""Realised-path metrics, the parts that need no GPU: the fp64 mirror
(tests/metrics_mirror.py) against known answers and against brute force; the C-ABI of
include/scpqp_metrics.h: exports, ctypes layout (gcc probe of the header) and argument
validation without touching a device; the batch summary."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import metrics_mirror as MM
from scpqp import _lib as LB
from scpqp.build import LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scpqp_metrics.h")
L, W = 0.98, 0.88
PI = math.pi


def header_functions():
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"^int\s+(scpqp_\w+)\(", txt, re.M)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        pytest.fail("libscpqp.so not built: run __graft_entry__.build()")
    return LB.load()


# ---------------------------------------------------------------- known answers
def test_gap_axis_aligned():
    assert MM.footprint_gap((0, 0, 0, L, W), (3, 0, 0, L, W)) == pytest.approx(3 - 0.49 - 0.49, abs=1e-15)


def test_gap_second_turned_quarter():
    g = MM.footprint_gap((0, 0, 0, L, W), (3, 0, PI / 2, L, W))
    assert abs(g - (3 - 0.49 - 0.44)) <= 1e-15


def test_gap_corner_to_corner():
    g = MM.footprint_gap((0, 0, 0, L, W), (3, 4, 0, L, W))
    assert abs(g - math.hypot(3 - 0.98, 4 - 0.88)) <= 1e-15


def test_gap_unit_squares_second_at_45_degrees():
    g = MM.footprint_gap((0, 0, 0, 1, 1), (3, 0, PI / 4, 1, 1))
    assert abs(g - (3 - 0.5 - math.sqrt(2) / 2)) <= 1e-15


def test_centres_half_a_metre_apart_collide():
    a, b = (0, 0, 0, L, W), (0.5, 0, 0, L, W)
    assert MM.footprint_gap(a, b) == 0.0 and MM.overlap(a, b)


def test_crossed_thin_rectangles_collide_with_no_corner_inside():
    a, b = (0, 0, 0, 4, 0.2), (0, 0, PI / 2, 4, 0.2)
    assert MM.footprint_gap(a, b) == 0.0 and MM.overlap(a, b)
    # no corner of either lies inside the other: the corner distances alone miss it
    ra, rb = MM._rect(*a), MM._rect(*b)
    assert MM._corners_to(ra, rb) > 1.0 and MM._corners_to(rb, ra) > 1.0


def test_rotated_square_off_the_corner_is_separated_only_by_its_own_axes():
    a = (0, 0, 0, 1, 1)
    c = 0.5 + 0.9 / math.sqrt(2)      # centre on the diagonal, 0.9 past a's corner
    b = (c, c, PI / 4, 1, 1)
    m = MM.separation_margins(MM._rect(*a), MM._rect(*b))
    assert m[0] < 0 and m[1] < 0                 # a's axes do not separate
    assert max(m[2], m[3]) > 0                   # one of b's does
    g = MM.footprint_gap(a, b)
    assert not MM.overlap(a, b) and abs(g - 0.4) <= 1e-15


def test_touching_counts_as_overlap():
    assert MM.footprint_gap((0, 0, 0, 1, 1), (1, 0, 0, 1, 1)) == 0.0
    assert MM.footprint_gap((0, 0, 0, 1, 1), (1.0 + 2.0 ** -40, 0, 0, 1, 1)) > 0.0


def test_cross_track():
    line = [(-100.0, 0.0), (100.0, 0.0)]
    assert abs(MM.cross_track(line, 5.0, 0.3) - 0.3) <= 1e-15
    assert abs(MM.cross_track(line, 150.0, 0.3) - 0.3) <= 1e-15     # the end is extended
    assert abs(MM.cross_track(line, -150.0, -0.3) - 0.3) <= 1e-15
    bent = [(0.0, 0.0), (10.0, 0.0), (10.0, 10.0)]
    # outside the corner: nearest to the corner itself
    assert abs(MM.cross_track(bent, 11.0, -1.0) - math.sqrt(2)) <= 1e-15
    # an interior clamp holds: past the first segment's end the corner, not the line
    assert abs(MM.cross_track(bent, 13.0, -4.0) - 5.0) <= 1e-15
    # the last segment extends beyond its end
    assert abs(MM.cross_track(bent, 10.5, 30.0) - 0.5) <= 1e-15


# ---------------------------------------------------------------- brute force
SEED = 20240
N_PAIRS, N_EDGE = 200, 2000


def _random_rect(rng):
    return (rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(-PI, PI),
            rng.uniform(0.3, 3.0), rng.uniform(0.3, 3.0))


def _boundary(r, n):
    cx, cy, h, ln, wd = r
    c, s = math.cos(h), math.sin(h)
    t = np.arange(n) / n
    hx, hy = ln / 2, wd / 2
    loc = np.concatenate([
        np.stack([-hx + 2 * hx * t, np.full(n, -hy)], 1), np.stack([np.full(n, hx), -hy + 2 * hy * t], 1),
        np.stack([hx - 2 * hx * t, np.full(n, hy)], 1), np.stack([np.full(n, -hx), hy - 2 * hy * t], 1)])
    return np.stack([cx + loc[:, 0] * c - loc[:, 1] * s, cy + loc[:, 0] * s + loc[:, 1] * c], 1)


def _outside(r, pts):
    """max(|px| - hx, |py| - hy) in the rectangle's frame: <= 0 inside or on the edge."""
    cx, cy, h, ln, wd = r
    c, s = math.cos(h), math.sin(h)
    dx, dy = pts[..., 0] - cx, pts[..., 1] - cy
    return np.maximum(np.abs(dx * c + dy * s) - ln / 2, np.abs(dy * c - dx * s) - wd / 2)


def _grid_overlap(a, b, n=65, levels=4):
    """Is some grid point inside both rectangles?  The grid covers both, then zooms three
    times onto the two cells around its most-inside point (the function is convex)."""
    lo, hi = np.array([-5.0, -5.0]), np.array([5.0, 5.0])
    for _ in range(levels):
        xs, ys = np.linspace(lo[0], hi[0], n), np.linspace(lo[1], hi[1], n)
        g = np.stack(np.meshgrid(xs, ys, indexing="ij"), -1)
        f = np.maximum(_outside(a, g), _outside(b, g))
        if f.min() <= 0.0:
            return True
        i, j = np.unravel_index(np.argmin(f), f.shape)
        step = (hi - lo) / (n - 1)
        mid = np.array([xs[i], ys[j]])
        lo, hi = mid - 2 * step, mid + 2 * step
    return False


def test_mirror_against_brute_force():
    """200 seeded random rectangle pairs.  Gap: the smallest distance between 2000
    boundary samples per edge lies in [gap, gap + sampling spacing].  Overlap flag: a
    grid point-in-both-rectangles test; pairs within 1e-3 of touching (gap below 1e-3 or
    overlapping by less than 1e-3 on some axis) are left out of the flag comparison, at
    most 5 % of them."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(SEED)
    left_out = n_overlap = n_apart = 0
    for _ in range(N_PAIRS):
        a, b = _random_rect(rng), _random_rect(rng)
        gap, hit = MM.footprint_gap(a, b), MM.overlap(a, b)
        assert (gap == 0.0) == hit
        margin = max(MM.separation_margins(MM._rect(*a), MM._rect(*b)))
        if not hit:
            spacing = max(a[3], a[4], b[3], b[4]) / N_EDGE
            brute = cKDTree(_boundary(a, N_EDGE)).query(_boundary(b, N_EDGE))[0].min()
            assert gap - 1e-12 <= brute <= gap + spacing, (a, b, gap, brute)
            assert margin <= gap + 1e-12       # every separating axis bounds the distance
        if (not hit and gap < 1e-3) or (hit and margin > -1e-3):
            left_out += 1
            continue
        assert _grid_overlap(a, b) == hit, (a, b, gap, margin)
        n_overlap += hit
        n_apart += not hit
    print(f"left out {left_out}, compared {n_overlap} overlapping and {n_apart} separated pairs")
    assert left_out <= 0.05 * N_PAIRS
    assert n_overlap >= 40 and n_apart >= 40


# ---------------------------------------------------------------- mirror accumulator
def test_mirror_accumulator_tie_and_collision_rules():
    C_ = MM.Constants([1, 1], [1, 1], np.full((2, 2), 2.5), [], [], [[(-9, 0), (9, 0)]] * 2, 0.01)
    far, near, hit = 5.0, 2.0, 0.5
    xs = [far, near, near, far, hit, hit, far]
    path = np.zeros((1, 2, len(xs), 6))
    path[0, 1, :, 0] = xs
    path[0, :, :, 1] = 0.25
    out = MM.run(C_, [(path[:, :, :4], 10, 0), (path[:, :, 3:], 13, 1)], 1)
    assert out["n_ticks_seen"][0] == 7
    assert out["min_gap_veh"][0] == 0.0 and list(out["argmin_gap_veh"][0]) == [14, 0, 1]
    assert out["first_collision_tick"][0] == 14 and out["n_collision_ticks"][0] == 2
    assert out["min_margin_veh"][0] == hit - 2.5
    assert out["min_gap_obs"][0] == math.inf and list(out["argmin_gap_obs"][0]) == [-1, -1, -1]
    assert np.all(out["max_xtrack"][0] == 0.25)
    assert np.allclose(out["sum_sq_xtrack"][0], 7 * 0.0625, rtol=0, atol=1e-15)
    # the same gap at ticks 11 and 12: the earlier one is kept, inside a call and across
    one = MM.run(C_, [(path[:, :, :4], 10, 0)], 1)
    assert list(one["argmin_gap_veh"][0]) == [11, 0, 1] and one["min_gap_veh"][0] == near - 1.0
    two = MM.run(C_, [(path[:, :, :2], 10, 0), (path[:, :, 1:4], 11, 1)], 1)
    assert list(two["argmin_gap_veh"][0]) == [11, 0, 1]


# ---------------------------------------------------------------- ABI
def test_metrics_header_declares_the_boundary():
    assert header_functions() == sorted(LB.METRICS_EXPORTS)
    assert not set(LB.METRICS_EXPORTS) & (set(LB.EXPORTS) | set(LB.NOISE_EXPORTS))


def test_library_exports_every_metrics_symbol(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\sT\s(scpqp_\w+)", out))
    assert set(header_functions()) <= exported
    for name in LB.METRICS_EXPORTS:
        assert hasattr(lib, name)


STRUCTS = {"scpqp_metrics_params": LB.MetricsParams, "scpqp_metrics_acc": LB.MetricsAcc,
           "scpqp_metrics_dense": LB.MetricsDense}


def test_metrics_ctypes_layout_matches_header(tmp_path):
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "scpqp_metrics.h"',
             'int main(void) {']
    for cname, cls in STRUCTS.items():
        lines.append(f'  printf("{cname}.size %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", f"-I{os.path.dirname(HEADER)}", str(src), "-o", str(exe)],
                   check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, cls in STRUCTS.items():
        assert int(got[f"{cname}.size"]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)
    # every member the header declares is bound, in the header's order
    txt = open(HEADER).read()
    for cname, cls in STRUCTS.items():
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), txt, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [re.findall(r"\w+", decl)[-1] for decl in body.split(";") if decl.strip()]
        assert [n for n in names if n] == [f for f, _ in cls._fields_], cname


def _params(**kw):
    keep = dict(length=np.array([L, L]), width=np.array([W, W]), dsafe_veh=np.full(4, 2.0),
                dsafe_obs=np.full(2, 2.0), obstacles=np.array([5.0, 5, 0, 0, 2, 2]),
                ref_polyline=np.array([[[-9.0, 0], [9, 0]], [[-9.0, 1], [9, 1]]]),
                ref_npts=np.array([2, 2], np.int32))
    f = dict(n_veh=2, n_obst=1, ref_max_pts=2, pad0=0, tick_length=0.01)
    f.update({k: v for k, v in kw.items() if k not in keep})
    for k, a in keep.items():
        a = kw.get(k, a)
        if a is None:
            f[k] = None
        else:
            a = np.ascontiguousarray(a)
            keep[k] = a
            f[k] = a.ctypes.data_as(C.POINTER(C.c_int32 if k == "ref_npts" else C.c_double))
    return LB.MetricsParams(**f), keep


def test_metrics_argument_validation_without_gpu(lib):
    E_ARG, E_SIZE = -1, -4
    h = C.c_void_p()

    def create(**kw):
        p, keep = _params(**kw)
        rc = lib.scpqp_metrics_create(C.byref(p), 0, C.byref(h))
        del keep
        return rc

    for bad in (dict(n_veh=0), dict(n_veh=17), dict(n_obst=-1), dict(n_obst=33),
                dict(ref_max_pts=1), dict(ref_max_pts=9), dict(tick_length=0.0),
                dict(tick_length=-0.01), dict(tick_length=float("nan")), dict(length=None),
                dict(width=None), dict(dsafe_veh=None), dict(dsafe_obs=None), dict(obstacles=None),
                dict(ref_polyline=None), dict(ref_npts=None),
                dict(ref_npts=np.array([2, 1], np.int32)), dict(ref_npts=np.array([3, 2], np.int32))):
        assert create(**bad) == E_ARG, bad
        assert h.value is None
    assert create(n_veh=17) == E_ARG and b"n_veh" in lib.scpqp_last_error()
    assert create(n_obst=33) == E_ARG and b"n_obst" in lib.scpqp_last_error()
    assert create(ref_max_pts=9) == E_ARG and b"ref_max_pts" in lib.scpqp_last_error()
    assert create(tick_length=0.0) == E_ARG and b"tick_length" in lib.scpqp_last_error()
    assert lib.scpqp_metrics_create(None, 0, C.byref(h)) == E_ARG
    p, keep = _params()
    assert lib.scpqp_metrics_create(C.byref(p), 0, None) == E_ARG
    assert lib.scpqp_metrics_create(C.byref(p), -1, C.byref(h)) == E_ARG

    assert lib.scpqp_metrics_destroy(None) == 0

    acc = LB.MetricsAcc()

    def accumulate(B=1, n_ticks=4, tick0=0, k_first=0):
        return lib.scpqp_metrics_accumulate(None, B, n_ticks, tick0, k_first, None, C.byref(acc),
                                            None, None)

    assert accumulate(k_first=2) == E_ARG and b"k_first" in lib.scpqp_last_error()
    assert accumulate(k_first=-1) == E_ARG and b"k_first" in lib.scpqp_last_error()
    assert accumulate(n_ticks=-1) == E_ARG and b"n_ticks" in lib.scpqp_last_error()
    assert accumulate(B=-1) == E_ARG and b"batch" in lib.scpqp_last_error()
    assert accumulate(tick0=-1) == E_ARG and b"tick0" in lib.scpqp_last_error()
    assert accumulate(tick0=2 ** 31 - 2, n_ticks=2) == E_SIZE
    assert accumulate() == E_ARG and b"handle" in lib.scpqp_last_error()
    assert lib.scpqp_metrics_reset(None, -1, C.byref(acc), None) == E_ARG \
        and b"batch" in lib.scpqp_last_error()
    assert lib.scpqp_metrics_reset(None, 1, C.byref(acc), None) == E_ARG \
        and b"handle" in lib.scpqp_last_error()


# ---------------------------------------------------------------- summary
def test_wilson_interval_and_summary():
    from scpqp import metrics as M
    lo, hi = M.wilson_interval(0, 100)
    assert abs(lo) < 1e-15 and abs(hi - 0.036995) < 1e-5        # 0 of 100: upper bound z^2/(n+z^2)
    assert abs(hi - M.WILSON_Z ** 2 / (100 + M.WILSON_Z ** 2)) < 1e-15
    lo, hi = M.wilson_interval(10, 100)
    assert abs(lo - 0.05523) < 1e-4 and abs(hi - 0.17437) < 1e-4
    lo, hi = M.wilson_interval(100, 100)
    assert abs(hi - 1.0) < 1e-15 and abs(lo - (1 - 0.036995)) < 1e-5

    def res(gaps, first, seen, ssq, xmax, margin):
        n = len(gaps)
        return dict(min_gap_veh=np.array(gaps, float), min_gap_obs=np.full(n, np.inf),
                    min_margin_veh=np.array(margin, float), min_margin_obs=np.full(n, np.inf),
                    first_collision_tick=np.array(first, np.int32),
                    n_ticks_seen=np.full(n, seen, np.int32), sum_sq_xtrack=np.array(ssq, float),
                    max_xtrack=np.array(xmax, float))
    a = res([1.0, 0.0], [-1, 7], 10, [[0.1, 0.3], [0.2, 0.2]], [[0.1, 0.2], [0.3, 0.1]], [0.5, -1.0])
    b = res([3.0, 2.0], [-1, -1], 10, [[0.0, 0.0], [0.1, 0.1]], [[0.0, 0.0], [0.2, 0.1]], [2.0, 1.0])
    s = M.summarize([a, b])
    assert s["n_realisations"] == 4 and s["n_collisions"] == 1 and s["collision_rate"] == 0.25
    assert s["collision_rate_wilson95"] == list(M.wilson_interval(1, 4))
    assert s["min_gap_veh"]["min"] == 0.0 and s["min_gap_veh"]["q50"] == 1.5
    assert s["min_gap_obs"] is None and s["frac_margin_obs_below_0"] is None
    assert s["frac_margin_veh_below_0"] == 0.25
    assert abs(s["xtrack_rms"] - math.sqrt(1.0 / 80)) < 1e-15 and s["xtrack_max"] == 0.3
    assert M.summarize(a)["n_realisations"] == 2
    # one vehicle and obstacles: the pair fields are None, the obstacle fields are not
    c = res([np.inf, np.inf], [-1, 3], 10, [[0.1], [0.2]], [[0.1], [0.3]], [np.inf, np.inf])
    c["min_gap_obs"], c["min_margin_obs"] = np.array([0.5, 0.0]), np.array([-0.1, -2.0])
    s1 = M.summarize(c)
    assert s1["min_gap_veh"] is None and s1["frac_margin_veh_below_0"] is None
    assert s1["min_gap_obs"]["min"] == 0.0 and s1["frac_margin_obs_below_0"] == 1.0
    assert all(isinstance(v, (int, float, list, dict, type(None))) for v in s.values())
