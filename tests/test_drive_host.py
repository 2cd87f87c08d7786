"""Drive truth, the parts that need no GPU: the C-ABI of include/scpqp_drive.h (exports, ctypes
layout by a gcc probe of the header, argument validation without touching a device), the CPU
mirror (tests/drive_mirror.py) against its 80-bit self, the closed form and the known answers
of the hold rule, the mirror's sampler, the conditions on the case table
(tests/drive_cases.py), the derivation of the GPU tolerance, and scpqp.drive's host side."""
import ctypes as C
import glob
import math
import os
import re
import subprocess

import numpy as np
import pytest

import drive_cases as DC
import drive_mirror as DM
import noise_mirror as NM
import truth_mirror as TM
from scpqp import _lib as LB
from scpqp import drive as DRV
from scpqp.build import LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scpqp_drive.h")
E_ARG, E_SIZE = -1, -4
INF, NAN = math.inf, math.nan


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
def test_drive_header_declares_the_boundary():
    assert header_functions() == sorted(LB.DRIVE_EXPORTS)
    others = (set(LB.EXPORTS) | set(LB.NOISE_EXPORTS) | set(LB.TRUTH_EXPORTS)
              | set(LB.GOV_EXPORTS) | set(LB.YLD_EXPORTS))
    assert not set(LB.DRIVE_EXPORTS) & others


def test_library_exports_every_drive_symbol(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\sT\s(scpqp_\w+)", out))
    assert set(header_functions()) <= exported
    for name in LB.DRIVE_EXPORTS:
        assert hasattr(lib, name)


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "scpqp_drive.h"
int main(void) {
  int (*step)(const scpqp_plant_params*, int32_t, int32_t, double, const double*, const double*,
              const double*, const double*, const scpqp_noise*, const double*, const double*,
              double*, double, void*) = scpqp_plant_step_drive;
  int (*fill)(int32_t, int32_t, double*, void*) = scpqp_drive_fill_ideal;
  int (*samp)(const scpqp_drive_dist*, int32_t, double*, void*) = scpqp_drive_sample;
  (void)step; (void)fill; (void)samp;
  printf("size %zu\n", sizeof(scpqp_drive_dist));
  printf("n_veh %zu\n", offsetof(scpqp_drive_dist, n_veh));
  printf("mean %zu\n", offsetof(scpqp_drive_dist, mean));
  printf("field %zu\n", offsetof(scpqp_drive_dist, field));
  printf("seed %zu\n", offsetof(scpqp_drive_dist, seed));
  printf("b_offset %zu\n", offsetof(scpqp_drive_dist, b_offset));
  printf("np %d\n", SCPQP_DRIVE_NP);
  printf("idx %d%d%d%d%d%d\n", SCPQP_DRIVE_TAU_A, SCPQP_DRIVE_GAIN_A, SCPQP_DRIVE_BIAS_A,
         SCPQP_DRIVE_A_MAX, SCPQP_DRIVE_B_MAX, SCPQP_DRIVE_HOLD);
  printf("site %d\n", SCPQP_NOISE_SITE_DRIVE);
  printf("maxveh %d\n", SCPQP_MAX_VEH);
  return 0;
}
"""


def test_drive_ctypes_layout_matches_header(tmp_path):
    """The constants, the structure and the three prototypes (a pointer of the written type
    takes each function: a mismatch does not compile under -Werror)."""
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    obj = tmp_path / "probe.o"
    subprocess.run(["gcc", "-std=c99", "-Werror", "-c", f"-I{os.path.dirname(HEADER)}", str(src),
                    "-o", str(obj)], check=True)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", str(obj), "-Wl,--unresolved-symbols=ignore-all", "-o", str(exe)],
                   check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(LB.DriveDist)
    for f in ("n_veh", "mean", "field", "seed", "b_offset"):
        assert int(got[f]) == getattr(LB.DriveDist, f).offset, f
    assert int(got["np"]) == LB.DRIVE_NP == DM.NP == DRV.NP == 6
    assert got["idx"] == "012345"
    assert (LB.DRIVE_TAU_A, LB.DRIVE_GAIN_A, LB.DRIVE_BIAS_A, LB.DRIVE_A_MAX, LB.DRIVE_B_MAX,
            LB.DRIVE_HOLD) == (0, 1, 2, 3, 4, 5) == (DM.TAU_A, DM.GAIN_A, DM.BIAS_A, DM.A_MAX,
                                                      DM.B_MAX, DM.HOLD)
    assert int(got["site"]) == LB.NOISE_SITE_DRIVE == DM.SITE_DRIVE == 9
    assert int(got["maxveh"]) == LB.MAX_VEH
    assert LB.DRIVE_FIELDS == DM.FIELDS


def test_site_nine_is_free_in_every_header():
    """Every SCPQP_NOISE_SITE_* of include/: nine other sites, 0 to 8, and the drive's 9.  The
    site is the top byte of c2 and the rest of c2 stays below 2^24, so no counter of site 9 is
    a counter of another site."""
    sites = {}
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        for name, val in re.findall(r"#define\s+(SCPQP_NOISE_SITE_\w+)\s+(\d+)", open(h).read()):
            assert sites.setdefault(name, int(val)) == int(val)
    assert sites.pop("SCPQP_NOISE_SITE_DRIVE") == 9
    assert sorted(sites.values()) == list(range(9))
    d = DM.Dist(LB.MAX_VEH, 1, 0)
    _, c1, c2, _ = DM.counters(d, 3)
    assert np.all(c2 >> 24 == 9) and np.all(c1 == 0)
    assert NM.counter2(8, 0xFFFF, 0xFF) >> 24 == 8           # the largest c2 below site 9


# ---------------------------------------------------------------------------
# 2. argument validation without a GPU
# ---------------------------------------------------------------------------
def _pp(n=2):
    pp = LB.PlantParams(n_veh=n)
    for v in range(max(n, 0)):
        pp.lf[v] = pp.lr[v] = 0.34
    return pp


def test_plant_step_drive_argument_validation_without_gpu(lib):
    pp = _pp()
    nz = LB.Noise(seed=1, sigma=3e-6, epoch=0, b_offset=0)
    P, N = C.byref(pp), C.byref(nz)
    dummy = (C.c_double * 64)()
    D = C.cast(dummy, C.c_void_p)

    def plant(p=P, B=1, n_ticks=40, tick=0.01, truth=None, noise=None, n=None, arr=None,
              a_cmd=None, drive=None, h_max=2.5e-3):
        return lib.scpqp_plant_step_drive(p, B, n_ticks, tick, arr, arr, truth, noise, n, a_cmd,
                                          drive, arr, h_max, None)

    def err():
        return lib.scpqp_last_error()

    assert plant(p=None) == E_ARG and b"null" in err()
    for n in (0, 17):
        assert plant(p=C.byref(LB.PlantParams(n_veh=n))) == E_ARG and b"n_veh" in err()
    assert plant(p=C.byref(LB.PlantParams(n_veh=2)), B=0) == 0
    assert plant(noise=D, n=N) == E_ARG and b"not both" in err()
    assert plant(B=0, noise=D, n=N) == E_ARG
    for s in (-1e-6, INF, NAN):
        assert plant(n=C.byref(LB.Noise(seed=1, sigma=s))) == E_ARG and b"sigma" in err()
    assert plant(B=-1) == E_ARG
    assert plant(n_ticks=-1) == E_ARG
    assert plant(tick=0.0) == E_ARG and b"tick" in err()
    assert plant(h_max=0.0) == E_ARG
    assert plant(h_max=NAN) == E_ARG
    assert plant(n_ticks=65536, n=N) == E_SIZE and b"65536" in err()
    assert plant(B=0, n_ticks=65536) == 0
    # B = 0 is a no-op with NULL arrays
    assert plant(B=0) == 0
    assert plant(B=0, n=N) == 0
    # with work: truth, a_cmd and drive must be non-NULL, then the other arrays
    assert plant(B=3, arr=D, a_cmd=D, drive=D) == E_ARG and b"truth" in err()
    assert plant(B=3, arr=D, truth=D, drive=D) == E_ARG and b"a_cmd" in err()
    assert plant(B=3, arr=D, truth=D, a_cmd=D) == E_ARG and b"drive" in err()
    assert plant(B=3, truth=D, a_cmd=D, drive=D) == E_ARG and b"null array" in err()
    assert plant(B=1 << 20, n_ticks=1 << 10, truth=D, a_cmd=D, drive=D, arr=D) == E_SIZE \
        and b"too large" in err()


def _dist(n_veh=2):
    d = LB.DriveDist()
    d.n_veh = n_veh
    for v in range(LB.MAX_VEH):
        for f in range(6):
            d.mean[f][v] = DM.IDEAL_ROW[f]
    d.seed = 5
    return d


def _field(d, f, kind, spread=0.0, lo=-INF, hi=INF, mean=None):
    d.field[f].kind, d.field[f].spread, d.field[f].lo, d.field[f].hi = kind, spread, lo, hi
    if mean is not None:
        for v in range(LB.MAX_VEH):
            d.mean[f][v] = mean
    return d


def test_drive_sample_and_fill_argument_validation_without_gpu(lib):
    dummy = (C.c_double * 64)()
    D = C.cast(dummy, C.c_void_p)
    U, Nm = LB.TRUTH_UNIFORM, LB.TRUTH_NORMAL

    def sample(d, B=0, out=None):
        return lib.scpqp_drive_sample(None if d is None else C.byref(d), B, out, None)

    def err():
        return lib.scpqp_last_error()

    assert sample(None) == E_ARG and b"null" in err()
    assert sample(_dist()) == 0                           # all FIXED at ideal, B = 0, NULL array
    for n in (0, -1, 17):
        assert sample(_dist(n)) == E_ARG and b"n_veh" in err()
    for f, name in enumerate(LB.DRIVE_FIELDS[:5]):
        nm = name.encode()
        for kind in (-1, 3):
            assert sample(_field(_dist(), f, kind)) == E_ARG and nm in err() and b"kind" in err()
        for kind in (U, Nm):
            for s in (-1e-3, INF, NAN):
                assert sample(_field(_dist(), f, kind, s, 0.01, 1.0, mean=0.5)) == E_ARG
                assert nm in err() and b"spread" in err()
            assert sample(_field(_dist(), f, kind, 0.01, 1.0, 0.5, mean=0.5)) == E_ARG
            assert nm in err() and b"lo" in err()
            assert sample(_field(_dist(), f, kind, 0.01, NAN, 0.5, mean=0.5)) == E_ARG
            assert sample(_field(_dist(), f, kind, 0.01, 0.05, 1.0, mean=0.5)) == 0
            # a drawn field needs a finite mean
            for m in (INF, NAN):
                assert sample(_field(_dist(), f, kind, 0.01, 0.05, 1.0, mean=m)) == E_ARG
                assert nm in err() and b"mean" in err()
        # a FIXED field ignores spread, lo and hi
        assert sample(_field(_dist(), f, LB.TRUTH_FIXED, -1.0, 2.0, 1.0)) == 0
    # HOLD is FIXED at 0 or 1
    for kind in (U, Nm):
        assert sample(_field(_dist(), 5, kind, 0.1, 0.0, 1.0)) == E_ARG and b"hold" in err()
    for h in (0.5, -1.0, 2.0, NAN):
        assert sample(_field(_dist(), 5, 0, mean=h)) == E_ARG and b"hold" in err()
    assert sample(_field(_dist(), 5, 0, mean=1.0)) == 0
    # the smallest row the sampler can emit must be one the plant integrates
    for f, nm in ((0, b"tau_a"), (3, b"a_max"), (4, b"b_max")):
        assert sample(_field(_dist(), f, U, 0.1, -0.01, 1.0, mean=0.5)) == E_ARG and nm in err()
        assert sample(_field(_dist(), f, Nm, 0.1, mean=0.5)) == E_ARG and nm in err()   # lo = -inf
        assert sample(_field(_dist(), f, U, 0.1, 0.0, 1.0, mean=0.5)) == 0
        assert sample(_field(_dist(), f, 0, mean=-0.1)) == E_ARG and nm in err()
        assert sample(_field(_dist(), f, 0, mean=NAN)) == E_ARG and nm in err()
    assert sample(_field(_dist(), 0, 0, mean=INF)) == 0    # the plant takes an infinite lag
    for f, nm in ((1, b"gain_a"), (2, b"bias_a")):
        for m in (INF, -INF, NAN):
            assert sample(_field(_dist(), f, 0, mean=m)) == E_ARG and nm in err()
        assert sample(_field(_dist(), f, U, 0.1, INF, INF, mean=0.5)) == E_ARG and nm in err()
        assert sample(_field(_dist(), f, U, 0.1, -INF, -INF, mean=0.5)) == E_ARG and nm in err()
        assert sample(_field(_dist(), f, Nm, 0.1, mean=0.5)) == 0
    d = _dist()
    d.mean[3][1] = -1.0
    assert sample(d) == E_ARG and b"a_max" in err()
    d.n_veh = 1                                           # vehicle 1 is outside: not looked at
    assert sample(d) == 0
    # sizes and arrays
    assert sample(_dist(), B=-1) == E_ARG
    assert sample(_dist(), B=3) == E_ARG and b"drive" in err()
    assert sample(_dist(16), B=1 << 30, out=D) == E_SIZE

    def fill(n, B=0, out=None):
        return lib.scpqp_drive_fill_ideal(n, B, out, None)

    for n in (0, -1, 17):
        assert fill(n) == E_ARG and b"n_veh" in err()
    assert fill(2) == 0
    assert fill(2, B=-1) == E_ARG
    assert fill(2, B=3) == E_ARG and b"drive" in err()
    assert fill(16, B=1 << 30, out=D) == E_SIZE


# ---------------------------------------------------------------------------
# 3. the mirror: against its 80-bit self, the closed form, the hold rule's known answers
# ---------------------------------------------------------------------------
TROW = TM.nominal_row(0.30, 0.34)
X0 = np.array([1.0, -2.0, 0.3, 4.0, 1.0, 0.01])


def _row(tau=0.0, gain=1.0, bias=0.0, a_max=INF, b_max=INF, hold=0.0):
    return np.array([tau, gain, bias, a_max, b_max, hold])


def _flow(x, a_cmd, drow, T, fm=DM.F64, h_max=DC.H_MAX, watch=None):
    return DM.rk4_flow(x, 0.02, a_cmd, TROW, drow, T, DM.steps_for(T, h_max), fm=fm, watch=watch)


def test_a_eff_is_two_roundings_and_a_clamp():
    rng = np.random.default_rng(4)
    fused = 0
    for _ in range(300):
        g, c, b = rng.uniform(0.5, 1.5), rng.uniform(-4, 4), rng.uniform(-0.5, 0.5)
        want = np.float64(g) * np.float64(c) + np.float64(b)
        assert DM.a_eff(_row(gain=g, bias=b), c) == want
        exact = np.longdouble(g) * np.longdouble(c) + np.longdouble(b)
        fused += float(exact) != want                         # what one rounding would give
        assert DM.a_eff(_row(gain=g, bias=b, a_max=0.25), c) == min(want, 0.25)
        assert DM.a_eff(_row(gain=g, bias=b, b_max=0.25), c) == max(want, -0.25)
    assert fused > 30                                         # the two differ often enough to tell
    assert DM.a_eff(DM.ideal_row(), -0.0) == 0.0
    assert DM.a_eff(_row(a_max=0.0, b_max=0.0), 3.0) == 0.0 == DM.a_eff(_row(a_max=0.0, b_max=0.0), -3.0)


def test_mirror_float64_against_its_80_bit_self():
    for form in DC.FORMS:
        lo, hi = DC.mirror(form, DM.F64), DC.mirror(form, DM.F80)
        assert lo.dtype == np.float64 and hi.dtype == np.longdouble
        r = DC.ratio(lo, hi)
        print(f"drive mirror float64 against 80-bit, {form}: {r:.3g}")
        assert r <= DC.MIRROR_ROUNDING
        # the gate and the projection took the same branches: exact zeros in the same places
        assert np.array_equal(lo[..., 3] == 0.0, hi[..., 3] == 0.0)


def test_mirror_lag_against_the_closed_form():
    """The fixed-step RK4 over the lag at HOLD = 0 against a(t) and s(t) of the header, for tau
    from 8 h_max upwards.  The figures are measured here and recorded (drive_cases.LAG_ERROR and
    the header's Accuracy paragraph): each recorded figure bounds its measurement and is within
    a factor of two of it.  In 80-bit the same steps give the same figures: they are the
    method's error, not rounding."""
    for tau, (rec_a, rec_s) in DC.LAG_ERROR.items():
        assert tau >= 8 * DC.H_MAX
        drow = _row(tau=tau)
        for fm in (DM.F64, DM.F80):
            ea = es = 0.0
            for k in range(1, 11):
                T = k * DC.TICK
                x = _flow(np.array([0.0, 0.0, 0.1, 4.0, 1.0, 0.01]), -3.0, drow, T, fm)
                a, s = DM.closed_form(4.0, 1.0, -3.0, tau, T)
                ea, es = max(ea, abs(float(x[4] - a))), max(es, abs(float(x[3] - s)))
            print(f"tau_a {tau} ({fm.dtype.__name__}): |a - closed form| {ea:.3g}, |s - closed form| {es:.3g}")
            assert 0.5 * rec_a <= ea <= rec_a and 0.5 * rec_s <= es <= rec_s
    # the method is of fourth order: halving h_max divides the error by about 16
    e = [abs(float(_flow(X0, -3.0, _row(tau=0.1), 0.5, DM.F80, h)[4]
                   - DM.closed_form(4.0, 1.0, -3.0, 0.1, 0.5)[0])) for h in (2.5e-3, 1.25e-3)]
    assert 12 < e[0] / e[1] < 20


def test_hold_stops_at_exactly_zero_and_stays():
    x = X0.copy()
    x[3] = 0.31
    drow = _row(hold=1.0)
    w = dict(speeds=[], accels=[], projected=0)
    crossed = False
    for k in range(1, 9):
        T = k * DC.TICK
        rnd = DM.steps_for(T, DC.H_MAX) * 2.0 ** -53            # a rounding of a speed below 1 a step
        y = _flow(x, -3.0, drow, T, watch=w)
        if T < 0.31 / 3.0:
            assert abs(y[3] - (0.31 - 3.0 * T)) <= rnd
        else:
            crossed = True
            assert y[3] == 0.0 and not np.signbit(y[3])       # exactly +0.0, while x[4] < 0
            assert y[4] == -3.0
        free = _flow(x, -3.0, _row(), T)                      # HOLD = 0 on the same lane
        assert abs(free[3] - (0.31 - 3.0 * T)) <= rnd
    assert crossed and w["projected"] >= 1 and free[3] < -0.8
    # position and heading stop with the speed
    a, b = _flow(x, -3.0, drow, 0.3), _flow(x, -3.0, drow, 0.4)
    assert np.array_equal(a[:4], b[:4])


def test_hold_releases_when_the_lagged_acceleration_turns_positive():
    """At rest with a realised a0 < 0 and a_eff > 0 behind a lag: held until
    t* = tau ln((a_eff - a0) / a_eff), then s(t) = a_eff (t - t*) - a_eff tau (1 - e^-(t - t*)/tau)
    (the closed form restarted at t* with a = 0).  The RK4 step that holds t* evaluates the gate
    at its stages, so the release is resolved to a step of h = 2.5 ms, in which the acceleration
    stays below h a_eff / tau: at most h^2 a_eff / (2 tau) = 3.1e-5 m/s of speed, the bound
    below; measured 4.8e-7."""
    tau, a0, ae = 0.1, -2.0, 1.0
    t_star = tau * math.log((ae - a0) / ae)
    x = X0.copy()
    x[3], x[4] = 0.0, a0
    drow = _row(tau=tau, hold=1.0)
    worst = 0.0
    for k in range(1, 11):
        T = k * DC.TICK
        y = _flow(x, ae, drow, T)
        a, _ = DM.closed_form(0.0, a0, ae, tau, T)
        assert abs(float(y[4] - a)) <= DC.LAG_ERROR[0.1][0]
        if T < t_star:
            assert y[3] == 0.0
        else:
            _, s = DM.closed_form(0.0, 0.0, ae, tau, T - t_star)
            worst = max(worst, abs(float(y[3] - s)))
            assert y[3] > 0.0
    print(f"release at t* = {t_star:.5f}: max |s - closed form| = {worst:.3g}")
    # the step that holds t* is of length h = 2.5 ms and the acceleration there is below
    # h (a_eff - a0) / tau * e^(-t*/tau) = h a_eff / tau = 0.025: at most h * 0.025 / 2 of speed
    assert worst <= 0.5 * DC.H_MAX * DC.H_MAX * ae / tau
    # HOLD = 0 on the same lane goes negative first
    assert _flow(x, ae, _row(tau=tau), 0.1)[3] < -0.05


def test_ideal_row_is_the_truth_mirror_with_a_eff_bitwise():
    rng = np.random.default_rng(0)
    for i in range(40):
        x = rng.uniform(-1, 1, 6) * np.array([30, 30, 3, 6, 0.5, 0.3])
        u, cmd = rng.uniform(-0.3, 0.3), rng.uniform(-3, 2)
        trow = np.array([0.3, 0.34, rng.uniform(0.08, 0.2), rng.uniform(0.8, 1.25), 0.01])
        T = 0.05 * (1 + i % 4)
        n = DM.steps_for(T, DC.H_MAX)
        z = rng.standard_normal((4 * n, 2)) if i % 2 else None
        pair = (0.0, 0.0) if i % 3 else tuple(rng.standard_normal(2) * 1e-3)
        got = DM.rk4_flow(x, u, cmd, trow, DM.ideal_row(), T, n, z, 1e-2, pair)
        x2 = x.copy()
        x2[4] = DM.a_eff(DM.ideal_row(), cmd)
        assert x2[4] == cmd
        if z is None and pair != (0.0, 0.0):
            continue                                      # truth_mirror has no constant pair
        assert np.array_equal(got, TM.rk4_flow(x2, u, trow, T, n, z, 1e-2))
    # a row that is not the ideal one but does the same: limits that are never reached
    row = _row(a_max=1e30, b_max=1e30)
    assert np.array_equal(_flow(X0, -2.0, row, 0.2), _flow(X0, -2.0, DM.ideal_row(), 0.2))


# ---------------------------------------------------------------------------
# 4. the mirror sampler
# ---------------------------------------------------------------------------
def _mirror_dist(seed=11, b_offset=0):
    d = DM.Dist(2, seed, b_offset)
    return d.fixed(DM.TAU_A, 0.2).fixed(DM.B_MAX, 3.0)


def test_mirror_sampler_fixed_uniform_and_clamps():
    d = DM.Dist(2, 11)
    s = DM.sample(d, 5)
    assert s.shape == (5, 2, 6)
    assert np.array_equal(s, np.broadcast_to(DM.IDEAL_ROW, s.shape))   # FIXED: exactly the mean
    d = _mirror_dist().set(DM.TAU_A, DM.UNIFORM, 0.15, 0.1, 0.3).set(DM.B_MAX, DM.NORMAL, 1.0, 1.5)
    d.fixed(DM.HOLD, 1.0)
    s = DM.sample(d, 400)
    assert np.all(s[..., DM.TAU_A] >= 0.1) and np.all(s[..., DM.TAU_A] <= 0.3)
    assert (s[..., DM.TAU_A] == 0.1).any() and (s[..., DM.TAU_A] == 0.3).any()
    assert np.all(s[..., DM.B_MAX] >= 1.5) and (s[..., DM.B_MAX] == 1.5).any()
    assert np.all(s[..., DM.HOLD] == 1.0) and np.all(s[..., DM.A_MAX] == INF)
    assert np.all(s[..., DM.GAIN_A] == 1.0)
    assert not any(DM.is_bad(r, 0.0) for r in s.reshape(-1, 6))
    x = DM.xi(d.set(DM.GAIN_A, DM.UNIFORM, 0.1), 8)
    assert not np.any(x[..., DM.TAU_A] == x[..., DM.GAIN_A])
    assert not np.any(x[:, 0, DM.TAU_A] == x[:, 1, DM.TAU_A])
    assert np.all(x[..., DM.HOLD] == 0.0)                  # a FIXED field draws nothing


def test_mirror_sampler_does_not_depend_on_the_sharding():
    def dist(off):
        return _mirror_dist(77, off).set(DM.TAU_A, DM.UNIFORM, 0.1, 0.1).set(DM.GAIN_A, DM.NORMAL, 0.1, 0.5, 1.5)
    whole = DM.sample(dist(0), 6)
    parts = np.concatenate([DM.sample(dist(0), 3), DM.sample(dist(3), 3)])
    assert np.array_equal(whole, parts)
    assert not np.array_equal(whole[:3, :, DM.TAU_A], whole[3:, :, DM.TAU_A])


def test_mirror_sampler_draws_differ_from_the_truth_samplers():
    """The same seed, field index, vehicle and realisation at site 3 and at site 9."""
    t = TM.Dist(np.zeros((5, 2)), 11).set(TM.LF, TM.UNIFORM, 1.0)
    d = _mirror_dist(11).set(DM.TAU_A, DM.UNIFORM, 1.0)
    assert not np.any(TM.xi(t, 16)[..., 0] == DM.xi(d, 16)[..., 0])


# ---------------------------------------------------------------------------
# 5. the case table's conditions, none left out
# ---------------------------------------------------------------------------
def test_case_table_covers_what_it_says():
    d = DC.inputs()
    assert d["x_start"].shape == (DC.B, DC.V, 6) and d["u_tick"].shape == (DC.B, DC.V, DC.N_TICKS + 1)
    assert DC.B * DC.V * (DC.N_TICKS + 1) > 256              # more than one workgroup
    assert {"ideal", "lag_8h", "lag_01", "lag_04", "gain_bias", "amax_on", "amax_off", "bmax_on",
            "bmax_off", "hold_early", "hold_late", "hold_never", "hold_released",
            "hold_lag_released", "hold_lag_cross", "free_early", "mixed"} <= set(DC.KINDS)
    assert d["drive"][DC.rows_of("lag_8h")[0]][DM.TAU_A] == 8 * DC.H_MAX
    for b, v in DC.rows_of("ideal") + DC.rows_of("ideal_zero"):
        assert np.array_equal(d["drive"][b, v], DM.IDEAL_ROW)
    # every kind of bad row, each bad for one reason, next to good ones
    assert len(DC.BAD) == 9
    for r in range(DC.B * DC.V):
        b, v = r // DC.V, r % DC.V
        assert DM.is_bad(d["drive"][b, v], d["a_cmd"][b, v]) == (r in DC.BAD)
    for r in DC.BAD:
        assert r - 1 not in DC.BAD or r + 1 not in DC.BAD
    # rows of different paths share a wave: lag / no lag and hold / no hold within rows 0..6
    first = d["drive"][:4].reshape(-1, 6)[:7]
    assert len(set(first[:, DM.TAU_A] > 0)) == 2
    assert len({(t > 0, h) for t, h in d["drive"].reshape(-1, 6)[7:14, [0, 5]]}) >= 3
    assert not np.any(d["u_tick"] == 0.0)


def test_no_clamp_argument_is_near_its_limit():
    d = DC.inputs()
    on = off = 0
    for r in range(DC.B * DC.V):
        b, v = r // DC.V, r % DC.V
        if r in DC.BAD:
            continue
        row = d["drive"][b, v]
        raw = float(DM.raw_command(row, d["a_cmd"][b, v]))
        for lim in (row[DM.A_MAX], -row[DM.B_MAX]):
            if math.isfinite(lim):
                assert abs(raw - lim) >= DC.SEP, (r, raw, lim)
                on += (raw > lim) if lim >= 0 else (raw < lim)
                off += not ((raw > lim) if lim >= 0 else (raw < lim))
    assert on >= 4 and off >= 4
    for kind, active in (("amax_on", True), ("amax_off", False)):
        b, v = DC.rows_of(kind)[0]
        assert (DM.a_eff(d["drive"][b, v], d["a_cmd"][b, v]) == d["drive"][b, v, DM.A_MAX]) == active
    for kind, active in (("bmax_on", True), ("bmax_off", False)):
        b, v = DC.rows_of(kind)[0]
        assert (DM.a_eff(d["drive"][b, v], d["a_cmd"][b, v]) == -d["drive"][b, v, DM.B_MAX]) == active


@pytest.mark.parametrize("form", DC.FORMS)
def test_no_rounding_can_flip_the_gate_or_the_projection(form):
    d = DC.inputs()
    out, watch = DC.mirror(form), DC.mirror(form, watch=True)
    seen = 0
    for r in range(DC.B * DC.V):
        b, v = r // DC.V, r % DC.V
        if r in DC.BAD or d["drive"][b, v, DM.HOLD] != 1.0:
            continue
        for k in range(DC.N_TICKS + 1):
            w = watch[(b, v, k)]
            sp = np.array(w["speeds"])
            assert np.all((sp == 0.0) | (np.abs(sp) >= 1e-9)), (DC.KINDS[r], k)
            assert all(abs(a) >= 1e-9 for a in w["accels"]), (DC.KINDS[r], k)
            seen += len(sp)
    assert seen > 10000
    # every crossing lane really crosses, the others never do
    for kind in set(DC.KINDS):
        for b, v in DC.rows_of(kind):
            if kind.startswith("bad_"):
                assert np.isnan(out[b, v]).all()
                continue
            proj = [watch[(b, v, k)]["projected"] for k in range(DC.N_TICKS + 1)]
            if kind in DC.CROSSING:
                assert d["x_start"][b, v, 3] > 0 and proj[-1] == 1 and out[b, v, -1, 3] == 0.0
                assert max(proj) == 1
            else:
                assert sum(proj) == 0, kind
    (b, v), = DC.rows_of("hold_early")
    assert np.all(out[b, v, 1:, 3] == 0.0)                    # early: inside the first tick
    (b, v), = DC.rows_of("hold_late")
    assert np.all(out[b, v, :7, 3] > 0.0) and np.all(out[b, v, 7:, 3] == 0.0)
    for b, v in DC.rows_of("hold_never"):
        assert np.all(out[b, v, :, 3] > 1.0)
    (b, v), = DC.rows_of("hold_released")
    assert out[b, v, 0, 3] == 0.0 and np.all(np.diff(out[b, v, :, 3]) > 0.04)
    (b, v), = DC.rows_of("hold_lag_released")
    assert np.all(out[b, v, :3, 3] == 0.0) and np.all(out[b, v, 3:, 3] > 0.0)
    (b, v), = DC.rows_of("free_early")
    assert out[b, v, -1, 3] < -1.0
    assert not np.isnan(out[[r // DC.V for r in range(32) if r not in DC.BAD],
                            [r % DC.V for r in range(32) if r not in DC.BAD]]).any()


def test_tolerance_is_sixteen_times_the_rounding_of_the_definition():
    worst = {form: DC.ratio(DC.mirror(form, DM.F64), DC.mirror(form, DM.F80)) for form in DC.FORMS}
    print("drive mirror float64 against 80-bit:", {k: f"{v:.3g}" for k, v in worst.items()})
    big = max(worst.values())
    assert 0.5 * DC.MIRROR_ROUNDING <= big <= DC.MIRROR_ROUNDING
    assert DC.TOL == DC.pow2_ceil(16 * DC.MIRROR_ROUNDING)


# ---------------------------------------------------------------------------
# 6. scpqp.drive on the host
# ---------------------------------------------------------------------------
def test_rows_ideal_and_validate():
    r = DRV.rows(3, 2, tau=[0.3, 0.0], b_max=1.5, hold=1, device="cpu")
    assert tuple(r.shape) == (3, 2, 6) and r.dtype.is_floating_point
    assert r[1, 0].tolist() == [0.3, 1.0, 0.0, INF, 1.5, 1.0] and r[2, 1, 0] == 0.0
    assert np.array_equal(DRV.ideal_rows(2), np.broadcast_to(DM.IDEAL_ROW, (2, 6)))
    assert DRV.is_ideal(DRV.rows(4, 2, device="cpu")) and not DRV.is_ideal(r)
    assert not DRV.is_ideal(DRV.rows(4, 2, a_max=1e30, device="cpu"))
    good = r.numpy().copy()
    DRV.validate(good, 2.5e-3)
    DRV.validate(r, 2.5e-3)
    for f, vals, msg in ((0, (-0.1, NAN), "tau_a must be >= 0"), (0, (INF,), "tau_a is not finite"),
                         (1, (INF, NAN), "gain_a is not finite"), (2, (-INF, NAN), "bias_a is not finite"),
                         (3, (-1.0, NAN), "a_max must be >= 0"), (4, (-1e-9, NAN), "b_max must be >= 0"),
                         (5, (0.5, -1.0, NAN, 2.0), "hold must be 0 or 1")):
        for bad in vals:
            t = good.copy()
            t[2, 1, f] = bad
            with pytest.raises(ValueError, match=msg):
                DRV.validate(t, 2.5e-3)
    t = good.copy()
    t[1, 0, 0] = 0.0199
    with pytest.raises(ValueError, match="8 \\* h_max"):
        DRV.validate(t, 2.5e-3)
    t[1, 0, 0] = 0.02
    DRV.validate(t, 2.5e-3)
    with pytest.raises(ValueError, match="8 \\* h_max"):
        DRV.validate(good, 0.04)                              # tau_a = 0.3 < 8 * 0.04
    DRV.validate(DRV.ideal_rows(2)[None], 1.0)                # no lag: any h_max
    with pytest.raises(ValueError, match="\\[B, nVeh, 6\\]"):
        DRV.validate(good[..., :5], 2.5e-3)


def test_drive_dist_object_and_its_refusals():
    d = DRV.DriveDist(2, seed=9, b_offset=4)
    c = d.c_struct()
    assert (c.n_veh, c.seed, c.b_offset) == (2, 9, 4)
    assert [c.field[f].kind for f in range(6)] == [LB.TRUTH_FIXED] * 6
    assert [c.mean[f][1] for f in range(6)] == list(DM.IDEAL_ROW)
    d.fixed("tau_a", 0.2).uniform("tau_a", 0.1, 0.1, 0.3).fixed("b_max", [3.0, 2.5])
    d.normal("b_max", 0.5, lo=1.0).fixed("hold", 1)
    c = d.c_struct()
    assert (c.field[0].kind, c.field[0].spread, c.field[0].lo, c.field[0].hi) == (1, 0.1, 0.1, 0.3)
    assert (c.field[4].kind, c.mean[4][0], c.mean[4][1], c.field[4].lo) == (2, 3.0, 2.5, 1.0)
    assert c.mean[5][0] == 1.0 and c.field[5].kind == LB.TRUTH_FIXED
    e = d.with_offset(100)
    assert (e.b_offset, d.b_offset, e.seed) == (100, 4, 9) and e.kind == d.kind
    fresh = lambda: DRV.DriveDist(2, seed=1)
    for bad in (lambda: fresh().uniform("mass", 0.1), lambda: fresh().uniform("gain_a", -0.1),
                lambda: fresh().uniform("gain_a", NAN), lambda: fresh().normal("gain_a", 0.1, 1.0, 0.5),
                lambda: fresh().uniform("hold", 0.5, 0.0, 1.0), lambda: fresh().fixed("hold", 0.5),
                lambda: fresh().uniform("b_max", 0.5, lo=1.0),            # its mean is +inf
                lambda: fresh().fixed("b_max", 3.0).normal("b_max", 0.5),  # lo = -inf
                lambda: fresh().fixed("tau_a", 0.2).uniform("tau_a", 0.3, lo=-0.1),
                lambda: fresh().fixed("tau_a", -0.2), lambda: fresh().fixed("gain_a", INF),
                lambda: fresh().fixed("a_max", NAN), lambda: fresh().uniform("bias_a", 0.1, INF, INF),
                lambda: DRV.DriveDist(2, seed=-1), lambda: DRV.DriveDist(0, seed=1),
                lambda: DRV.DriveDist(2, seed=1, b_offset=2 ** 32)):
        with pytest.raises(ValueError):
            bad()


def test_from_table_gathers_rows():
    import torch
    rows = np.arange(3 * 2 * 6, dtype=float).reshape(3, 2, 6)
    t = DRV.from_table(rows, [2, 0, 0, 1], device="cpu")
    assert t.dtype == torch.float64 and tuple(t.shape) == (4, 2, 6) and t.is_contiguous()
    assert np.array_equal(t.numpy(), rows[[2, 0, 0, 1]])
    with pytest.raises(ValueError):
        DRV.from_table(rows, [3], device="cpu")
    with pytest.raises(ValueError):
        DRV.from_table(rows[..., :5], [0], device="cpu")


def test_plant_step_takes_the_pair_or_neither():
    from scpqp import plant as PL
    p = PL.plant_params([0.3], [0.34])
    x, u = np.zeros((1, 1, 6)), np.zeros((1, 1, 3))
    for kw in (dict(drive=DRV.ideal_rows(1)[None]), dict(a_cmd=np.zeros((1, 1)))):
        with pytest.raises(ValueError, match="drive and a_cmd"):
            PL.plant_step(p, x, u, 0.01, device="cpu", **kw)
    assert "drive" not in PL.delay_compensate.__code__.co_varnames   # the controller's prediction
