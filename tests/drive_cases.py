"""The inputs of the drive-truth tests, shared by the CPU tests (tests/test_drive_host.py: the
conditions on the table and the tolerance are pinned there, on the mirror alone) and the GPU
tests (tests/test_gpu_drive.py), so that both see exactly the same numbers.

One table: B = 16 realisations of 2 vehicles, 8 ticks of 0.05 s at h_max = 2.5 ms (up to 160
RK4 steps a lane).  That is 32 (b, v) rows of 9 output ticks, 288 lanes: two workgroups of 256
with a ragged tail, and every wave of 64 lanes holds about seven rows of different kinds, so
the rows are mixed within a wave.  Row r = 2 b + v is of kind ``KINDS[r]``:

  ideal, ideal_zero              the ideal row (a command of 0 for the second)
  lag_8h, lag_01, lag_04         a lag only, TAU_A = 8 h_max, 0.1 and 0.4
  gain_bias                      GAIN_A 0.8, BIAS_A -0.3
  amax_on / amax_off             A_MAX = 1 with a command of 2 / of 0.5
  bmax_on / bmax_off             B_MAX = 1.5 with a command of -3 / of -1
  hold_early / hold_late / hold_never
                                 HOLD lanes braking at 3 m/s^2 from 0.05, 0.95 and 4 m/s: the
                                 speed crosses zero inside the first tick, inside the seventh,
                                 and not at all
  hold_released                  HOLD, at rest, a command of +1: it drives off at once
  hold_lag_released              HOLD, at rest with a realised -2 m/s^2, a command of +1 behind
                                 TAU_A = 0.1: held until t* = tau ln 3 = 0.11 s, then off
  hold_lag_cross                 HOLD, 0.3 m/s, a realised -1, a command of -3, TAU_A = 0.1
  free_early                     hold_early's lane with HOLD = 0: it goes negative
  bad_*                          every kind of bad row, next to good ones
  mixed                          HOLD, lag 0.4, gain, bias and both clamps set, B_MAX active
  lag_amax                       lag 0.1 with A_MAX active

The truth rows alternate between the nominal one and rows away from it.  Three forms: noise
free, a constant pair, and seeded (sigma = 1e-2, as the plant's noise tests use).

Conditions, checked by test_drive_host.py with none left out: no clamp argument within
SEP = 1e-9 of its limit; in HOLD lanes no stage speed of the float64 mirror within 1e-9 of zero
unless it is exactly zero, and no acceleration within 1e-9 of zero where the gate's speed test
holds, so no rounding can flip the gate or the projection; every crossing lane really crosses."""
from __future__ import annotations

import functools
import math

import numpy as np

import drive_mirror as DM
import truth_mirror as TM

B, V, N_TICKS = 16, 2, 8
TICK, H_MAX = 0.05, 2.5e-3
SEP = 1e-9
SEED = 9107
SIGMA = 1e-2
SEEDED = (0x5EEDD21FE, SIGMA, 3, 200)        # seed, sigma, epoch, b_offset
FORMS = ("free", "pair", "seeded")
INF, NAN = math.inf, math.nan

#        name               tau    gain  bias  a_max b_max hold  a_cmd  speed  a0
TABLE = (
    ("ideal",             0.0,   1.0,  0.0,  INF,  INF,  0,   -1.3,  None,  None),
    ("lag_8h",            0.02,  1.0,  0.0,  INF,  INF,  0,   -3.0,  None,  1.0),
    ("lag_01",            0.1,   1.0,  0.0,  INF,  INF,  0,   -3.0,  None,  0.4),
    ("lag_04",            0.4,   1.0,  0.0,  INF,  INF,  0,    1.2,  None,  -2.0),
    ("gain_bias",         0.0,   0.8,  -0.3, INF,  INF,  0,   -2.1,  None,  None),
    ("amax_on",           0.0,   1.0,  0.0,  1.0,  INF,  0,    2.0,  None,  None),
    ("amax_off",          0.0,   1.0,  0.0,  1.0,  INF,  0,    0.5,  None,  None),
    ("bmax_on",           0.0,   1.0,  0.0,  INF,  1.5,  0,   -3.0,  None,  None),
    ("bmax_off",          0.0,   1.0,  0.0,  INF,  1.5,  0,   -1.0,  None,  None),
    ("hold_early",        0.0,   1.0,  0.0,  INF,  INF,  1,   -3.0,  0.05,  None),
    ("hold_late",         0.0,   1.0,  0.0,  INF,  INF,  1,   -3.0,  0.95,  None),
    ("hold_never",        0.0,   1.0,  0.0,  INF,  INF,  1,   -3.0,  4.0,   None),
    ("hold_released",     0.0,   1.0,  0.0,  INF,  INF,  1,    1.0,  0.0,   None),
    ("hold_lag_released", 0.1,   1.0,  0.0,  INF,  INF,  1,    1.0,  0.0,   -2.0),
    ("hold_lag_cross",    0.1,   1.0,  0.0,  INF,  INF,  1,   -3.0,  0.3,   -1.0),
    ("free_early",        0.0,   1.0,  0.0,  INF,  INF,  0,   -3.0,  0.05,  None),
    ("bad_tau_neg",       -0.1,  1.0,  0.0,  INF,  INF,  0,   -1.0,  None,  None),
    ("ideal",             0.0,   1.0,  0.0,  INF,  INF,  0,    0.7,  None,  None),
    ("bad_tau_nan",       NAN,   1.0,  0.0,  INF,  INF,  0,   -1.0,  None,  None),
    ("bad_gain_inf",      0.0,   INF,  0.0,  INF,  INF,  0,   -1.0,  None,  None),
    ("hold_never",        0.1,   1.0,  0.0,  INF,  INF,  1,   -2.0,  None,  0.0),
    ("bad_bias_nan",      0.0,   1.0,  NAN,  INF,  INF,  0,   -1.0,  None,  None),
    ("bad_amax_neg",      0.0,   1.0,  0.0,  -1.0, INF,  0,   -1.0,  None,  None),
    ("mixed",             0.4,   0.9,  -0.2, 2.0,  1.5,  1,   -3.0,  None,  0.3),
    ("bad_bmax_nan",      0.0,   1.0,  0.0,  INF,  NAN,  0,   -1.0,  None,  None),
    ("bad_hold_half",     0.0,   1.0,  0.0,  INF,  INF,  0.5, -1.0,  None,  None),
    ("ideal_zero",        0.0,   1.0,  0.0,  INF,  INF,  0,    0.0,  None,  None),
    ("bad_cmd_inf",       0.0,   1.0,  0.0,  INF,  INF,  0,    INF,  None,  None),
    ("lag_amax",          0.1,   1.0,  0.0,  1.0,  INF,  0,    2.5,  None,  -0.5),
    ("bad_cmd_nan",       0.0,   1.0,  0.0,  INF,  INF,  0,    NAN,  None,  None),
    ("hold_never",        0.4,   1.0,  0.0,  INF,  3.5,  1,   -3.0,  3.0,   0.5),
    ("gain_bias",         0.02,  1.1,  0.25, 4.0,  4.0,  0,   -2.0,  None,  0.1),
)
assert len(TABLE) == B * V
KINDS = tuple(t[0] for t in TABLE)
CROSSING = ("hold_early", "hold_late", "hold_lag_cross")     # must be projected to zero
BAD = tuple(r for r, k in enumerate(KINDS) if k.startswith("bad_"))


def rows_of(kind):
    """The (b, v) of every row of a kind."""
    return [(r // V, r % V) for r, k in enumerate(KINDS) if k == kind]


@functools.lru_cache(maxsize=None)
def inputs():
    """dict of float64 numpy arrays: x_start [B, V, 6], u_tick [B, V, K], truth [B, V, 5], a_cmd
    [B, V], drive [B, V, 6], pair [B, V, 2], and lf, lr per vehicle."""
    rng = np.random.default_rng(SEED)
    K = N_TICKS + 1
    lf, lr = [0.30, 0.32], [0.34, 0.35]
    x = np.zeros((B, V, 6))
    x[..., 0:2] = rng.uniform(-30, 30, (B, V, 2))
    x[..., 2] = rng.uniform(-np.pi, np.pi, (B, V))
    x[..., 3] = rng.uniform(3.0, 4.0, (B, V))
    x[..., 4] = rng.uniform(-0.5, 0.5, (B, V))
    x[..., 5] = rng.uniform(-0.05, 0.05, (B, V))
    u = rng.uniform(-0.078, 0.078, (B, V, K))
    truth = np.zeros((B, V, 5))
    drive = np.zeros((B, V, 6))
    a_cmd = np.zeros((B, V))
    for r, (_, tau, gain, bias, amax, bmax, hold, cmd, speed, a0) in enumerate(TABLE):
        b, v = r // V, r % V
        drive[b, v] = (tau, gain, bias, amax, bmax, hold)
        a_cmd[b, v] = cmd
        if speed is not None:
            x[b, v, 3] = speed
        if a0 is not None:
            x[b, v, 4] = a0
        truth[b, v] = TM.nominal_row(lf[v], lr[v]) if r % 3 == 0 else \
            (0.34 * (1.3 if r & 1 else 0.7), 0.34 * (0.7 if r & 2 else 1.3),
             0.08 if r & 4 else 0.2, 0.8 if r % 5 else 1.25, 0.01 if r & 8 else -0.01)
    pair = rng.standard_normal((B, V, 2)) * 1e-3
    return dict(x_start=x, u_tick=u, truth=truth, a_cmd=a_cmd, drive=drive, pair=pair, lf=lf, lr=lr)


_mirror_cache = {}


def mirror(form, fm=DM.F64, watch=False):
    """The table's plant step on the mirror in ``fm``: [B, V, K, 6], computed once per form and
    number format and shared; with ``watch`` the per-lane watch dict of the float64 run."""
    key = (form, fm.dtype)
    if key not in _mirror_cache:
        d = inputs()
        w = {} if fm is DM.F64 else None
        out = DM.plant_step(d["x_start"], d["u_tick"], d["truth"], d["a_cmd"], d["drive"], TICK,
                            H_MAX, pair=d["pair"] if form == "pair" else None,
                            seeded=SEEDED if form == "seeded" else None, fm=fm, watch=w)
        out.setflags(write=False)
        _mirror_cache[key] = (out, w)
    return _mirror_cache[key][1 if watch else 0]


# ---------------------------------------------------------------------------
# The comparison and its tolerance
# ---------------------------------------------------------------------------
def ratio(dev, mir):
    """The one figure of the comparison: max |dev - mir| / (1 + |mir|) over the six states of
    every lane, with ``mir`` the reference; the NaN patterns must be identical."""
    x, m = np.asarray(dev, dtype=np.longdouble), np.asarray(mir, dtype=np.longdouble)
    assert x.shape == m.shape and (np.isnan(x) == np.isnan(m)).all()
    ok = ~np.isnan(m)
    return float((np.abs(x - m)[ok] / (1.0 + np.abs(m[ok]))).max())


def pow2_ceil(v):
    return 2.0 ** math.ceil(math.log2(v))


# Tolerance of the device against the float64 mirror, in the figure of ``ratio``.  It is derived
# on the CPU from the reference alone (tests/test_drive_host.py,
# test_tolerance_is_sixteen_times_the_rounding_of_the_definition): the largest figure between the
# mirror in float64 and the mirror in 80-bit over the table's three forms is MIRROR_ROUNDING.
# The device contracts multiply-adds and has its own tan, atan, sin, cos, sqrt and division: 16
# times the figure, rounded up to a power of two.
# Per form: free 6.75e-15, pair 8.07e-15, seeded 6.75e-15 (positions of up to 30 m over up to
# 160 RK4 steps).
MIRROR_ROUNDING = 8.07e-15
TOL = 2.0 ** -42                  # 16 * 8.07e-15 = 1.29e-13 <= 2^-42 = 2.27e-13

# The lag's distance from its closed form at HOLD = 0 (include/scpqp_drive.h, Accuracy), measured
# by tests/test_drive_host.py::test_mirror_lag_against_the_closed_form and recorded there and in
# the header: tau -> (error of a, error of s), h_max = 2.5 ms, ten ticks of 0.05 s, a0 - a_eff = 4.
LAG_ERROR = {0.4: (1.9e-11, 7.6e-12), 0.1: (4.9e-9, 4.9e-10), 0.04: (2.0e-7, 7.7e-9),
             0.02: (1.9e-6, 3.8e-8)}
