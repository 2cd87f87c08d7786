"""Sensing truth, the parts that need no GPU: the C-ABI of include/scpqp_sensing.h (exports,
ctypes layout by a gcc probe of the header, argument validation without touching a device),
the CPU mirror's self-checks (tests/sensing_mirror.py) and scpqp.sensing's host side."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import noise_mirror as NM
import sensing_mirror as SM
from scpqp import _lib as LB
from scpqp import sensing as SE
from scpqp.build import LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scpqp_sensing.h")
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
def test_sensing_header_declares_the_boundary():
    assert header_functions() == sorted(LB.SENSE_EXPORTS)
    others = (set(LB.EXPORTS) | set(LB.NOISE_EXPORTS) | set(LB.METRICS_EXPORTS)
              | set(LB.VARIANT_EXPORTS) | set(LB.TRUTH_EXPORTS) | set(LB.OBSTACLE_EXPORTS))
    assert not set(LB.SENSE_EXPORTS) & others


def test_library_exports_every_sensing_symbol(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\sT\s(scpqp_\w+)", out))
    assert set(header_functions()) <= exported
    for name in LB.SENSE_EXPORTS:
        assert hasattr(lib, name)


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "scpqp_sensing.h"
int main(void) {
  printf("size %zu\n", sizeof(scpqp_sense_dist));
  printf("n_veh %zu\n", offsetof(scpqp_sense_dist, n_veh));
  printf("mean %zu\n", offsetof(scpqp_sense_dist, mean));
  printf("field %zu\n", offsetof(scpqp_sense_dist, field));
  printf("seed %zu\n", offsetof(scpqp_sense_dist, seed));
  printf("b_offset %zu\n", offsetof(scpqp_sense_dist, b_offset));
  printf("ssize %zu\n", sizeof(scpqp_sense_stream));
  printf("sseed %zu\n", offsetof(scpqp_sense_stream, seed));
  printf("sepoch %zu\n", offsetof(scpqp_sense_stream, epoch));
  printf("sb_offset %zu\n", offsetof(scpqp_sense_stream, b_offset));
  printf("fsize %zu\n", sizeof(scpqp_truth_field));
  printf("np %d\n", SCPQP_SENSE_NP);
  printf("onp %d\n", SCPQP_OSENSE_NP);
  printf("idx %d%d%d%d%d%d%d%d\n", SCPQP_SENSE_SIG_POS, SCPQP_SENSE_SIG_HEADING,
         SCPQP_SENSE_SIG_SPEED, SCPQP_SENSE_SIG_STEER, SCPQP_SENSE_BIAS_HEADING,
         SCPQP_SENSE_SCALE_SPEED, SCPQP_SENSE_P_DROP, SCPQP_SENSE_LAG);
  printf("oidx %d%d%d\n", SCPQP_OSENSE_SIG_POS, SCPQP_OSENSE_SIG_HEADING, SCPQP_OSENSE_SIG_SPEED);
  printf("sites %d%d%d\n", SCPQP_NOISE_SITE_SENSE, SCPQP_NOISE_SITE_SENSE_DRAW,
         SCPQP_NOISE_SITE_SENSE_OBST);
  printf("maxveh %d\n", SCPQP_MAX_VEH);
  return 0;
}
"""


def test_sensing_ctypes_layout_matches_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", f"-I{os.path.dirname(HEADER)}", str(src), "-o", str(exe)],
                   check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(LB.SenseDist)
    for f in ("n_veh", "mean", "field", "seed", "b_offset"):
        assert int(got[f]) == getattr(LB.SenseDist, f).offset, f
    assert int(got["ssize"]) == C.sizeof(LB.SenseStream) == 16
    for f in ("seed", "epoch", "b_offset"):
        assert int(got["s" + f]) == getattr(LB.SenseStream, f).offset, f
    assert int(got["fsize"]) == C.sizeof(LB.TruthField)
    assert int(got["np"]) == LB.SENSE_NP == SM.NP == SE.NP == 8
    assert int(got["onp"]) == LB.OSENSE_NP == SM.ONP == SE.ONP == 3
    assert got["idx"] == "01234567" and got["oidx"] == "012"
    assert (LB.SENSE_SIG_POS, LB.SENSE_SIG_HEADING, LB.SENSE_SIG_SPEED, LB.SENSE_SIG_STEER,
            LB.SENSE_BIAS_HEADING, LB.SENSE_SCALE_SPEED, LB.SENSE_P_DROP, LB.SENSE_LAG) \
        == tuple(range(8)) == (SM.SIG_POS, SM.SIG_HEADING, SM.SIG_SPEED, SM.SIG_STEER,
                               SM.BIAS_HEADING, SM.SCALE_SPEED, SM.P_DROP, SM.LAG)
    assert len(LB.SENSE_FIELDS) == 8 and len(LB.OSENSE_FIELDS) == 3
    assert got["sites"] == "567"
    assert (LB.NOISE_SITE_SENSE, LB.NOISE_SITE_SENSE_DRAW, LB.NOISE_SITE_SENSE_OBST) == (5, 6, 7) \
        == (SM.SITE_SENSE, SM.SITE_SENSE_DRAW, SM.SITE_SENSE_OBST)
    assert not {5, 6, 7} & {LB.NOISE_SITE_DELAY, LB.NOISE_SITE_PLANT, LB.NOISE_SITE_LINEARIZE,
                            LB.NOISE_SITE_TRUTH, LB.NOISE_SITE_OBSTACLE}
    assert int(got["maxveh"]) == LB.MAX_VEH


# ---------------------------------------------------------------------------
# 2. argument validation without a GPU
# ---------------------------------------------------------------------------
def _dummy():
    buf = (C.c_double * 256)()
    return buf, C.cast(buf, C.c_void_p)


def test_measure_argument_validation_without_gpu(lib):
    _keep, D = _dummy()
    st = LB.SenseStream(seed=1, epoch=0, b_offset=0)
    S = C.byref(st)

    def err():
        return lib.scpqp_last_error()

    def measure(B=0, n_veh=3, n_ticks=40, k_meas=37, x=None, rows=None, s=None, held=None,
                deliv=None, out=None):
        return lib.scpqp_sense_measure(B, n_veh, n_ticks, k_meas, x, rows, s, held, deliv, out, None)

    assert measure() == 0                                   # B = 0: a no-op, NULL arrays
    assert measure(n_ticks=0, k_meas=0) == 0                # the step-0 form
    assert measure(k_meas=40) == 0 and measure(k_meas=0) == 0
    assert measure(B=-1) == E_ARG and b"batch" in err()
    for n in (0, -1, LB.MAX_VEH + 1):
        assert measure(n_veh=n) == E_ARG and b"n_veh" in err()
    assert measure(n_veh=LB.MAX_VEH) == 0
    assert measure(n_ticks=-1, k_meas=0) == E_ARG and b"n_ticks" in err()
    for k in (41, -1, 2 ** 31 - 1):
        assert measure(k_meas=k) == E_ARG and b"k_meas" in err()
    assert measure(n_ticks=0, k_meas=1) == E_ARG and b"k_meas" in err()
    full = dict(x=D, rows=D, s=S, held=D, out=D)
    for missing, word in (("x", b"x_path"), ("rows", b"sense"), ("s", b"stream"),
                          ("held", b"x_held"), ("out", b"output")):
        kw = dict(full)
        kw[missing] = None
        assert measure(B=3, **kw) == E_ARG and word in err(), missing
    # sizes before the pointers; delivered may be NULL (nothing is launched for a size error)
    assert measure(B=1 << 24, n_veh=16, n_ticks=40, **full) == E_SIZE and b"too large" in err()
    assert measure(B=1 << 24, n_veh=16, n_ticks=40) == E_SIZE
    assert measure(B=1, n_veh=16, n_ticks=2 ** 31 - 2, k_meas=0) == E_SIZE


def test_fill_and_predict_sensed_argument_validation_without_gpu(lib):
    _keep, D = _dummy()
    st = LB.SenseStream(seed=1, epoch=0, b_offset=0)
    S = C.byref(st)

    def err():
        return lib.scpqp_last_error()

    def fill(B=0, n_veh=2, out=None):
        return lib.scpqp_sense_fill_nominal(B, n_veh, out, None)

    assert fill() == 0
    assert fill(B=-1) == E_ARG and b"batch" in err()
    for n in (0, LB.MAX_VEH + 1):
        assert fill(n_veh=n) == E_ARG and b"n_veh" in err()
    assert fill(B=3) == E_ARG and b"sense" in err()
    assert fill(B=1 << 30, n_veh=16, out=D) == E_SIZE

    def predict(B=0, n_obst=3, hp=10, rows=None, osense=None, s=None, t=0.4, lead=0.43, dt=0.4,
                out=None):
        return lib.scpqp_obstacles_predict_sensed(B, n_obst, hp, rows, osense, s, t, lead, dt, out,
                                                  None)

    assert predict() == 0
    assert predict(B=-1) == E_ARG and b"batch" in err()
    for n in (0, -1, LB.MAX_OBST + 1):
        assert predict(n_obst=n) == E_ARG and b"n_obst" in err()
    for hp in (0, -3, LB.MAX_HP + 1):
        assert predict(hp=hp) == E_ARG and b"hp" in err()
    assert predict(n_obst=LB.MAX_OBST, hp=LB.MAX_HP) == 0
    for kw in (dict(t=math.nan), dict(lead=math.inf), dict(dt=-math.inf)):
        assert predict(**kw) == E_ARG and b"finite" in err()
    full = dict(rows=D, osense=D, s=S, out=D)
    for missing, word in (("rows", b"rows"), ("osense", b"osense"), ("s", b"stream"),
                          ("out", b"output")):
        kw = dict(full)
        kw[missing] = None
        assert predict(B=3, **kw) == E_ARG and word in err(), missing
    assert predict(B=1 << 22, n_obst=32, hp=64, **full) == E_SIZE and b"too large" in err()
    assert predict(B=1 << 22, n_obst=32, hp=64) == E_SIZE


def _dist(n_veh=2):
    d = LB.SenseDist()
    d.n_veh = n_veh
    for v in range(LB.MAX_VEH):
        d.mean[LB.SENSE_SCALE_SPEED][v] = 1.0
    d.seed = 5
    return d


def _field(d, f, kind, spread=0.0, lo=-math.inf, hi=math.inf):
    d.field[f].kind, d.field[f].spread, d.field[f].lo, d.field[f].hi = kind, spread, lo, hi
    return d


def test_sample_argument_validation_without_gpu(lib):
    _keep, D = _dummy()

    def sample(d, B=0, out=None):
        return lib.scpqp_sense_sample(None if d is None else C.byref(d), B, out, None)

    def err():
        return lib.scpqp_last_error()

    assert sample(None) == E_ARG and b"null" in err()
    assert sample(_dist()) == 0                           # all FIXED at nominal, B = 0, NULL array
    for n in (0, -1, LB.MAX_VEH + 1):
        assert sample(_dist(n)) == E_ARG and b"n_veh" in err()
    for f, name in enumerate(LB.SENSE_FIELDS):
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
        # a non-finite mean, fixed or not, inside n_veh only
        for bad in (math.nan, math.inf):
            d = _dist()
            d.mean[f][1] = bad
            assert sample(d) == E_ARG and nm in err() and b"mean" in err()
            assert sample(_field(d, f, U, 0.1, 0.0, 1.0)) == E_ARG and nm in err()
            d.n_veh = 1                                   # vehicle 1 is outside: not looked at
            assert sample(d) == 0
    # a distribution whose floor could emit a bad row: every sigma, P_DROP and LAG below 0
    for f in (LB.SENSE_SIG_POS, LB.SENSE_SIG_HEADING, LB.SENSE_SIG_SPEED, LB.SENSE_SIG_STEER,
              LB.SENSE_P_DROP, LB.SENSE_LAG):
        nm = LB.SENSE_FIELDS[f].encode()
        assert sample(_field(_dist(), f, U, 0.5)) == E_ARG and nm in err()          # lo = -inf
        assert sample(_field(_dist(), f, N, 0.5, -1e-9, 1.0)) == E_ARG and nm in err()
        assert sample(_field(_dist(), f, U, 0.5, 0.0, 1.0)) == 0
        d = _dist()
        d.mean[f][0] = -0.5                               # FIXED: its floor is the mean
        assert sample(d) == E_ARG and nm in err() and b">= 0" in err()
    # P_DROP above 1: the floor, the hi, a FIXED mean
    f, nm = LB.SENSE_P_DROP, b"p_drop"
    assert sample(_field(_dist(), f, U, 0.5, 0.0, 1.5)) == E_ARG and nm in err() and b"[0, 1]" in err()
    assert sample(_field(_dist(), f, N, 0.5, 0.0)) == E_ARG and nm in err()         # hi = +inf
    assert sample(_field(_dist(), f, U, 0.5, 1.5, 2.0)) == E_ARG and nm in err()
    d = _dist()
    d.mean[f][1] = 1.5
    assert sample(d) == E_ARG and nm in err() and b"[0, 1]" in err()
    d.mean[f][1] = 1.0
    assert sample(d) == 0
    # the offset and the scale need no floor
    assert sample(_field(_dist(), LB.SENSE_BIAS_HEADING, N, 0.02)) == 0
    assert sample(_field(_dist(), LB.SENSE_SCALE_SPEED, U, 0.05)) == 0
    # sizes and arrays
    assert sample(_dist(), B=-1) == E_ARG
    assert sample(_dist(), B=3) == E_ARG and b"sense" in err()
    assert sample(_dist(16), B=1 << 30, out=D) == E_SIZE


# ---------------------------------------------------------------------------
# 3. the mirror checks itself
# ---------------------------------------------------------------------------
def _path(B, V, K, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-50, 50, (B, V, K, 6))
    x[..., 2] = rng.uniform(-math.pi, math.pi, (B, V, K))
    x[..., 3] = rng.uniform(0, 10, (B, V, K))
    x[..., 5] = rng.uniform(-0.3, 0.3, (B, V, K))
    return x


def test_mirror_nominal_row_is_the_identity():
    x = _path(2, 3, 5)
    x[1, 2, 3, 0] = -0.0
    held = np.full((2, 3, 6), np.nan)
    got, deliv = SM.measure(x, 3, SM.nominal_rows(2, 3), 7, 0, 0, held)
    assert np.array_equal(got.view(np.int64), np.ascontiguousarray(x[:, :, 3]).view(np.int64))
    assert np.array_equal(held.view(np.int64), got.view(np.int64)) and deliv.all()
    # an all-zero osense row is obstacle_mirror.predict
    import obstacle_mirror as OM
    rows = np.array([[[7.0, -15.0, 1.2, 2.0, 4.0, 2.0, 0.3], [1.0, 2.0, -0.4, 1.0, 2.0, 1.0, 0.0]]])
    want = OM.predict(rows, 1.6, 0.43, 0.4, 4)
    assert np.array_equal(SM.predict_sensed(rows, np.zeros((1, 2, 3)), 9, 1, 0, 1.6, 0.43, 0.4, 4), want)
    osense = np.zeros((1, 2, 3))
    osense[0, 1] = [0.1, 0.0, 0.0]
    got = SM.predict_sensed(rows, osense, 9, 1, 0, 1.6, 0.43, 0.4, 4)
    assert np.array_equal(got[0, 0], want[0, 0])
    z0, z1, _ = SM.call(9, 0, 1, SM.SITE_SENSE_OBST, 1, 0)
    # position noise shifts the whole prediction of that obstacle by (0.1 z0, 0.1 z1)
    assert np.abs(got[0, 1, 0] - want[0, 1, 0] - 0.1 * z0).max() <= 2.0 ** -46
    assert np.abs(got[0, 1, 1] - want[0, 1, 1] - 0.1 * z1).max() <= 2.0 ** -46
    osense[0, 0, 2] = -1.0
    assert np.isnan(SM.predict_sensed(rows, osense, 9, 1, 0, 1.6, 0.43, 0.4, 4)[0, 0]).all()


def test_mirror_measurement_formula_and_lag():
    x = _path(1, 2, 6)
    rows = SM.nominal_rows(1, 2)
    rows[0, 0] = [0.05, 0.01, 0.1, 0.002, 0.02, 1.03, 0.0, 2.0]
    rows[0, 1] = [0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 9.0]          # only late: clamps to tick 0
    held = np.full((1, 2, 6), np.nan)
    got, deliv = SM.measure(x, 4, rows, 11, 5, 100, held)
    assert deliv.tolist() == [[1, 1]]
    a0, a1, _ = SM.call(11, 0, 5, 6, 0, 100)
    b0, b1, _ = SM.call(11, 1, 5, 6, 0, 100)
    c0, _, _ = SM.call(11, 2, 5, 6, 0, 100)
    src = x[0, 0, 2]
    want = [src[0] + 0.05 * a0, src[1] + 0.05 * a1, (src[2] + 0.02) + 0.01 * b0,
            1.03 * src[3] + 0.1 * b1, src[4], src[5] + 0.002 * c0]
    assert got[0, 0].tolist() == want
    assert np.array_equal(got[0, 1], x[0, 1, 0])                   # sigma 0: x + 0 * z = x
    assert np.array_equal(NM.normals(11, 0, 5, (6 << 24) | 0, 100), (a0, a1))


def test_mirror_drop_logic_with_a_nan_x_held():
    B, V, K = 4, 2, 3
    rows = SM.nominal_rows(B, V)
    rows[0, :, SM.P_DROP] = 1.0
    rows[1, :, SM.P_DROP] = 0.5
    rows[2, :, SM.SIG_POS] = 0.05                                  # P_DROP = 0: never lost
    rows[3, 0, SM.P_DROP] = 1.5                                    # a bad row
    held = np.full((B, V, 6), np.nan)
    firsts, pattern = None, []
    for epoch in range(8):
        x = _path(B, V, K, seed=epoch)
        got, deliv = SM.measure(x, 2, rows, 21, epoch, 0, held)
        if epoch == 0:
            # NaN in x_held: the first measurement is delivered whatever P_DROP says
            assert deliv[:3].all() and deliv[3].tolist() == [0, 1]
            firsts = got[0].copy()
        else:
            assert not deliv[0].any() and np.array_equal(got[0], firsts)   # held for ever
            assert deliv[2].all()
        assert np.isnan(got[3, 0]).all() and np.isnan(held[3, 0]).all() and deliv[3, 0] == 0
        assert np.array_equal(got[3, 1], x[3, 1, 2])               # its neighbour: untouched
        lost = deliv[1] == 0
        assert np.array_equal(got[1][~lost], x[1, :, 2][~lost])
        pattern.append(deliv[1].copy())
        assert np.array_equal(held[:3], got[:3])
    pattern = np.array(pattern)
    assert 0 < pattern[1:].sum() < pattern[1:].size               # p = 0.5: both happen
    u2 = np.array([[SM.call(21, 3, e, 6, v, 1)[2] for v in range(V)] for e in range(1, 8)])
    assert np.array_equal(pattern[1:], (u2 >= 0.5).astype(np.int32))


def test_mirror_bad_rows():
    good = np.array([0.05, 0.0, 0.1, 0.0, -0.3, 0.97, 1.0, 3.0])
    assert not SM.bad_row(good) and not SM.bad_row(SM.NOMINAL)
    for f, value in ((0, math.nan), (2, -1e-9), (4, math.inf), (6, 1.5), (6, -0.1), (7, 0.5),
                     (7, -1.0), (5, math.nan)):
        r = good.copy()
        r[f] = value
        assert SM.bad_row(r), (f, value)


def test_sense_sites_share_no_counter_with_the_other_sites():
    """Equal seeds: the c2 words of the sites 5, 6 and 7 differ from every c2 the sites 0..4
    can form ((site << 24) | (k << 8) | v with k < 65536, v < 256), so no counter, and no
    draw, is shared."""
    import obstacle_mirror as OM
    import truth_mirror as TM
    top = lambda c2: c2 >> 24                                       # noqa: E731
    old = {top(NM.counter2(s, k, v)) for s in (0, 1, 2, 3, 4) for k in (0, 65535) for v in (0, 255)}
    new = {top((s << 24) | i) for s in (SM.SITE_SENSE, SM.SITE_SENSE_DRAW, SM.SITE_SENSE_OBST)
           for i in (0, 15, 31)}
    assert old == {0, 1, 2, 3, 4} and new == {5, 6, 7}
    seed = 11
    sd = SM.Dist(4, seed)
    for f in range(SM.NP):
        sd.set(f, SM.UNIFORM, 1.0)
    xs = SM.xi(sd, 8)                                              # site 5, c0 = f, c1 = 0
    td = TM.Dist(np.ones((5, 4)), seed)
    for f in range(TM.NP):
        td.set(f, TM.UNIFORM, 1.0)
    od = OM.Dist(np.ones((7, 4)), seed)
    for f in range(OM.NP):
        od.set(f, OM.UNIFORM, 1.0)
    others = np.concatenate([TM.xi(td, 8).ravel(), OM.xi(od, 8).ravel()])
    assert not np.isin(xs.ravel(), others).any()
    # sites 6 and 7 at epoch 0 against the noise sites' first evaluations at epoch 0
    b, v, c0 = np.meshgrid(np.arange(8), np.arange(4), np.arange(4), indexing="ij")
    noise = np.concatenate([np.ravel(NM.normals(seed, c0, 0, NM.counter2(s, 0, v), b))
                            for s in (0, 1, 2)])
    for site in (SM.SITE_SENSE_DRAW, SM.SITE_SENSE_OBST):
        z0, z1, _ = SM.calls(seed, c0, 0, site, v, b)
        assert not np.isin(np.concatenate([z0.ravel(), z1.ravel()]), noise).any()
    a = SM.calls(seed, c0, 0, SM.SITE_SENSE_DRAW, v, b)[0]
    assert not np.isin(a, SM.calls(seed, c0, 0, SM.SITE_SENSE_OBST, v, b)[0]).any()


def test_mirror_sampler():
    d = SM.Dist(3, 11)
    s = SM.sample(d, 5)
    assert s.shape == (5, 3, 8) and np.array_equal(s, SM.nominal_rows(5, 3))
    d.set(SM.SIG_POS, SM.UNIFORM, 0.05, 0.0, 0.08, mean=0.05).set(SM.LAG, SM.UNIFORM, 3.0, 0.0, 5.0,
                                                                  mean=2.0)
    d.set(SM.BIAS_HEADING, SM.NORMAL, 0.02)
    s = SM.sample(d, 400)
    assert np.all(s[..., SM.LAG] == np.rint(s[..., SM.LAG]))
    assert set(np.unique(s[..., SM.LAG])) == {0.0, 1.0, 2.0, 3.0, 4.0, 5.0}
    assert s[..., SM.SIG_POS].min() >= 0.0 and s[..., SM.SIG_POS].max() == 0.08
    assert not any(SM.bad_row(r) for r in s.reshape(-1, 8))
    whole = SM.sample(d, 6)
    d2 = SM.Dist(3, 11, 3)
    d2.__dict__.update({k: v for k, v in d.__dict__.items() if k != "b_offset"})
    assert np.array_equal(whole, np.concatenate([SM.sample(d, 3), SM.sample(d2, 3)]))


# ---------------------------------------------------------------------------
# 4. scpqp.sensing on the host
# ---------------------------------------------------------------------------
def test_validate_names_the_row_and_the_field():
    good = np.broadcast_to(SE.nominal_rows(3)[None], (4, 3, 8)).copy()
    good[1, 2] = [0.05, 0.01, 0.1, 0.002, -0.02, 1.03, 0.5, 7.0]
    SE.validate(good)
    SE.validate(good, max_lag=7)
    assert np.array_equal(SE.nominal_rows(3), SM.nominal_rows(1, 3)[0])
    assert SE.is_nominal(SE.nominal_rows(3)[None]) and not SE.is_nominal(good)
    for f, name in enumerate(SE.FIELDS):
        for bad in (math.nan, math.inf, -math.inf):
            t = good.copy()
            t[2, 1, f] = bad
            with pytest.raises(ValueError, match=rf"rows\[2, 1\]: {name} is not finite"):
                SE.validate(t)
    for f in range(4):
        t = good.copy()
        t[3, 0, f] = -1e-9
        with pytest.raises(ValueError, match=rf"rows\[3, 0\]: {SE.FIELDS[f]} must be >= 0"):
            SE.validate(t)
    for value in (1.5, -0.1):
        t = good.copy()
        t[0, 2, 6] = value
        with pytest.raises(ValueError, match=r"rows\[0, 2\]: p_drop must be in \[0, 1\]"):
            SE.validate(t)
    for value, what in ((0.5, "whole number"), (-1.0, ">= 0")):
        t = good.copy()
        t[1, 1, 7] = value
        with pytest.raises(ValueError, match=rf"rows\[1, 1\]: lag must be .*{what}"):
            SE.validate(t)
    with pytest.raises(ValueError, match=r"rows\[1, 2\]: lag must be <= 6 ticks"):
        SE.validate(good, max_lag=6)
    with pytest.raises(ValueError, match=r"\[B, nVeh, 8\]"):
        SE.validate(good[..., :7])
    with pytest.raises(ValueError, match=r"\[B, nVeh, 8\]"):
        SE.validate(good[0])
    # every row validate passes is one the mirror does not call bad, and the other way round
    for row in (good[1, 2], SM.NOMINAL):
        assert not SM.bad_row(row)
    os_ = np.zeros((2, 3, 3))
    SE.validate_obstacle_sensing(os_)
    os_[1, 2, 1] = -0.1
    with pytest.raises(ValueError, match=r"obstacle_sensing\[1, 2\]: sig_heading must be >= 0"):
        SE.validate_obstacle_sensing(os_)
    os_[1, 2, 1] = math.nan
    with pytest.raises(ValueError, match=r"obstacle_sensing\[1, 2\]: sig_heading is not finite"):
        SE.validate_obstacle_sensing(os_)
    with pytest.raises(ValueError, match=r"\[B, nObst, 3\]"):
        SE.validate_obstacle_sensing(np.zeros((2, 3, 4)))


def test_sense_dist_object():
    d = SE.SenseDist(3, seed=9, b_offset=4)
    c = d.c_struct()
    assert (c.n_veh, c.seed, c.b_offset) == (3, 9, 4)
    assert [c.field[f].kind for f in range(8)] == [F] * 8
    assert [c.mean[f][1] for f in range(8)] == list(SE.NOMINAL_ROW)
    d.normal("sig_pos", 0.01, 0.0, 0.1, mean=0.05).uniform("lag", 2.0, 0.0, 5.0, mean=2.0)
    d.fixed("p_drop", [0.0, 0.1, 1.0]).normal("bias_heading", 0.02)
    c = d.c_struct()
    assert (c.field[0].kind, c.field[0].spread, c.field[0].lo, c.field[0].hi) == (N, 0.01, 0.0, 0.1)
    assert [c.mean[0][v] for v in range(3)] == [0.05] * 3
    assert (c.field[7].kind, c.field[7].spread, c.field[7].lo, c.field[7].hi) == (U, 2.0, 0.0, 5.0)
    assert c.field[6].kind == F and [c.mean[6][v] for v in range(3)] == [0.0, 0.1, 1.0]
    assert (c.field[4].kind, c.field[4].lo, c.field[4].hi) == (N, -math.inf, math.inf)
    e = d.with_offset(100)
    assert (e.b_offset, d.b_offset, e.seed) == (100, 4, 9) and e.kind == d.kind
    e.fixed("sig_pos", 0.0)
    assert d.mean[0, 0] == 0.05                            # with_offset copies
    sc = type("Sc", (), {"nVeh": 2})()
    assert SE.SenseDist(sc, seed=1).n_veh == 2             # a scenario supplies nVeh
    for bad, what in ((lambda: d.uniform("mass", 0.1), "unknown sensing field"),
                      (lambda: d.uniform("sig_pos", -0.1, 0.0), "sig_pos: spread"),
                      (lambda: d.normal("sig_speed", 0.1, 1.0, 0.5), "sig_speed: lo must be <= hi"),
                      (lambda: d.uniform("sig_steer", 0.5), "sig_steer: the smallest value"),
                      (lambda: d.normal("lag", 0.5, -0.1, 3.0), "lag: the smallest value"),
                      (lambda: d.uniform("p_drop", 0.5, 0.0, 1.5), r"p_drop: .*\[0, 1\]"),
                      (lambda: d.fixed("p_drop", 1.5), r"p_drop: .*\[0, 1\]"),
                      (lambda: d.fixed("sig_heading", -1.0), "sig_heading: the smallest value"),
                      (lambda: d.fixed("scale_speed", math.nan), "scale_speed: a fixed value"),
                      (lambda: d.uniform(8, 0.1), "out of range"),
                      (lambda: SE.SenseDist(3, seed=-1), "seed"),
                      (lambda: SE.SenseDist(3, seed=1, b_offset=2 ** 32), "b_offset"),
                      (lambda: SE.SenseDist(0, seed=1), "vehicles")):
        with pytest.raises(ValueError, match=what):
            bad()


def test_from_table_gathers_rows():
    import torch
    rows = np.arange(3 * 2 * 8, dtype=float).reshape(3, 2, 8)
    t = SE.from_table(rows, [2, 0, 0, 1], device="cpu")
    assert t.dtype == torch.float64 and tuple(t.shape) == (4, 2, 8) and t.is_contiguous()
    assert np.array_equal(t.numpy(), rows[[2, 0, 0, 1]])
    with pytest.raises(ValueError):
        SE.from_table(rows, [3], device="cpu")
    with pytest.raises(ValueError):
        SE.from_table(rows[..., :7], [0], device="cpu")


def test_the_wrappers_refuse_host_tensors():
    import torch
    rows = torch.zeros((2, 3, 8), dtype=torch.float64)
    x = torch.zeros((2, 3, 5, 6), dtype=torch.float64)
    held = torch.zeros((2, 3, 6), dtype=torch.float64)
    with pytest.raises(ValueError, match="on the GPU"):
        SE.measure(x, 0, rows, 1, 0, 0, held)
    with pytest.raises(ValueError, match="on the GPU"):
        SE.predict_sensed(torch.zeros((2, 3, 7), dtype=torch.float64),
                          torch.zeros((2, 3, 3), dtype=torch.float64), 1, 0, 0, 0.0, 0.43, 0.4, 10)
