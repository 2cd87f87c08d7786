"""Interacting-multiple-model obstacle tracker, the parts that need no GPU: the C-ABI of
include/scpqp_imm.h (exports, constants by a gcc probe of the header, argument validation
without touching a device), the CPU mirror's properties (tests/imm_mirror.py), the derivation of
the tolerances the GPU tests use, and scpqp.imm's host side.

Bounds.
  Probabilities: in [0, 1], summing to 1 within 1e-14 (M <= 4 quotients of one sum: 4 ulp);
  unchanged within 1e-13 by a constant added to every l_j (the shift changes l - max l by the
  rounding of |l| <= 100: 100 ulp = 1.4e-14, which exp turns into a relative error of the same
  size); within 1e-12 of exp(-nis / 2) / sqrt(det S) in 80-bit on a well-scaled case.
  The tolerance of the device test: imm_cases.TOL, 16 times the largest figure between the
  float64 and the 80-bit mirror, rounded up to a power of two.  Measured: 5.87e-14 (M = 1),
  9.87e-13 (M = 2), 9.38e-13 (M = 3), 2.66e-13 (M = 4), each at (12, 22, 10) and, from M = 2
  on, in a probability of the last step.
  The reductions to the single filter: bitwise for one mode and for Pi = I with mu0 = (1, 0),
  1.03e-13 for three identical modes; imm_cases.RED_TOL is 16 times that, rounded up.
  Permuting the modes: twice the float64 against 80-bit figure of the shape at M = 3 (the sums
  over the modes run in another order; both runs are about that far from the exact result):
  1.88e-12 at (12, 22, 10), 6.0e-14 at (2, 3, 5).  Measured: 6.10e-13 and 1.40e-14.
  Mode response: see imm_cases.RESP_K.  Measured on the mirror, batch means of (straight, arc,
  brake): (0.66, 0.29, 0.045) at the last cruising call, (0.0000, 0.0001, 0.9999) at the first
  braking call.
  Consistency: five standard deviations of the mean of 18000 chi-square(4) variables, 0.105."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import imm_cases as IC
import imm_mirror as IM
import manoeuvre_mirror as MNM
import tracker_accel_cases as TC
import tracker_accel_mirror as AM
from scpqp import _lib as LB
from scpqp import imm as IMM
from scpqp.build import LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scpqp_imm.h")
E_ARG, E_SIZE = -1, -4
LD = np.longdouble


def header_functions():
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"^int\s+(scpqp_\w+)\(", txt, re.M)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        pytest.fail("libscpqp.so not built: run __graft_entry__.build()")
    return LB.load()


# ---------------------------------------------------------------------------
# 1. boundary
# ---------------------------------------------------------------------------
def test_header_declares_the_boundary():
    assert header_functions() == sorted(LB.IMM_EXPORTS) == ["scpqp_obstacles_track_imm"]
    others = (set(LB.EXPORTS) | set(LB.NOISE_EXPORTS) | set(LB.METRICS_EXPORTS)
              | set(LB.VARIANT_EXPORTS) | set(LB.TRUTH_EXPORTS) | set(LB.OBSTACLE_EXPORTS)
              | set(LB.SENSE_EXPORTS) | set(LB.EST_EXPORTS) | set(LB.TRK_EXPORTS)
              | set(LB.MAN_EXPORTS) | set(LB.TRKA_EXPORTS))
    assert not set(LB.IMM_EXPORTS) & others
    txt = open(HEADER).read()
    for word in ("mu0", "Pi[i][j]", "not wrapped", "skipped, not multiplied", "Off lane", "Bad lane",
                 "no new Philox site", "not a rate", "lies\n * between them", "footprint",
                 "no sampler", "whatever the call's length", "delta_ij"):
        assert word in txt, word


def test_library_exports_the_symbol(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\sT\s(scpqp_\w+)", out))
    assert set(header_functions()) <= exported
    for name in LB.IMM_EXPORTS:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None


PROBE = r"""
#include <stdio.h>
#include "scpqp_imm.h"
int main(void) {
  printf("modes %d\n", SCPQP_IMM_MAX_MODES);
  printf("sumtol %.17g\n", SCPQP_IMM_SUM_TOL);
  printf("ns %d\n", SCPQP_TRKA_NS);
  printf("np %d\n", SCPQP_TRKA_NP);
  return 0;
}
"""


def test_ctypes_layout_matches_header(tmp_path, lib):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", f"-I{os.path.dirname(HEADER)}", str(src), "-o", str(exe)],
                   check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["modes"]) == LB.IMM_MAX_MODES == IM.MAX_MODES == IMM.MAX_MODES == 4
    assert float(got["sumtol"]) == LB.IMM_SUM_TOL == IM.SUM_TOL == IMM.SUM_TOL == 1e-12
    assert int(got["ns"]) == IMM.NS == IM.NS == 6 and int(got["np"]) == IMM.NP == IM.NP == 14
    # the declared argument list: that of scpqp_obstacles_track_accel with n_modes after hp, sw
    # after trk, and mu, x_hat after cov
    proto = re.search(r"int scpqp_obstacles_track_imm\((.*?)\);", open(HEADER).read(), re.S).group(1)
    args = [a.strip() for a in proto.replace("\n", " ").split(",")]
    names = [a.split()[-1].lstrip("*") for a in args]
    assert names == ["B", "n_obst", "hp", "n_modes", "rows", "osense", "st", "trk", "sw", "t_meas",
                     "t_since", "lead", "dt", "x_imm", "cov", "mu", "x_hat", "z_out", "nis",
                     "obst_out", "stream"]
    assert len(args) == len(lib.scpqp_obstacles_track_imm.argtypes) == 21
    for a, t in zip(args, lib.scpqp_obstacles_track_imm.argtypes):
        if a.startswith("double "):
            assert t is C.c_double, a
        elif a.startswith("int32_t "):
            assert t is C.c_int32, a
        else:
            assert "*" in a and t in (C.c_void_p, C.POINTER(LB.SenseStream)), a


def test_argument_validation_without_gpu(lib):
    buf = (C.c_double * 256)()
    D = C.cast(buf, C.c_void_p)
    ST = LB.SenseStream(seed=1, epoch=0, b_offset=0)

    def err():
        return lib.scpqp_last_error()

    def track(B=0, n_obst=3, hp=5, M=3, rows=None, osense=None, st=None, trk=None, sw=None,
              t_meas=0.0, t_since=0.4, lead=0.1, dt=0.4, x=None, cov=None, mu=None, xh=None, z=None,
              nis=None, out=None):
        return lib.scpqp_obstacles_track_imm(B, n_obst, hp, M, rows, osense,
                                             None if st is None else C.byref(st), trk, sw, t_meas,
                                             t_since, lead, dt, x, cov, mu, xh, z, nis, out, None)

    assert track() == 0                                     # B = 0: a no-op, NULL arrays
    assert track(t_since=0.0) == 0
    assert track(B=-1) == E_ARG and b"batch" in err()
    for n in (0, -1, LB.MAX_OBST + 1):
        assert track(n_obst=n) == E_ARG and b"n_obst" in err()
    for h in (0, -1, LB.MAX_HP + 1):
        assert track(hp=h) == E_ARG and b"hp" in err()
    for m in (0, -1, 5):
        assert track(M=m) == E_ARG and b"n_modes" in err()
    for m in (1, 2, 3, 4):
        assert track(M=m) == 0
    for t in (-1e-9, -0.4, math.nan, math.inf):
        assert track(t_since=t) == E_ARG and b"t_since" in err()
    for kw in (dict(t_meas=math.nan), dict(lead=math.inf), dict(dt=math.nan)):
        assert track(**kw) == E_ARG and b"finite" in err()
    full = dict(rows=D, trk=D, sw=D, x=D, cov=D, mu=D, xh=D, out=D)
    for missing, word in (("rows", b"rows"), ("trk", b"trk"), ("sw", b"sw"), ("x", b"x_imm"),
                          ("cov", b"cov"), ("mu", b"mu"), ("xh", b"x_hat"), ("out", b"output")):
        kw = dict(full)
        kw[missing] = None
        assert track(B=3, **kw) == E_ARG and word in err(), missing
    assert track(B=3, osense=D, **full) == E_ARG and b"stream" in err()
    # sizes before the pointers: nothing is launched for a size error.  2^24 * 4 * 36 > 2^31 - 1
    assert track(B=1 << 24, n_obst=1, M=4, **full) == E_SIZE and b"36" in err()
    assert track(B=1 << 24, n_obst=1, M=4) == E_SIZE
    assert track(B=1 << 22, n_obst=4, hp=64, M=1, osense=D, st=ST, **full) == E_SIZE and b"hp" in err()


# ---------------------------------------------------------------------------
# 2. scpqp.imm's host side
# ---------------------------------------------------------------------------
def test_bank_builds_the_named_modes_and_validate_refuses_bad_banks():
    osense = np.broadcast_to(TC.CONS_SIGMA, (3, 2, 3)).copy()
    trk, sw = IMM.bank(osense, device="cpu")
    trk, sw = trk.numpy(), sw.numpy()
    assert trk.shape == (3, 2, 3, 14) and sw.shape == (3, 2, 4, 3) and IMM.MODES == (
        "straight", "arc", "brake")
    s, a, b = (trk[0, 0, j] for j in range(3))
    assert s[AM.W_HOLD] == 0 and s[AM.A_HOLD] == 0
    assert a[AM.W_HOLD] > 100 and a[AM.A_HOLD] == 0
    assert b[AM.W_HOLD] > 100 and b[AM.A_HOLD] > 100 and b[AM.Q_ACCEL] > a[AM.Q_ACCEL]
    assert (trk[..., :3] == TC.CONS_SIGMA).all()
    assert (sw[..., 0, :] == 1 / 3).all() and (sw[0, 0, 1:] == np.where(np.eye(3), 0.9, (1 - 0.9) / 2)).all()
    t4, s4 = IMM.bank(osense, modes=("brake", "straight", "arc", "brake"), stay=0.7, device="cpu")
    assert t4.shape == (3, 2, 4, 14) and np.allclose(s4.numpy()[1, 1, 1], [0.7, 0.1, 0.1, 0.1])
    t1, s1 = IMM.bank(osense, modes=("arc",), device="cpu")
    assert (s1.numpy() == 1).all()
    for bad in (dict(modes=()), dict(modes=("arc",) * 5), dict(modes=("glide",)), dict(stay=1.5)):
        with pytest.raises(ValueError):
            IMM.bank(osense, device="cpu", **bad)
    IMM.validate(trk, sw)
    off_t, off_s = np.zeros_like(trk), np.zeros_like(sw)
    IMM.validate(off_t, off_s)                              # the sw of an off lane is not read
    assert IMM.is_off(off_t) and not IMM.is_off(trk)
    for lane, idx, val, word in (((1, 0), ("trk", (2, 7)), -1.0, "mode 2.*q_accel"),
                                 ((2, 1), ("trk", (1,)), 0.0, r"trk\[2, 1\]: off and non-off"),
                                 ((0, 1), ("sw", (2, 0)), -0.05, r"sw\[0, 1, 2, 0\]"),
                                 ((0, 1), ("sw", (0, 2)), math.nan, r"sw\[0, 1, 0, 2\]"),
                                 ((1, 1), ("sw", (0, 0)), 1 / 3 + 1e-6, "mu0 does not sum"),
                                 ((1, 1), ("sw", (3, 0)), 0.05 + 1e-6, "row 2 of Pi")):
        t, s_ = trk.copy(), sw.copy()
        (t if idx[0] == "trk" else s_)[lane + idx[1]] = val
        with pytest.raises(ValueError, match=word):
            IMM.validate(t, s_)
        assert IM.is_bad_lane(t[lane], s_[lane])            # the mirror's rule agrees
    with pytest.raises(ValueError):
        IMM.validate(trk, sw[:, :, :3])
    with pytest.raises(ValueError):
        IMM.validate(trk[:, :, 0], sw)


def test_the_case_table_holds_every_kind_of_lane():
    for M in IC.MODES:
        k = IC.kinds(12, 22, M)
        assert k["off"] == 38 and k["identity"] >= 20 and k["bad_row"] == 3
        assert k["sw_negative"] == k["sw_nan"] == k["sw_sum"] == 1
        if M > 1:
            assert k["dead"] >= 20 and k["mu0_zero"] >= 20 and k["mixed"] == 1
    assert [since for _, since in IC.times()].count(0.0) == 2 and IC.times()[4][1] == 0.0
    # the sum that is off is off by 1e-6, not by rounding
    _, _, _, _, sw = IC.case(12, 22, 3)
    assert abs(sw[divmod(212, 22)][3].sum() - 1.0) > 5e-7


# ---------------------------------------------------------------------------
# 3. probabilities
# ---------------------------------------------------------------------------
def test_probabilities_are_a_distribution_and_ignore_a_common_shift():
    rng = np.random.default_rng(3)
    for _ in range(300):
        M = int(rng.integers(1, 5))
        c = rng.uniform(0.0, 1.0, M)
        c[rng.uniform(size=M) < 0.25] = 0.0
        if not c.any():
            c[0] = 0.3
        c /= c.sum()
        l = rng.uniform(-60.0, 40.0, M)
        mu = IM.probabilities(c, l)
        assert ((mu >= 0) & (mu <= 1)).all() and abs(mu.sum() - 1.0) <= 1e-14
        assert (mu[c == 0] == 0).all() and (mu[c > 0] > 0).all()
        shifted = IM.probabilities(c, l + rng.uniform(-50.0, 50.0))
        assert np.abs(shifted - mu).max() <= 1e-13
    # far apart: no overflow, the better mode takes everything
    mu = IM.probabilities(np.array([0.5, 0.5]), np.array([-1e4, 700.0]))
    assert mu[0] == 0.0 and mu[1] == 1.0
    assert np.isnan(IM.probabilities(np.zeros(3), np.zeros(3))).all()


def test_the_mirror_matches_the_plain_gaussian_form_in_80_bit():
    """One lane, three modes, one update from a mixed start: mu against
    c_j exp(-nis_j / 2) / sqrt(det S_j), normalised, in 80-bit."""
    rows, man, osense = IC.response_inputs(B=1, n_obst=1)
    trk, sw, names = IC.response_bank(osense)
    x, cov, mu = IM.alloc(1, 1, 3)
    for s in range(3):
        before = (x.copy(), cov.copy(), mu.copy())
        snap = MNM.state(rows, man, s * IC.RESP_T)
        _, _, z, nis = IM.step(snap, osense, IC.RESP_SEED, s, 0, trk, sw, 0.0,
                               0.0 if s == 0 else IC.RESP_T, IC.RESP_LEAD, IC.RESP_DT, IC.RESP_HP, x,
                               cov, mu)
    xb, Pb, mub = (np.asarray(a[0, 0], dtype=LD) for a in before)
    c, x0, P0 = IM.mix(xb, Pb, mub, np.asarray(sw[0, 0, 1:], dtype=LD), IM.F80)
    like = np.empty(3, dtype=LD)
    for j in range(3):
        xp, Pp = AM.predict(x0[j], P0[j], LD(IC.RESP_T), AM.q_diag(trk[0, 0, j], IM.F80), IM.F80)
        S = Pp[:4, :4] + np.diag(AM.r_diag(trk[0, 0, j], IM.F80))
        y = np.asarray(z[0, 0], dtype=LD) - xp[:4]
        Sf = np.asarray(S, float)
        det = LD(np.linalg.det(Sf))
        d = y @ np.asarray(np.linalg.solve(Sf, np.asarray(y, float)), dtype=LD)
        assert abs(float(d) - float(nis[0, 0, j])) <= 1e-10 * max(1.0, float(d))
        like[j] = c[j] * np.exp(-d / 2) / np.sqrt(det)
    want = like / like.sum()
    assert np.abs(np.asarray(mu[0, 0], dtype=LD) - want).max() <= 1e-12
    assert 0.05 < float(mu[0, 0].min()) and float(mu[0, 0].max()) < 0.9    # a well-scaled case


# ---------------------------------------------------------------------------
# 4. reductions to the single filter, permutation
# ---------------------------------------------------------------------------
def _run_reduction(kind, B, nO, hp):
    rows, man, osense, trk14, trk, sw = IC.reduction_case(B, nO, kind)
    M = trk.shape[2]
    x, cov, mu = IM.alloc(B, nO, M)
    x1, c1 = AM.alloc(B, nO)
    worst = 0.0
    for s, (t, since) in enumerate(IC.times()):
        snap = MNM.state(rows, man, t)
        ob, xh, z, nis = IM.step(snap, osense, IC.SEED, s, 3, trk, sw, 0.0, since, IC.LEAD, IC.DT,
                                 hp, x, cov, mu)
        ob1, z1, nis1 = AM.step(snap, osense, IC.SEED, s, 3, trk14, 0.0, since, IC.LEAD, IC.DT, hp,
                                x1, c1)
        assert np.array_equal(z, z1, equal_nan=True)
        worst = max(worst, IC.reduction_ratio((xh, cov, nis, ob), (x1, c1, nis1, ob1)))
        if kind == "identity":
            live = ~np.isnan(mu[..., 0]) & (trk != 0).any(axis=(2, 3))
            assert (mu[live] == [1.0, 0.0]).all()
    return worst


@pytest.mark.parametrize("kind", IC.REDUCTIONS)
def test_reductions_reproduce_the_single_filter(kind):
    worst = _run_reduction(kind, 12, 22, 10)
    print(f"{kind}: bank mirror against tracker_accel_mirror.step {worst:.3e} "
          f"(recorded {IC.REDUCTION_MEASURED[kind]:.3e}, RED_TOL {IC.RED_TOL:.3e})")
    if kind != "identical":
        assert worst == 0.0
    # the recorded figure is the measured one, and RED_TOL is 16 times the largest, rounded up
    assert worst <= 1.05 * IC.REDUCTION_MEASURED[kind] and (
        worst >= 0.95 * IC.REDUCTION_MEASURED[kind])
    assert IC.RED_TOL == IC.pow2_ceil(16 * max(IC.REDUCTION_MEASURED.values()))


@pytest.mark.parametrize("B,nO,hp", list(IC.PERM_SHAPES))
def test_permuting_the_modes_permutes_the_modes_and_keeps_the_combination(B, nO, hp):
    M, worst = 3, 0.0
    rows, man, osense, trk, sw = IC.case(B, nO, M)
    perm = [2, 0, 1]
    trk_p = trk[:, :, perm]
    sw_p = np.concatenate([sw[:, :, :1][..., perm], sw[:, :, 1:][:, :, perm][..., perm]], axis=2)
    a, b = IM.alloc(B, nO, M), IM.alloc(B, nO, M)
    for s, (t, since) in enumerate(IC.times()):
        snap = MNM.state(rows, man, t)
        oa = IM.step(snap, osense, IC.SEED, s, 0, trk, sw, 0.0, since, IC.LEAD, IC.DT, hp, *a)
        ob = IM.step(snap, osense, IC.SEED, s, 0, trk_p, sw_p, 0.0, since, IC.LEAD, IC.DT, hp, *b)
        got = (b[0], b[1], b[2], ob[1], ob[3], ob[0], ob[2])
        want = (a[0][:, :, perm], a[1][:, :, perm], a[2][:, :, perm], oa[1], oa[3][:, :, perm],
                oa[0], oa[2])
        worst = max(worst, IC.ratio(got, want))
    print(f"({B}, {nO}, {hp}): permuted against unpermuted {worst:.3e} "
          f"(bound {IC.PERM_SHAPES[(B, nO, hp)]:.3e})")
    assert worst <= IC.PERM_SHAPES[(B, nO, hp)]


# ---------------------------------------------------------------------------
# 5. the tolerance of the device test
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("M", IC.MODES)
def test_tolerance_is_sixteen_times_the_rounding_the_definition_amplifies(M):
    worst = {}
    for B, nO, hp in IC.SHAPES:
        a = IC.run_mirror(B, nO, hp, M, IM.F64)
        b = IC.run_mirror(B, nO, hp, M, IM.F80)
        worst[(B, nO, hp)] = max(IC.ratio(p, q) for p, q in zip(a, b))
        print(f"M = {M} ({B}, {nO}, {hp}): float64 against 80-bit {worst[(B, nO, hp)]:.3e}")
        # the conditioning limit of tests/test_gpu_tracker.py
        assert max(np.nanmax(np.abs(p[6][..., :2])) for p in a) <= 16.0
    small = worst[(2, 3, 5)]
    assert 0.95 * IC.MIRROR_ROUNDING_SMALL[M] <= small <= 1.05 * IC.MIRROR_ROUNDING_SMALL[M]
    top = max(worst.values())
    assert 0.95 * IC.MIRROR_ROUNDING_BY_M[M] <= top <= 1.05 * IC.MIRROR_ROUNDING_BY_M[M]
    assert IC.MIRROR_ROUNDING == max(IC.MIRROR_ROUNDING_BY_M.values())
    assert IC.TOL == IC.pow2_ceil(16 * IC.MIRROR_ROUNDING)


# ---------------------------------------------------------------------------
# 6. mode response and consistency
# ---------------------------------------------------------------------------
def test_the_bank_believes_straight_while_cruising_and_brake_after_the_onset():
    rows, man, osense = IC.response_inputs()
    trk, sw, names = IC.response_bank(osense)
    x, cov, mu = IM.alloc(IC.RESP_B, IC.RESP_NO, len(names))
    means = []
    for s in range(IC.RESP_CRUISE + IC.RESP_BRAKE):
        snap = MNM.state(rows, man, s * IC.RESP_T)
        # the braking sets in after the last cruising call
        assert (snap[..., 3] == rows[..., 3]).all() == (s < IC.RESP_CRUISE)
        IM.step(snap, osense, IC.RESP_SEED, s, 0, trk, sw, 0.0, 0.0 if s == 0 else IC.RESP_T,
                IC.RESP_LEAD, IC.RESP_DT, IC.RESP_HP, x, cov, mu)
        means.append(mu.mean(axis=(0, 1)))
        print(f"call {s}: mean mu {dict(zip(names, np.round(means[-1], 4)))}")
    means = np.array(means)
    cruising, first = IC.response_verdict(means, names)
    assert cruising and first is not None and first <= IC.RESP_K
    # the margins imm_cases.py states
    i, j, last = names.index("straight"), names.index("brake"), IC.RESP_CRUISE - 1
    assert means[last, i] - means[last, j] > 0.3 and means[last + 1, j] - means[last + 1, i] > 0.9


def test_innovations_of_the_matched_mode_are_consistent():
    rows, man, osense, trk14, _ = TC.consistency_inputs()
    assert TC.no_lane_stops(rows, man)
    trk, sw = IC.consistency_bank(trk14)
    B, nO = rows.shape[:2]
    x, cov, mu = IM.alloc(B, nO, 2)
    every = []
    for s in range(TC.CONS_STEPS + 1):
        snap = MNM.state(rows, man, s * TC.CONS_T)
        _, _, _, nis = IM.step(snap, osense, TC.CONS_SEED, s, 0, trk, sw, 0.0,
                               0.0 if s == 0 else TC.CONS_T, TC.CONS_LEAD, TC.CONS_DT, TC.CONS_HP, x,
                               cov, mu)
        if s:
            every.append(nis[..., 0].copy())
    every = np.array(every, float)
    assert np.isfinite(every).all() and every.size == 18000
    assert (mu == [1.0, 0.0]).all()
    mean, bound = float(every.mean()), 5.0 * math.sqrt(8.0 / every.size)
    print(f"mean NIS of the matched mode {mean:.3f} (|mean - 4| <= {bound:.3f})")
    assert abs(mean - 4.0) <= bound
