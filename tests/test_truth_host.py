"""Plant truth, the parts that need no GPU: the C-ABI of include/scpqp_truth.h (exports,
ctypes layout by a gcc probe of the header, argument validation without touching a
device), the CPU mirror (tests/truth_mirror.py) pinned by closed forms, the mirror's
sampler, and scpqp.truth's host side."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import truth_mirror as TM
from oracle import scp_reference as R
from scpqp import _lib as LB
from scpqp import truth as TR
from scpqp.build import LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scpqp_truth.h")
E_ARG, E_SIZE = -1, -4


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
def test_truth_header_declares_the_boundary():
    assert header_functions() == sorted(LB.TRUTH_EXPORTS)
    others = (set(LB.EXPORTS) | set(LB.NOISE_EXPORTS) | set(LB.METRICS_EXPORTS)
              | set(LB.VARIANT_EXPORTS))
    assert not set(LB.TRUTH_EXPORTS) & others


def test_library_exports_every_truth_symbol(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\sT\s(scpqp_\w+)", out))
    assert set(header_functions()) <= exported
    for name in LB.TRUTH_EXPORTS:
        assert hasattr(lib, name)


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "scpqp_truth.h"
int main(void) {
  printf("size %zu\n", sizeof(scpqp_truth_dist));
  printf("n_veh %zu\n", offsetof(scpqp_truth_dist, n_veh));
  printf("mean %zu\n", offsetof(scpqp_truth_dist, mean));
  printf("field %zu\n", offsetof(scpqp_truth_dist, field));
  printf("seed %zu\n", offsetof(scpqp_truth_dist, seed));
  printf("b_offset %zu\n", offsetof(scpqp_truth_dist, b_offset));
  printf("fsize %zu\n", sizeof(scpqp_truth_field));
  printf("kind %zu\n", offsetof(scpqp_truth_field, kind));
  printf("spread %zu\n", offsetof(scpqp_truth_field, spread));
  printf("lo %zu\n", offsetof(scpqp_truth_field, lo));
  printf("hi %zu\n", offsetof(scpqp_truth_field, hi));
  printf("np %d\n", SCPQP_TRUTH_NP);
  printf("idx %d%d%d%d%d\n", SCPQP_TRUTH_LF, SCPQP_TRUTH_LR, SCPQP_TRUTH_TAU, SCPQP_TRUTH_GAIN,
         SCPQP_TRUTH_BIAS);
  printf("kinds %d%d%d\n", SCPQP_TRUTH_FIXED, SCPQP_TRUTH_UNIFORM, SCPQP_TRUTH_NORMAL);
  printf("site %d\n", SCPQP_NOISE_SITE_TRUTH);
  printf("maxveh %d\n", SCPQP_MAX_VEH);
  return 0;
}
"""


def test_truth_ctypes_layout_matches_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", f"-I{os.path.dirname(HEADER)}", str(src), "-o", str(exe)],
                   check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(LB.TruthDist)
    for f in ("n_veh", "mean", "field", "seed", "b_offset"):
        assert int(got[f]) == getattr(LB.TruthDist, f).offset, f
    assert int(got["fsize"]) == C.sizeof(LB.TruthField)
    for f in ("kind", "spread", "lo", "hi"):
        assert int(got[f]) == getattr(LB.TruthField, f).offset, f
    assert int(got["np"]) == LB.TRUTH_NP == TM.NP == 5
    assert got["idx"] == "01234" and got["kinds"] == "012"
    assert (LB.TRUTH_LF, LB.TRUTH_LR, LB.TRUTH_TAU, LB.TRUTH_GAIN, LB.TRUTH_BIAS) == (0, 1, 2, 3, 4)
    assert int(got["site"]) == LB.NOISE_SITE_TRUTH == TM.SITE_TRUTH == 3
    assert LB.NOISE_SITE_TRUTH not in (LB.NOISE_SITE_DELAY, LB.NOISE_SITE_PLANT,
                                       LB.NOISE_SITE_LINEARIZE)
    assert int(got["maxveh"]) == LB.MAX_VEH


# ---------------------------------------------------------------------------
# 2. argument validation without a GPU
# ---------------------------------------------------------------------------
def _pp(n=2):
    pp = LB.PlantParams(n_veh=n)
    for v in range(max(n, 0)):
        pp.lf[v] = pp.lr[v] = 0.34
    return pp


def test_plant_step_truth_argument_validation_without_gpu(lib):
    pp = _pp()
    nz = LB.Noise(seed=1, sigma=3e-6, epoch=0, b_offset=0)
    P, N = C.byref(pp), C.byref(nz)
    dummy = (C.c_double * 64)()
    D = C.cast(dummy, C.c_void_p)

    def plant(p=P, B=1, n_ticks=40, tick=0.01, truth=None, noise=None, n=None, arr=None,
              h_max=2.5e-3):
        return lib.scpqp_plant_step_truth(p, B, n_ticks, tick, arr, arr, truth, noise, n, arr,
                                          h_max, None)

    def err():
        return lib.scpqp_last_error()

    assert plant(p=None) == E_ARG and b"null" in err()
    for n in (0, 17):
        assert plant(p=C.byref(LB.PlantParams(n_veh=n))) == E_ARG and b"n_veh" in err()
    # p supplies n_veh only: its own geometry is not looked at
    assert plant(p=C.byref(LB.PlantParams(n_veh=2)), B=0) == 0
    # both noise sources at once
    assert plant(noise=D, n=N) == E_ARG and b"not both" in err()
    assert plant(B=0, noise=D, n=N) == E_ARG
    # the noise parameters, when given
    for s in (-1e-6, float("inf"), float("nan")):
        assert plant(n=C.byref(LB.Noise(seed=1, sigma=s))) == E_ARG and b"sigma" in err()
    # sizes, as scpqp_plant_step_noisy
    assert plant(B=-1) == E_ARG
    assert plant(n_ticks=-1) == E_ARG
    assert plant(tick=0.0) == E_ARG and b"tick" in err()
    assert plant(h_max=0.0) == E_ARG
    assert plant(n_ticks=65536, n=N) == E_SIZE and b"65536" in err()
    assert plant(B=0, n_ticks=65536, n=N) == E_SIZE
    assert plant(B=0, n_ticks=65536) == 0                 # the 16-bit tick field is the seeded one's
    # B = 0 is a no-op with NULL arrays, truth included
    assert plant(B=0) == 0
    assert plant(B=0, n=N) == 0
    # with work: truth must be non-NULL, then the other arrays
    assert plant(B=3, arr=D) == E_ARG and b"truth" in err()
    assert plant(B=3, truth=D) == E_ARG and b"null array" in err()
    assert plant(B=1 << 20, n_ticks=1 << 10, truth=D, arr=D) == E_SIZE and b"too large" in err()


def _dist(n_veh=2):
    d = LB.TruthDist()
    d.n_veh = n_veh
    for v in range(LB.MAX_VEH):
        d.mean[LB.TRUTH_LF][v] = d.mean[LB.TRUTH_LR][v] = 0.34
        d.mean[LB.TRUTH_TAU][v] = 0.1
        d.mean[LB.TRUTH_GAIN][v] = 1.0
    d.seed = 5
    return d


def _field(d, f, kind, spread=0.0, lo=-math.inf, hi=math.inf):
    d.field[f].kind, d.field[f].spread, d.field[f].lo, d.field[f].hi = kind, spread, lo, hi
    return d


def test_truth_sample_and_fill_argument_validation_without_gpu(lib):
    dummy = (C.c_double * 64)()
    D = C.cast(dummy, C.c_void_p)

    def sample(d, B=0, out=None):
        return lib.scpqp_truth_sample(None if d is None else C.byref(d), B, out, None)

    def err():
        return lib.scpqp_last_error()

    assert sample(None) == E_ARG and b"null" in err()
    assert sample(_dist()) == 0                           # all FIXED at nominal, B = 0, NULL array
    for n in (0, -1, 17):
        assert sample(_dist(n)) == E_ARG and b"n_veh" in err()
    for f, name in enumerate(LB.TRUTH_FIELDS):
        nm = name.encode()
        for kind in (-1, 3):
            assert sample(_field(_dist(), f, kind)) == E_ARG and nm in err() and b"kind" in err()
        for kind in (LB.TRUTH_UNIFORM, LB.TRUTH_NORMAL):
            for s in (-1e-3, float("inf"), float("nan")):
                assert sample(_field(_dist(), f, kind, s, 0.01, 1.0)) == E_ARG
                assert nm in err() and b"spread" in err()
            assert sample(_field(_dist(), f, kind, 0.01, 1.0, 0.5)) == E_ARG
            assert nm in err() and b"lo" in err()
            assert sample(_field(_dist(), f, kind, 0.01, float("nan"), 0.5)) == E_ARG
            assert sample(_field(_dist(), f, kind, 0.01, 0.05, 1.0)) == 0
        # a FIXED field ignores spread, lo and hi
        assert sample(_field(_dist(), f, LB.TRUTH_FIXED, -1.0, 2.0, 1.0)) == 0
    # the smallest row the sampler can emit must be one the plant integrates
    U = LB.TRUTH_UNIFORM
    assert sample(_field(_dist(), LB.TRUTH_LF, U, 0.1, -0.34, 1.0)) == E_ARG and b"lf" in err()
    assert sample(_field(_dist(), LB.TRUTH_LF, U, 0.1, -0.33, 1.0)) == 0
    assert sample(_field(_dist(), LB.TRUTH_LR, U, 0.1)) == E_ARG          # lo = -inf
    assert sample(_field(_dist(), LB.TRUTH_TAU, U, 0.01, 0.0, 1.0)) == E_ARG and b"tau" in err()
    assert sample(_field(_dist(), LB.TRUTH_TAU, LB.TRUTH_NORMAL, 0.01)) == E_ARG and b"tau" in err()
    assert sample(_field(_dist(), LB.TRUTH_TAU, U, 0.01, 0.02, 1.0)) == 0
    d = _dist()
    d.mean[LB.TRUTH_TAU][1] = 0.0                         # FIXED: its floor is the mean
    assert sample(d) == E_ARG and b"tau" in err()
    d = _dist()
    d.mean[LB.TRUTH_LF][1] = float("nan")
    assert sample(d) == E_ARG and b"lf" in err()
    d.n_veh = 1                                           # vehicle 1 is outside: not looked at
    assert sample(d) == 0
    # sizes and arrays
    assert sample(_dist(), B=-1) == E_ARG
    assert sample(_dist(), B=3) == E_ARG and b"truth" in err()
    assert sample(_dist(16), B=1 << 30, out=D) == E_SIZE

    def fill(p, B=0, out=None):
        return lib.scpqp_truth_fill_nominal(None if p is None else C.byref(p), B, out, None)

    assert fill(None) == E_ARG and b"null" in err()
    assert fill(LB.PlantParams(n_veh=0)) == E_ARG
    assert fill(LB.PlantParams(n_veh=2)) == E_ARG and b"lf + lr" in err()
    assert fill(_pp()) == 0
    assert fill(_pp(), B=-1) == E_ARG
    assert fill(_pp(), B=3) == E_ARG and b"truth" in err()
    assert fill(_pp(16), B=1 << 30, out=D) == E_SIZE


# ---------------------------------------------------------------------------
# 3. the mirror is pinned by closed forms
# ---------------------------------------------------------------------------
ROWS = [np.array([0.30, 0.25, 0.07, 0.8, 0.01]), np.array([0.45, 0.40, 0.2, 1.25, -0.01]),
        np.array([0.24, 0.44, 0.1, 1.0, 0.0])]


@pytest.mark.parametrize("row", ROWS)
def test_mirror_steering_lag_closed_form(row):
    """dx[5] reads x[5] only: delta(T) = u_eff + (delta0 - u_eff) exp(-T / tau)."""
    x = np.array([1.0, -2.0, 0.3, 4.0, 0.2, -0.02])
    u = 0.05
    ue = row[TM.GAIN] * u + row[TM.BIAS]
    assert TM.u_eff(row, u) == ue
    for T in (0.01, 0.1, 0.43):
        want = ue + (x[5] - ue) * math.exp(-T / row[TM.TAU])
        assert abs(TM.exact_flow(x, u, row, T)[5] - want) <= 1e-12
        assert abs(TM.rk4_flow(x, u, row, T, TM.steps_for(T, 2.5e-3))[5] - want) <= 1e-9


@pytest.mark.parametrize("row", ROWS)
def test_mirror_steady_steering_is_a_circle_of_the_truth_geometry(row):
    """delta0 = u_eff and no acceleration: steering, speed and slip angle are constant,
    the yaw rate is omega = vc tan(delta) cos(beta) / L, and the position runs a circle of
    radius vc / omega around a fixed centre."""
    u = 0.06
    ue = TM.u_eff(row, u)
    v, psi0 = 4.0, 0.4
    x = np.array([3.0, -1.0, psi0, v, 0.0, ue])
    L = row[TM.LF] + row[TM.LR]
    rho = row[TM.LR] / L
    beta = math.atan(rho * math.tan(ue))
    vc = v * math.sqrt(1 + (rho * math.tan(ue)) ** 2)
    om = vc * math.tan(ue) * math.cos(beta) / L
    rad = vc / om
    for T in (0.05, 0.43):
        y = TM.exact_flow(x, u, row, T)
        a0, a1 = psi0 + beta, psi0 + beta + om * T
        want = np.array([x[0] + rad * (math.sin(a1) - math.sin(a0)),
                         x[1] - rad * (math.cos(a1) - math.cos(a0)), psi0 + om * T, v, 0.0, ue])
        assert np.abs(y - want).max() <= 1e-10
        centre = np.array([x[0] - rad * math.sin(a0), x[1] + rad * math.cos(a0)])
        assert abs(np.hypot(*(y[:2] - centre)) - abs(rad)) <= 1e-10


def test_mirror_nominal_row_is_the_oracle_right_hand_side_bitwise():
    rng = np.random.default_rng(0)
    for _ in range(200):
        x = rng.uniform(-1, 1, 6) * np.array([30, 30, 3, 6, 0.5, 0.3])
        u = rng.uniform(-0.3, 0.3)
        Lf, Lr = rng.uniform(0.2, 0.5, 2)
        nz = rng.standard_normal(2) * 3e-6
        row = TM.nominal_row(Lf, Lr)
        assert TM.u_eff(row, u) == u
        assert np.array_equal(TM.rhs(x, TM.u_eff(row, u), row, nz),
                              R.bicycle_rhs(x, u, Lf, Lr, noise=nz))


# ---------------------------------------------------------------------------
# 4. the mirror sampler
# ---------------------------------------------------------------------------
def _mirror_dist(seed=11, b_offset=0):
    mean = np.array([[0.34, 0.30], [0.34, 0.38], [0.1, 0.1], [1.0, 1.0], [0.0, 0.0]])
    return TM.Dist(mean, seed, b_offset)


def test_mirror_sampler_fixed_uniform_and_clamps():
    d = _mirror_dist()
    s = TM.sample(d, 5)
    assert s.shape == (5, 2, 5)
    assert np.array_equal(s, np.broadcast_to(d.mean.T[None], s.shape))   # FIXED: exactly the mean
    d.set(TM.LF, TM.UNIFORM, 0.05).set(TM.TAU, TM.UNIFORM, 0.03, 0.09, 0.12)
    d.set(TM.BIAS, TM.NORMAL, 0.01, -0.005, 0.02)
    s = TM.sample(d, 400)
    for v in range(2):
        m = d.mean[TM.LF, v]
        assert np.all(s[:, v, TM.LF] >= m - 0.05) and np.all(s[:, v, TM.LF] < m + 0.05)
        assert s[:, v, TM.LF].min() < m - 0.04 and s[:, v, TM.LF].max() > m + 0.04
    assert np.all(s[..., TM.TAU] >= 0.09) and np.all(s[..., TM.TAU] <= 0.12)
    assert (s[..., TM.TAU] == 0.09).any() and (s[..., TM.TAU] == 0.12).any()
    assert np.all(s[..., TM.BIAS] >= -0.005) and np.all(s[..., TM.BIAS] <= 0.02)
    assert (s[..., TM.BIAS] == -0.005).any()
    assert np.array_equal(s[..., TM.LR], np.broadcast_to(d.mean[TM.LR][None], (400, 2)))
    # fields and vehicles draw from distinct counters
    x = TM.xi(d.set(TM.LR, TM.UNIFORM, 0.01), 8)
    assert not np.any(x[..., TM.LF] == x[..., TM.LR])
    assert not np.any(x[:, 0, TM.LF] == x[:, 1, TM.LF])
    assert np.all(x[..., TM.GAIN] == 0.0)                  # a FIXED field draws nothing


def test_mirror_sampler_does_not_depend_on_the_sharding():
    def dist(off):
        return (_mirror_dist(77, off).set(TM.LF, TM.UNIFORM, 0.05)
                .set(TM.GAIN, TM.NORMAL, 0.1, 0.5, 1.5))
    whole = TM.sample(dist(0), 6)
    parts = np.concatenate([TM.sample(dist(0), 3), TM.sample(dist(3), 3)])
    assert np.array_equal(whole, parts)
    assert not np.array_equal(whole[:3, :, TM.LF], whole[3:, :, TM.LF])


def test_mirror_sampler_moments():
    """4096 draws at seed 2024 (2048 realisations x 2 vehicles): uniform xi has mean 0 and
    variance 1/3 (standard errors sqrt(1/3n) and sqrt(4/45n)), normal xi mean 0 and
    variance 1 (sqrt(1/n), sqrt(2/n)); each within four standard errors."""
    d = _mirror_dist(2024).set(TM.LF, TM.UNIFORM, 1.0).set(TM.GAIN, TM.NORMAL, 1.0)
    x = TM.xi(d, 2048)
    u, z = x[..., TM.LF].ravel(), x[..., TM.GAIN].ravel()
    n = u.size
    assert n == 4096 and np.all(u >= -1.0) and np.all(u < 1.0) and np.all(np.isfinite(z))
    scores = (u.mean() / math.sqrt(1 / (3 * n)), (u.var() - 1 / 3) / math.sqrt(4 / (45 * n)),
              z.mean() * math.sqrt(n), (z.var() - 1.0) / math.sqrt(2.0 / n))
    print("z-scores (uniform mean, variance; normal mean, variance):", scores)
    assert all(abs(s) < 4.0 for s in scores), scores


# ---------------------------------------------------------------------------
# 5. scpqp.truth on the host
# ---------------------------------------------------------------------------
def test_validate_raises_on_each_bad_row_kind():
    sc = R.circle_scenario(3, Hp=10)
    good = np.broadcast_to(TR.nominal_rows(sc)[None], (2, 3, 5)).copy()
    assert np.array_equal(good[0, 1], TM.nominal_row(sc.Lf[1], sc.Lr[1]))
    TR.validate(good, 2.5e-3)
    for f in range(5):
        for bad in (float("nan"), float("inf")):
            t = good.copy()
            t[1, 2, f] = bad
            with pytest.raises(ValueError, match="finite"):
                TR.validate(t, 2.5e-3)
    t = good.copy()
    t[0, 1, 0] = -t[0, 1, 1]
    with pytest.raises(ValueError, match="lf \\+ lr"):
        TR.validate(t, 2.5e-3)
    for tau in (0.0, -0.1):
        t = good.copy()
        t[1, 0, 2] = tau
        with pytest.raises(ValueError, match="tau must be > 0"):
            TR.validate(t, 2.5e-3)
    t = good.copy()
    t[1, 0, 2] = 0.0199
    with pytest.raises(ValueError, match="8 \\* h_max"):
        TR.validate(t, 2.5e-3)
    t[1, 0, 2] = 0.02
    TR.validate(t, 2.5e-3)
    TR.validate(good, 0.0125)                             # tau = 0.1 = 8 h_max: the floor itself
    with pytest.raises(ValueError, match="8 \\* h_max"):
        TR.validate(good, 0.0126)
    with pytest.raises(ValueError, match="\\[B, nVeh, 5\\]"):
        TR.validate(good[..., :4], 2.5e-3)


def test_truth_dist_object():
    sc = R.circle_scenario(2, Hp=10)
    d = TR.TruthDist(sc, seed=9, b_offset=4)
    c = d.c_struct()
    assert (c.n_veh, c.seed, c.b_offset) == (2, 9, 4)
    assert [c.field[f].kind for f in range(5)] == [LB.TRUTH_FIXED] * 5
    assert [c.mean[f][1] for f in range(5)] == [sc.Lf[1], sc.Lr[1], 0.1, 1.0, 0.0]
    d.relative(10)
    c = d.c_struct()
    for f, nom in ((0, sc.Lf[0]), (1, sc.Lr[0]), (2, 0.1), (3, 1.0)):
        assert c.field[f].kind == LB.TRUTH_UNIFORM
        assert c.field[f].spread == 0.1 * nom
        assert (c.field[f].lo, c.field[f].hi) == (nom * 0.9, nom * 1.1)
    assert c.field[4].kind == LB.TRUTH_FIXED
    d.normal("bias", 0.01, -0.02, 0.02).fixed("tau", 0.15)
    c = d.c_struct()
    assert (c.field[4].kind, c.field[4].spread, c.field[4].lo, c.field[4].hi) == (2, 0.01, -0.02, 0.02)
    assert c.field[2].kind == LB.TRUTH_FIXED and c.mean[2][0] == c.mean[2][1] == 0.15
    e = d.with_offset(100)
    assert (e.b_offset, d.b_offset, e.seed) == (100, 4, 9) and e.kind == d.kind
    for bad in (lambda: d.uniform("mass", 0.1), lambda: d.uniform("lf", -0.1),
                lambda: d.uniform("lf", float("nan")), lambda: d.normal("lf", 0.1, 1.0, 0.5),
                lambda: d.relative(100), lambda: TR.TruthDist(sc, seed=-1),
                lambda: TR.TruthDist(sc, seed=1, b_offset=2 ** 32)):
        with pytest.raises(ValueError):
            bad()


def test_from_table_gathers_rows():
    import torch
    rows = np.arange(3 * 2 * 5, dtype=float).reshape(3, 2, 5)
    t = TR.from_table(rows, [2, 0, 0, 1], device="cpu")
    assert t.dtype == torch.float64 and tuple(t.shape) == (4, 2, 5) and t.is_contiguous()
    assert np.array_equal(t.numpy(), rows[[2, 0, 0, 1]])
    with pytest.raises(ValueError):
        TR.from_table(rows, [3], device="cpu")
    with pytest.raises(ValueError):
        TR.from_table(rows[..., :4], [0], device="cpu")


def test_only_the_plant_step_takes_a_truth():
    from scpqp import plant as PL
    assert "truth" in PL.plant_step.__code__.co_varnames
    assert "truth" not in PL.delay_compensate.__code__.co_varnames   # the controller's prediction
