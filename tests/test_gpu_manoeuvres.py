"""The obstacle manoeuvres on the device (include/scpqp_manoeuvres.h) against the CPU mirror
(tests/manoeuvre_mirror.py): state and pose with mixed lanes, the off and bad rules, the
independence of the lanes, the chain into the existing prediction entry points, the sampler,
the posed metrics, and the rollout.

Shapes (B, n_obst, n_ticks): (1, 1, 1); (2, 3, 5), no power of two; (12, 22, 10): 264 (b, o)
lanes, two workgroups of 256 with a ragged tail, and 2904 (b, o, tick) lanes.

Tolerance of the device against the mirror, one relative figure for state and pose:
|d| <= TOL max(1, |value|), and identical NaN patterns.  The obstacles stay within 16 m of the
origin, so the figure measures arithmetic and not magnitude.  The device's sin and cos differ
from libm's by an ulp and its sums are fused; a lane walks up to five closed-form pieces.
Measured on an MI355X against the mirror (the test prints the figure; DESIGN §7, "Obstacle
manoeuvres"): the figures are in the comment above TOL below.  TOL is 16 times the largest,
rounded up to a power of two, the convention of tests/test_gpu_tracker.py.  The largest
figure is not sincos: it sits in the position of a lane that brakes to a stop in a turn with
theta = -0.128, just above the switch of p and r at 0.1.  There the closed form of p rounds
cos theta + theta sin theta (above 1, half an ulp is 1.1e-16) before it subtracts 1 and divides
by theta^2 = 0.0164, so one rounding is 6.8e-15 of p (include/scpqp_manoeuvres.h: the closed
forms are within 5e-14 relative on [0.1, 0.5]); the device fuses theta sin theta into the sum and
rounds differently from the mirror.  Against a 40-digit evaluation of that lane the mirror is
3.1e-15 m off and the device 6.0e-15 m, on opposite sides.  Every other kind of lane measures
at most 3.9e-16.

The metrics against the mirror are compared as tests/test_gpu_obstacle_metrics.py compares
them, with its tolerance (1.4e-13 m): integer outputs, infinities and exact zeros exactly.
"""
import math
import types

import numpy as np
import pytest
import torch

import manoeuvre_mirror as MNM
import metrics_mirror as MM
import obstacle_mirror as OM
import sensing_mirror as SM
from oracle import scp_reference as R
from scpqp import manoeuvres as MAN
from scpqp import obstacles as OB
from scpqp import sensing as SE
from scpqp import tracker as TRK

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 3, 5), (12, 22, 10)]          # (B, n_obst, n_ticks)
TICK = 0.05
# measured: (1, 1, 1) 0.0, (2, 3, 5) 2.220e-16, (12, 22, 10) 9.104e-15
TOL = 2.0 ** -42                  # 16 * 9.104e-15 = 1.46e-13 <= 2^-42 = 2.27e-13
LEAD, DT, HP = 0.13, 0.4, 5
M_TOL = 10 * 1.421e-14            # metres: tests/test_gpu_obstacle_metrics.py


def _eq(a, b):
    return a.shape == b.shape and bool(torch.equal(a, b))


def _beq(a, b):
    """Bitwise equality of float64 tensors (NaN payloads and the sign of zero included)."""
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int64),
                                                   b.contiguous().view(torch.int64)))


def _dev(a, gpu, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=gpu)


def _templates(s):
    """Schedules for a row of speed s and turn rate 0.2 (templates 4, 5: turn rate 0)."""
    return [
        # brakes to a stop inside the piece (s / 1.5 s after t = 0.5), a boundary at 0.5
        [(0.5, 0.0, 0.0), (3.0, -1.5, 0.1), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)],
        # theta = w T on both sides of the p / r switch at 0.1: w = 0.2 -+ 0.11, T = 1
        [(1.0, 0.8, -0.11), (1.0, -0.6, -0.09), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)],
        # a zero-duration piece in the middle is skipped
        [(1.0, 1.0, 0.2), (0.0, 5.0, 5.0), (1.0, -1.0, -0.2), (0.5, 0.0, 0.3)],
        # stops, stands through a coast and a braking piece, starts again
        [(0.25, 0.0, 0.0), (2.5, -2.0, -0.4), (0.5, -1.0, 0.3), (1.0, 1.2, 0.5)],
        # w == 0 exactly with a != 0 (the row's turn rate is 0 in these lanes)
        [(0.75, 1.5, 0.0), (1.25, -0.5, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)],
        # A = theta / 2 on both sides of the sinc switch at 1e-4 (turn rate 0 + dyaw), T = 1
        [(1.0, 0.5, 1.8e-4), (1.0, -0.5, 2.2e-4), (0.5, 0.3, 0.0), (0.0, 0.0, 0.0)],
        # a lane change, coasting first
        [(0.5, 0.0, 0.0), (1.5, 0.0, 0.3), (1.5, 0.0, -0.3), (0.0, 0.0, 0.0)],
    ]


def _case(B, nO, seed=3):
    """Rows within 2 m of the origin at speeds up to 2 m/s, evaluated up to t = 5 s: every
    pose within 16 m (asserted on the mirror).  Lane g: every seventh is off (every other of
    them with pieces that do nothing, not zeros); the lanes that are not off take the seven
    templates in turn, counted over those lanes alone, so every template is used."""
    rng = np.random.default_rng(seed + 100 * B + nO)
    g = np.arange(B * nO).reshape(B, nO)
    rows = np.zeros((B, nO, 7))
    rows[..., OM.X], rows[..., OM.Y] = rng.uniform(-2, 2, (B, nO)), rng.uniform(-2, 2, (B, nO))
    rows[..., OM.HEADING] = rng.uniform(-3.0, 3.0, (B, nO))
    rows[..., OM.SPEED] = rng.uniform(0.5, 2.0, (B, nO))
    rows[..., OM.LENGTH], rows[..., OM.WIDTH] = 4.0, 2.0
    rows[..., OM.YAW_RATE] = 0.2
    man = np.zeros((B, nO, 4, 3))
    used = 0                                                 # lanes that are not off so far
    for b in range(B):
        for o in range(nO):
            k = int(g[b, o])
            if k % 7 == 3:
                if k % 14 == 3:
                    man[b, o] = [(0.0, -3.0, 0.2), (1.5, 0.0, 0.0), (0.0, 0.0, 0.0), (2.0, -0.0, 0.0)]
                continue
            t = used % 7
            used += 1
            if t in (4, 5):
                rows[b, o, OM.YAW_RATE] = 0.0
            man[b, o] = _templates(rows[b, o, OM.SPEED])[t]
    return rows, man


# state times: 0, inside pieces, on boundaries (0.5, 1.0, 2.0), past every end (4.25 s at most)
T_STATE = [0.0, 0.3, 0.5, 1.0, 1.7, 2.0, 3.1, 5.0]
# pose ticks: tick0 = 6 covers t = 0.3 .. 0.8 with the boundary 0.5 at tick 10 (10 * 0.05 is
# exactly 0.5); tick0 = 90 lies past the end of every schedule
TICK0 = [6, 90]


def _figure(got, want):
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    return float((np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))).max())


# ---------------------------------------------------------------------------
# 1. state and pose against the mirror
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,nO,n_ticks", SHAPES)
def test_state_and_pose_match_the_mirror(gpu, B, nO, n_ticks):
    rows, man = _case(B, nO)
    if B * nO > 1:
        man[-1, -1, 2, 1] = math.nan                       # one bad lane among the others
    r, m = _dev(rows, gpu), _dev(man, gpu)
    worst = 0.0
    for t in T_STATE:
        got = MAN.state(r, m, t).cpu().numpy()
        want = MNM.state(rows, man, t)
        worst = max(worst, _figure(got, want))
        # what a snapshot copies is copied
        ok = ~np.isnan(want[..., 0])
        assert np.array_equal(got[ok][:, 4:6], rows[ok][:, 4:6])
    for tick0 in TICK0:
        got = MAN.pose(r, m, TICK, tick0, n_ticks).cpu().numpy()
        want = MNM.poses(rows, man, TICK, tick0, n_ticks)
        assert got.shape == (B, nO, n_ticks + 1, 3)
        worst = max(worst, _figure(got, want))
        assert np.abs(want[~np.isnan(want)].reshape(-1, 3)[:, :2]).max() < 16.0
    print(f"({B}, {nO}, {n_ticks}): largest |device - mirror| / max(1, |value|) = {worst:.3e} "
          f"(TOL {TOL:.3e})")
    assert worst <= TOL
    if B * nO > 1:
        assert np.isnan(MAN.state(r, m, 1.0)[-1, -1].cpu().numpy()).all()
    # the speeds that are exactly 0 on the mirror are exactly 0 on the device, with turn rate 0
    got, want = MAN.state(r, m, 5.0).cpu().numpy(), MNM.state(rows, man, 5.0)
    stopped = want[..., OM.SPEED] == 0.0
    assert (got[..., OM.SPEED][stopped] == 0.0).all() and (got[..., OM.YAW_RATE][stopped] == 0.0).all()
    # a NULL schedule is every lane off
    assert _beq(MAN.state(r, None, 1.7), MAN.state(r, torch.zeros_like(m), 1.7))
    assert _beq(MAN.pose(r, None, TICK, 6, n_ticks), OB.pose(r, TICK, 6, n_ticks))


def test_turn_rate_in_effect_on_boundaries_and_while_stopped(gpu):
    rows, man = _case(2, 8)              # 16 lanes, 3 and 10 off: every template twice
    assert [int(np.flatnonzero([np.array_equal(man.reshape(-1, 4, 3)[g], np.array(t))
                                for t in _templates(0.0)])[0]) for g in (4, 12)] == [3, 3]
    r, m = _dev(rows, gpu), _dev(man, gpu)
    for t in (0.0, 0.5, 1.0, 2.0, 2.75, 3.25, 4.25, 5.0):
        got = MAN.state(r, m, t).cpu().numpy()[..., OM.YAW_RATE]
        want = MNM.state(rows, man, t)[..., OM.YAW_RATE]
        assert np.array_equal(got, want), t
    at = MAN.state(r, m, 0.5).cpu().numpy()
    assert at[0, 0, OM.YAW_RATE] == 0.2 + 0.1               # template 0: the later piece's
    assert at[0, 3, OM.YAW_RATE] == 0.2                      # the off lane keeps the row's
    # template 3 (lanes 4 and 12), on the device itself: it stops inside the braking piece
    # (0.25 + s / 2 <= 1.25 s), stands with its heading through the rest of that piece and the
    # next one (ACCEL < 0, a turn-rate offset), and the piece with ACCEL > 0 starts it from 0
    st = {t: MAN.state(r, m, t).view(-1, 7)[[4, 12]] for t in (2.0, 3.1, 3.25, 4.25, 5.0)}
    assert (st[2.0][:, OM.SPEED] == 0).all() and (st[2.0][:, OM.YAW_RATE] == 0).all()
    assert _beq(st[3.1], st[2.0])
    assert _beq(st[3.25][:, :6], st[2.0][:, :6]) and (st[3.25][:, OM.YAW_RATE] == 0.2 + 0.5).all()
    assert (st[4.25][:, OM.SPEED] == 1.2).all() and (st[4.25][:, OM.YAW_RATE] == 0.2).all()
    assert (st[5.0][:, OM.SPEED] == 1.2).all()
    assert not _beq(st[4.25][:, :3], st[2.0][:, :3]) and not _beq(st[5.0][:, :2], st[4.25][:, :2])


# ---------------------------------------------------------------------------
# 2. bitwise and isolation checks
# ---------------------------------------------------------------------------
def test_off_lanes_are_the_obstacle_pose(gpu):
    B, nO, n_ticks = 12, 22, 10
    rows, man = _case(B, nO)
    off = MAN.off_lanes(man)
    assert off.sum() >= 30 and not MAN.is_off(man)
    r, m = _dev(rows, gpu), _dev(man, gpu)
    for tick0 in TICK0:
        got, base = MAN.pose(r, m, TICK, tick0, n_ticks), OB.pose(r, TICK, tick0, n_ticks)
        sel = torch.as_tensor(off, device=gpu)
        assert _beq(got[sel], base[sel])
        assert not _beq(got[~sel], base[~sel])
        # the state of an off lane: the same formulas in another kernel
        st = MAN.state(r, m, tick0 * TICK).cpu().numpy()[off]
        p0 = base[:, :, 0].cpu().numpy()[off]
        fig = float((np.abs(st[:, :3] - p0) / np.maximum(1.0, np.abs(p0))).max())
        print(f"tick0 {tick0}: state of the off lanes against obstacles.pose {fig:.3e}")
        assert fig <= TOL
        assert np.array_equal(st[:, 3:], rows[off][:, 3:])


def test_a_split_batch_gives_what_the_whole_gives(gpu):
    B, nO, n_ticks = 12, 22, 10
    rows, man = _case(B, nO)
    r, m = _dev(rows, gpu), _dev(man, gpu)
    whole_s, whole_p = MAN.state(r, m, 1.7), MAN.pose(r, m, TICK, 6, n_ticks)
    parts_s = torch.cat([MAN.state(r[lo:hi].contiguous(), m[lo:hi].contiguous(), 1.7)
                         for lo, hi in ((0, 5), (5, 12))])
    parts_p = torch.cat([MAN.pose(r[lo:hi].contiguous(), m[lo:hi].contiguous(), TICK, 6, n_ticks)
                         for lo, hi in ((0, 5), (5, 12))])
    assert _beq(whole_s, parts_s) and _beq(whole_p, parts_p)
    d = _dist(nO, 99)[0]
    whole = d.sample(B, device=gpu)
    parts = torch.cat([d.with_offset(o).sample(n, device=gpu) for o, n in ((0, 5), (5, 7))])
    assert _beq(whole, parts) and not _beq(whole[:5], whole[5:10])


def test_changing_the_last_lane_changes_only_that_lane(gpu):
    B, nO, n_ticks = 12, 22, 10
    rows, man = _case(B, nO)
    other = man.copy()
    other[-1, -1] = [(0.4, -1.0, 0.3), (1.0, 2.0, -0.5), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)]
    r = _dev(rows, gpu)
    s0, s1 = (MAN.state(r, _dev(x, gpu), 1.7) for x in (man, other))
    p0, p1 = (MAN.pose(r, _dev(x, gpu), TICK, 6, n_ticks) for x in (man, other))
    assert _beq(s0.view(-1, 7)[:-1], s1.view(-1, 7)[:-1]) and not _beq(s0[-1, -1], s1[-1, -1])
    K = n_ticks + 1
    assert _beq(p0.view(-1, K, 3)[:-1], p1.view(-1, K, 3)[:-1]) and not _beq(p0[-1, -1], p1[-1, -1])


# (piece, field) of the lane's schedule and the value that makes it bad
BAD = {"nan": ((2, 1), math.nan), "inf": ((0, 2), -math.inf), "dur<0": ((1, 0), -0.25)}


@pytest.mark.parametrize("kind", ["nan", "inf", "dur<0", "speed<0", "row"])
def test_a_bad_lane_is_nan_in_its_own_lane_only(gpu, kind):
    B, nO, n_ticks = 2, 3, 5
    rows, man = _case(B, nO)
    r, m = _dev(rows, gpu), _dev(man, gpu)
    good_s, good_p = MAN.state(r, m, 1.7), MAN.pose(r, m, TICK, 6, n_ticks)
    rows2, man2 = rows.copy(), man.copy()
    lane = (1, 1)                                            # lane 4: not off
    assert not MAN.off_lanes(man)[lane]
    if kind == "speed<0":
        rows2[lane][OM.SPEED] = -0.5
    elif kind == "row":
        rows2[lane][OM.WIDTH] = -1.0
    else:
        (i, f), val = BAD[kind]
        man2[lane][i, f] = val
    s = MAN.state(_dev(rows2, gpu), _dev(man2, gpu), 1.7)
    p = MAN.pose(_dev(rows2, gpu), _dev(man2, gpu), TICK, 6, n_ticks)
    torch.cuda.synchronize()
    assert torch.isnan(s[lane]).all() and torch.isnan(p[lane]).all()
    keep = torch.ones((B, nO), dtype=torch.bool, device=gpu)
    keep[lane] = False
    assert _beq(s[keep], good_s[keep]) and _beq(p[keep], good_p[keep])
    assert np.array_equal(np.isnan(s.cpu().numpy()), np.isnan(MNM.state(rows2, man2, 1.7)))
    if kind == "speed<0":
        # a reversing row is legal under an off schedule
        assert torch.isfinite(MAN.state(_dev(rows2, gpu), None, 1.7)).all()


# ---------------------------------------------------------------------------
# 3. the chain into the existing entry points, the sampler
# ---------------------------------------------------------------------------
def _rel(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def test_the_snapshot_measured_at_zero_feeds_the_existing_predictions(gpu):
    B, nO = 12, 22
    rows, man = _case(B, nO)
    r, m = _dev(rows, gpu), _dev(man, gpu)
    off = MAN.off_lanes(man)
    osense = np.zeros((B, nO, 3))
    osense[..., 0], osense[..., 1], osense[..., 2] = 0.05, 0.01, 0.1
    osense[::3] = 0.0
    os_d = _dev(osense, gpu)
    for t in (0.5, 1.7):
        snap = MAN.state(r, m, t)
        snap_m = MNM.state(rows, man, t)
        got = OB.predict(snap, 0.0, LEAD, DT, HP).cpu().numpy()
        base = OB.predict(r, t, LEAD, DT, HP).cpu().numpy()
        figs = [_rel(got, OM.predict(snap_m, 0.0, LEAD, DT, HP)), _rel(got[off], base[off])]
        assert _rel(got[~off], base[~off]) > 1e-3
        got = SE.predict_sensed(snap, os_d, 31, 2, 0, 0.0, LEAD, DT, HP).cpu().numpy()
        base = SE.predict_sensed(r, os_d, 31, 2, 0, t, LEAD, DT, HP).cpu().numpy()
        figs += [_rel(got, SM.predict_sensed(snap_m, osense, 31, 2, 0, 0.0, LEAD, DT, HP)),
                 _rel(got[off], base[off])]
        print(f"t = {t}: predict against the mirror {figs[0]:.3e}, its off lanes against the rows "
              f"{figs[1]:.3e}; predict_sensed {figs[2]:.3e}, {figs[3]:.3e}")
        assert max(figs) <= TOL


def _dist(nO, seed, b_offset=0):
    d = MAN.ManoeuvreDist(nO, seed, b_offset)
    d.uniform(0, "dur", 2.0, 2.0, lo=0.0, hi=3.5).fixed(1, "dur", 3.0)
    d.uniform(1, "accel", -3.0, 1.0, hi=-2.5).normal(1, "dyaw", 0.0, 0.2, -0.3, 0.3)
    d.normal(2, "dur", 1.0, 1.0, lo=0.0)
    m = MNM.Dist(nO, seed, b_offset)
    m.set(0, 0, MNM.UNIFORM, 2.0, 2.0, 0.0, 3.5).set(1, 0, MNM.FIXED, 3.0)
    m.set(1, 1, MNM.UNIFORM, -3.0, 1.0, hi=-2.5).set(1, 2, MNM.NORMAL, 0.0, 0.2, -0.3, 0.3)
    m.set(2, 0, MNM.NORMAL, 1.0, 1.0, lo=0.0)
    return d, m


def test_sampler_matches_the_mirror(gpu):
    """FIXED and UNIFORM fields bitwise; NORMAL fields within the tolerance of a normal draw of
    tests/test_gpu_obstacles.py::test_sampler_matches_the_mirror (64 * 2^-52 * 10) times
    spread."""
    seed, b_off, B, nO = 0x123456789ABCDEF, 1000, 16, 22
    d, m = _dist(nO, seed, b_off)
    got = d.sample(B, device=gpu).cpu().numpy()
    want = MNM.sample(m, B)
    assert got.shape == want.shape == (B, nO, 4, 3)
    normal = np.zeros((4, 3), bool)
    normal[1, 2] = normal[2, 0] = True
    assert np.array_equal(got[..., ~normal], want[..., ~normal])
    atol = 64 * 2.0 ** -52 * 10
    for (i, f), spread in (((1, 2), 0.2), ((2, 0), 1.0)):
        err = np.abs(got[..., i, f] - want[..., i, f]).max()
        print(f"piece {i} field {f}: max |device - mirror| = {err:.3e} (atol {atol * spread:.3e})")
        assert err <= atol * spread
    assert (got[..., 1, 0] == 3.0).all() and (got[..., 3, :] == 0.0).all()
    assert got[..., 0, 0].min() >= 0.0 and got[..., 0, 0].max() == 3.5
    assert got[..., 1, 1].max() == -2.5 and got[..., 2, 0].min() == 0.0
    assert np.abs(got[..., 1, 2]).max() == 0.3
    MAN.validate(got)
    assert not _eq(d.sample(B, device=gpu), _dist(nO, seed + 1, b_off)[0].sample(B, device=gpu))


# ---------------------------------------------------------------------------
# 4. the posed metrics
# ---------------------------------------------------------------------------
M_SHAPES = [(3, 2, 3, 5), (3, 1, 22, 41)]                   # (B, n_veh, n_obst, K)
M_TICK0 = 40
INT_FIELDS = ("argmin_gap_veh", "argmin_gap_obs", "first_collision_tick", "n_collision_ticks",
              "n_ticks_seen")
DBL_FIELDS = ("min_gap_veh", "min_gap_obs", "min_margin_veh", "min_margin_obs", "max_xtrack",
              "sum_sq_xtrack")


def _m_scenario(rng, nV, nO, span, tick):
    obstacles = [(rng.uniform(-span, span), rng.uniform(-span, span), rng.uniform(-3, 3),
                  rng.uniform(0.5, 2.5), rng.uniform(1, 4), rng.uniform(0.5, 2)) for _ in range(nO)]
    return types.SimpleNamespace(
        nVeh=nV, nObst=nO, Length=list(rng.uniform(0.5, 2.0, nV)), Width=list(rng.uniform(0.4, 1.0, nV)),
        obstacles=[np.asarray(o, float) for o in obstacles],
        dsafeVehicles=np.full((nV, nV), 2.0) + 0.01 * np.arange(nV * nV).reshape(nV, nV),
        dsafeObstacles=np.full((nV, nO), 2.0) + 0.01 * np.arange(nV * nO).reshape(nV, nO),
        referenceTrajectories=[np.asarray([(-100.0, float(v)), (100.0, float(v))]) for v in range(nV)],
        tick_length=tick)


def _m_path(rng, B, nV, K, span):
    x = np.zeros((B, nV, K, 6))
    x[..., 0:2] = rng.uniform(-span, span, (B, nV, K, 2))
    x[..., 2] = rng.uniform(-math.pi, math.pi, (B, nV, K))
    return x


def _m_case(shape, seed):
    B, nV, nO, K = shape
    rng = np.random.default_rng(seed)
    span = 3.0 if nV <= 2 else 14.0
    sc = _m_scenario(rng, nV, nO, span, TICK)
    rows = np.broadcast_to(OM.nominal_rows(sc)[None], (B, nO, 7)).copy()
    rows[..., 6] = rng.uniform(-0.4, 0.4, (B, nO))
    man = _case(B, nO)[1]
    x1 = _m_path(rng, B, nV, K, span)
    x2 = _m_path(rng, B, nV, K, span)
    x2[:, :, 0] = x1[:, :, -1]
    return sc, rows, man, [(x1, M_TICK0, 0), (x2, M_TICK0 + K - 1, 1)]


def _close(name, got, want, tol=M_TOL):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, name
    special = np.isinf(want) | np.isinf(got)
    if "gap" in name:
        special |= (want == 0.0) | (got == 0.0)
    assert np.array_equal(got[special], want[special]), name
    d = float(np.abs(got[~special] - want[~special]).max()) if (~special).any() else 0.0
    print(f"max |device - mirror| {name}: {d:.3e}")
    assert d <= tol, (name, d)


def _check_result(res, want, tag):
    for k in INT_FIELDS:
        assert np.array_equal(res[k].cpu().numpy(), want[k]), (tag, k)
    for k in DBL_FIELDS[:-1]:
        _close(f"{tag}.{k}", res[k].cpu().numpy(), want[k])
    n, e = float(want["n_ticks_seen"].max()), float(want["max_xtrack"].max())
    _close(f"{tag}.sum_sq_xtrack", res["sum_sq_xtrack"].cpu().numpy(), want["sum_sq_xtrack"],
           tol=max(n * M_TOL * (2 * e + M_TOL), 1e-300))


def _smallest_margin(base, rows, man, calls):
    m = math.inf
    for x, t0, _ in calls:
        pose = MNM.poses(rows, man, base.tick_length, t0, x.shape[2] - 1)
        for b in range(x.shape[0]):
            Cn = MNM.PosedConstants(base, rows[b], pose[b], t0)
            for k in range(x.shape[2]):
                rects = [MM._rect(x[b, v, k, 0], x[b, v, k, 1], x[b, v, k, 2], Cn.length[v], Cn.width[v])
                         for v in range(Cn.nV)]
                obs = [Cn.obstacle_rect(o, t0 + k) for o in range(Cn.nO)]
                for v in range(Cn.nV):
                    for other in rects[v + 1:] + obs:
                        m = min(m, min(abs(t) for t in MM.separation_margins(rects[v], other)))
    return m


@pytest.mark.parametrize("shape", M_SHAPES)
def test_metrics_with_manoeuvres_match_the_mirror(gpu, shape):
    """Two consecutive calls, dense outputs of both, against the mirror with the obstacles at
    the mirror's poses.  Realisation 0 drives its vehicle 0 onto the manoeuvring obstacle 0 at
    entry 2 of the second call: a gap of 0.0 and a collision tick."""
    from scpqp.metrics import PathMetrics
    B, nV, nO, K = shape
    sc, rows, man, calls = _m_case(shape, 53)
    assert not MAN.off_lanes(man)[0, 0]
    hit = calls[1][1] + 2
    px, py, ph = MNM.walk(rows[0, 0], man[0, 0], hit * TICK)[:3]
    calls[1][0][0, 0, 2, 0:2] = (px, py)
    base = MM.Constants.of_scenario(sc)
    margin = _smallest_margin(base, rows, man, calls)
    print(f"smallest separation margin: {margin:.3e}")
    assert margin > 1e-6
    pm = PathMetrics(sc, B, gpu)
    pm.reset(B)
    r, m = _dev(rows, gpu), _dev(man, gpu)
    dense = [pm.accumulate(_dev(x, gpu), t0, kf, dense=True, obstacles=r, manoeuvres=m)
             for x, t0, kf in calls]
    res = pm.result()
    torch.cuda.synchronize()
    tag = f"man{nV}x{nO}"
    for (x, t0, _), d in zip(calls, dense):
        pose = MNM.poses(rows, man, TICK, t0, K - 1)
        for b in range(B):
            md = MM.dense(MNM.PosedConstants(base, rows[b], pose[b], t0), x[b], t0)
            for k in ("gap_veh", "gap_obs", "xtrack"):
                _close(f"{tag}.{k}", d[k][b].cpu().numpy(), md[k])
    _check_result(res, MNM.run(base, rows, man, calls, B), tag)
    assert float(dense[1]["gap_obs"][0, 2, 0, 0]) == 0.0
    assert float(res["min_gap_obs"][0]) == 0.0 and 0 <= int(res["first_collision_tick"][0]) <= hit
    # the schedule is read: the rows alone give other gaps
    pm.reset(B)
    other = pm.accumulate(_dev(calls[0][0], gpu), M_TICK0, 0, dense=True, obstacles=r)
    assert not torch.equal(other["gap_obs"], dense[0]["gap_obs"])
    pm.close()


def test_an_off_schedule_through_the_posed_entry_is_the_rows(gpu):
    """The integers, infinities and zeros are compared exactly, the other doubles within the
    metrics' tolerance: the posed path takes the obstacle's position from the pose kernel and
    the rows path computes it inside the metrics kernel, the same formulas in two kernels, and
    no rounding order is promised between them (include/scpqp_obstacles.h).  An off schedule
    that is not forced takes the rows path itself and is compared bitwise."""
    from scpqp.metrics import PathMetrics
    shape = M_SHAPES[1]
    B, nV, nO, K = shape
    sc, rows, _, calls = _m_case(shape, 59)
    r, off = _dev(rows, gpu), MAN.off(B, nO, device=gpu)
    out = {}
    for name, kw in (("rows", {}), ("off", dict(manoeuvres=off)),
                     ("posed", dict(manoeuvres=off, check_off=False))):
        pm = PathMetrics(sc, B, gpu)
        pm.reset(B)
        d = [pm.accumulate(_dev(x, gpu), t0, kf, dense=True, obstacles=r, **kw) for x, t0, kf in calls]
        out[name] = (d, pm.result())
        pm.close()
    for i in range(2):
        for k in out["rows"][0][i]:
            assert torch.equal(out["rows"][0][i][k], out["off"][0][i][k]), k   # the same kernel
            _close(f"posed.{k}", out["posed"][0][i][k].cpu().numpy(), out["rows"][0][i][k].cpu().numpy())
    for k in out["rows"][1]:
        assert torch.equal(out["rows"][1][k], out["off"][1][k]), k
    _check_result(out["posed"][1], {k: v.cpu().numpy() for k, v in out["rows"][1].items()}, "posed")


@pytest.mark.parametrize("kind", ["schedule", "row"])
def test_a_bad_lane_leaves_its_realisation_untouched(gpu, kind):
    from scpqp.metrics import PathMetrics
    shape = M_SHAPES[0]
    B, nV, nO, K = shape
    sc, rows, man, calls = _m_case(shape, 61)
    x, t0, _ = calls[0]
    pm = PathMetrics(sc, B, gpu)
    pm.reset(B)
    good_dense = pm.accumulate(_dev(x, gpu), t0, 0, dense=True, obstacles=_dev(rows, gpu),
                               manoeuvres=_dev(man, gpu))
    good = pm.result()
    pm.reset(B)
    cleared = pm.result()
    rows2, man2 = rows.copy(), man.copy()
    if kind == "schedule":
        man2[1, nO - 1, 1, 0] = -1.0
    else:
        rows2[1, nO - 1, OM.LENGTH] = math.nan
    sentinel = -7.0
    d = pm.accumulate(_dev(x, gpu), t0, 0, dense=True, obstacles=_dev(rows2, gpu),
                      manoeuvres=_dev(man2, gpu), check_off=False)
    res = pm.result()
    for k in res:
        assert torch.equal(res[k][1], cleared[k][1]), k            # the reset values
        assert torch.equal(res[k][0], good[k][0]) and torch.equal(res[k][2], good[k][2]), k
    assert res["n_ticks_seen"].tolist() == [K, 0, K]
    for k in ("gap_veh", "gap_obs", "xtrack"):
        assert torch.equal(d[k][0], good_dense[k][0]) and torch.equal(d[k][2], good_dense[k][2]), k
    # the dense rows of realisation 1 are not written either
    import ctypes as C
    from scpqp import _lib as LB
    gap = torch.full((B, K, nV, nO), sentinel, dtype=torch.float64, device=gpu)
    D = LB.MetricsDense(gap_veh=None, gap_obs=gap.data_ptr(), xtrack=None)
    xd, rd = _dev(x, gpu), _dev(rows2, gpu)
    pd = MAN.pose(rd, _dev(man2, gpu), TICK, t0, K - 1)
    rc = pm.lib.scpqp_metrics_accumulate_posed(
        pm.h, B, K - 1, t0, 0, C.c_void_p(xd.data_ptr()), None, C.byref(D), None,
        C.c_void_p(rd.data_ptr()), C.c_void_p(pd.data_ptr()), pm._stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert (gap[1] == sentinel).all() and torch.equal(gap[0], good_dense["gap_obs"][0])
    with pytest.raises(ValueError, match="manoeuvres needs obstacles"):
        pm.accumulate(_dev(x, gpu), t0, 0, manoeuvres=_dev(man, gpu))
    for bad in (_dev(man, gpu)[:2], _dev(man, gpu).float(), man):
        with pytest.raises(ValueError, match="manoeuvres must be"):
            pm.accumulate(_dev(x, gpu), t0, 0, obstacles=_dev(rows, gpu), manoeuvres=bad)
    pm.close()


# ---------------------------------------------------------------------------
# 5. the rollout
# ---------------------------------------------------------------------------
STEPS = 4
KEYS = ("x0", "u0", "umax", "U", "traj", "n_scp", "status", "path", "u_tick", "obst")
MAN_KEYS = ("obst_state",)
TRK_KEYS = ("obst_est", "obst_nis", "obst_meas")
SENSE_SEED = 31


def _x_init(sc, B):
    rng = np.random.default_rng(12)
    return np.array(sc.x0, float)[None] + rng.standard_normal((B, sc.nVeh, 6)) * np.array(
        [0.05, 0.05, 0.005, 0.02, 0.0, 0.002])


def _snapshot(cl):
    return types.SimpleNamespace(
        hist=[{k: h[k].clone() for k in KEYS + MAN_KEYS + TRK_KEYS if k in h} for h in cl.history],
        metrics=cl.metrics(), control=cl.control.clone())


@pytest.fixture(scope="module")
def rollouts(gpu):
    from scpqp.rollout import ClosedLoopBatch
    sc = R.frog_scenario(Hp=10)
    B, nO = 4, sc.nObst
    x_init = _x_init(sc, B)
    rows = np.broadcast_to(OM.nominal_rows(sc), (B, nO, 7)).copy()
    rows[..., OM.YAW_RATE] = np.random.default_rng(21).uniform(-0.3, 0.3, (B, nO))
    # every obstacle brakes at 3 m/s^2 until it stands, from a time inside the four steps
    t0 = np.random.default_rng(22).uniform(0.0, STEPS * sc.dt * 0.75, (B, nO))
    brake = MAN.rows(B, nO, MAN.brake(t0, 3.0, 20.0), device="cpu").numpy()
    osense = np.zeros((B, nO, 3))
    osense[..., 0], osense[..., 1], osense[..., 2] = 0.05, 0.01, 0.1
    trk = TRK.matched(osense, device="cpu").numpy()
    sense = dict(obstacle_sensing=osense, sense_seed=SENSE_SEED)
    cl = ClosedLoopBatch(sc, B, device=gpu, keep_path=True, metrics=True)
    runs = {}
    for name, kw in (("plain", {}), ("none", dict(manoeuvres=None)),
                     ("off", dict(manoeuvres=np.zeros((B, nO, 4, 3)))),
                     ("brake", dict(manoeuvres=brake)),
                     ("brake_trk", dict(manoeuvres=_dev(brake, gpu), tracker=trk, **sense))):
        cl.reset(x_init, seed=1, obstacles=rows, **kw)
        cl.run(STEPS)
        runs[name] = _snapshot(cl)
        if name == "brake":
            plot = cl.result_for_plot(1)
    half = ClosedLoopBatch(sc, 2, device=gpu, keep_path=True, metrics=True)
    for o in (0, 2):
        half.reset(x_init[o:o + 2], seed=1, b_offset=o, obstacles=rows[o:o + 2],
                   manoeuvres=brake[o:o + 2], tracker=trk[o:o + 2],
                   obstacle_sensing=osense[o:o + 2], sense_seed=SENSE_SEED)
        half.run(STEPS)
        runs[f"half{o}"] = _snapshot(half)
    half.close()
    torch.cuda.synchronize()
    yield types.SimpleNamespace(sc=sc, cl=cl, B=B, x_init=x_init, rows=rows, brake=brake,
                                osense=osense, trk=trk, runs=runs, plot=plot)
    cl.close()


@pytest.mark.parametrize("same", ["none", "off"])
def test_rollout_without_manoeuvres_is_the_rollout_of_before(rollouts, same):
    a, b = rollouts.runs["plain"], rollouts.runs[same]
    assert len(a.hist) == len(b.hist) == STEPS
    for i in range(STEPS):
        assert a.hist[i].keys() == b.hist[i].keys() and "obst_state" not in b.hist[i]
        for k in a.hist[i]:
            if a.hist[i][k].dtype == torch.float64:
                assert _beq(a.hist[i][k], b.hist[i][k]), (i, k)
            else:
                assert _eq(a.hist[i][k], b.hist[i][k]), (i, k)
    assert _beq(a.control, b.control)
    for k, v in a.metrics.items():
        assert _eq(v, b.metrics[k]), k


def test_rollout_records_the_snapshot_and_predicts_from_it(rollouts, gpu):
    ro, sc = rollouts, rollouts.sc
    rows, man = _dev(ro.rows, gpu), _dev(ro.brake, gpu)
    lead = sc.delay_x + sc.dt + sc.delay_u
    differs = False
    for i, rec in enumerate(ro.runs["brake"].hist):
        g1 = max(0, i * sc.ticks_per_sim - sc.ticks_delay_x)
        snap = MAN.state(rows, man, g1 * sc.tick_length)
        assert _beq(rec["obst_state"], snap), i
        assert _beq(rec["obst"], OB.predict(rec["obst_state"], 0.0, lead, sc.dt, sc.Hp)), i
        differs |= not _beq(rec["obst"], ro.runs["plain"].hist[i]["obst"])
    assert differs
    last = ro.runs["brake"].hist[-1]["obst_state"]
    assert (last[..., OM.SPEED] < _dev(ro.rows, gpu)[..., OM.SPEED]).any()
    assert not all(_eq(v, ro.runs["plain"].metrics[k]) for k, v in ro.runs["brake"].metrics.items())


def test_rollout_with_a_tracker_is_a_replay_of_step_on_the_snapshots(rollouts, gpu):
    ro, sc = rollouts, rollouts.sc
    rows, man = _dev(ro.rows, gpu), _dev(ro.brake, gpu)
    osense, trk = _dev(ro.osense, gpu), _dev(ro.trk, gpu)
    x, cov = TRK.alloc(ro.B, sc.nObst, gpu)
    lead = sc.delay_x + sc.dt + sc.delay_u
    g0 = 0
    for i, rec in enumerate(ro.runs["brake_trk"].hist):
        g1 = max(0, i * sc.ticks_per_sim - sc.ticks_delay_x)
        snap = MAN.state(rows, man, g1 * sc.tick_length)
        ob, z, nis = TRK.step(snap, osense, SENSE_SEED, i, 0, trk, 0.0, (g1 - g0) * sc.tick_length,
                              lead, sc.dt, sc.Hp, x, cov)
        g0 = g1
        assert _beq(rec["obst_state"], snap), i
        assert _beq(rec["obst"], ob) and _beq(rec["obst_est"], x), i
        assert _beq(rec["obst_nis"], nis) and _beq(rec["obst_meas"], z), i
    assert torch.isfinite(ro.runs["brake_trk"].hist[-1]["obst_nis"]).all()


def test_rollout_with_manoeuvres_does_not_depend_on_the_sharding(rollouts):
    ro = rollouts
    for i, whole in enumerate(ro.runs["brake_trk"].hist):
        for k in KEYS + MAN_KEYS + TRK_KEYS:
            parts = torch.cat([ro.runs["half0"].hist[i][k], ro.runs["half2"].hist[i][k]])
            if whole[k].dtype == torch.float64:
                assert _beq(whole[k], parts), (i, k)
            else:
                assert _eq(whole[k], parts), (i, k)
    for k, v in ro.runs["brake_trk"].metrics.items():
        assert _eq(v, torch.cat([ro.runs["half0"].metrics[k], ro.runs["half2"].metrics[k]])), k


def test_result_for_plot_draws_the_manoeuvring_obstacles(rollouts, gpu):
    ro, sc = rollouts, rollouts.sc
    T = int(sc.ticks_total)
    p = MAN.pose(_dev(ro.rows[1:2], gpu), _dev(ro.brake[1:2], gpu), sc.tick_length, 0, T)[0].cpu().numpy()
    obs = ro.plot["obstaclePathFullRes"]
    assert obs.shape == (sc.nObst, 2, T + 1)
    assert np.array_equal(obs[:, 0], p[:, :, 0]) and np.array_equal(obs[:, 1], p[:, :, 1])
    straight = OB.pose(_dev(ro.rows[1:2], gpu), sc.tick_length, 0, T)[0].cpu().numpy()
    assert not np.array_equal(obs[:, 0], straight[:, :, 0])


def test_reset_refuses_bad_manoeuvres_before_anything_is_launched(rollouts, gpu):
    ro, cl = rollouts, rollouts.cl
    cl.reset(ro.x_init, seed=1, obstacles=ro.rows, manoeuvres=ro.brake)
    cl.run(1)
    n_hist, i = len(cl.history), cl.i
    state, man_before = cl.state.clone(), cl.man_rows.clone()
    good = ro.brake
    neg, nan = good.copy(), good.copy()
    neg[2, 1, 1, 0] = -0.1
    nan[0, 0, 1, 1] = math.nan
    back = ro.rows.copy()
    back[3, 2, OM.SPEED] = -1.0
    for bad in (good[:2], good[:, :1], good[..., :2], good.reshape(4, -1, 12), neg,
                torch.as_tensor(neg), nan):
        with pytest.raises(ValueError):
            cl.reset(ro.x_init, seed=1, obstacles=ro.rows, manoeuvres=bad)
    with pytest.raises(ValueError, match=r"man\[2, 1, 1\]: dur must be >= 0"):
        cl.reset(ro.x_init, seed=1, obstacles=ro.rows, manoeuvres=neg)
    with pytest.raises(ValueError, match=r"man\[0, 0, 1\]: accel is not finite"):
        cl.reset(ro.x_init, seed=1, obstacles=ro.rows, manoeuvres=nan)
    with pytest.raises(ValueError, match=r"man\[3, 2\]: a manoeuvre needs a row with speed >= 0"):
        cl.reset(ro.x_init, seed=1, obstacles=back, manoeuvres=good)
    with pytest.raises(ValueError, match=r"manoeuvres needs obstacles= rows"):
        cl.reset(ro.x_init, seed=1, manoeuvres=good)
    assert len(cl.history) == n_hist and cl.i == i           # the refused resets changed nothing
    assert _eq(cl.state, state) and _beq(cl.man_rows, man_before)
