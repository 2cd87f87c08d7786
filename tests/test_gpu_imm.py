"""The interacting-multiple-model obstacle tracker on the device (include/scpqp_imm.h) against
the CPU mirror (tests/imm_mirror.py): eight steps on manoeuvre snapshots with mixed lanes for
M = 1 .. 4, the off and bad-lane rules, the independence of the lanes, recovery after trouble,
the reductions to the single filter, the mode response, and the rollout.  The inputs are those
of tests/imm_cases.py, which the CPU tests use too.

Shapes (B, n_obst, hp) of tests/tracker_accel_cases.py: (12, 22, 10): 264 lanes of four threads,
five workgroups of 256 with a ragged tail; (2, 3, 5); (1, 1, 1).

Tolerance of the device against the mirror: the relative figure of
``tracker_accel_cases.ratio`` over the estimates of every mode, the combined estimate, the
measurement, the obst block, the covariances and the innovations, with mu compared absolutely
(``imm_cases.ratio``), and identical NaN patterns.  TOL is not fitted to the device: it is
derived on the CPU from the reference alone, on exactly these inputs (tests/test_imm_host.py,
test_tolerance_is_sixteen_times_the_rounding_the_definition_amplifies).  The largest figure
between the mirror in float64 and the mirror in 80-bit is 9.87e-13 (M = 2, (12, 22, 10), a
probability of the last step: the likelihood turns an error of nis / 2 into a relative error of
mu); the device contracts multiply-adds and has its own sincos, exp and log, so TOL is 16 times
it, rounded up to a power of two: 2^-35 = 2.91e-11.

The reductions compare the device bank against ``tracker_accel.step`` on the device, both
sides device results: bitwise for one mode and for Pi = I with mu0 = (1, 0), as on the mirrors,
and within RED_TOL for identical modes: 16 times what the host test measured between the two
mirrors (1.03e-13), rounded up to a power of two, 2^-39 = 1.82e-12.

The mode response asserts what the host test asserts of the mirror and nothing tighter
(imm_cases.RESP_K).  The frog rollout reports the summed prediction error next to the two
single filters' and asserts nothing about it: the host tests do not show an order on the CPU.

Measured on an MI355X (the tests print the figures):
  device against mirror at (12, 22, 10): 6.29e-14 (M = 1), 9.19e-13 (2), 1.19e-12 (3), 5.91e-13 (4);
  at (2, 3, 5) at most 3.89e-14, at (1, 1, 1) at most 1.47e-14
  reductions against tracker_accel.step: 0 (one_mode), 0 (identity), 6.82e-14 (identical)
  mode response, batch mean of mu (straight, arc, brake): (0.663, 0.292, 0.045) at the last
  cruising call, (0.0000, 0.0001, 0.9999) at the first braking call
  frog rollout, braking at 3 m/s^2, summed prediction error from step 3 on: 386.56 m with the
  bank, 329.56 m with the six-state filter, 1514.80 m with the five-state, 1509.21 m untracked
"""
import math
import types

import numpy as np
import pytest
import torch

import imm_cases as IC
import imm_mirror as IM
import manoeuvre_mirror as MNM
import obstacle_mirror as OM
import tracker_accel_cases as TC
from oracle import scp_reference as R
from scpqp import imm as IMM
from scpqp import manoeuvres as MAN
from scpqp import obstacles as OB
from scpqp import sensing as SE
from scpqp import tracker as TRK
from scpqp import tracker_accel as TRKA

pytestmark = pytest.mark.gpu

TOL = IC.TOL
MAN_TOL = 2.0 ** -42              # tests/test_gpu_manoeuvres.py
LEAD, DT, SEED = IC.LEAD, IC.DT, IC.SEED


def _eq(a, b):
    return a.shape == b.shape and bool(torch.equal(a, b))


def _beq(a, b):
    """Bitwise equality of float64 tensors (NaN payloads and the sign of zero included)."""
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int64),
                                                   b.contiguous().view(torch.int64)))


def _dev(a, gpu, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=gpu)


def _np(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------
# 1. device against mirror
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("M", IC.MODES)
@pytest.mark.parametrize("B,nO,hp", IC.SHAPES)
def test_eight_steps_match_the_mirror(gpu, B, nO, hp, M):
    rows, man, osense, trk, sw = IC.case(B, nO, M)
    rows_d, man_d, os_d, trk_d, sw_d = (_dev(a, gpu) for a in (rows, man, osense, trk, sw))
    st_d = IMM.alloc(B, nO, M, gpu)
    st_m = IM.alloc(B, nO, M)
    on = (trk != 0).any(axis=(2, 3))
    worst, seen_update = 0.0, False
    for s, (t, since) in enumerate(IC.times()):
        snap_d = MAN.state(rows_d, man_d, t)
        snap = _np(snap_d)
        want = MNM.state(rows, man, t)
        assert np.array_equal(np.isnan(snap), np.isnan(want))
        ok = ~np.isnan(want)
        assert (np.abs(snap - want)[ok] <= MAN_TOL * np.maximum(1.0, np.abs(want[ok]))).all()
        ob_d, xh_d, z_d, nis_d = IMM.step(snap_d, os_d, SEED, s, IC.B_OFFSET, trk_d, sw_d, 0.0, since,
                                          LEAD, DT, hp, *st_d)
        ob_m, xh_m, z_m, nis_m = IM.step(snap, osense, SEED, s, IC.B_OFFSET, trk, sw, 0.0, since,
                                         LEAD, DT, hp, *st_m)
        x_d, cov_d, mu_d = (_np(a) for a in st_d)
        # the off lanes: untouched state
        assert np.isnan(x_d[~on]).all() and (cov_d[~on] == 0).all() and (mu_d[~on] == 0).all()
        worst = max(worst, IC.ratio((x_d, cov_d, mu_d, _np(xh_d), _np(nis_d), _np(ob_d), _np(z_d)),
                                    (*st_m, xh_m, nis_m, ob_m, z_m)))
        seen_update |= bool(np.isfinite(nis_m).any())
        assert np.array_equal(cov_d, np.swapaxes(cov_d, -1, -2), equal_nan=True)
        live = ~np.isnan(mu_d[..., 0]) & on
        assert (np.abs(mu_d[live].sum(axis=-1) - 1.0) <= 1e-14).all()
    print(f"M = {M} ({B}, {nO}, {hp}): largest device - mirror ratio {worst:.3e} (TOL {TOL:.3e})")
    assert seen_update or B * nO == 1 and not on.any()
    if B * nO > 214:
        # one bad lane of each kind, NaN in every output of its own lane
        for lane, kind in {**TC.BAD_LANES, **IC.BAD_LANES}.items():
            if kind == "mixed" and M == 1:
                continue
            b, o = divmod(lane, nO)
            assert torch.isnan(st_d[0][b, o]).all() and torch.isnan(st_d[2][b, o]).all(), kind
            assert torch.isnan(ob_d[b, o]).all() and torch.isnan(xh_d[b, o]).all(), kind
    assert worst <= TOL


# ---------------------------------------------------------------------------
# 2. off lanes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sensed", [False, True])
def test_off_lanes_give_the_untracked_prediction_and_leave_the_state(gpu, sensed):
    B, nO, hp, M = 12, 22, 10, 3
    rows, man, osense, trk, sw = IC.case(B, nO, M)
    snap = MNM.state(rows, man, 0.8)
    rng = np.random.default_rng(5)
    st0 = tuple(_dev(rng.standard_normal(s), gpu) for s in ((B, nO, M, 6), (B, nO, M, 6, 6),
                                                             (B, nO, M)))
    rows_d = _dev(snap, gpu)
    os_d = _dev(osense, gpu) if sensed else None
    want = SE.predict_sensed(rows_d, os_d, SEED, 4, 2, 0.0, LEAD, DT, hp) if sensed \
        else OB.predict(rows_d, 0.0, LEAD, DT, hp)
    st = tuple(a.clone() for a in st0)
    ob, xh, z, nis = IMM.step(rows_d, os_d, SEED, 4, 2, *IMM.off(B, nO, M, gpu), 0.0, IC.T_STEP,
                              LEAD, DT, hp, *st)
    assert _beq(ob, want) and all(_beq(a, b) for a, b in zip(st, st0))
    assert torch.isnan(nis).all() and torch.isnan(xh).all()
    # the off lanes among lanes with a bank: the same block, the same untouched state
    st = tuple(a.clone() for a in st0)
    ob, xh, z, nis = IMM.step(rows_d, os_d, SEED, 4, 2, _dev(trk, gpu), _dev(sw, gpu), 0.0,
                              IC.T_STEP, LEAD, DT, hp, *st)
    off = torch.as_tensor(~(trk != 0).any(axis=(2, 3)), device=gpu)
    assert int(off.sum()) >= 30
    assert _beq(ob[off], want[off]) and all(_beq(a[off], b[off]) for a, b in zip(st, st0))
    assert torch.isnan(nis[off]).all() and torch.isnan(xh[off]).all()


# ---------------------------------------------------------------------------
# 3. split batch, lane independence, bad lanes, recovery
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def snapshots():
    rows, man, _, _ = TC.case(12, 22)
    return [MNM.state(rows, man, t) for t, _ in IC.times()[:3]]


def _run(snaps, osense, trk, sw, gpu, hp=10, lo=0, hi=None, rows_edit=None):
    B, nO, M = trk[lo:hi].shape[:3]
    st = IMM.alloc(B, nO, M, gpu)
    os_d, trk_d, sw_d = _dev(osense[lo:hi], gpu), _dev(trk[lo:hi], gpu), _dev(sw[lo:hi], gpu)
    out = []
    for s, ((t, since), snap) in enumerate(zip(IC.times(), snaps)):
        snap = snap if rows_edit is None else rows_edit(snap.copy())
        ob, xh, z, nis = IMM.step(_dev(snap[lo:hi], gpu), os_d, SEED, s, lo, trk_d, sw_d, 0.0, since,
                                  LEAD, DT, hp, *st)
        out.append((st[0].clone(), st[1].clone(), st[2].clone(), xh, nis, ob, z))
    return out


N_OUT = 7
Z = 6                              # the index of the measurement among the outputs


@pytest.mark.parametrize("M", [2, 3])
def test_a_split_batch_gives_what_the_whole_gives(gpu, snapshots, M):
    _, _, osense, trk, sw = IC.case(12, 22, M)
    whole = _run(snapshots, osense, trk, sw, gpu)
    a = _run(snapshots, osense, trk, sw, gpu, lo=0, hi=5)
    b = _run(snapshots, osense, trk, sw, gpu, lo=5, hi=12)
    for s, w in enumerate(whole):
        for k in range(N_OUT):
            assert _beq(w[k], torch.cat([a[s][k], b[s][k]])), (s, k)


def _good_last_lane(M):
    _, _, osense, trk, sw = IC.case(12, 22, M)
    trk[-1, -1] = IC.widen(np.array([[[0.05, 0.01, 0.1, 0.01, 0.005, 0.02, 0.02, 1.0, 0.5, 3.0, 1.0,
                                       6.0, 2.0, 1.0]]]), M)[0, 0]
    osense[-1, -1] = [0.05, 0.01, 0.1]
    sw[-1, -1, 0] = 1.0 / M
    sw[-1, -1, 1:] = np.where(np.eye(M), 0.75, 0.25 / (M - 1))
    return osense, trk, sw


def test_changing_the_last_lanes_sw_changes_only_that_lane(gpu, snapshots):
    M = 3
    osense, trk, sw = _good_last_lane(M)
    base = _run(snapshots, osense, trk, sw, gpu)
    other = sw.copy()
    other[-1, -1, 1:] = np.where(np.eye(M), 0.5, 0.25)
    got = _run(snapshots, osense, trk, other, gpu)
    for s in range(len(base)):
        for k in range(N_OUT):
            w, g = base[s][k].flatten(0, 1), got[s][k].flatten(0, 1)
            assert _beq(w[:-1], g[:-1]), (s, k)
        assert _beq(base[s][Z], got[s][Z])                  # the measurement does not read sw
    assert not _beq(base[-1][2][-1, -1], got[-1][2][-1, -1])
    assert not _beq(base[-1][5][-1, -1], got[-1][5][-1, -1])


BAD = [("trk", (0, 0), math.nan), ("trk", (1, 7), math.inf), ("trk", (2, 13), -1e-300),
       ("trk", (1, 2), 0.0), ("trk", (2, slice(None)), 0.0), ("sw", (1, 0), -1e-3),
       ("sw", (0, 2), math.nan), ("sw", (3, 1), math.inf), ("sw", (0, 0), 1.0 / 3 + 1e-6),
       ("sw", (2, 2), 0.75 + 1e-6)]


def test_every_kind_of_bad_lane_is_nan_in_its_own_lane_only(gpu, snapshots):
    M = 3
    osense, trk, sw = _good_last_lane(M)
    base = _run(snapshots, osense, trk, sw, gpu)
    assert all(torch.isfinite(base[-1][k][-1, -1]).all() for k in range(N_OUT))

    def only_the_last_lane_is_nan(got, what, z_nan):
        for s in range(len(base)):
            for k in range(N_OUT):
                w, g = base[s][k].flatten(0, 1), got[s][k].flatten(0, 1)
                assert _beq(w[:-1], g[:-1]), (what, s, k)
                if k != Z or z_nan:
                    assert torch.isnan(g[-1]).all(), (what, s, k)
                else:
                    assert _beq(w[-1], g[-1]), (what, s, k)

    for which, idx, val in BAD:
        t, s_ = trk.copy(), sw.copy()
        (t if which == "trk" else s_)[(-1, -1) + idx] = val
        assert IM.is_bad_lane(t[-1, -1], s_[-1, -1]) and not IM.is_off_lane(t[-1, -1])
        only_the_last_lane_is_nan(_run(snapshots, osense, t, s_, gpu), (which, idx), False)
    # a bad obstacle row and a bad osense row: the same, and no measurement
    for f, val in ((OM.LENGTH, -1.0), (OM.X, math.nan)):
        def edit(snap, f=f, val=val):
            snap[-1, -1, f] = val
            return snap
        only_the_last_lane_is_nan(_run(snapshots, osense, trk, sw, gpu, rows_edit=edit), ("rows", f),
                                  True)
    bad = osense.copy()
    bad[-1, -1, 0] = -0.1
    only_the_last_lane_is_nan(_run(snapshots, bad, trk, sw, gpu), "osense", True)


def test_a_lane_turned_nan_recovers_on_the_next_call(gpu):
    B, nO, hp = 2, 3, 5
    rows, man, osense, _ = TC.case(B, nO)
    snaps = [_dev(MNM.state(rows, man, t), gpu) for t in (0.0, 0.4, 0.8)]
    os_d = _dev(osense, gpu)
    trk, sw = IMM.bank(os_d)
    M = trk.shape[2]
    st = IMM.alloc(B, nO, M, gpu)
    IMM.step(snaps[0], os_d, SEED, 0, 0, trk, sw, 0.0, 0.0, LEAD, DT, hp, *st)
    good = tuple(a.clone() for a in st)
    assert _beq(st[2], sw[:, :, 0])                          # mu = mu0 after the initialisation
    st[1][1, 2, 1] = -torch.eye(6, dtype=torch.float64, device=gpu)    # no Cholesky in one mode
    st[0][0, 1, 2, 3] = math.inf                             # a non-finite prediction in one mode
    st[2][1, 0, 0] = math.nan                                # a probability that is not finite
    st[2][0, 2] = 0.0                                        # no mode with c > 0
    lost = ((1, 2), (0, 1), (1, 0), (0, 2))
    ob, xh, z, nis = IMM.step(snaps[1], os_d, SEED, 1, 0, trk, sw, 0.0, 0.4, LEAD, DT, hp, *st)
    for b, o in lost:
        assert all(torch.isnan(a[b, o]).all() for a in st) and torch.isnan(nis[b, o]).all()
        assert torch.isnan(ob[b, o]).all() and torch.isnan(xh[b, o]).all()
        assert torch.isfinite(z[b, o]).all()
    ref = tuple(a.clone() for a in good)
    ob_r, xh_r, z_r, nis_r = IMM.step(snaps[1], os_d, SEED, 1, 0, trk, sw, 0.0, 0.4, LEAD, DT, hp, *ref)
    keep = torch.ones((B, nO), dtype=torch.bool, device=gpu)
    for b, o in lost:
        keep[b, o] = False
    assert all(_beq(a[keep], r[keep]) for a, r in zip(st, ref))
    assert _beq(nis[keep], nis_r[keep]) and _beq(ob[keep], ob_r[keep]) and _beq(z, z_r)
    # the next call initialises the lanes again
    ob, xh, z, nis = IMM.step(snaps[2], os_d, SEED, 2, 0, trk, sw, 0.0, 0.4, LEAD, DT, hp, *st)
    for b, o in lost:
        for j in range(M):
            assert _beq(st[0][b, o, j, :4], z[b, o]) and (st[0][b, o, j, 4:] == 0).all()
        assert _beq(st[2][b, o], sw[b, o, 0]) and torch.isnan(nis[b, o]).all()
        assert torch.isfinite(ob[b, o]).all() and torch.isfinite(st[1][b, o]).all()
    assert torch.isfinite(nis[keep]).all()


# ---------------------------------------------------------------------------
# 4. the reductions to the single filter, on the device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", IC.REDUCTIONS)
def test_the_device_bank_reduces_to_the_single_filter(gpu, kind):
    B, nO, hp = 12, 22, 10
    rows, man, osense, trk14, trk, sw = IC.reduction_case(B, nO, kind)
    M = trk.shape[2]
    rows_d, man_d, os_d, t14, trk_d, sw_d = (_dev(a, gpu) for a in (rows, man, osense, trk14, trk, sw))
    st = IMM.alloc(B, nO, M, gpu)
    x1, c1 = TRKA.alloc(B, nO, gpu)
    worst = 0.0
    for s, (t, since) in enumerate(IC.times()):
        snap = MAN.state(rows_d, man_d, t)
        ob, xh, z, nis = IMM.step(snap, os_d, SEED, s, 3, trk_d, sw_d, 0.0, since, LEAD, DT, hp, *st)
        ob1, z1, nis1 = TRKA.step(snap, os_d, SEED, s, 3, t14, 0.0, since, LEAD, DT, hp, x1, c1)
        assert _beq(z, z1)                                   # the same measurement, bitwise
        worst = max(worst, IC.reduction_ratio((_np(xh), _np(st[1]), _np(nis), _np(ob)),
                                              (_np(x1), _np(c1), _np(nis1), _np(ob1))))
    print(f"{kind}: device bank against tracker_accel.step {worst:.3e} (RED_TOL {IC.RED_TOL:.3e})")
    if kind != "identical":
        assert worst == 0.0
    assert worst <= IC.RED_TOL


# ---------------------------------------------------------------------------
# 5. mode response: the host test's inputs and its condition on the device
# ---------------------------------------------------------------------------
def test_the_bank_believes_straight_while_cruising_and_brake_after_the_onset(gpu):
    rows, man, osense = IC.response_inputs()
    trk, sw, names = IC.response_bank(osense)
    rows_d, man_d, os_d, trk_d, sw_d = (_dev(a, gpu) for a in (rows, man, osense, trk, sw))
    st = IMM.alloc(IC.RESP_B, IC.RESP_NO, len(names), gpu)
    means = []
    for s in range(IC.RESP_CRUISE + IC.RESP_BRAKE):
        snap = MAN.state(rows_d, man_d, s * IC.RESP_T)
        IMM.step(snap, os_d, IC.RESP_SEED, s, 0, trk_d, sw_d, 0.0, 0.0 if s == 0 else IC.RESP_T,
                 IC.RESP_LEAD, IC.RESP_DT, IC.RESP_HP, *st)
        means.append(_np(st[2].mean(dim=(0, 1))))
    means = np.array(means)
    cruising, first = IC.response_verdict(means, names)
    print("batch mean of mu per call (straight, arc, brake):\n", np.round(means, 4))
    assert cruising and first is not None and first <= IC.RESP_K


# ---------------------------------------------------------------------------
# 6. rollout: frog, 1 vehicle, 22 obstacles braking at 3 m/s^2, Hp 10, B = 4, 6 steps, an
#    exact sensor
# ---------------------------------------------------------------------------
STEPS = TC.FROG_STEPS
KEYS = ("x0", "u0", "umax", "U", "traj", "n_scp", "status", "path", "u_tick", "obst", "obst_state")
IMM_KEYS = ("obst_est", "obst_mu", "obst_nis", "obst_meas")


def _x_init(sc, B):
    rng = np.random.default_rng(12)
    return np.array(sc.x0, float)[None] + rng.standard_normal((B, sc.nVeh, 6)) * np.array(
        [0.05, 0.05, 0.005, 0.02, 0.0, 0.002])


def _snapshot(cl):
    return types.SimpleNamespace(
        hist=[{k: h[k].clone() for k in KEYS + IMM_KEYS if k in h} for h in cl.history],
        metrics=cl.metrics(), control=cl.control.clone())


@pytest.fixture(scope="module")
def rollouts(gpu):
    from scpqp.rollout import ClosedLoopBatch
    sc = R.frog_scenario(Hp=10)
    B, nO = 4, sc.nObst
    x_init = _x_init(sc, B)
    rows, brake = TC.frog_inputs(sc, B)
    exact = np.zeros((B, nO, 3))
    bank = tuple(a.numpy() for a in IMM.bank(exact, device="cpu"))
    M = bank[0].shape[2]
    trka = TRKA.matched(exact, device="cpu").numpy()
    trk5 = TRK.matched(exact, device="cpu").numpy()
    cl = ClosedLoopBatch(sc, B, device=gpu, keep_path=True, metrics=True)
    runs = {}
    for name, kw in (("plain", {}), ("none", dict(imm=None)),
                     ("off", dict(imm=(np.zeros((B, nO, M, 14)), np.zeros((B, nO, M + 1, M))))),
                     ("off_dev", dict(imm=IMM.off(B, nO, M, gpu))),
                     ("trk5", dict(tracker=trk5)), ("trka", dict(tracker_accel=trka)),
                     ("imm", dict(imm=tuple(_dev(a, gpu) for a in bank)))):
        cl.reset(x_init, seed=1, obstacles=rows, manoeuvres=brake, **kw)
        cl.run(STEPS)
        runs[name] = _snapshot(cl)
    half = ClosedLoopBatch(sc, 2, device=gpu, keep_path=True, metrics=True)
    for o in (0, 2):
        half.reset(x_init[o:o + 2], seed=1, b_offset=o, obstacles=rows[o:o + 2],
                   manoeuvres=brake[o:o + 2], imm=tuple(a[o:o + 2] for a in bank))
        half.run(STEPS)
        runs[f"half{o}"] = _snapshot(half)
    half.close()
    torch.cuda.synchronize()
    yield types.SimpleNamespace(sc=sc, cl=cl, B=B, M=M, x_init=x_init, rows=rows, brake=brake,
                                bank=bank, trka=trka, trk5=trk5, runs=runs)
    cl.close()


@pytest.mark.parametrize("same", ["none", "off", "off_dev"])
def test_rollout_without_the_bank_is_the_rollout_of_before(rollouts, same):
    a, b = rollouts.runs["plain"], rollouts.runs[same]
    assert len(a.hist) == len(b.hist) == STEPS
    for i in range(STEPS):
        assert a.hist[i].keys() == b.hist[i].keys()
        assert not any(k in b.hist[i] for k in IMM_KEYS) and "obst_state" in b.hist[i]
        for k in a.hist[i]:
            if a.hist[i][k].dtype == torch.float64:
                assert _beq(a.hist[i][k], b.hist[i][k]), (i, k)
            else:
                assert _eq(a.hist[i][k], b.hist[i][k]), (i, k)
    assert _beq(a.control, b.control)
    for k, v in a.metrics.items():
        assert _eq(v, b.metrics[k]), k


def test_rollout_records_what_step_gives(rollouts, gpu):
    ro, sc = rollouts, rollouts.sc
    rows, man = _dev(ro.rows, gpu), _dev(ro.brake, gpu)
    trk, sw = (_dev(a, gpu) for a in ro.bank)
    st = IMM.alloc(ro.B, sc.nObst, ro.M, gpu)
    lead = sc.delay_x + sc.dt + sc.delay_u
    g0 = 0
    for i, rec in enumerate(ro.runs["imm"].hist):
        g1 = max(0, i * sc.ticks_per_sim - sc.ticks_delay_x)
        snap = MAN.state(rows, man, g1 * sc.tick_length)
        ob, xh, z, nis = IMM.step(snap, None, 0, i, 0, trk, sw, 0.0, (g1 - g0) * sc.tick_length,
                                  lead, sc.dt, sc.Hp, *st)
        g0 = g1
        assert _beq(rec["obst_state"], snap), i
        assert _beq(rec["obst"], ob) and _beq(rec["obst_est"], xh), i
        assert _beq(rec["obst_nis"], nis) and _beq(rec["obst_meas"], z), i
        assert _beq(rec["obst_mu"], st[2]), i
        assert tuple(rec["obst_est"].shape) == (ro.B, sc.nObst, 6)
        assert tuple(rec["obst_mu"].shape) == tuple(rec["obst_nis"].shape) == (ro.B, sc.nObst, ro.M)
    last = ro.runs["imm"].hist[-1]
    assert torch.isfinite(last["obst_nis"]).all() and torch.isfinite(last["obst_mu"]).all()
    assert not _beq(last["obst"], ro.runs["trka"].hist[-1]["obst"])
    assert not _beq(last["obst"], ro.runs["plain"].hist[-1]["obst"])


def test_rollout_with_the_bank_does_not_depend_on_the_sharding(rollouts):
    ro = rollouts
    for i, whole in enumerate(ro.runs["imm"].hist):
        for k in KEYS + IMM_KEYS:
            parts = torch.cat([ro.runs["half0"].hist[i][k], ro.runs["half2"].hist[i][k]])
            if whole[k].dtype == torch.float64:
                assert _beq(whole[k], parts), (i, k)
            else:
                assert _eq(whole[k], parts), (i, k)
    for k, v in ro.runs["imm"].metrics.items():
        assert _eq(v, torch.cat([ro.runs["half0"].metrics[k], ro.runs["half2"].metrics[k]])), k


def test_reset_refuses_the_bank_with_a_tracker_and_bad_banks_before_anything_is_launched(rollouts):
    ro, cl = rollouts, rollouts.cl
    cl.reset(ro.x_init, seed=1, obstacles=ro.rows, manoeuvres=ro.brake, imm=ro.bank)
    cl.run(1)
    n_hist, i = len(cl.history), cl.i
    state = cl.state.clone()
    rows_before = tuple(a.clone() for a in cl.imm_rows)
    st_before = tuple(a.clone() for a in cl.imm_state)
    trk, sw = ro.bank
    with pytest.raises(ValueError, match="one of tracker=, tracker_accel= and imm="):
        cl.reset(ro.x_init, seed=1, obstacles=ro.rows, tracker=ro.trk5, imm=ro.bank)
    with pytest.raises(ValueError, match="one of tracker=, tracker_accel= and imm="):
        cl.reset(ro.x_init, seed=1, obstacles=ro.rows, tracker_accel=ro.trka, imm=ro.bank)
    with pytest.raises(ValueError, match="imm needs obstacles= rows"):
        cl.reset(ro.x_init, seed=1, imm=ro.bank)
    neg, nosum, mixed = sw.copy(), sw.copy(), trk.copy()
    neg[2, 1, 1, 0] = -0.1
    nosum[1, 0, 0, 0] += 1e-6
    mixed[0, 3, 1] = 0.0
    for bad in ((trk[:2], sw[:2]), (trk[:, :1], sw[:, :1]), (trk, sw[:, :, :3]), (trk, neg),
                (trk, torch.as_tensor(nosum)), (mixed, sw), trk, (trk,)):
        with pytest.raises(ValueError):
            cl.reset(ro.x_init, seed=1, obstacles=ro.rows, imm=bad)
    with pytest.raises(ValueError, match=r"sw\[2, 1, 1, 0\] must be finite and >= 0"):
        cl.reset(ro.x_init, seed=1, obstacles=ro.rows, imm=(trk, neg))
    assert len(cl.history) == n_hist and cl.i == i           # the refused resets changed nothing
    assert _eq(cl.state, state) and cl.trk_rows is None and cl.trka_rows is None
    assert all(_beq(a, b) for a, b in zip(cl.imm_rows, rows_before))
    assert all(_beq(a, b) for a, b in zip(cl.imm_state, st_before))


def test_the_prediction_error_against_braking_obstacles_is_reported(rollouts, gpu):
    ro, sc = rollouts, rollouts.sc
    rows, man = _dev(ro.rows, gpu), _dev(ro.brake, gpu)
    tps, tdx, tdu, Hp = sc.ticks_per_sim, sc.ticks_delay_x, sc.ticks_delay_u, sc.Hp
    ahead = [(k + 1) * tps + tdx + tps + tdu for k in range(Hp)]       # tau_k in ticks
    err = {}
    for name in ("plain", "trk5", "trka", "imm"):
        total = 0.0
        for i in range(3, STEPS):
            g1 = max(0, i * tps - tdx)
            true = MAN.pose(rows, man, sc.tick_length, g1, ahead[-1])[:, :, ahead, 0:2]
            d = ro.runs[name].hist[i]["obst"].transpose(2, 3) - true   # [B, nO, Hp, 2]
            total += float(d.norm(dim=-1).sum().item())
        err[name] = total
    print("summed prediction error from step 3 on: " + ", ".join(
        f"{k} {v:.2f} m" for k, v in err.items()))
    assert all(math.isfinite(v) for v in err.values())
    mu = ro.runs["imm"].hist[-1]["obst_mu"].mean(dim=(0, 1))
    print("batch mean of mu at the last step (straight, arc, brake):", _np(mu).round(4))
