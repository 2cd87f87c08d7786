/*
 * scpqp_tracker_accel.h — obstacle tracker with an acceleration state: a six-state extended
 * Kalman filter per (realisation, obstacle) between the obstacle sensing and the obstacle
 * prediction of closed-loop rollouts (csrc/tracker_accel.hip).
 *
 * With obstacle manoeuvres (scpqp_manoeuvres.h) an obstacle brakes, accelerates and changes
 * its turn rate in pieces.  The tracker of scpqp_tracker.h runs on constant speed and turn
 * rate: it does not know a deceleration, and it carries a learnt arc over the whole horizon.
 * This tracker runs on the model the manoeuvring truth itself uses, one manoeuvre piece of
 * constant acceleration and constant turn rate with its stop rule: it estimates both, its
 * horizon prediction brakes to a stop and never reverses, and it can let go of either
 * quantity after a hold time.  scpqp_tracker.h is unchanged and stays available; a lane
 * runs one of the two.
 *
 * State.  SCPQP_TRKA_NS = 6: x, y, heading h, speed s, turn rate w, acceleration a,
 * numbered 0..5.
 *
 * Measurement.  z = (xm, ym, hm, sm), H = [I4 | 0]: exactly the measurement of
 * scpqp_tracker.h and of scpqp_obstacles_predict_sensed.  With (x, y, h) the true pose of
 * rows[b][o] at t_meas (pose_at of csrc/scpqp_obstacle_pose.h) and s the row's speed:
 *
 *   xm = x + SIG_POS * z0(c0 = 0)       ym = y + SIG_POS * z1(c0 = 0)
 *   hm = h + SIG_HEADING * z0(c0 = 1)   sm = s + SIG_SPEED * z1(c0 = 1)
 *   counter  c1 = epoch   c2 = (SCPQP_NOISE_SITE_SENSE_OBST << 24) | o   c3 = b_offset + b
 *
 * every product and every sum its own rounding, the draws mapped as scpqp_sensing.h maps
 * them.  No new Philox site is introduced: the tracker sees the draws the five-state
 * tracker and the untracked prediction of the same step would have seen.  With
 * osense == NULL (then st may be NULL too), or an all-zero osense row, the sensor is exact,
 * z = (x, y, h, s), and nothing is drawn.  A manoeuvring obstacle is measured through its
 * snapshot row at t_meas = 0 (scpqp_manoeuvres_state).
 *
 * Rows.  trk[B][n_obst][SCPQP_TRKA_NP], SCPQP_TRKA_NP = 14 doubles:
 *
 *   index         unit            meaning
 *    0 R_POS      m               assumed sigma of the x and of the y measurement
 *    1 R_HEADING  rad             assumed sigma of the heading measurement
 *    2 R_SPEED    m/s             assumed sigma of the speed measurement
 *    3 Q_POS      m/sqrt(s)       process-noise density on x and on y
 *    4 Q_HEADING  rad/sqrt(s)     the same on the heading
 *    5 Q_SPEED    m/s/sqrt(s)     the same on the speed
 *    6 Q_YAW      rad/s/sqrt(s)   the same on the turn rate
 *    7 Q_ACCEL    m/s^2/sqrt(s)   the same on the acceleration
 *    8 P0_YAW     rad/s           sigma of the turn rate at initialisation
 *    9 P0_ACCEL   m/s^2           sigma of the acceleration at initialisation
 *   10 W_CLAMP    rad/s           the prediction uses w clamped to +-W_CLAMP
 *   11 A_CLAMP    m/s^2           and a clamped to +-A_CLAMP
 *   12 W_HOLD     s               the prediction keeps the turn rate for this long
 *   13 A_HOLD     s               and the acceleration for this long
 *
 *   R = diag(R_POS^2, R_POS^2, R_HEADING^2, R_SPEED^2)
 *   Q = diag(Q_POS^2, Q_POS^2, Q_HEADING^2, Q_SPEED^2, Q_YAW^2, Q_ACCEL^2)
 *
 * State carried between steps (in/out, caller-owned):
 *
 *   x_trk [B][n_obst][6]     the estimate.  The caller fills it with NaN before the first
 *                            step: x_trk[b][o][0] being NaN means "not initialised".
 *   cov   [B][n_obst][6][6]  P, symmetric.  Only its upper triangle is read; both
 *                            triangles are written.
 *
 * One call per MPC step, scpqp_obstacles_track_accel.  T = t_since >= 0 is the time since
 * the previous call's measurement, a scalar, the same for every lane.  Per lane:
 *
 * 1. Predict.  Skipped when the lane is not initialised.  The flow is one piece of
 *    scpqp_manoeuvres.h from (x, y, h, s0), s0 = max(s, 0), with acceleration a and turn
 *    rate w over T: `advance` of csrc/scpqp_manoeuvre_pose.h itself, with its stop rule
 *      T_e = min(T, tau_stop),  tau_stop = s0 / (-a) for a < 0, 0 for a == 0 and s0 == 0,
 *            infinity otherwise.
 *    x, y and h become the piece's; s becomes the piece's end speed, s0 + a T_e, exactly 0
 *    at a stop (the heading then stands from T_e on); w and a are kept.
 *      F = the unit diagonal plus the partial derivatives of the piece's formulas at
 *      (h, s0, w, a) with T_e held fixed.  With theta = w T_e, A = theta / 2, g = sinc(A)
 *      (switch 1e-4), g' of scpqp_tracker.h (SCPQP_TRK_DSINC_SWITCH), c = s0 T_e, p, r of
 *      scpqp_manoeuvres.h and (dx, dy) the displacement of the piece, recomputed from these
 *      terms:
 *        F02 = -dy                        F12 = dx
 *        F03 = T_e g cos(h + A)           F13 = T_e g sin(h + A)
 *        F04 = c (T_e / 2) (g' cos(h + A) - g sin(h + A)) + a T_e^3 (p' cos h - r' sin h)
 *        F14 = c (T_e / 2) (g' sin(h + A) + g cos(h + A)) + a T_e^3 (p' sin h + r' cos h)
 *        F05 = T_e^2 (p cos h - r sin h)  F15 = T_e^2 (p sin h + r cos h)
 *        F24 = T_e                        F35 = T_e
 *      twelve nonzeros off the diagonal.  The a T_e^2 terms of dx, dy and the a T_e^3 terms
 *      are formed whatever a is (a == 0 makes them zeros).
 *      p'(theta) = -int_0^1 u^2 sin(theta u) du
 *                = (theta^2 cos theta - 2 theta sin theta - 2 cos theta + 2) / theta^3
 *                = -sum_k (-1)^k theta^(2k + 1) / ((2k + 1)! (2k + 4))     -> -theta / 4
 *      r'(theta) = int_0^1 u^2 cos(theta u) du
 *                = ((theta^2 - 2) sin theta + 2 theta cos theta) / theta^3
 *                = sum_k (-1)^k theta^(2k) / ((2k)! (2k + 3))              -> 1 / 3
 *      Each takes its six-term series (through theta^11 and theta^10) below
 *      |theta| = SCPQP_TRKA_DPR_SWITCH = 0.3 and its closed form at and above it.  Against
 *      an 80-bit evaluation the series are within 5e-16 relative below the switch; the
 *      closed forms cancel in the numerator, p' to about 8 ulp / theta^4 and r' to about
 *      6 ulp / theta^3: p' is within 2e-13 relative on [0.3, 4] and r' within 3e-14
 *      relative on [0.3, 2].  (r' has a zero at theta = 2.08; from 2 on its closed form is
 *      within 2e-16 absolute.)
 *      At a stop T_e is the stop time and is held fixed: F does not carry the dependence of
 *      the stop time on s and a.  The position rows lose nothing to first order (the speed
 *      at the stop is 0); the heading row lacks w / (-a) and w s0 / a^2 in the columns of s
 *      and a, and F33 = 1, F35 = T_e although the speed stands at 0.
 *      P <- F P F' + T Q (T, not T_e), then P <- (P + P') / 2
 * 2. Initialise, on a lane that is not initialised: x = (z, 0, 0),
 *    P = diag(R_POS^2, R_POS^2, R_HEADING^2, R_SPEED^2, P0_YAW^2, P0_ACCEL^2), nis = NaN.
 * 3. Update, otherwise: exactly the update of scpqp_tracker.h on the 4 x 4 S and the 6 x 4
 *    gain, in this order:
 *      y = z - x[0:4].  The heading innovation is not wrapped.
 *      S = P[0:4, 0:4] + R = L L' by Cholesky
 *      nis = y' S^-1 y
 *      x  += P[:, 0:4] S^-1 y.  The speed estimate is not clamped.
 *      P  <- P - P[:, 0:4] S^-1 P[0:4, :], then P <- (P + P') / 2
 * 4. Predict the horizon.  With wc = min(max(w, -W_CLAMP), W_CLAMP),
 *    ac = min(max(a, -A_CLAMP), A_CLAMP), t1 = min(W_HOLD, A_HOLD), t2 = max(W_HOLD, A_HOLD)
 *    the obstacle moves from q0 = (x, y, h, s0) in three pieces, each evaluated by `advance`:
 *      piece 1  (ac, wc)                      on [0, t1)
 *      piece 2  (ac, 0) when A_HOLD > W_HOLD,
 *               (0, wc) otherwise             on [t1, t2)
 *      piece 3  (0, 0)                        from t2 on
 *    The boundary states q1 = piece 1 from q0 over t1 and q2 = piece 2 from q1 over t2 - t1
 *    are formed once per lane.  With tau_k = (k + 1) * dt + lead, obst[b][o][0 / 1][k] is
 *    x, y of
 *      piece 1 from q0 over tau_k         when tau_k < t1
 *      piece 2 from q1 over tau_k - t1    when t1 <= tau_k < t2
 *      piece 3 from q2 over tau_k - t2    when t2 <= tau_k.
 *    A hold of 0 drops that quantity from the prediction (both 0: the straight line at
 *    constant speed from the filtered pose); a hold >= the last tau_k keeps it for the whole
 *    horizon.  Once the predicted speed has reached 0 the points stay where they are: the
 *    stop rule of every later piece holds them, and the prediction never moves backwards.
 * 5. Trouble in a lane.  A Cholesky pivot <= 0 or not finite, a non-finite result
 *    (estimate, P or nis), a bad obstacle row or a bad osense row (the rules of
 *    scpqp_obstacles.h and scpqp_sensing.h) turn that lane's x_trk, cov and nis to NaN and
 *    its [2][hp] block to NaN.  The lane initialises itself again on the next call.
 *    Numerical trouble never aborts a batch: the call returns 0.
 *
 * Off row: all fourteen fields exactly 0 (a -0.0 compares equal).  There is no filter: the
 * lane's obst block is bitwise what scpqp_obstacles_predict writes when osense is NULL,
 * and bitwise what scpqp_obstacles_predict_sensed writes otherwise (the entry point
 * launches that very kernel into obst_out first, and the tracker's kernel skips the off
 * lanes).  x_trk[b][o] and cov[b][o] are left alone and nis = NaN.
 *
 * Bad row: any field non-finite or negative, or a row that is not off with some R_* = 0.
 * Zeros in P0_*, *_CLAMP and *_HOLD are legal.  The lane writes NaN to its x_trk, cov, nis
 * and obst block.  It touches nothing of any other lane and the call returns 0.
 *
 * Measurement output.  z_out [B][n_obst][4] (may be NULL) receives the measurement of
 * every lane whose obstacle row and osense row are good, the off lanes and the lanes with
 * a bad tracker row included; the other lanes receive NaN.
 *
 * What the tracker does not know.  A jerk: an acceleration or a turn rate that changes
 * faster than Q_ACCEL and Q_YAW allow is followed late.  The schedule itself: when a piece
 * ends; W_HOLD and A_HOLD are a tuning, not knowledge.  The footprint (LENGTH, WIDTH: the
 * dsafe tables stay the controller's knowledge).  There is no sampler: a tuning is chosen,
 * not drawn.
 *
 * Conventions of scpqp_sensing.h: device pointers, asynchronous on `stream`, 0 or a
 * negative SCPQP_E_* code with the message in scpqp_last_error().  Every argument is
 * validated on the host before any HIP call.  B = 0 is a no-op (the arrays may then be
 * NULL).
 */
#ifndef SCPQP_TRACKER_ACCEL_H
#define SCPQP_TRACKER_ACCEL_H

#include "scpqp_manoeuvres.h"
#include "scpqp_tracker.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCPQP_TRKA_NS 6
#define SCPQP_TRKA_NZ 4
#define SCPQP_TRKA_NP 14
#define SCPQP_TRKA_R_POS 0
#define SCPQP_TRKA_R_HEADING 1
#define SCPQP_TRKA_R_SPEED 2
#define SCPQP_TRKA_Q_POS 3
#define SCPQP_TRKA_Q_HEADING 4
#define SCPQP_TRKA_Q_SPEED 5
#define SCPQP_TRKA_Q_YAW 6
#define SCPQP_TRKA_Q_ACCEL 7
#define SCPQP_TRKA_P0_YAW 8
#define SCPQP_TRKA_P0_ACCEL 9
#define SCPQP_TRKA_W_CLAMP 10
#define SCPQP_TRKA_A_CLAMP 11
#define SCPQP_TRKA_W_HOLD 12
#define SCPQP_TRKA_A_HOLD 13

#define SCPQP_TRKA_DPR_SWITCH 0.3

/* One tracker step of every lane, as described above.  rows [B][n_obst][SCPQP_OBST_NP],
 * osense [B][n_obst][SCPQP_OSENSE_NP] or NULL, trk [B][n_obst][SCPQP_TRKA_NP].  Sizes and
 * t_meas, lead, dt as scpqp_obstacles_predict; t_since finite and >= 0.  B * n_obst * 36
 * and B * n_obst * 2 * hp must fit int32 (SCPQP_E_SIZE).  At B > 0, rows, trk, x_trk, cov
 * and obst_out must be non-NULL, and st if osense is given; z_out and nis may be NULL. */
int scpqp_obstacles_track_accel(int32_t B, int32_t n_obst, int32_t hp, const double* rows,
                                const double* osense, const scpqp_sense_stream* st,
                                const double* trk, double t_meas, double t_since, double lead,
                                double dt, double* x_trk, double* cov, double* z_out,
                                double* nis, double* obst_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCPQP_TRACKER_ACCEL_H */
