/*
 * scpqp_tracker.h — obstacle tracker: an extended Kalman filter per (realisation,
 * obstacle) between the obstacle sensing and the obstacle prediction of closed-loop
 * rollouts (csrc/tracker.hip).
 *
 * With an obstacle truth (scpqp_obstacles.h) every obstacle turns at its own constant
 * rate, and with an obstacle sensing (scpqp_sensing.h) the controller measures its pose
 * and speed with noise.  scpqp_obstacles_predict extrapolates the measured pose on a
 * straight line and never sees the turn rate; scpqp_obstacles_predict_sensed extrapolates
 * one noisy measurement, so the heading noise times the horizon times the speed lands in
 * the constraint rows of the QP.  The tracker is what a vehicle would run between its
 * obstacle sensor and its planner: it filters the measurements of every obstacle on the
 * constant-turn-rate-and-speed model the obstacle truth itself uses, estimates the turn
 * rate, and writes the controller's obst [B][n_obst][2][hp] from its estimate on the arc.
 * Its tuning is a row per lane, so a tuning sweep runs in one batch.
 *
 * State.  SCPQP_TRK_NS = 5: x, y, heading, speed, turn rate w, numbered 0..4.
 *
 * Measurement.  z = (xm, ym, hm, sm), H = [I4 | 0]: exactly the measurement
 * scpqp_obstacles_predict_sensed forms.  With (x, y, h) the true pose of rows[b][o] at
 * t_meas (pose_at of csrc/scpqp_obstacle_pose.h) and s the row's speed:
 *
 *   xm = x + SIG_POS * z0(c0 = 0)       ym = y + SIG_POS * z1(c0 = 0)
 *   hm = h + SIG_HEADING * z0(c0 = 1)   sm = s + SIG_SPEED * z1(c0 = 1)
 *   counter  c1 = epoch   c2 = (SCPQP_NOISE_SITE_SENSE_OBST << 24) | o   c3 = b_offset + b
 *
 * every product and every sum its own rounding, the draws mapped as scpqp_sensing.h maps
 * them.  No new Philox site is introduced: the tracker sees the draws the untracked
 * prediction of the same step would have seen.  With osense == NULL (then st may be NULL
 * too), or an all-zero osense row, the sensor is exact, z = (x, y, h, s), and nothing is
 * drawn.
 *
 * Rows.  trk[B][n_obst][SCPQP_TRK_NP], SCPQP_TRK_NP = 9 doubles:
 *
 *   index        unit            meaning
 *   0 R_POS      m               assumed sigma of the x and of the y measurement
 *   1 R_HEADING  rad             assumed sigma of the heading measurement
 *   2 R_SPEED    m/s             assumed sigma of the speed measurement
 *   3 Q_POS      m/sqrt(s)       process-noise density on x and on y
 *   4 Q_HEADING  rad/sqrt(s)     the same on the heading
 *   5 Q_SPEED    m/s/sqrt(s)     the same on the speed
 *   6 Q_YAW      rad/s/sqrt(s)   the same on the turn rate
 *   7 P0_YAW     rad/s           sigma of the turn rate at initialisation
 *   8 W_CLAMP    rad/s           the prediction uses w clamped to +-W_CLAMP; 0 gives a
 *                                straight prediction from the filtered pose
 *
 *   R = diag(R_POS^2, R_POS^2, R_HEADING^2, R_SPEED^2)
 *   Q = diag(Q_POS^2, Q_POS^2, Q_HEADING^2, Q_SPEED^2, Q_YAW^2)
 *
 * State carried between steps (in/out, caller-owned):
 *
 *   x_trk [B][n_obst][5]     the estimate.  The caller fills it with NaN before the first
 *                            step: x_trk[b][o][0] being NaN means "not initialised".
 *   cov   [B][n_obst][5][5]  P, symmetric.  Only its upper triangle is read; both
 *                            triangles are written.
 *
 * One call per MPC step, scpqp_obstacles_track.  T = t_since >= 0 is the time since the
 * previous call's measurement, a scalar, the same for every lane.  Per lane:
 *
 * 1. Predict.  Skipped when the lane is not initialised.  With a = 0.5 w T, c = s T and
 *    g = sinc(a) as in scpqp_obstacles.h (switch 1e-4):
 *      F = the unit diagonal plus, evaluated at the estimate before the flow,
 *        F02 = -c g sin(h + a)   F03 = T g cos(h + a)
 *        F04 = c (T / 2) (g' cos(h + a) - g sin(h + a))
 *        F12 =  c g cos(h + a)   F13 = T g sin(h + a)
 *        F14 = c (T / 2) (g' sin(h + a) + g cos(h + a))
 *        F24 = T
 *      g'(a) = -a / 3 + a^3 / 30 - a^5 / 840   for |a| < SCPQP_TRK_DSINC_SWITCH = 0.02
 *              (a cos a - sin a) / a^2           otherwise
 *        (the series' next term a^7 / 45360 is 1e-15 relative to a / 3 at the switch,
 *        and the cancellation of the closed form there costs about ulp / a^2 = 3e-13
 *        relative: both branches agree with an 80-bit evaluation to 3e-12 relative
 *        anywhere between 0.01 and 0.05)
 *      x <- pose_at((x, y, h, s, ., ., w), T): the shared device function, its w == 0
 *           branch included; h <- h + w T; s and w are kept
 *      P <- F P F' + T Q, then P <- (P + P') / 2
 * 2. Initialise, on a lane that is not initialised: x = (z, 0),
 *    P = diag(R_POS^2, R_POS^2, R_HEADING^2, R_SPEED^2, P0_YAW^2), nis = NaN.
 * 3. Update, otherwise, in this order:
 *      y = z - x[0:4].  The heading innovation is not wrapped: the sensor adds its noise
 *          without wrapping and the heading of a row is continuous (scpqp_estimator.h).
 *      S = P[0:4, 0:4] + R = L L' by Cholesky
 *      nis = y' S^-1 y
 *      x  += P[:, 0:4] S^-1 y
 *      P  <- P - P[:, 0:4] S^-1 P[0:4, :], then P <- (P + P') / 2
 * 4. Predict the horizon.  With wc = min(max(w, -W_CLAMP), W_CLAMP) and
 *    tau_k = (k + 1) * dt + lead:
 *      obst[b][o][0 / 1][k] = x, y of pose_at((x, y, h, s, ., ., wc), tau_k)
 * 5. Trouble in a lane.  A Cholesky pivot <= 0 or not finite, a non-finite result
 *    (estimate, P or nis), a bad obstacle row or a bad osense row (the rules of
 *    scpqp_obstacles.h and scpqp_sensing.h) turn that lane's x_trk, cov and nis to NaN and
 *    its [2][hp] block to NaN.  The lane initialises itself again on the next call.
 *    Numerical trouble never aborts a batch: the call returns 0.
 *
 * Off row: all nine fields exactly 0 (a -0.0 compares equal).  There is no filter: the
 * lane's obst block is bitwise what scpqp_obstacles_predict writes when osense is NULL,
 * and bitwise what scpqp_obstacles_predict_sensed writes otherwise (the entry point
 * launches that very kernel into obst_out first, and the tracker's kernel skips the off
 * lanes).  x_trk[b][o] and cov[b][o] are left alone and nis = NaN.
 *
 * Bad row: any field non-finite or negative, or a row that is not off with some R_* = 0.
 * P0_YAW = 0 and W_CLAMP = 0 are legal.  The lane writes NaN to its x_trk, cov, nis and
 * obst block.  It touches nothing of any other lane and the call returns 0.
 *
 * Measurement output.  z_out [B][n_obst][4] (may be NULL) receives the measurement of
 * every lane whose obstacle row and osense row are good, the off lanes and the lanes with
 * a bad tracker row included; the other lanes receive NaN.
 *
 * What the tracker does not know.  The footprint (LENGTH, WIDTH: the dsafe tables stay
 * the controller's knowledge), an acceleration, and a turn rate that changes faster than
 * Q_YAW allows.  There is no sampler: a tuning is chosen, not drawn.
 *
 * Conventions of scpqp_sensing.h: device pointers, asynchronous on `stream`, 0 or a
 * negative SCPQP_E_* code with the message in scpqp_last_error().  Every argument is
 * validated on the host before any HIP call.  B = 0 is a no-op (the arrays may then be
 * NULL).
 */
#ifndef SCPQP_TRACKER_H
#define SCPQP_TRACKER_H

#include "scpqp_sensing.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCPQP_TRK_NS 5
#define SCPQP_TRK_NZ 4
#define SCPQP_TRK_NP 9
#define SCPQP_TRK_R_POS 0
#define SCPQP_TRK_R_HEADING 1
#define SCPQP_TRK_R_SPEED 2
#define SCPQP_TRK_Q_POS 3
#define SCPQP_TRK_Q_HEADING 4
#define SCPQP_TRK_Q_SPEED 5
#define SCPQP_TRK_Q_YAW 6
#define SCPQP_TRK_P0_YAW 7
#define SCPQP_TRK_W_CLAMP 8

#define SCPQP_TRK_DSINC_SWITCH 0.02

/* One tracker step of every lane, as described above.  rows [B][n_obst][SCPQP_OBST_NP],
 * osense [B][n_obst][SCPQP_OSENSE_NP] or NULL, trk [B][n_obst][SCPQP_TRK_NP].  Sizes and
 * t_meas, lead, dt as scpqp_obstacles_predict; t_since finite and >= 0.  B * n_obst * 25
 * and B * n_obst * 2 * hp must fit int32 (SCPQP_E_SIZE).  At B > 0, rows, trk, x_trk, cov
 * and obst_out must be non-NULL, and st if osense is given; z_out and nis may be NULL. */
int scpqp_obstacles_track(int32_t B, int32_t n_obst, int32_t hp, const double* rows,
                          const double* osense, const scpqp_sense_stream* st, const double* trk,
                          double t_meas, double t_since, double lead, double dt,
                          double* x_trk, double* cov, double* z_out, double* nis,
                          double* obst_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCPQP_TRACKER_H */
