/*
 * scpqp_manoeuvres.h — obstacle manoeuvres: braking, accelerating and turning obstacles
 * of closed-loop rollouts (csrc/manoeuvres.hip, csrc/metrics.hip).
 *
 * A row of scpqp_obstacles.h moves its obstacle at constant speed and constant turn
 * rate for the whole rollout.  A manoeuvre schedule gives every (realisation, obstacle)
 * up to SCPQP_MAN_NSEG = 4 pieces of constant acceleration and constant turn-rate offset
 * on top of the row: a lead obstacle that brakes, one that stops, one that changes lane.
 * The world (the realised-path metrics, the plotted obstacle path) follows the schedule;
 * the controller knows nothing of it: at each MPC step it measures the true pose and the
 * true current speed, as it does of a row.
 *
 * A schedule holds SCPQP_MAN_NSEG * SCPQP_MAN_NF = 12 doubles per lane:
 * man[B][n_obst][SCPQP_MAN_NSEG][SCPQP_MAN_NF].
 *
 *   index    field                                 off
 *   0 DUR    duration of the piece, s, >= 0        0
 *   1 ACCEL  acceleration during the piece, m/s^2  0
 *   2 DYAW   turn-rate offset during it, rad/s     0
 *
 * The pieces follow each other from t = 0; piece i starts at t_i = DUR_0 + ... + DUR_(i-1)
 * (summed in this order, skipped pieces left out).  A piece with DUR == 0 is skipped.
 * During a piece the acceleration is ACCEL and the turn rate is the row's YAW_RATE + DYAW.
 * After the last piece the obstacle keeps the speed it has reached, with acceleration 0
 * and the row's YAW_RATE.
 *
 * Off lane: every piece has DUR == 0 or (ACCEL == 0 and DYAW == 0).  The all-zero block
 * is off, and so is a NULL `man`.  An off lane is the row's own motion: it is evaluated by
 * the pose of scpqp_obstacles.h and by nothing else.
 *
 * One piece starts at (x, y, h, s) with acceleration a and turn rate w.  Over a time tau
 * let T = min(tau, tau_stop), tau_stop = s / (-a) for a < 0, 0 for a == 0 and s == 0,
 * and infinity otherwise; theta = w T, A = theta / 2:
 *
 *   x += s T sinc(A) cos(h + A) + a T^2 (p(theta) cos h - r(theta) sin h)
 *   y += s T sinc(A) sin(h + A) + a T^2 (p(theta) sin h + r(theta) cos h)
 *   h += theta
 *   s += a T      (exactly 0 once T == tau_stop)
 *
 *   p(theta) = (cos theta + theta sin theta - 1) / theta^2
 *            = sum_k (-1)^k theta^(2k)     (2k + 1) / (2k + 2)!      -> 1/2
 *   r(theta) = (sin theta - theta cos theta) / theta^2
 *            = sum_k (-1)^k theta^(2k + 1) (2k + 2) / (2k + 3)!      -> theta / 3
 *
 * (the integral of (s + a tau)(cos, sin)(h + w tau)).  sinc is that of scpqp_obstacles.h
 * with its switch at 1e-4.  p and r take the six-term series (through theta^10 and
 * theta^11) below |theta| = SCPQP_MAN_PR_SWITCH = 0.1 and the closed forms at and above
 * it: the series is within 4e-16 relative there, the closed forms within 5e-14 relative
 * on [0.1, 0.5], and the two differ by less than 4e-14 at the switch.  The a T^2 term is
 * left out when a == 0.0 exactly (it is a zero).
 *
 * Stopped obstacles.  While the speed is 0 the obstacle stands and its heading does not
 * change: for the rest of a braking piece and through later pieces with ACCEL <= 0.  A
 * later piece with ACCEL > 0 starts it again from 0.
 *
 * No rounding order beyond this is promised (scpqp_obstacles.h): the device contracts
 * a * b + c where it can and its sincos is within an ulp.  The time of global tick g is
 * g * tick_length (one rounding), and the time into a piece is t - t_i (one rounding).
 *
 * Snapshot row (scpqp_manoeuvres_state).  The state of a lane at t as a row of
 * scpqp_obstacles.h: X, Y, HEADING and SPEED at t, LENGTH and WIDTH copied, YAW_RATE the
 * turn rate in effect at t (at a boundary the later piece's, while stopped 0; an off
 * lane: the row's).  The pose of a row at t = 0 is its X, Y and HEADING exactly, so
 * scpqp_obstacles_predict, scpqp_obstacles_predict_sensed and scpqp_obstacles_track,
 * called with the snapshot and t_meas = 0, measure the manoeuvring obstacle with their
 * own kernels, draws and counters.
 *
 * Bad lane: a non-finite field, DUR < 0, a schedule that is not off on a row with
 * SPEED < 0, or a bad row (scpqp_obstacles.h).
 *   - state writes NaN to that lane's [SCPQP_OBST_NP] block, pose to its
 *     [n_ticks + 1][3] block; no other output is touched.
 *   - the metrics leave a realisation with any bad lane untouched (its poses are NaN).
 *   - the calls return 0.
 *
 * Sampler.  scpqp_manoeuvres_sample draws field f of piece i of (b, o) from ONE
 * Philox4x32-10 call (key and FIXED / UNIFORM / NORMAL mapping of scpqp_obstacles.h):
 *
 *   counter  c0 = 3 i + f   c1 = 0   c2 = (SCPQP_NOISE_SITE_MANOEUVRE << 24) | o
 *            c3 = b_offset + b
 *   value    fmin(fmax(__dadd_rn(mean, __dmul_rn(spread, xi)), lo), hi)
 *
 * Site 8 is disjoint from the sites 0..7.  One scpqp_truth_field and one mean per
 * (piece, field), shared by the obstacles.
 *
 * Conventions of scpqp.h: device pointers, asynchronous on `stream`, 0 or a negative
 * SCPQP_E_* code with the message in scpqp_last_error().  Every argument is validated on
 * the host before any HIP call.  B = 0 is a no-op (the arrays may then be NULL).
 */
#ifndef SCPQP_MANOEUVRES_H
#define SCPQP_MANOEUVRES_H

#include "scpqp_obstacles.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCPQP_MAN_NSEG 4
#define SCPQP_MAN_NF 3
#define SCPQP_MAN_DUR 0
#define SCPQP_MAN_ACCEL 1
#define SCPQP_MAN_DYAW 2
#define SCPQP_MAN_PR_SWITCH 0.1

#define SCPQP_NOISE_SITE_MANOEUVRE 8

typedef struct scpqp_manoeuvres_dist {
    int32_t  n_obst;     /* 1..SCPQP_MAX_OBST */
    int32_t  pad0;
    double   mean[SCPQP_MAN_NSEG][SCPQP_MAN_NF];
    scpqp_truth_field field[SCPQP_MAN_NSEG][SCPQP_MAN_NF];
    uint64_t seed;
    uint32_t b_offset;   /* c3 = b_offset + b */
    uint32_t pad1;
} scpqp_manoeuvres_dist;

/* state_out [B][n_obst][SCPQP_OBST_NP]: the snapshot row of every lane at time t (finite,
 * >= 0).  rows [B][n_obst][SCPQP_OBST_NP]; man [B][n_obst][SCPQP_MAN_NSEG][SCPQP_MAN_NF] or
 * NULL (every lane off).  B * n_obst * 12 must fit int32 (SCPQP_E_SIZE). */
int scpqp_manoeuvres_state(int32_t B, int32_t n_obst, const double* rows, const double* man,
                           double t, double* state_out, void* stream);

/* pose_out [B][n_obst][n_ticks + 1][3] in the layout and with the tick times of
 * scpqp_obstacles_pose, which is launched into pose_out first; the lanes that are not off
 * then overwrite their blocks, so an off lane is bitwise scpqp_obstacles_pose's. */
int scpqp_manoeuvres_pose(int32_t B, int32_t n_obst, const double* rows, const double* man,
                          double tick_length, int32_t tick0, int32_t n_ticks, double* pose_out,
                          void* stream);

/* man_out[b][o][i][f] drawn as described above.  SCPQP_E_ARG (the message names the piece
 * and the field) unless: n_obst in 1..SCPQP_MAX_OBST; every kind in range; every spread
 * finite and >= 0; lo <= hi; every mean finite; and no DUR can come out negative: lo >= 0
 * where DUR is not FIXED, mean >= 0 where it is. */
int scpqp_manoeuvres_sample(const scpqp_manoeuvres_dist* d, int32_t B, double* man_out,
                            void* stream);

/* scpqp_metrics_accumulate_obstacles with obstacle o of realisation b at
 * pose[b][o][k][0..2] (x, y, heading), k = 0..n_ticks: scpqp_manoeuvres_pose's output for the
 * same tick0 and n_ticks.  The half extents are LENGTH / 2, WIDTH / 2 of rows[b][o].  A
 * realisation with a bad row or a non-finite pose entry is left untouched.  rows and pose
 * must be non-NULL once B > 0. */
int scpqp_metrics_accumulate_posed(scpqp_metrics* m, int32_t B, int32_t n_ticks, int32_t tick0,
                                   int32_t k_first, const double* x_path,
                                   const scpqp_metrics_acc* acc, const scpqp_metrics_dense* dense,
                                   const int32_t* variant, const double* rows, const double* pose,
                                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCPQP_MANOEUVRES_H */
