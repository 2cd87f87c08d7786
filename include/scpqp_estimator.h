/*
 * scpqp_estimator.h — state estimator: an extended Kalman filter per (realisation,
 * vehicle) between the sensor and the planner of closed-loop rollouts
 * (csrc/estimator.hip).
 *
 * With a sensing truth (scpqp_sensing.h) the controller's measurement is noisy and a
 * lost one is replaced by a held one that is a whole MPC step old.  The estimator is
 * what a vehicle would run between its sensor and its planner: it predicts with the
 * controller's own nominal model and the commands the controller itself issued, and
 * corrects with every measurement that arrives.  Its tuning is a row per lane, so a
 * tuning sweep runs in one batch.
 *
 * Filtered states.  The SCPQP_EST_NS = 5 states (0, 1, 2, 3, 5) of Model.py:72: x, y,
 * heading, speed, steering angle; below they are numbered 0..4 in that order.  State 4
 * of the model, the acceleration, is passed through from the measurement exactly, as
 * the sensor passes it; the right-hand side uses it as an input.
 *
 * Rows.  est[B][n_veh][SCPQP_EST_NP], SCPQP_EST_NP = 8 doubles:
 *
 *   index        unit         meaning
 *   0 R_POS      m            assumed sigma of the x and of the y measurement
 *   1 R_HEADING  rad          assumed sigma of the heading measurement
 *   2 R_SPEED    m/s          assumed sigma of the speed measurement
 *   3 R_STEER    rad          assumed sigma of the steering measurement
 *   4 Q_POS      m/sqrt(s)    process-noise density on x and on y
 *   5 Q_HEADING  rad/sqrt(s)  the same on the heading
 *   6 Q_SPEED    m/s/sqrt(s)  the same on the speed
 *   7 Q_STEER    rad/sqrt(s)  the same on the steering angle
 *
 *   R = diag(R_POS^2, R_POS^2, R_HEADING^2, R_SPEED^2, R_STEER^2)
 *   Q = diag(Q_POS^2, Q_POS^2, Q_HEADING^2, Q_SPEED^2, Q_STEER^2)
 *
 * Off row: all eight fields exactly 0 (a -0.0 compares equal).  The lane copies the
 * six doubles of the measurement to x_est[b][v] bit for bit, leaves cov[b][v] alone
 * and writes nis = NaN: there is no filter.
 *
 * Bad row: any field non-finite or negative, or a row that is not off with some
 * R_* = 0.  The lane writes NaN to x_est[b][v], cov[b][v] and nis.  It touches
 * nothing of any other lane and the call returns 0.
 *
 * State carried between steps (in/out, caller-owned):
 *
 *   x_est [B][n_veh][6]     the estimate, all six model states.  The caller fills it
 *                           with NaN before the first step: x_est[b][v][0] being NaN
 *                           means "not initialised".
 *   cov   [B][n_veh][5][5]  P, symmetric.  Only its upper triangle is read; both
 *                           triangles are written.
 *
 * One call per MPC step, scpqp_est_step.  u_span[b][v][j], j < n_span, is the command
 * that acted over tick j of the span since the previous call; x_meas[b][v] is this
 * step's measurement m; delivered[b][v] (int32, the array may be NULL: every
 * measurement was delivered) says whether it arrived.  Per lane, with T = tick:
 *
 * 1. Predict.  Skipped when the lane is not initialised.  For j = 0 .. n_span - 1:
 *      A = the analytic Jacobian of Model.py:46-52 at the current estimate, restricted
 *          to the five states.  Its nine nonzeros, with rho = lr / (lf + lr),
 *          t = tan(x[5]), kap = sqrt(rho^2 t^2 + 1), th = x[2] + atan(rho t), v = x[3]:
 *            A02 = -v sin(th) kap    A03 = cos(th) kap
 *            A04 = rho^2 v cos(th) t (t^2 + 1) / kap - rho v sin(th) (t^2 + 1) / kap
 *            A12 =  v cos(th) kap    A13 = sin(th) kap
 *            A14 = rho v cos(th) (t^2 + 1) / kap + rho^2 v sin(th) t (t^2 + 1) / kap
 *            A23 = t / (lf + lr)     A24 = v (t^2 + 1) / (lf + lr)     A44 = -10
 *      F = I + T A + (T^2 / 2) A A
 *      x <- the nominal flow of plant.hip over T with the command u_span[j]:
 *           steps_for(T, h_max) RK4 steps of the nominal vehicle (p->lf, p->lr, steering
 *           lag 0.1 s), no noise; all six states, so x[4] stays what it was
 *      P <- F P F' + T Q, then P <- (P + P') / 2
 * 2. A measurement counts when delivered is NULL or delivered[b][v] = 1, and all six
 *    of its doubles are finite.  Otherwise it is lost: the estimate is the prediction
 *    and nis = NaN.
 * 3. Initialise, on the first measurement that counts of a lane that is not
 *    initialised: x_est = m (six doubles), P = R, nis = NaN.  A lane that is neither
 *    initialised nor measured stays NaN.
 * 4. Update (H = I), in this order:
 *      y = m - x on the five states.  The heading innovation is not wrapped: the sensor
 *          adds its noise without wrapping and paths are continuous.
 *      S = P + R = L L' by Cholesky
 *      nis = y' S^-1 y
 *      x  += P S^-1 y
 *      P  <- P - P S^-1 P, then P <- (P + P') / 2
 *      x[4] of the model = m[4]
 * 5. Trouble in a lane.  A Cholesky pivot <= 0 or not finite, or a non-finite result
 *    (estimate, P or nis), turns that lane's x_est, cov and nis to NaN.  The lane then
 *    initialises itself again on its next measurement that counts.  Numerical trouble
 *    never aborts a batch.
 *
 * What the filter does not know.  It does not know the sensor's LAG, BIAS_HEADING or
 * SCALE_SPEED (scpqp_sensing.h): it treats every delivered measurement as the unbiased
 * state at the measurement tick.  Those remain unmodelled errors of the estimate, as
 * they are of the raw measurement.  There is no sampler: a tuning is chosen, not drawn.
 *
 * Conventions of scpqp_sensing.h: device pointers, asynchronous on `stream`, 0 or a
 * negative SCPQP_E_* code with the message in scpqp_last_error().  Every argument is
 * validated on the host before any HIP call.  B = 0 is a no-op (the arrays may then
 * be NULL).
 */
#ifndef SCPQP_ESTIMATOR_H
#define SCPQP_ESTIMATOR_H

#include "scpqp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCPQP_EST_NS 5
#define SCPQP_EST_NP 8
#define SCPQP_EST_R_POS 0
#define SCPQP_EST_R_HEADING 1
#define SCPQP_EST_R_SPEED 2
#define SCPQP_EST_R_STEER 3
#define SCPQP_EST_Q_POS 4
#define SCPQP_EST_Q_HEADING 5
#define SCPQP_EST_Q_SPEED 6
#define SCPQP_EST_Q_STEER 7

/* One filter step of every lane, as described above.  p as scpqp_plant_step's (n_veh in
 * 1..SCPQP_MAX_VEH, lf + lr > 0); B >= 0; n_span >= 0; tick and h_max finite and > 0.
 * B * n_veh * 25 and B * n_veh * n_span must fit int32 (SCPQP_E_SIZE).  At B > 0, x_meas,
 * est, x_est and cov must be non-NULL, and u_span if n_span > 0; delivered and nis may be
 * NULL. */
int scpqp_est_step(const scpqp_plant_params* p, int32_t B, int32_t n_span, double tick,
                   double h_max, const double* u_span, const double* x_meas,
                   const int32_t* delivered, const double* est, double* x_est, double* cov,
                   double* nis, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCPQP_ESTIMATOR_H */
