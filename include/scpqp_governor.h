/*
 * scpqp_governor.h — speed governor: a longitudinal command per (realisation, vehicle) of
 * closed-loop rollouts, taken from the planner's own plan (csrc/governor.hip).
 *
 * The planner steers.  Model.py:81-82 gives the vehicle an acceleration state that nothing
 * commands (dx[4] = 0), and a vehicle that steers by at most 3 degrees cannot go round what
 * stops in its lane.  The governor is the longitudinal half: when the plan the solve returned
 * comes closer to an obstacle or to another vehicle than it is allowed to, the vehicle brakes;
 * when the way is clear it returns to its cruise speed.  The solver is not changed: the
 * linearisation carries x0[4], so the prediction, the delay compensation and the reference
 * sampler see a decelerating vehicle as it is.  Its tuning is a row per lane, so a tuning
 * sweep runs in one batch.
 *
 * Rows.  gov[B][n_veh][SCPQP_GOV_NP], SCPQP_GOV_NP = 7 doubles:
 *
 *   index      unit    meaning
 *   0 V_REF    m/s     cruise speed
 *   1 A_ACC    m/s^2   largest acceleration
 *   2 A_BRAKE  m/s^2   largest deceleration (a magnitude)
 *   3 K_V      1/s     gain of the speed loop
 *   4 J_MAX    m/s^3   largest change of the command per second of hold time; +inf: no slew
 *                      limit
 *   5 LOOK     steps   how many plan steps are examined (an integer-valued double)
 *   6 BAND     m       clearance demanded on top of the required distance
 *
 * One call per MPC step, after the solve, scpqp_governor_step.  Inputs:
 *
 *   x0          [B][n_veh][6]          the state the plan starts from (the output of the
 *                                      delay compensation); s = x0[3], a_now = x0[4]
 *   traj        [B][hp_b][2][n_veh]    scpqp_batch_out.traj, as the solve wrote it
 *   obst        [B][n_obst][2][hp_b]   scpqp_batch_in.obst, as the solve was given it
 *   obst_margin [B][n_obst][hp_b]      the array of scpqp_solve_margin, or NULL (= 0)
 *   hp          [B]                    scpqp_batch_in.hp, or NULL (= hp_max)
 *   dreq_obs    [B][n_veh][n_obst]     the required centre distance to every obstacle
 *   dreq_veh    [B][n_veh][n_veh]      and to every other vehicle (the diagonal is not read)
 *
 * The slots are those of the solve: hp_max * 2 * n_veh doubles of traj, n_obst * 2 * hp_max of
 * obst and n_obst * hp_max of obst_margin per problem, with the problem's own horizon hp_b as
 * the packed prefix.  obst and dreq_obs may be NULL when n_obst = 0.  The governor needs
 * neither a handle nor a variant table: the caller gathers the required distances.
 * t_hold > 0 is the time the command stays in force: the MPC step dt.  t_back >= 0 is how long
 * after the moment the command takes effect the plan's start lies: the control transport delay.
 *
 * Outputs: a_cmd [B][n_veh] the commanded acceleration; k_conf [B][n_veh] (int32) the first
 * conflicting step; clear [B][n_veh] the smallest clearance found.  k_conf and clear may be
 * NULL.
 *
 * Per lane (b, v):
 *
 * 1. Clearance.  For every step k < min(LOOK, hp_b), with p_v(k) = traj[b][k][0..1][v]:
 *      for every obstacle o:
 *        c = |p_v(k) - obst[b][o][.][k]| - ((dreq_obs[b][v][o] + obst_margin[b][o][k]) + BAND)
 *      for every other vehicle w != v:
 *        c = |p_v(k) - p_w(k)| - (dreq_veh[b][v][w] + BAND)
 *    with |d| = sqrt(dx dx + dy dy).  clear is the minimum of all c, +inf when nothing was
 *    examined (LOOK = 0, or one vehicle and no obstacle).  k_conf is the smallest k that holds
 *    a c < 0, else -1.  A non-finite entry of traj, obst, obst_margin or dreq_* among the
 *    examined ones counts as a conflict at that step, with c = -inf, and so does a c that is
 *    not a number: a plan that is not a number is not a clear road.  Entries of steps at or
 *    past min(LOOK, hp_b) are never read.
 * 2. Wish.  If k_conf >= 0: a_des = -A_BRAKE.  Otherwise
 *      a_des = min(max(K_V (V_REF - s), -A_BRAKE), A_ACC).
 * 3. Slew.  a_cmd = min(max(a_des, a_now - J_MAX t_hold), a_now + J_MAX t_hold); skipped when
 *    J_MAX is +inf.
 * 4. Stop rule, last, so it may break the slew limit:
 *      s_app = max(s - a_now t_back, 0)     the speed at the moment the command takes effect
 *                                           under the nominal model
 *      a_cmd = max(a_cmd, -s_app / t_hold)  the vehicle is never told to reverse
 *    Speed is linear in time under a constant acceleration, so a command held for t_hold ends
 *    at a speed s_app + a_cmd t_hold >= 0, up to rounding.
 * 5. Off row: all seven fields exactly 0 (a -0.0 compares equal).  a_cmd = a_now bit for bit,
 *    k_conf = -1, clear = NaN: there is no governor, and nothing else of the lane is read.
 * 6. Bad lane: a field negative, or non-finite other than J_MAX = +inf; LOOK not an integer or
 *    above SCPQP_MAX_HP; s or a_now non-finite; a horizon hp[b] outside 1..hp_max.  The lane
 *    writes a_cmd = NaN, k_conf = -2, clear = NaN, touches nothing of any other lane, and the
 *    call returns 0.  An off row is off whatever its state holds.
 *
 * The minima are free of order, so k_conf and clear do not depend on how the device maps the
 * (step, other) pairs to its threads.
 *
 * What the governor does not know.  It uses the plan's points only: not the footprints, not
 * the obstacles' speeds, no time to collision.  Both vehicles of a conflicting pair brake:
 * there is no right of way, so a ring of vehicles can stop one another.  It brakes fully or not
 * at all on a conflict: there is no stop-before-the-conflict profile.  It has no hysteresis
 * beyond the slew limit.  The longitudinal actuator has neither a lag nor a truth row.  The
 * reference points are spaced by the current speed (stepSize = speed dt), so a braking
 * vehicle's tracking cost is not the cruising one's.  There are no rows per variant and no
 * sampler: a tuning is chosen, not drawn.
 *
 * Conventions of scpqp_sensing.h: device pointers, asynchronous on `stream`, 0 or a negative
 * SCPQP_E_* code with the message in scpqp_last_error().  Every argument is validated on the
 * host before any HIP call.  B = 0 is a no-op (the arrays may then be NULL).
 */
#ifndef SCPQP_GOVERNOR_H
#define SCPQP_GOVERNOR_H

#include "scpqp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCPQP_GOV_NP 7
#define SCPQP_GOV_V_REF 0
#define SCPQP_GOV_A_ACC 1
#define SCPQP_GOV_A_BRAKE 2
#define SCPQP_GOV_K_V 3
#define SCPQP_GOV_J_MAX 4
#define SCPQP_GOV_LOOK 5
#define SCPQP_GOV_BAND 6

/* One governor step of every lane, as described above.  1 <= n_veh <= SCPQP_MAX_VEH,
 * 0 <= n_obst <= SCPQP_MAX_OBST, 1 <= hp_max <= SCPQP_MAX_HP, B >= 0; t_hold finite and > 0,
 * t_back finite and >= 0.  B * n_veh * 2 * hp_max, B * n_obst * 2 * hp_max and
 * B * n_veh * max(n_veh, n_obst, SCPQP_GOV_NP) must fit int32 (SCPQP_E_SIZE).  At B > 0, x0,
 * traj, dreq_veh, gov and a_cmd must be non-NULL, and obst and dreq_obs if n_obst > 0;
 * obst_margin, hp, k_conf and clear may be NULL. */
int scpqp_governor_step(int32_t n_veh, int32_t n_obst, int32_t hp_max, int32_t B, double t_hold,
                        double t_back, const double* x0, const double* traj, const double* obst,
                        const double* obst_margin, const int32_t* hp, const double* dreq_obs,
                        const double* dreq_veh, const double* gov, double* a_cmd,
                        int32_t* k_conf, double* clear, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCPQP_GOVERNOR_H */
