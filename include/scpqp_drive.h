/*
 * scpqp_drive.h — drive truth: a longitudinal actuator between the governor and the plant.
 *
 * The speed governor (scpqp_governor.h) and its ranked form (scpqp_yield.h) command an
 * acceleration.  Without a drive the rollout writes that command into the plant state: the
 * vehicle decelerates at exactly the commanded rate from the first tick of the next step, on
 * any road, with no lag.  A drive gives every (realisation, vehicle) its own longitudinal
 * actuator, read by scpqp_plant_step_drive only; nothing the controller or the governor
 * computes sees it.  It is to the acceleration what scpqp_truth.h is to the steering.
 *
 * A drive row holds SCPQP_DRIVE_NP = 6 doubles: drive[B][n_veh][SCPQP_DRIVE_NP].
 *
 *   index  field   ideal  meaning
 *   0 TAU_A        0      lag of the realised acceleration, s; 0: no lag
 *   1 GAIN_A       1      a_eff = clamp(gain * a_cmd + bias)
 *   2 BIAS_A       0      m/s^2 (grade, drag, a dragging brake)
 *   3 A_MAX        +inf   largest realisable acceleration, >= 0
 *   4 B_MAX        +inf   largest realisable deceleration, a magnitude, >= 0 (the road)
 *   5 HOLD         0      1: the brakes hold the vehicle at rest and it never reverses;
 *                         0: no such rule
 *
 * a_cmd[B][n_veh] is the commanded acceleration, constant over one plant step (the command
 * changes at MPC step boundaries only).  scpqp_plant_step_drive takes the arguments of
 * scpqp_plant_step_truth plus a_cmd and drive; truth is required (callers without one pass
 * the rows of scpqp_truth_fill_nominal), and noise / nz follow the rules stated there.
 *
 * The lane of (b, v, k) is the lane of scpqp_plant_step_truth: it restarts from x_start over
 * k * tick with steps_for(k * tick, h_max) RK4 steps.  A drive row never changes the step
 * count, so a seeded lane draws exactly the counters it draws without.
 *
 *   - a_eff is formed once per lane, before the integration, as
 *       fmin(fmax(__dadd_rn(__dmul_rn(gain, a_cmd), bias), -B_MAX), A_MAX):
 *     two roundings, no fused multiply-add, as u_eff is formed.
 *   - TAU_A == 0:  x[4] = a_eff before the integration and dx[4] = 0: the right-hand side
 *     is that of the truth row.
 *   - TAU_A > 0:   x[4] starts at x_start[4], the realised acceleration, which is
 *     continuous across steps, and dx[4] = (a_eff - x[4]) / TAU_A.
 *   - HOLD == 1, in every right-hand-side evaluation: dx[3] = 0 when !(x[3] > 0) and
 *     x[4] < 0, else dx[3] = x[4]: brakes do not push a standing vehicle backwards.
 *   - HOLD == 1, after every RK4 step: a speed that was >= 0 before the step and is < 0
 *     after it is set to exactly 0.0.  (The step that crosses zero overshoots by at most
 *     h |x[4]|; the projection removes it, and from then on the gate holds the speed.)
 *   - A lane that starts below zero speed is outside the rule: the gate freezes its speed
 *     while x[4] < 0 and the projection never fires.  The rollout never produces one.
 *   - The ideal row (0, 1, 0, +inf, +inf, 0) gives bitwise what scpqp_plant_step_truth gives
 *     when x_start[4] is replaced by a_eff = __dadd_rn(__dmul_rn(1, a_cmd), 0) (a_cmd itself,
 *     but for -0.0, which becomes +0.0): noise-free, with a constant pair and seeded.
 *   - A bad row (NaN included): !(TAU_A >= 0), a non-finite GAIN_A or BIAS_A, !(A_MAX >= 0),
 *     !(B_MAX >= 0), HOLD neither 0 nor 1, or a non-finite a_cmd.  It writes NaN to all six
 *     states of every output tick k of its (b, v), k = 0 included, and integrates nothing.
 *     No other lane is affected and the call returns 0.  The bad rule of the truth row
 *     (scpqp_truth.h) stays, with the same effect.
 *
 * Accuracy.  With a lag the acceleration is a first-order response, at HOLD = 0 in closed
 * form:
 *
 *   a(t) = a_eff + (a0 - a_eff) e^(-t/tau)
 *   s(t) = s0 + a_eff t + (a0 - a_eff) tau (1 - e^(-t/tau))
 *
 * The fixed-step RK4's distance from it grows with h_max / tau, as for the steering lag.
 * Measured on the CPU mirror (tests/test_drive_host.py) at h_max = 2.5 ms, the largest over
 * ten ticks of 0.05 s, for a0 - a_eff = 4 m/s^2, as (error of a in m/s^2, of s in m/s):
 *   tau = 0.4 (160 h_max)  (1.9e-11, 7.6e-12)
 *   tau = 0.1  (40 h_max)  (4.9e-9,  4.9e-10)
 *   tau = 0.04 (16 h_max)  (2.0e-7,  7.7e-9)
 *   tau = 0.02  (8 h_max)  (1.9e-6,  3.8e-8)
 * scpqp.drive.validate refuses 0 < TAU_A < 8 h_max; a caller who wants the speed within
 * 1e-9 m/s keeps h_max <= TAU_A / 40.
 *
 * Sampler.  scpqp_drive_sample draws field f of (b, v) from ONE Philox4x32-10 call, with the
 * field kinds, the key and the u1 / u2 / Box-Muller mapping of scpqp_truth_sample:
 *
 *   counter  c0 = f   c1 = 0   c2 = (SCPQP_NOISE_SITE_DRIVE << 24) | v   c3 = b_offset + b
 *
 * Site 9 is disjoint from the sites 0..8 of the other headers, and c3 is the global
 * realisation index: a sharded batch samples what one call would.
 *
 * What it does not know
 *   - No speed-dependent drag and no tyre model: BIAS_A is a constant.
 *   - No dead time of the drive beyond the one-step compute delay of the command.
 *   - B_MAX is a constant, not a friction circle shared with the steering.
 *   - The controller, the governor's stop rule and the delay compensation assume the ideal
 *     drive: with a lag or a weak road the vehicle stops later than the governor reckons.
 *   - HOLD has no release dynamics: the brakes let go the instant x[4] >= 0.
 *   - No rows per scenario variant: a row belongs to a (realisation, vehicle).
 */
#ifndef SCPQP_DRIVE_H
#define SCPQP_DRIVE_H

#include "scpqp_truth.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCPQP_DRIVE_NP 6
#define SCPQP_DRIVE_TAU_A 0
#define SCPQP_DRIVE_GAIN_A 1
#define SCPQP_DRIVE_BIAS_A 2
#define SCPQP_DRIVE_A_MAX 3
#define SCPQP_DRIVE_B_MAX 4
#define SCPQP_DRIVE_HOLD 5

#define SCPQP_NOISE_SITE_DRIVE 9

typedef struct scpqp_drive_dist {
    int32_t  n_veh;
    int32_t  pad0;
    double   mean[SCPQP_DRIVE_NP][SCPQP_MAX_VEH];
    scpqp_truth_field field[SCPQP_DRIVE_NP];   /* kinds of scpqp_truth.h */
    uint64_t seed;
    uint32_t b_offset;   /* c3 = b_offset + b */
    uint32_t pad1;
} scpqp_drive_dist;

/* scpqp_plant_step_truth with a commanded acceleration a_cmd [B][n_veh] and a drive row
 * drive [B][n_veh][SCPQP_DRIVE_NP] per (b, v).  Every argument is checked on the host before
 * any HIP call, in the order of scpqp_plant_step_truth; then truth, a_cmd and drive must be
 * non-NULL.  B = 0 is a no-op with NULL arrays. */
int scpqp_plant_step_drive(const scpqp_plant_params* p, int32_t B, int32_t n_ticks, double tick,
                           const double* x_start, const double* u_tick, const double* truth,
                           const double* noise, const scpqp_noise* nz, const double* a_cmd,
                           const double* drive, double* x_path, double h_max, void* stream);

/* drive[b][v] = (0, 1, 0, +inf, +inf, 0) */
int scpqp_drive_fill_ideal(int32_t n_veh, int32_t B, double* drive, void* stream);

/* drive[b][v][f] drawn as described above.  SCPQP_E_ARG (the message names the field)
 * unless: n_veh in 1..SCPQP_MAX_VEH; every kind in range; HOLD is FIXED at 0 or 1; for a
 * field that is not FIXED a finite mean, a spread finite and >= 0 and lo <= hi; and, with
 * floor(f, v) = mean[f][v] of a FIXED field and lo otherwise, floor(TAU_A, v) >= 0,
 * floor(A_MAX, v) >= 0 and floor(B_MAX, v) >= 0 for every vehicle, and a GAIN_A and BIAS_A
 * that stay finite (a finite FIXED mean; otherwise lo < +inf and hi > -inf): the sampler
 * never emits a row the plant would NaN. */
int scpqp_drive_sample(const scpqp_drive_dist* d, int32_t B, double* drive, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCPQP_DRIVE_H */
