/*
 * scpqp_truth.h — plant truth: per-realisation model mismatch of the plant step.
 *
 * The controller plans with the scenario's nominal bicycle model: the delay
 * compensation ("MPC_init is part of the controller", main.py:121-123), the
 * linearisation, the QP, the dynamic steering limit (main.py:105-109) and the
 * clipping all read scenario.Lf / Lr and the steering lag 0.1 s of Model.py:83.
 * The plant that realises the path (main.py:184-191) need not be that vehicle.
 * A truth gives every (realisation, vehicle) its own plant parameters, read by
 * scpqp_plant_step_truth only; nothing the controller computes sees them.
 *
 * A truth row holds SCPQP_TRUTH_NP = 5 doubles: truth[B][n_veh][SCPQP_TRUTH_NP].
 *
 *   index  field                      nominal          enters Model.ode (Model.py:61-87) as
 *   0 LF   lf                         scenario.Lf[v]   L = lf + lr, R = lr / L
 *   1 LR   lr                         scenario.Lr[v]   same
 *   2 TAU  steering lag, s            0.1              dx[5] = (u_eff - x[5]) / tau
 *   3 GAIN steering gain              1                u_eff = gain * u_ref + bias
 *   4 BIAS steering offset, rad       0                same
 *
 * The lane of (b, v, k) (one output tick k of the plant step, as in scpqp.h):
 *
 *   - u_eff is formed once, before the integration (the command of a lane is
 *     constant over it), as  __dadd_rn(__dmul_rn(gain, u_ref), bias):  two
 *     roundings, no fused multiply-add.  The right-hand side is otherwise the
 *     nominal one, with tau dividing where 0.1 does.
 *   - The number of RK4 steps stays steps_for(k * tick, h_max): a truth never
 *     changes it, so a seeded lane draws exactly the counters it draws without.
 *   - The nominal row (Lf[v], Lr[v], 0.1, 1, 0) gives bitwise what
 *     scpqp_plant_step / scpqp_plant_step_noisy give.
 *   - A bad row, !(lf + lr > 0) or !(tau > 0) (NaN included), writes NaN to all
 *     six states of every output tick k of its (b, v), k = 0 included, and
 *     integrates nothing.  No other lane is affected and the call returns 0:
 *     numerical trouble never aborts a batch.
 *
 * Accuracy: the fixed-step RK4's distance from the exact flow grows with
 * h_max / tau ("Plant truth").  At h_max = 2.5 ms it is 8.4e-11 at
 * the nominal tau = 0.1, 2.0e-10 at 0.08, 1.9e-9 at 0.04 and 4.7e-8 at 0.02;
 * scpqp.truth.validate refuses tau < 8 h_max, and a caller who wants the
 * nominal 1e-10 keeps h_max <= tau / 40.
 *
 * Sampler.  scpqp_truth_sample draws field f of (b, v) from ONE Philox4x32-10
 * call (generator, key and the u1 / u2 / Box-Muller mapping of scpqp_noise.h):
 *
 *   key      (seed & 0xffffffff, seed >> 32)
 *   counter  c0 = f   c1 = 0   c2 = (SCPQP_NOISE_SITE_TRUTH << 24) | v
 *            c3 = b_offset + b
 *
 * Site 3 is disjoint from the sites 0..2 of scpqp_noise.h, so a truth seed
 * equal to the noise seed shares no counter with the noise.  With u1 in (0, 1]
 * and u2 in [0, 1):
 *
 *   FIXED    mean[f][v] exactly (spread, lo, hi ignored; no draw)
 *   UNIFORM  xi = 2 u2 - 1                       exact in fp64, in [-1, 1)
 *   NORMAL   xi = sqrt(-2 ln u1) cos(2 pi u2)
 *   value    fmin(fmax(__dadd_rn(mean, __dmul_rn(spread, xi)), lo), hi)
 *
 * c3 is the global realisation index, so a batch sharded over calls or ranks
 * (b_offset = first realisation of the call) samples what one call would.
 */
#ifndef SCPQP_TRUTH_H
#define SCPQP_TRUTH_H

#include "scpqp_noise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCPQP_TRUTH_NP 5
#define SCPQP_TRUTH_LF 0
#define SCPQP_TRUTH_LR 1
#define SCPQP_TRUTH_TAU 2
#define SCPQP_TRUTH_GAIN 3
#define SCPQP_TRUTH_BIAS 4

#define SCPQP_TRUTH_TAU_NOMINAL 0.1   /* Model.py:83 */

#define SCPQP_NOISE_SITE_TRUTH 3

#define SCPQP_TRUTH_FIXED 0
#define SCPQP_TRUTH_UNIFORM 1
#define SCPQP_TRUTH_NORMAL 2

typedef struct scpqp_truth_field {
    int32_t kind;        /* SCPQP_TRUTH_FIXED / UNIFORM / NORMAL          */
    int32_t pad0;
    double  spread;      /* half width (UNIFORM) or sigma (NORMAL); >= 0  */
    double  lo, hi;      /* clamp of the drawn value; lo <= hi            */
} scpqp_truth_field;

typedef struct scpqp_truth_dist {
    int32_t  n_veh;
    int32_t  pad0;
    double   mean[SCPQP_TRUTH_NP][SCPQP_MAX_VEH];
    scpqp_truth_field field[SCPQP_TRUTH_NP];
    uint64_t seed;
    uint32_t b_offset;   /* c3 = b_offset + b */
    uint32_t pad1;
} scpqp_truth_dist;

/* scpqp_plant_step / scpqp_plant_step_noisy with a truth row per (b, v).
 * truth [B][n_veh][SCPQP_TRUTH_NP] must be non-NULL (callers without one use the
 * existing entry points); p supplies n_veh only.  noise (constant pair,
 * [B][n_veh][2]) and nz (per-evaluation draws, site 1) may each be NULL; both
 * non-NULL is SCPQP_E_ARG.  With nz, n_ticks >= 65536 returns SCPQP_E_SIZE. */
int scpqp_plant_step_truth(const scpqp_plant_params* p, int32_t B, int32_t n_ticks, double tick,
                           const double* x_start, const double* u_tick, const double* truth,
                           const double* noise, const scpqp_noise* nz,
                           double* x_path, double h_max, void* stream);

/* truth[b][v] = (p->lf[v], p->lr[v], 0.1, 1, 0) */
int scpqp_truth_fill_nominal(const scpqp_plant_params* p, int32_t B, double* truth, void* stream);

/* truth[b][v][f] drawn as described above.  SCPQP_E_ARG (the message names the
 * field) unless: n_veh in 1..SCPQP_MAX_VEH; every kind in range; every spread
 * finite and >= 0; lo <= hi; and, with floor(f, v) = mean[f][v] of a FIXED field
 * and lo otherwise, floor(LF, v) + floor(LR, v) > 0 and floor(TAU, v) > 0 for
 * every vehicle: the sampler never emits a row the plant would NaN. */
int scpqp_truth_sample(const scpqp_truth_dist* d, int32_t B, double* truth, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCPQP_TRUTH_H */
