/*
 * scpqp_noise.h — the reference's per-evaluation plant noise on the device.
 *
 * With Simulation(..., isNoise) the reference's BicyleModel adds a fresh
 * N(0, sigma^2) draw (sigma = 3e-6) to dx[0] and to dx[1] on EVERY evaluation
 * of the right-hand side (Model.py:84-86, :112-114): in the delay compensation
 * (MPC_Iter.py:24-33), in the plant integration (main.py:185-190) and in the
 * one ode call of comp_jacobian (Model.py:58; the solver's ec_noise input).
 * The entry points below draw that noise inside the integrators from a
 * counter-based generator, so a noisy Monte-Carlo batch costs one seed, is
 * reproducible, and does not depend on how the batch is split over calls,
 * streams or GPUs.
 *
 * Generator: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random
 * numbers: as easy as 1, 2, 3", SC'11), multipliers 0xD2511F53 / 0xCD9E8D57,
 * key increments 0x9E3779B9 / 0xBB67AE85, ten rounds.  One call yields four
 * 32-bit words w0..w3 and from them the two draws of one right-hand-side
 * evaluation:
 *
 *   u1 = (((w0 << 32 | w1) >> 11) + 1) * 2^-53        in (0, 1]
 *   u2 =  ((w2 << 32 | w3) >> 11)      * 2^-53        in [0, 1)
 *   r  = sqrt(-2 ln u1)
 *   noise of dx[0] = sigma * r * cos(2 pi u2)
 *   noise of dx[1] = sigma * r * sin(2 pi u2)
 *
 * Key      (seed & 0xffffffff, seed >> 32)
 * Counter  c0  index of the right-hand-side evaluation within the lane's
 *              integration, 0, 1, 2, ... in call order: k1, k2, k3, k4 of the
 *              first RK4 step, then the next step, and so on.  The delay
 *              compensation keeps counting across its n_out - 1 spans.
 *          c1  epoch: the MPC step index, supplied by the caller
 *          c2  (site << 24) | (k << 8) | v
 *                site  0 delay compensation, 1 plant step, 2 linearisation draw
 *                k     the plant step's output tick (0 at the other sites)
 *                v     the vehicle
 *          c3  b_offset + b: the global realisation index (a rank that holds
 *              realisations [r * per_rank, (r + 1) * per_rank) passes
 *              b_offset = r * per_rank)
 *
 * A quirk kept on purpose: the plant step integrates every output tick k from
 * t0 again, in a lane of its own, because main.py:188-190 does.  In the
 * reference each of those restarts consumes fresh draws of the global
 * generator, so here each k has its own noise stream (k is part of c2).  The
 * state carried into the next MPC step is the k = n_ticks lane's.
 *
 * The integration is fixed-step RK4 (scpqp.h), four draws per step; the
 * reference's own draw count follows scipy's adaptive step control and is not
 * reproduced.
 */
#ifndef SCPQP_NOISE_H
#define SCPQP_NOISE_H

#include "scpqp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCPQP_NOISE_SITE_DELAY 0
#define SCPQP_NOISE_SITE_PLANT 1
#define SCPQP_NOISE_SITE_LINEARIZE 2
#define SCPQP_NOISE_MAX_TICKS 65536   /* k takes 16 bits of c2 */

typedef struct scpqp_noise {
    uint64_t seed;
    double   sigma;      /* 3e-6 in the reference (Model.py:85-86); >= 0, finite */
    uint32_t epoch;      /* c1: the MPC step index                               */
    uint32_t b_offset;   /* c3 = b_offset + b                                    */
} scpqp_noise;

/* scpqp_delay_compensate with the noise drawn per right-hand-side evaluation
 * (site 0); states 2..5 are those of scpqp_delay_compensate with noise = NULL. */
int scpqp_delay_compensate_noisy(const scpqp_plant_params* p, int32_t B, double horizon,
                                 int32_t n_out, const double* x_meas, const double* u_hold,
                                 const scpqp_noise* nz, double* x0_out, double* traj_out,
                                 double h_max, void* stream);

/* scpqp_plant_step with the noise drawn per right-hand-side evaluation (site 1,
 * one stream per output tick k).  n_ticks >= 65536 returns SCPQP_E_SIZE. */
int scpqp_plant_step_noisy(const scpqp_plant_params* p, int32_t B, int32_t n_ticks, double tick,
                           const double* x_start, const double* u_tick, const scpqp_noise* nz,
                           double* x_path, double h_max, void* stream);

/* Raw draws: out[B][n_veh][n_eval][2] = sigma * (z0, z1) for c0 = 0..n_eval-1 at
 * (site, k).  site = 2, k = 0, n_eval = 1 is the [B][n_veh][2] ec_noise input of
 * scpqp_solve, scpqp_linearize and scpqp_evaluate. */
int scpqp_noise_fill(const scpqp_noise* nz, int32_t B, int32_t n_veh, int32_t site, int32_t k,
                     int32_t n_eval, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCPQP_NOISE_H */
