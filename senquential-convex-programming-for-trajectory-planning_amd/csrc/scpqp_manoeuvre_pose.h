// scpqp_manoeuvre_pose.h — the state of one manoeuvring obstacle at time t, the off rule
// and the bad rule (device side of include/scpqp_manoeuvres.h, which fixes the formulas),
// for manoeuvres.hip.
#ifndef SCPQP_MANOEUVRE_POSE_H
#define SCPQP_MANOEUVRE_POSE_H

#include <hip/hip_runtime.h>

#include <math.h>

#include "scpqp_manoeuvres.h"
#include "scpqp_obstacle_pose.h"

namespace scpqp_man_dev {

constexpr int NSEG = SCPQP_MAN_NSEG;
constexpr int NF = SCPQP_MAN_NF;

struct State {
    double x, y, h, s, w;   // position, heading, speed, the turn rate in effect
};

// a non-finite field or DUR < 0 (the row's part of the bad rule is the caller's)
__device__ __forceinline__ bool bad_schedule(const double* __restrict__ m) {
    bool bad = false;
#pragma unroll
    for (int i = 0; i < NSEG * NF; ++i) bad |= !isfinite(m[i]);
#pragma unroll
    for (int i = 0; i < NSEG; ++i) bad |= m[i * NF + SCPQP_MAN_DUR] < 0.0;
    return bad;
}

// every piece has DUR == 0 or (ACCEL == 0 and DYAW == 0); of a schedule that is not bad
__device__ __forceinline__ bool off_schedule(const double* __restrict__ m) {
    bool off = true;
#pragma unroll
    for (int i = 0; i < NSEG; ++i)
        off &= m[i * NF + SCPQP_MAN_DUR] == 0.0 ||
               (m[i * NF + SCPQP_MAN_ACCEL] == 0.0 && m[i * NF + SCPQP_MAN_DYAW] == 0.0);
    return off;
}

__device__ __forceinline__ double p_of(double th) {
    const double t2 = th * th;
    if (fabs(th) < SCPQP_MAN_PR_SWITCH)
        return 1.0 / 2.0 - t2 * (1.0 / 8.0 - t2 * (1.0 / 144.0 - t2 * (1.0 / 5760.0 -
               t2 * (1.0 / 403200.0 - t2 * (1.0 / 43545600.0)))));
    double sn, cs;
    sincos(th, &sn, &cs);
    return (cs + th * sn - 1.0) / t2;
}

__device__ __forceinline__ double r_of(double th) {
    const double t2 = th * th;
    if (fabs(th) < SCPQP_MAN_PR_SWITCH)
        return th * (1.0 / 3.0 - t2 * (1.0 / 30.0 - t2 * (1.0 / 840.0 - t2 * (1.0 / 45360.0 -
               t2 * (1.0 / 3991680.0 - t2 * (1.0 / 518918400.0))))));
    double sn, cs;
    sincos(th, &sn, &cs);
    return (sn - th * cs) / t2;
}

// one piece of acceleration a and turn rate w over tau >= 0, from a speed q.s >= 0
__device__ __forceinline__ void advance(State& q, double a, double w, double tau) {
    const double stop = a < 0.0 ? q.s / -a : (a == 0.0 && q.s == 0.0 ? 0.0 : INFINITY);
    const bool stops = tau >= stop;
    const double T = stops ? stop : tau;
    const double th = w * T, A = 0.5 * th;
    const double sinc = fabs(A) < 1e-4 ? 1.0 - A * A / 6.0 : sin(A) / A;
    double sa, ca;
    sincos(q.h + A, &sa, &ca);
    const double chord = (q.s * T) * sinc;
    double dx = chord * ca, dy = chord * sa;
    if (a != 0.0) {
        double sh, ch;
        sincos(q.h, &sh, &ch);
        const double p = p_of(th), r = r_of(th), aT2 = a * (T * T);
        dx += aT2 * (p * ch - r * sh);
        dy += aT2 * (p * sh + r * ch);
    }
    q.x += dx;
    q.y += dy;
    q.h += th;
    q.s = stops ? 0.0 : fmax(q.s + a * T, 0.0);
    // while stopped the turn rate in effect is 0; a piece that accelerates turns from its start
    q.w = q.s == 0.0 && a <= 0.0 ? 0.0 : w;
}

// the state at t >= 0 of a row (not bad, SPEED >= 0) under a schedule (not bad): a walk over
// the pieces that have begun at t, then the coast after the last one
__device__ __forceinline__ State state_at(const double* __restrict__ r, const double* __restrict__ m,
                                          double t) {
    State q{r[SCPQP_OBST_X], r[SCPQP_OBST_Y], r[SCPQP_OBST_HEADING], r[SCPQP_OBST_SPEED],
            r[SCPQP_OBST_YAW_RATE]};
    const double w0 = r[SCPQP_OBST_YAW_RATE];
    double ti = 0.0;   // start of the piece
    for (int i = 0; i < NSEG; ++i) {
        const double dur = m[i * NF + SCPQP_MAN_DUR];
        if (dur == 0.0) continue;
        if (t < ti) return q;
        advance(q, m[i * NF + SCPQP_MAN_ACCEL], w0 + m[i * NF + SCPQP_MAN_DYAW], fmin(t - ti, dur));
        ti += dur;
    }
    if (t >= ti) advance(q, 0.0, w0, t - ti);
    return q;
}

}  // namespace scpqp_man_dev

#endif  // SCPQP_MANOEUVRE_POSE_H
