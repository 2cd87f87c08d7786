// scpqp_obstacle_pose.h — the pose of one obstacle row at time t and the bad-row rule
// (device side of include/scpqp_obstacles.h, which fixes the formulas), shared by
// obstacles.hip and the obstacle-row path of metrics.hip.
#ifndef SCPQP_OBSTACLE_POSE_H
#define SCPQP_OBSTACLE_POSE_H

#include <hip/hip_runtime.h>

#include <math.h>

#include "scpqp_obstacles.h"

namespace scpqp_obst_dev {

struct Pose {
    double x, y, h, c, s;   // centre, heading, cos / sin of the heading
};

// any field non-finite, LENGTH < 0 or WIDTH < 0
__device__ __forceinline__ bool bad_row(const double* __restrict__ r) {
    bool bad = false;
#pragma unroll
    for (int f = 0; f < SCPQP_OBST_NP; ++f) bad |= !isfinite(r[f]);
    return bad || r[SCPQP_OBST_LENGTH] < 0.0 || r[SCPQP_OBST_WIDTH] < 0.0;
}

__device__ __forceinline__ Pose pose_at(const double* __restrict__ r, double t) {
    const double sp = r[SCPQP_OBST_SPEED], w = r[SCPQP_OBST_YAW_RATE];
    Pose p;
    if (w == 0.0) {
        // the straight line of scpqp_metrics.h, in its own order of operations
        p.h = r[SCPQP_OBST_HEADING];
        sincos(p.h, &p.s, &p.c);
        p.x = t * sp * p.c + r[SCPQP_OBST_X];
        p.y = t * sp * p.s + r[SCPQP_OBST_Y];
        return p;
    }
    const double a = 0.5 * w * t;
    const double sinc = fabs(a) < 1e-4 ? 1.0 - a * a / 6.0 : sin(a) / a;
    double sa, ca;
    sincos(r[SCPQP_OBST_HEADING] + a, &sa, &ca);
    const double chord = (sp * t) * sinc;
    p.x = r[SCPQP_OBST_X] + chord * ca;
    p.y = r[SCPQP_OBST_Y] + chord * sa;
    p.h = r[SCPQP_OBST_HEADING] + w * t;
    sincos(p.h, &p.s, &p.c);
    return p;
}

}  // namespace scpqp_obst_dev

#endif  // SCPQP_OBSTACLE_POSE_H
