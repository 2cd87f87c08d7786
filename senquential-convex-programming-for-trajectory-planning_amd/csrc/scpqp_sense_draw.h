// scpqp_sense_draw.h — the sensor's Philox draw and the obstacle measurement (device side of
// include/scpqp_sensing.h, which fixes the counters, the mapping and the bad rule), shared by
// sensing.hip and the trackers that measure what scpqp_obstacles_predict_sensed measures.
#ifndef SCPQP_SENSE_DRAW_H
#define SCPQP_SENSE_DRAW_H

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "scpqp_obstacle_pose.h"
#include "scpqp_philox.h"
#include "scpqp_rounding.h"
#include "scpqp_sensing.h"

namespace scpqp_sense_dev {

struct Draw {
    double z0, z1, u2;   // the normal pair and the [0, 1) uniform of one Philox call
};

// the call of counter (c0, epoch, c2, b_global), mapped as scpqp_noise.h maps it
__device__ __forceinline__ Draw draw_at(const scpqp_sense_stream& st, uint32_t c0, uint32_t c2,
                                        uint32_t b_global) {
    uint32_t c[4] = {c0, st.epoch, c2, b_global};
    scpqp_noise_dev::philox4x32_10(c, (uint32_t)st.seed, (uint32_t)(st.seed >> 32));
    double u1, u2;
    scpqp_noise_dev::uniforms(c, u1, u2);
    const double r = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincos(6.283185307179586 * u2, &sn, &cs);
    return Draw{scpqp_round_dev::mul_1r(r, cs), scpqp_round_dev::mul_1r(r, sn), u2};
}

// the measurement (x, y, heading, speed) of lane g = (b, ob) at t_meas, as
// scpqp_obstacles_predict_sensed takes it: the pose of the row, plus the two calls of the
// site-7 counter, each value its own product and its own sum.  osense null: the exact sensor.
// Returns whether the obstacle row or the osense row is bad, and then leaves zm as the caller
// handed it in (NaN).  The stream goes by value and zm is the caller's to initialise: either
// way round the trackers compile to other instructions.  predict_sensed_kernel of sensing.hip
// leaves early on its bad and exact lanes and keeps its own text of the rule and the sums.
__device__ __forceinline__ bool measure_obstacle(const double* __restrict__ r,
                                                 const double* __restrict__ osense, int g,
                                                 scpqp_sense_stream st, int b, int ob,
                                                 double t_meas, double (&zm)[4]) {
    double sp = 0.0, sh = 0.0, ss = 0.0;
    if (osense) {
        sp = osense[(size_t)g * SCPQP_OSENSE_NP + SCPQP_OSENSE_SIG_POS];
        sh = osense[(size_t)g * SCPQP_OSENSE_NP + SCPQP_OSENSE_SIG_HEADING];
        ss = osense[(size_t)g * SCPQP_OSENSE_NP + SCPQP_OSENSE_SIG_SPEED];
    }
    const bool bad_meas = !isfinite(sp) || !isfinite(sh) || !isfinite(ss) || sp < 0.0 || sh < 0.0 ||
                          ss < 0.0 || scpqp_obst_dev::bad_row(r);
    if (!bad_meas) {
        const scpqp_obst_dev::Pose p = scpqp_obst_dev::pose_at(r, t_meas);
        zm[0] = p.x;
        zm[1] = p.y;
        zm[2] = p.h;
        zm[3] = r[SCPQP_OBST_SPEED];
        if (!(sp == 0.0 && sh == 0.0 && ss == 0.0)) {
            const uint32_t c2 = ((uint32_t)SCPQP_NOISE_SITE_SENSE_OBST << 24) | (uint32_t)ob;
            const uint32_t bg = st.b_offset + (uint32_t)b;
            const Draw d0 = draw_at(st, 0u, c2, bg), d1 = draw_at(st, 1u, c2, bg);
            zm[0] = scpqp_round_dev::mul_add_2r(sp, d0.z0, zm[0]);
            zm[1] = scpqp_round_dev::mul_add_2r(sp, d0.z1, zm[1]);
            zm[2] = scpqp_round_dev::mul_add_2r(sh, d1.z0, zm[2]);
            zm[3] = scpqp_round_dev::mul_add_2r(ss, d1.z1, zm[3]);
        }
    }
    return bad_meas;
}

}  // namespace scpqp_sense_dev

#endif  // SCPQP_SENSE_DRAW_H
