// obstacles.hip — obstacle truth on MI355X (fp64): the per-(realisation, obstacle)
// rows of include/scpqp_obstacles.h.
//
//   scpqp_obstacles_predict       the controller's straight-line prediction from the
//                                 true pose at the measurement time (MPC_Iter.py:45-51)
//   scpqp_obstacles_pose          x, y, heading of every row at a range of global ticks
//   scpqp_obstacles_fill_nominal  the rows of the scenario's own obstacles, turn rate 0
//   scpqp_obstacles_sample        rows drawn per field from one Philox call each
//
// All four are elementwise: one lane per output element group, the launch shape of
// plant.hip (256 threads, a ragged last workgroup cut by the bound check).  The pose is
// a handful of transcendental calls per lane and the outputs are a few doubles: next to
// the SCP solve of the same MPC step they do not show.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>

#include "scpqp_obstacle_pose.h"
#include "scpqp_obstacles.h"
#include "scpqp_philox.h"
#include "scpqp_rounding.h"

int scpqp_fail_(int code, const char* msg);   // scpqp.hip: sets scpqp_last_error()

namespace {

constexpr int NP = SCPQP_OBST_NP;
constexpr int PT = 256;   // threads per workgroup

using scpqp_obst_dev::Pose;

// include/scpqp_obstacles.h: __dadd_rn(mean, __dmul_rn(spread, xi))
using scpqp_round_dev::mul_add_2r;

// one lane per (b, o, k): obst[b][o][0 / 1][k]
__global__ __launch_bounds__(PT) void predict_kernel(int n, int hp, const double* __restrict__ rows,
                                                     double t_meas, double lead, double dt,
                                                     double* __restrict__ out) {
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= n) return;
    const int bo = g / hp, k = g - bo * hp;
    const double* r = rows + (size_t)bo * NP;
    double* o = out + (size_t)bo * 2 * hp + k;
    if (scpqp_obst_dev::bad_row(r)) {
        o[0] = NAN;
        o[hp] = NAN;
        return;
    }
    const Pose p = scpqp_obst_dev::pose_at(r, t_meas);
    const double step = ((double)(k + 1) * dt + lead) * r[SCPQP_OBST_SPEED];
    o[0] = step * p.c + p.x;
    o[hp] = step * p.s + p.y;
}

// one lane per (b, o, j): pose[b][o][j][0..2] at global tick tick0 + j
__global__ __launch_bounds__(PT) void pose_kernel(int n, int K, const double* __restrict__ rows,
                                                  double tick_length, int tick0,
                                                  double* __restrict__ out) {
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= n) return;
    const int bo = g / K, j = g - bo * K;
    const double* r = rows + (size_t)bo * NP;
    double* o = out + (size_t)g * 3;
    if (scpqp_obst_dev::bad_row(r)) {
        o[0] = o[1] = o[2] = NAN;
        return;
    }
    const Pose p = scpqp_obst_dev::pose_at(r, (double)(tick0 + j) * tick_length);
    o[0] = p.x;
    o[1] = p.y;
    o[2] = p.h;
}

struct Nominal {
    double ob[SCPQP_MAX_OBST][6];
};

// one lane per (b, o)
__global__ __launch_bounds__(PT) void nominal_kernel(Nominal nom, int B, int nO,
                                                     double* __restrict__ rows) {
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= B * nO) return;
    const int o = g % nO;
    double* row = rows + (size_t)g * NP;
#pragma unroll
    for (int f = 0; f < 6; ++f) row[f] = nom.ob[o][f];
    row[SCPQP_OBST_YAW_RATE] = 0.0;
}

// one lane per (b, o): field f from the one Philox call of counter
// (f, 0, (site 4 << 24) | o, b_offset + b)
__global__ __launch_bounds__(PT) void sample_kernel(scpqp_obstacles_dist d, int B,
                                                    double* __restrict__ rows) {
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= B * d.n_obst) return;
    const int b = g / d.n_obst, o = g % d.n_obst;
    double* row = rows + (size_t)g * NP;
    for (int f = 0; f < NP; ++f) {
        const scpqp_truth_field& fd = d.field[f];
        const double mean = d.mean[f][o];
        if (fd.kind == SCPQP_TRUTH_FIXED) {
            row[f] = mean;
            continue;
        }
        uint32_t c[4] = {(uint32_t)f, 0u, ((uint32_t)SCPQP_NOISE_SITE_OBSTACLE << 24) | (uint32_t)o,
                         d.b_offset + (uint32_t)b};
        scpqp_noise_dev::philox4x32_10(c, (uint32_t)d.seed, (uint32_t)(d.seed >> 32));
        double u1, u2;
        scpqp_noise_dev::uniforms(c, u1, u2);
        const double xi = fd.kind == SCPQP_TRUTH_UNIFORM
                              ? 2.0 * u2 - 1.0
                              : sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
        row[f] = fmin(fmax(mul_add_2r(fd.spread, xi, mean), fd.lo), fd.hi);
    }
}

const char* const FIELD[NP] = {"x", "y", "heading", "speed", "length", "width", "yaw_rate"};

int fail_field(const char* what, int f) {
    static thread_local char msg[112];
    snprintf(msg, sizeof msg, "obstacle field %s: %s", FIELD[f], what);
    return scpqp_fail_(SCPQP_E_ARG, msg);
}

int check_sizes(int32_t B, int32_t n_obst) {
    if (B < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size < 0");
    if (n_obst < 1 || n_obst > SCPQP_MAX_OBST) return scpqp_fail_(SCPQP_E_ARG, "n_obst out of range");
    return 0;
}

int check_dist(const scpqp_obstacles_dist* d) {
    if (!d) return scpqp_fail_(SCPQP_E_ARG, "null obstacle distribution");
    if (d->n_obst < 1 || d->n_obst > SCPQP_MAX_OBST)
        return scpqp_fail_(SCPQP_E_ARG, "n_obst out of range");
    for (int f = 0; f < NP; ++f) {
        const scpqp_truth_field& fd = d->field[f];
        if (fd.kind < SCPQP_TRUTH_FIXED || fd.kind > SCPQP_TRUTH_NORMAL)
            return fail_field("kind must be 0 (fixed), 1 (uniform) or 2 (normal)", f);
        for (int o = 0; o < d->n_obst; ++o)
            if (!isfinite(d->mean[f][o])) return fail_field("every mean must be finite", f);
        if (fd.kind == SCPQP_TRUTH_FIXED) continue;
        if (!(fd.spread >= 0.0) || isinf(fd.spread))
            return fail_field("spread must be finite and >= 0", f);
        if (!(fd.lo <= fd.hi)) return fail_field("lo must be <= hi", f);
    }
    // the smallest footprint the sampler can emit: never a bad row
    for (int f = SCPQP_OBST_LENGTH; f <= SCPQP_OBST_WIDTH; ++f)
        for (int o = 0; o < d->n_obst; ++o) {
            const double floor_fo = d->field[f].kind == SCPQP_TRUTH_FIXED ? d->mean[f][o] : d->field[f].lo;
            if (!(floor_fo >= 0.0)) return fail_field("the smallest value must be >= 0", f);
        }
    return 0;
}

int launched() {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return scpqp_fail_(SCPQP_E_HIP, hipGetErrorString(e));
    return 0;
}

}  // namespace

extern "C" {

int scpqp_obstacles_predict(int32_t B, int32_t n_obst, int32_t hp, const double* rows,
                            double t_meas, double lead, double dt, double* obst_out, void* stream) {
    if (int rc = check_sizes(B, n_obst)) return rc;
    if (hp < 1 || hp > SCPQP_MAX_HP) return scpqp_fail_(SCPQP_E_ARG, "hp out of range");
    if (!isfinite(t_meas) || !isfinite(lead) || !isfinite(dt))
        return scpqp_fail_(SCPQP_E_ARG, "t_meas, lead and dt must be finite");
    const long long n = (long long)B * n_obst * hp;
    if (2 * n > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_obst * 2 * hp too large");
    if (B == 0) return 0;
    if (!rows) return scpqp_fail_(SCPQP_E_ARG, "null rows array");
    if (!obst_out) return scpqp_fail_(SCPQP_E_ARG, "null output array");
    hipLaunchKernelGGL(predict_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), (int)n, hp, rows, t_meas, lead, dt, obst_out);
    return launched();
}

int scpqp_obstacles_pose(int32_t B, int32_t n_obst, const double* rows, double tick_length,
                         int32_t tick0, int32_t n_ticks, double* pose_out, void* stream) {
    if (int rc = check_sizes(B, n_obst)) return rc;
    if (!(tick_length > 0.0) || isinf(tick_length))
        return scpqp_fail_(SCPQP_E_ARG, "tick_length must be finite and > 0");
    if (tick0 < 0) return scpqp_fail_(SCPQP_E_ARG, "tick0 < 0");
    if (n_ticks < 0) return scpqp_fail_(SCPQP_E_ARG, "n_ticks < 0");
    if ((long long)tick0 + n_ticks > 0x7fffffffLL)
        return scpqp_fail_(SCPQP_E_SIZE, "tick0 + n_ticks too large");
    const long long K = (long long)n_ticks + 1;
    if (K > 0x7fffffffLL / 3 / n_obst || (long long)B * n_obst * K * 3 > 0x7fffffffLL)
        return scpqp_fail_(SCPQP_E_SIZE, "B * n_obst * (n_ticks + 1) * 3 too large");
    if (B == 0) return 0;
    if (!rows) return scpqp_fail_(SCPQP_E_ARG, "null rows array");
    if (!pose_out) return scpqp_fail_(SCPQP_E_ARG, "null output array");
    const long long n = (long long)B * n_obst * K;
    hipLaunchKernelGGL(pose_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), (int)n, (int)K, rows, tick_length, tick0,
                       pose_out);
    return launched();
}

int scpqp_obstacles_fill_nominal(int32_t n_obst, const double* obstacles_host, int32_t B,
                                 double* rows, void* stream) {
    if (int rc = check_sizes(B, n_obst)) return rc;
    if (!obstacles_host) return scpqp_fail_(SCPQP_E_ARG, "null obstacles array");
    Nominal nom = {};
    for (int o = 0; o < n_obst; ++o)
        for (int f = 0; f < 6; ++f) {
            const double x = obstacles_host[o * 6 + f];
            if (!isfinite(x)) return fail_field("must be finite", f);
            if ((f == SCPQP_OBST_LENGTH || f == SCPQP_OBST_WIDTH) && x < 0.0)
                return fail_field("must be >= 0", f);
            nom.ob[o][f] = x;
        }
    const long long n = (long long)B * n_obst;
    if (n * NP > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_obst too large");
    if (B == 0) return 0;
    if (!rows) return scpqp_fail_(SCPQP_E_ARG, "null rows array");
    hipLaunchKernelGGL(nominal_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), nom, B, n_obst, rows);
    return launched();
}

int scpqp_obstacles_sample(const scpqp_obstacles_dist* d, int32_t B, double* rows, void* stream) {
    if (int rc = check_dist(d)) return rc;
    if (B < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size < 0");
    const long long n = (long long)B * d->n_obst;
    if (n * NP > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_obst too large");
    if (B == 0) return 0;
    if (!rows) return scpqp_fail_(SCPQP_E_ARG, "null rows array");
    hipLaunchKernelGGL(sample_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), *d, B, rows);
    return launched();
}

}  // extern "C"
