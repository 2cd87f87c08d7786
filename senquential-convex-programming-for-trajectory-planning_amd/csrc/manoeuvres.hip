// manoeuvres.hip — obstacle manoeuvres on MI355X (fp64): the per-(realisation, obstacle)
// schedules of include/scpqp_manoeuvres.h on top of the rows of include/scpqp_obstacles.h.
//
//   scpqp_manoeuvres_state   the snapshot row of every lane at one time
//   scpqp_manoeuvres_pose    x, y, heading of every lane at a range of global ticks: the
//                            pose of the rows into pose_out (the existing kernel, for the
//                            off lanes), then the lanes with a schedule overwrite theirs
//   scpqp_manoeuvres_sample  schedules drawn per (piece, field) from one Philox call each
//
// One lane per (b, o) (state, sampler) or per (b, o, tick) (pose), 256 threads per
// workgroup, in the launch shape of tracker.hip.  Every lane walks its own pieces
// independently (state_at of scpqp_manoeuvre_pose.h: at most four pieces and the coast
// after them, each a closed form), reading the schedule from global memory piece by piece,
// so no per-thread array is indexed at run time.  No LDS.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>

#include "scpqp_manoeuvre_pose.h"
#include "scpqp_manoeuvres.h"
#include "scpqp_philox.h"
#include "scpqp_rounding.h"

int scpqp_fail_(int code, const char* msg);   // scpqp.hip: sets scpqp_last_error()

namespace {

constexpr int NP = SCPQP_OBST_NP;
constexpr int NSEG = SCPQP_MAN_NSEG;
constexpr int NF = SCPQP_MAN_NF;
constexpr int NM = NSEG * NF;
constexpr int PT = 256;   // threads per workgroup

using scpqp_man_dev::State;

// include/scpqp_manoeuvres.h: __dadd_rn(mean, __dmul_rn(spread, xi))
using scpqp_round_dev::mul_add_2r;

// the lane's class: 0 a schedule to walk, 1 off, 2 bad (include/scpqp_manoeuvres.h)
__device__ __forceinline__ int lane_class(const double* __restrict__ r, const double* __restrict__ m) {
    if (scpqp_obst_dev::bad_row(r)) return 2;
    if (!m) return 1;
    if (scpqp_man_dev::bad_schedule(m)) return 2;
    if (scpqp_man_dev::off_schedule(m)) return 1;
    return r[SCPQP_OBST_SPEED] < 0.0 ? 2 : 0;
}

// one lane per (b, o): state[b][o][0..6]
__global__ __launch_bounds__(PT) void state_kernel(int n, const double* __restrict__ rows,
                                                   const double* __restrict__ man, double t,
                                                   double* __restrict__ out) {
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= n) return;
    const double* r = rows + (size_t)g * NP;
    const double* m = man ? man + (size_t)g * NM : nullptr;
    double* o = out + (size_t)g * NP;
    const int cls = lane_class(r, m);
    if (cls == 2) {
#pragma unroll
        for (int f = 0; f < NP; ++f) o[f] = NAN;
        return;
    }
    State q;
    if (cls == 1) {
        // the row's own motion, by the pose of the obstacle truth and nothing else
        const scpqp_obst_dev::Pose p = scpqp_obst_dev::pose_at(r, t);
        q = State{p.x, p.y, p.h, r[SCPQP_OBST_SPEED], r[SCPQP_OBST_YAW_RATE]};
    } else {
        q = scpqp_man_dev::state_at(r, m, t);
    }
    o[SCPQP_OBST_X] = q.x;
    o[SCPQP_OBST_Y] = q.y;
    o[SCPQP_OBST_HEADING] = q.h;
    o[SCPQP_OBST_SPEED] = q.s;
    o[SCPQP_OBST_LENGTH] = r[SCPQP_OBST_LENGTH];
    o[SCPQP_OBST_WIDTH] = r[SCPQP_OBST_WIDTH];
    o[SCPQP_OBST_YAW_RATE] = q.w;
}

// one lane per (b, o, j): pose[b][o][j][0..2] at global tick tick0 + j.  out already holds
// the pose of every row; an off lane keeps it
__global__ __launch_bounds__(PT) void pose_kernel(int n, int K, const double* __restrict__ rows,
                                                  const double* __restrict__ man,
                                                  double tick_length, int tick0,
                                                  double* __restrict__ out) {
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= n) return;
    const int bo = g / K, j = g - bo * K;
    const double* r = rows + (size_t)bo * NP;
    const double* m = man + (size_t)bo * NM;
    double* o = out + (size_t)g * 3;
    const int cls = lane_class(r, m);
    if (cls == 1) return;
    if (cls == 2) {
        o[0] = o[1] = o[2] = NAN;
        return;
    }
    const State q = scpqp_man_dev::state_at(r, m, (double)(tick0 + j) * tick_length);
    o[0] = q.x;
    o[1] = q.y;
    o[2] = q.h;
}

// one lane per (b, o): its 12 values, value 3 i + f from the one Philox call of counter
// (3 i + f, 0, (site 8 << 24) | o, b_offset + b)
__global__ __launch_bounds__(PT) void sample_kernel(scpqp_manoeuvres_dist d, int B,
                                                    double* __restrict__ man) {
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= B * d.n_obst) return;
    const int b = g / d.n_obst, o = g % d.n_obst;
    double* m = man + (size_t)g * NM;
    for (int i = 0; i < NSEG; ++i) {
        for (int f = 0; f < NF; ++f) {
            const scpqp_truth_field& fd = d.field[i][f];
            const double mean = d.mean[i][f];
            if (fd.kind == SCPQP_TRUTH_FIXED) {
                m[i * NF + f] = mean;
                continue;
            }
            uint32_t c[4] = {(uint32_t)(NF * i + f), 0u,
                             ((uint32_t)SCPQP_NOISE_SITE_MANOEUVRE << 24) | (uint32_t)o,
                             d.b_offset + (uint32_t)b};
            scpqp_noise_dev::philox4x32_10(c, (uint32_t)d.seed, (uint32_t)(d.seed >> 32));
            double u1, u2;
            scpqp_noise_dev::uniforms(c, u1, u2);
            const double xi = fd.kind == SCPQP_TRUTH_UNIFORM
                                  ? 2.0 * u2 - 1.0
                                  : sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
            m[i * NF + f] = fmin(fmax(mul_add_2r(fd.spread, xi, mean), fd.lo), fd.hi);
        }
    }
}

const char* const FIELD[NF] = {"dur", "accel", "dyaw"};

int fail_field(const char* what, int i, int f) {
    static thread_local char msg[128];
    snprintf(msg, sizeof msg, "manoeuvre piece %d field %s: %s", i, FIELD[f], what);
    return scpqp_fail_(SCPQP_E_ARG, msg);
}

int check_sizes(int32_t B, int32_t n_obst) {
    if (B < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size < 0");
    if (n_obst < 1 || n_obst > SCPQP_MAX_OBST) return scpqp_fail_(SCPQP_E_ARG, "n_obst out of range");
    if ((long long)B * n_obst * NM > 0x7fffffffLL)
        return scpqp_fail_(SCPQP_E_SIZE, "B * n_obst * 12 too large");
    return 0;
}

int check_dist(const scpqp_manoeuvres_dist* d) {
    if (!d) return scpqp_fail_(SCPQP_E_ARG, "null manoeuvre distribution");
    if (d->n_obst < 1 || d->n_obst > SCPQP_MAX_OBST)
        return scpqp_fail_(SCPQP_E_ARG, "n_obst out of range");
    for (int i = 0; i < NSEG; ++i)
        for (int f = 0; f < NF; ++f) {
            const scpqp_truth_field& fd = d->field[i][f];
            if (fd.kind < SCPQP_TRUTH_FIXED || fd.kind > SCPQP_TRUTH_NORMAL)
                return fail_field("kind must be 0 (fixed), 1 (uniform) or 2 (normal)", i, f);
            if (!isfinite(d->mean[i][f])) return fail_field("the mean must be finite", i, f);
            if (fd.kind == SCPQP_TRUTH_FIXED) {
                // the smallest duration the sampler can emit: never a bad lane
                if (f == SCPQP_MAN_DUR && d->mean[i][f] < 0.0)
                    return fail_field("a fixed duration must be >= 0", i, f);
                continue;
            }
            if (!(fd.spread >= 0.0) || isinf(fd.spread))
                return fail_field("spread must be finite and >= 0", i, f);
            if (!(fd.lo <= fd.hi)) return fail_field("lo must be <= hi", i, f);
            if (f == SCPQP_MAN_DUR && !(fd.lo >= 0.0))
                return fail_field("lo must be >= 0 (a drawn duration is never negative)", i, f);
            if (f == SCPQP_MAN_DUR && isinf(fd.lo))
                return fail_field("lo must be finite", i, f);
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

int scpqp_manoeuvres_state(int32_t B, int32_t n_obst, const double* rows, const double* man,
                           double t, double* state_out, void* stream) {
    if (int rc = check_sizes(B, n_obst)) return rc;
    if (!(t >= 0.0) || isinf(t)) return scpqp_fail_(SCPQP_E_ARG, "t must be finite and >= 0");
    if (B == 0) return 0;
    if (!rows) return scpqp_fail_(SCPQP_E_ARG, "null rows array");
    if (!state_out) return scpqp_fail_(SCPQP_E_ARG, "null output array");
    const long long n = (long long)B * n_obst;
    hipLaunchKernelGGL(state_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), (int)n, rows, man, t, state_out);
    return launched();
}

int scpqp_manoeuvres_pose(int32_t B, int32_t n_obst, const double* rows, const double* man,
                          double tick_length, int32_t tick0, int32_t n_ticks, double* pose_out,
                          void* stream) {
    if (int rc = check_sizes(B, n_obst)) return rc;
    // the pose of every row as scpqp_obstacles_pose writes it (it validates the rest of the
    // arguments before its launch); then, in stream order, the lanes with a schedule
    // overwrite theirs.  An off lane so takes the code path of scpqp_obstacles_pose itself,
    // bitwise, whatever the compiler makes of either kernel.
    if (int rc = scpqp_obstacles_pose(B, n_obst, rows, tick_length, tick0, n_ticks, pose_out, stream))
        return rc;
    if (B == 0 || !man) return 0;
    const long long K = (long long)n_ticks + 1;
    const long long n = (long long)B * n_obst * K;
    hipLaunchKernelGGL(pose_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), (int)n, (int)K, rows, man, tick_length,
                       tick0, pose_out);
    return launched();
}

int scpqp_manoeuvres_sample(const scpqp_manoeuvres_dist* d, int32_t B, double* man_out,
                            void* stream) {
    if (int rc = check_dist(d)) return rc;
    if (int rc = check_sizes(B, d->n_obst)) return rc;
    if (B == 0) return 0;
    if (!man_out) return scpqp_fail_(SCPQP_E_ARG, "null output array");
    const long long n = (long long)B * d->n_obst;
    hipLaunchKernelGGL(sample_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), *d, B, man_out);
    return launched();
}

}  // extern "C"
