// sensing.hip — sensing truth on MI355X (fp64): the per-(realisation, vehicle) and
// per-(realisation, obstacle) sensor rows of include/scpqp_sensing.h.
//
//   scpqp_sense_measure             the measurement the controller gets of every vehicle:
//                                   noisy, biased, late or lost (held), per MPC step
//   scpqp_sense_fill_nominal        the rows of the exact sensor
//   scpqp_sense_sample              rows drawn per field from one Philox call each
//   scpqp_obstacles_predict_sensed  scpqp_obstacles_predict, then the blocks of the obstacles
//                                   with a noisy sensor again, from the noisy pose and speed
//
// All four are elementwise, one lane per (b, v) respectively (b, o), in the launch shape
// of obstacles.hip (256 threads, a ragged last workgroup cut by the bound check).  A lane
// reads one row and a handful of doubles, makes at most four Philox calls and writes a
// handful of doubles: next to the SCP solve of the same MPC step they do not show.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>

#include "scpqp_entry_checks.h"
#include "scpqp_obstacle_pose.h"
#include "scpqp_philox.h"
#include "scpqp_rounding.h"
#include "scpqp_sense_draw.h"
#include "scpqp_sensing.h"

namespace {

constexpr int NP = SCPQP_SENSE_NP;
constexpr int ONP = SCPQP_OSENSE_NP;
constexpr int PT = 256;   // threads per workgroup

using scpqp_obst_dev::Pose;

using scpqp_round_dev::add_1r;
using scpqp_round_dev::mul_1r;
using scpqp_round_dev::mul_add_2r;
using scpqp_sense_dev::Draw;
using scpqp_sense_dev::draw_at;

// any field non-finite, a sigma < 0, P_DROP outside [0, 1], LAG < 0 or not whole
__device__ __forceinline__ bool bad_sense_row(const double (&r)[NP]) {
    bool bad = false;
#pragma unroll
    for (int f = 0; f < NP; ++f) bad |= !isfinite(r[f]);
#pragma unroll
    for (int f = SCPQP_SENSE_SIG_POS; f <= SCPQP_SENSE_SIG_STEER; ++f) bad |= r[f] < 0.0;
    bad |= r[SCPQP_SENSE_P_DROP] < 0.0 || r[SCPQP_SENSE_P_DROP] > 1.0;
    bad |= r[SCPQP_SENSE_LAG] < 0.0 || r[SCPQP_SENSE_LAG] != rint(r[SCPQP_SENSE_LAG]);
    return bad;
}

// exactly (0, 0, 0, 0, 0, 1, 0, 0); a -0.0 compares equal to 0 and is nominal too
__device__ __forceinline__ bool nominal_sense_row(const double (&r)[NP]) {
    bool nom = r[SCPQP_SENSE_SCALE_SPEED] == 1.0;
#pragma unroll
    for (int f = 0; f < NP; ++f)
        if (f != SCPQP_SENSE_SCALE_SPEED) nom &= r[f] == 0.0;
    return nom;
}

// one lane per (b, v); K = n_ticks + 1 entries of 6 doubles per lane in x_path
__global__ __launch_bounds__(PT) void measure_kernel(int n, int nV, int K, int k_meas,
                                                     const double* __restrict__ x_path,
                                                     const double* __restrict__ sense,
                                                     scpqp_sense_stream st,
                                                     double* __restrict__ x_held,
                                                     int32_t* __restrict__ delivered,
                                                     double* __restrict__ out) {
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= n) return;
    const int b = g / nV, v = g - b * nV;
    double r[NP];
#pragma unroll
    for (int f = 0; f < NP; ++f) r[f] = sense[(size_t)g * NP + f];
    double* held = x_held + (size_t)g * 6;
    double* o = out + (size_t)g * 6;
    if (bad_sense_row(r)) {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            o[j] = NAN;
            held[j] = NAN;
        }
        if (delivered) delivered[g] = 0;
        return;
    }
    if (nominal_sense_row(r)) {
        const double* x = x_path + ((size_t)g * K + k_meas) * 6;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const double xj = x[j];
            o[j] = xj;
            held[j] = xj;
        }
        if (delivered) delivered[g] = 1;
        return;
    }
    const uint32_t c2 = ((uint32_t)SCPQP_NOISE_SITE_SENSE_DRAW << 24) | (uint32_t)v;
    const uint32_t bg = st.b_offset + (uint32_t)b;
    // lost: this step's measurement never arrives and the controller keeps the last one
    const double h0 = held[0];
    if (h0 == h0 && draw_at(st, 3u, c2, bg).u2 < r[SCPQP_SENSE_P_DROP]) {
#pragma unroll
        for (int j = 0; j < 6; ++j) o[j] = held[j];
        if (delivered) delivered[g] = 0;
        return;
    }
    const double lag = r[SCPQP_SENSE_LAG];
    const int k = lag >= (double)k_meas ? 0 : k_meas - (int)lag;
    const double* x = x_path + ((size_t)g * K + k) * 6;
    const Draw d0 = draw_at(st, 0u, c2, bg), d1 = draw_at(st, 1u, c2, bg), d2 = draw_at(st, 2u, c2, bg);
    double m[6];
    m[0] = mul_add_2r(r[SCPQP_SENSE_SIG_POS], d0.z0, x[0]);
    m[1] = mul_add_2r(r[SCPQP_SENSE_SIG_POS], d0.z1, x[1]);
    m[2] = mul_add_2r(r[SCPQP_SENSE_SIG_HEADING], d1.z0, add_1r(x[2], r[SCPQP_SENSE_BIAS_HEADING]));
    m[3] = mul_add_2r(r[SCPQP_SENSE_SIG_SPEED], d1.z1, mul_1r(r[SCPQP_SENSE_SCALE_SPEED], x[3]));
    m[4] = x[4];
    m[5] = mul_add_2r(r[SCPQP_SENSE_SIG_STEER], d2.z0, x[5]);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        o[j] = m[j];
        held[j] = m[j];
    }
    if (delivered) delivered[g] = 1;
}

// one lane per (b, v)
__global__ __launch_bounds__(PT) void nominal_kernel(int n, double* __restrict__ sense) {
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= n) return;
    double* row = sense + (size_t)g * NP;
#pragma unroll
    for (int f = 0; f < NP; ++f) row[f] = f == SCPQP_SENSE_SCALE_SPEED ? 1.0 : 0.0;
}

// one lane per (b, v): field f from the one Philox call of counter
// (f, 0, (site 5 << 24) | v, b_offset + b)
__global__ __launch_bounds__(PT) void sample_kernel(scpqp_sense_dist d, int B,
                                                    double* __restrict__ sense) {
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= B * d.n_veh) return;
    const int b = g / d.n_veh, v = g % d.n_veh;
    double* row = sense + (size_t)g * NP;
    for (int f = 0; f < NP; ++f) {
        const scpqp_truth_field& fd = d.field[f];
        const double mean = d.mean[f][v];
        double val = mean;
        if (fd.kind != SCPQP_TRUTH_FIXED) {
            uint32_t c[4] = {(uint32_t)f, 0u, ((uint32_t)SCPQP_NOISE_SITE_SENSE << 24) | (uint32_t)v,
                             d.b_offset + (uint32_t)b};
            scpqp_noise_dev::philox4x32_10(c, (uint32_t)d.seed, (uint32_t)(d.seed >> 32));
            double u1, u2;
            scpqp_noise_dev::uniforms(c, u1, u2);
            const double xi = fd.kind == SCPQP_TRUTH_UNIFORM
                                  ? 2.0 * u2 - 1.0
                                  : sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
            val = fmin(fmax(mul_add_2r(fd.spread, xi, mean), fd.lo), fd.hi);
        }
        // a latency is a whole number of ticks, drawn or fixed
        row[f] = f == SCPQP_SENSE_LAG ? rint(val) : val;
    }
}

// one lane per (b, o): obst[b][o][0 / 1][0 .. hp - 1]
__global__ __launch_bounds__(PT) void predict_sensed_kernel(int n, int nO, int hp,
                                                            const double* __restrict__ rows,
                                                            const double* __restrict__ osense,
                                                            scpqp_sense_stream st, double t_meas,
                                                            double lead, double dt,
                                                            double* __restrict__ out) {
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= n) return;
    const int b = g / nO, ob = g - b * nO;
    const double* r = rows + (size_t)g * SCPQP_OBST_NP;
    double* o = out + (size_t)g * 2 * hp;
    const double sp = osense[(size_t)g * ONP + SCPQP_OSENSE_SIG_POS];
    const double sh = osense[(size_t)g * ONP + SCPQP_OSENSE_SIG_HEADING];
    const double ss = osense[(size_t)g * ONP + SCPQP_OSENSE_SIG_SPEED];
    const bool bad = !isfinite(sp) || !isfinite(sh) || !isfinite(ss) || sp < 0.0 || sh < 0.0 ||
                     ss < 0.0 || scpqp_obst_dev::bad_row(r);
    if (bad) {
        for (int k = 0; k < 2 * hp; ++k) o[k] = NAN;
        return;
    }
    // an exact sensor: the block scpqp_obstacles_predict wrote before this launch stays
    if (sp == 0.0 && sh == 0.0 && ss == 0.0) return;
    Pose p = scpqp_obst_dev::pose_at(r, t_meas);
    const uint32_t c2 = ((uint32_t)SCPQP_NOISE_SITE_SENSE_OBST << 24) | (uint32_t)ob;
    const uint32_t bg = st.b_offset + (uint32_t)b;
    const Draw d0 = draw_at(st, 0u, c2, bg), d1 = draw_at(st, 1u, c2, bg);
    p.x = mul_add_2r(sp, d0.z0, p.x);
    p.y = mul_add_2r(sp, d0.z1, p.y);
    p.h = mul_add_2r(sh, d1.z0, p.h);
    const double speed = mul_add_2r(ss, d1.z1, r[SCPQP_OBST_SPEED]);
    sincos(p.h, &p.s, &p.c);
    // the extrapolation formula of scpqp_obstacles_predict
    for (int k = 0; k < hp; ++k) {
        const double step = ((double)(k + 1) * dt + lead) * speed;
        o[k] = step * p.c + p.x;
        o[hp + k] = step * p.s + p.y;
    }
}

const char* const FIELD[NP] = {"sig_pos", "sig_heading", "sig_speed", "sig_steer",
                               "bias_heading", "scale_speed", "p_drop", "lag"};

int fail_field(const char* what, int f) {
    static thread_local char msg[112];
    snprintf(msg, sizeof msg, "sensing field %s: %s", FIELD[f], what);
    return scpqp_fail_(SCPQP_E_ARG, msg);
}

int check_sizes(int32_t B, int32_t n_veh) {
    if (B < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size < 0");
    if (n_veh < 1 || n_veh > SCPQP_MAX_VEH) return scpqp_fail_(SCPQP_E_ARG, "n_veh out of range");
    return 0;
}

int check_dist(const scpqp_sense_dist* d) {
    if (!d) return scpqp_fail_(SCPQP_E_ARG, "null sensing distribution");
    if (d->n_veh < 1 || d->n_veh > SCPQP_MAX_VEH)
        return scpqp_fail_(SCPQP_E_ARG, "n_veh out of range");
    for (int f = 0; f < NP; ++f) {
        const scpqp_truth_field& fd = d->field[f];
        if (fd.kind < SCPQP_TRUTH_FIXED || fd.kind > SCPQP_TRUTH_NORMAL)
            return fail_field("kind must be 0 (fixed), 1 (uniform) or 2 (normal)", f);
        for (int v = 0; v < d->n_veh; ++v)
            if (!isfinite(d->mean[f][v])) return fail_field("every mean must be finite", f);
        if (fd.kind == SCPQP_TRUTH_FIXED) continue;
        if (!(fd.spread >= 0.0) || isinf(fd.spread))
            return fail_field("spread must be finite and >= 0", f);
        if (!(fd.lo <= fd.hi)) return fail_field("lo must be <= hi", f);
    }
    // the smallest (for P_DROP also the largest) value the sampler can emit: never a bad row
    for (int f = 0; f < NP; ++f) {
        if (f == SCPQP_SENSE_BIAS_HEADING || f == SCPQP_SENSE_SCALE_SPEED) continue;
        const bool fixed = d->field[f].kind == SCPQP_TRUTH_FIXED;
        for (int v = 0; v < d->n_veh; ++v) {
            const double floor_fv = fixed ? d->mean[f][v] : d->field[f].lo;
            if (!(floor_fv >= 0.0)) return fail_field("the smallest value must be >= 0", f);
            if (f != SCPQP_SENSE_P_DROP) continue;
            const double top_fv = fixed ? d->mean[f][v] : d->field[f].hi;
            if (!(floor_fv <= 1.0) || !(top_fv <= 1.0))
                return fail_field("the smallest and the largest value must be in [0, 1]", f);
        }
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

int scpqp_sense_measure(int32_t B, int32_t n_veh, int32_t n_ticks, int32_t k_meas,
                        const double* x_path, const double* sense, const scpqp_sense_stream* st,
                        double* x_held, int32_t* delivered, double* x_meas_out, void* stream) {
    if (int rc = check_sizes(B, n_veh)) return rc;
    if (n_ticks < 0) return scpqp_fail_(SCPQP_E_ARG, "n_ticks < 0");
    if (k_meas < 0 || k_meas > n_ticks)
        return scpqp_fail_(SCPQP_E_ARG, "k_meas outside 0..n_ticks");
    const long long K = (long long)n_ticks + 1;
    const long long n = (long long)B * n_veh;
    if (K > 0x7fffffffLL / 6 / n_veh || n * K * 6 > 0x7fffffffLL)
        return scpqp_fail_(SCPQP_E_SIZE, "B * n_veh * (n_ticks + 1) * 6 too large");
    if (B == 0) return 0;
    if (!x_path) return scpqp_fail_(SCPQP_E_ARG, "null x_path array");
    if (!sense) return scpqp_fail_(SCPQP_E_ARG, "null sense rows array");
    if (int rc = scpqp_host::check_stream(st)) return rc;
    if (!x_held) return scpqp_fail_(SCPQP_E_ARG, "null x_held array");
    if (!x_meas_out) return scpqp_fail_(SCPQP_E_ARG, "null output array");
    hipLaunchKernelGGL(measure_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), (int)n, n_veh, (int)K, k_meas, x_path,
                       sense, *st, x_held, delivered, x_meas_out);
    return launched();
}

int scpqp_sense_fill_nominal(int32_t B, int32_t n_veh, double* sense, void* stream) {
    if (int rc = check_sizes(B, n_veh)) return rc;
    const long long n = (long long)B * n_veh;
    if (n * NP > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_veh too large");
    if (B == 0) return 0;
    if (!sense) return scpqp_fail_(SCPQP_E_ARG, "null sense rows array");
    hipLaunchKernelGGL(nominal_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), (int)n, sense);
    return launched();
}

int scpqp_sense_sample(const scpqp_sense_dist* d, int32_t B, double* sense, void* stream) {
    if (int rc = check_dist(d)) return rc;
    if (B < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size < 0");
    const long long n = (long long)B * d->n_veh;
    if (n * NP > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_veh too large");
    if (B == 0) return 0;
    if (!sense) return scpqp_fail_(SCPQP_E_ARG, "null sense rows array");
    hipLaunchKernelGGL(sample_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), *d, B, sense);
    return launched();
}

int scpqp_obstacles_predict_sensed(int32_t B, int32_t n_obst, int32_t hp, const double* rows,
                                   const double* osense, const scpqp_sense_stream* st,
                                   double t_meas, double lead, double dt, double* obst_out,
                                   void* stream) {
    if (B < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size < 0");
    if (n_obst < 1 || n_obst > SCPQP_MAX_OBST) return scpqp_fail_(SCPQP_E_ARG, "n_obst out of range");
    if (hp < 1 || hp > SCPQP_MAX_HP) return scpqp_fail_(SCPQP_E_ARG, "hp out of range");
    if (!isfinite(t_meas) || !isfinite(lead) || !isfinite(dt))
        return scpqp_fail_(SCPQP_E_ARG, "t_meas, lead and dt must be finite");
    const long long n = (long long)B * n_obst;
    if (2 * n * hp > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_obst * 2 * hp too large");
    if (B == 0) return 0;
    if (!rows) return scpqp_fail_(SCPQP_E_ARG, "null rows array");
    if (!osense) return scpqp_fail_(SCPQP_E_ARG, "null osense rows array");
    if (int rc = scpqp_host::check_stream(st)) return rc;
    if (!obst_out) return scpqp_fail_(SCPQP_E_ARG, "null output array");
    // every block as the exact sensor predicts it; then, in stream order, the lanes whose
    // osense row is not all zero overwrite theirs.  An all-zero row so takes the code path of
    // scpqp_obstacles_predict itself, bitwise, whatever the compiler makes of either kernel.
    if (int rc = scpqp_obstacles_predict(B, n_obst, hp, rows, t_meas, lead, dt, obst_out, stream))
        return rc;
    hipLaunchKernelGGL(predict_sensed_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), (int)n, n_obst, hp, rows, osense, *st,
                       t_meas, lead, dt, obst_out);
    return launched();
}

}  // extern "C"
