// drive.hip — the plant step behind a longitudinal actuator, batched on MI355X (fp64).
//
//   scpqp_plant_step_drive   scpqp_plant_step_truth with a commanded acceleration and a
//                            drive row per (realisation, vehicle): gain, offset, limits, a
//                            first-order lag and the hold rule (include/scpqp_drive.h)
//   scpqp_drive_fill_ideal, scpqp_drive_sample
//                            the ideal rows and the sampler
//
// One lane per (problem, vehicle, output tick), everything in registers, as in plant.hip.
// A lane whose row has neither a lag nor the hold rule runs the truth lane's own flow with
// x[4] = a_eff; only the others pay for the gate, the lag and the projection, so the lanes of
// a wave whose rows differ there diverge, and ideal lanes cost what they cost without a drive.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>

#include "scpqp_bicycle.h"
#include "scpqp_drive.h"
#include "scpqp_noise.h"
#include "scpqp_philox.h"
#include "scpqp_rounding.h"

int scpqp_fail_(int code, const char* msg);   // scpqp.hip: sets scpqp_last_error()

namespace {

using namespace scpqp_plant_dev;   // scpqp_bicycle.h: NX, VehT, VehD, flow, flow_drive, steps_for

constexpr int PT = 256;   // threads per workgroup

using scpqp_round_dev::mul_add_2r;   // the __dadd_rn(__dmul_rn(a, b), c) of include/scpqp_drive.h

// plant_lane_truth (plant.hip) with the lane's drive row: six more loads and the command,
// both validity guards, u_eff and a_eff, then the same integration with the same step count.
template <bool kNoisy>
__device__ __forceinline__ void plant_lane_drive(int V, int B, int n_ticks, double tick,
                                                 double hmax, const double* x_start,
                                                 const double* u_tick, const double* truth,
                                                 const double* noise, const scpqp_noise& nz,
                                                 const double* a_cmd, const double* drive,
                                                 double* x_path) {
    const int K = n_ticks + 1;
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= B * V * K) return;
    const int k = g % K, bv = g / K, v = bv % V;
    const double* row = truth + (size_t)bv * SCPQP_TRUTH_NP;
    const double lf = row[SCPQP_TRUTH_LF], lr = row[SCPQP_TRUTH_LR], tau = row[SCPQP_TRUTH_TAU];
    const double gain = row[SCPQP_TRUTH_GAIN], bias = row[SCPQP_TRUTH_BIAS];
    const double* dr = drive + (size_t)bv * SCPQP_DRIVE_NP;
    const double tau_a = dr[SCPQP_DRIVE_TAU_A], gain_a = dr[SCPQP_DRIVE_GAIN_A];
    const double bias_a = dr[SCPQP_DRIVE_BIAS_A], a_max = dr[SCPQP_DRIVE_A_MAX];
    const double b_max = dr[SCPQP_DRIVE_B_MAX], hold = dr[SCPQP_DRIVE_HOLD];
    const double ac = a_cmd[bv];
    const bool bad = !(lf + lr > 0.0) || !(tau > 0.0) || !(tau_a >= 0.0) || !isfinite(gain_a) ||
                     !isfinite(bias_a) || !(a_max >= 0.0) || !(b_max >= 0.0) ||
                     !(hold == 0.0 || hold == 1.0) || !isfinite(ac);
    if (bad) {
#pragma unroll
        for (int i = 0; i < NX; ++i) x_path[(size_t)g * NX + i] = __builtin_nan("");
        return;
    }
    const double a_eff = fmin(fmax(mul_add_2r(gain_a, ac, bias_a), -b_max), a_max);
    VehT q{{lf, lr, mul_add_2r(gain, u_tick[g], bias), noise ? noise[2 * bv] : 0.0,
            noise ? noise[2 * bv + 1] : 0.0},
           tau};
    Stream ns{};
    if constexpr (kNoisy)
        ns = scpqp_noise_dev::make_stream(nz.seed, nz.sigma, nz.epoch, SCPQP_NOISE_SITE_PLANT,
                                          (uint32_t)k, (uint32_t)v, nz.b_offset + (uint32_t)(bv / V));
    double x[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = x_start[(size_t)bv * NX + i];
    const bool lag = tau_a > 0.0;
    if (!lag) x[4] = a_eff;
    if (k > 0) {
        const double T = k * tick;
        if (!lag && hold == 0.0) {
            flow<kNoisy>(x, q, T, steps_for(T, hmax), ns);
        } else {
            VehD d{q, a_eff, tau_a, lag, hold == 1.0};
            flow_drive<kNoisy>(x, d, T, steps_for(T, hmax), ns);
        }
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) x_path[(size_t)g * NX + i] = x[i];
}

__global__ __launch_bounds__(PT) void plant_kernel_drive(int V, int B, int n_ticks, double tick,
                                                         double hmax, const double* x_start,
                                                         const double* u_tick,
                                                         const double* truth,
                                                         const double* noise, const double* a_cmd,
                                                         const double* drive, double* x_path) {
    plant_lane_drive<false>(V, B, n_ticks, tick, hmax, x_start, u_tick, truth, noise,
                            scpqp_noise{}, a_cmd, drive, x_path);
}

__global__ __launch_bounds__(PT) void plant_kernel_drive_noisy(int V, int B, int n_ticks,
                                                               double tick, double hmax,
                                                               const double* x_start,
                                                               const double* u_tick,
                                                               const double* truth, scpqp_noise nz,
                                                               const double* a_cmd,
                                                               const double* drive,
                                                               double* x_path) {
    plant_lane_drive<true>(V, B, n_ticks, tick, hmax, x_start, u_tick, truth, nullptr, nz, a_cmd,
                           drive, x_path);
}

// one lane per (problem, vehicle): the ideal row of include/scpqp_drive.h
__global__ __launch_bounds__(PT) void drive_ideal_kernel(int n, double* drive) {
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= n) return;
    double* row = drive + (size_t)g * SCPQP_DRIVE_NP;
    row[SCPQP_DRIVE_TAU_A] = 0.0;
    row[SCPQP_DRIVE_GAIN_A] = 1.0;
    row[SCPQP_DRIVE_BIAS_A] = 0.0;
    row[SCPQP_DRIVE_A_MAX] = __builtin_inf();
    row[SCPQP_DRIVE_B_MAX] = __builtin_inf();
    row[SCPQP_DRIVE_HOLD] = 0.0;
}

// one lane per (problem, vehicle): field f from the one Philox call of counter
// (f, 0, (site 9 << 24) | v, b_offset + b)
__global__ __launch_bounds__(PT) void drive_sample_kernel(scpqp_drive_dist d, int B,
                                                          double* drive) {
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= B * d.n_veh) return;
    const int b = g / d.n_veh, v = g % d.n_veh;
    double* row = drive + (size_t)g * SCPQP_DRIVE_NP;
    for (int f = 0; f < SCPQP_DRIVE_NP; ++f) {
        const scpqp_truth_field& fd = d.field[f];
        const double mean = d.mean[f][v];
        if (fd.kind == SCPQP_TRUTH_FIXED) {
            row[f] = mean;
            continue;
        }
        uint32_t c[4] = {(uint32_t)f, 0u, ((uint32_t)SCPQP_NOISE_SITE_DRIVE << 24) | (uint32_t)v,
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

int check_noise(const scpqp_noise* nz) {
    if (!nz) return scpqp_fail_(SCPQP_E_ARG, "null noise parameters");
    if (!(nz->sigma >= 0.0) || isinf(nz->sigma))
        return scpqp_fail_(SCPQP_E_ARG, "sigma must be finite and >= 0");
    return 0;
}

const char* const DRIVE_FIELD[SCPQP_DRIVE_NP] = {"tau_a", "gain_a", "bias_a", "a_max", "b_max",
                                                 "hold"};

int fail_field(const char* what, int f) {
    static thread_local char msg[96];
    snprintf(msg, sizeof msg, "drive field %s: %s", DRIVE_FIELD[f], what);
    return scpqp_fail_(SCPQP_E_ARG, msg);
}

int check_drive_dist(const scpqp_drive_dist* d) {
    if (!d) return scpqp_fail_(SCPQP_E_ARG, "null drive distribution");
    if (d->n_veh < 1 || d->n_veh > SCPQP_MAX_VEH) return scpqp_fail_(SCPQP_E_ARG, "n_veh out of range");
    for (int f = 0; f < SCPQP_DRIVE_NP; ++f) {
        const scpqp_truth_field& fd = d->field[f];
        if (fd.kind < SCPQP_TRUTH_FIXED || fd.kind > SCPQP_TRUTH_NORMAL)
            return fail_field("kind must be 0 (fixed), 1 (uniform) or 2 (normal)", f);
        if (fd.kind == SCPQP_TRUTH_FIXED) continue;
        if (f == SCPQP_DRIVE_HOLD) return fail_field("must be fixed at 0 or 1", f);
        if (!(fd.spread >= 0.0) || isinf(fd.spread))
            return fail_field("spread must be finite and >= 0", f);
        if (!(fd.lo <= fd.hi)) return fail_field("lo must be <= hi", f);
        for (int v = 0; v < d->n_veh; ++v)
            if (!isfinite(d->mean[f][v])) return fail_field("a drawn field needs a finite mean", f);
    }
    // the smallest value the sampler can emit: never a row the plant would NaN
    auto fixed = [d](int f) { return d->field[f].kind == SCPQP_TRUTH_FIXED; };
    auto floor_of = [d, fixed](int f, int v) { return fixed(f) ? d->mean[f][v] : d->field[f].lo; };
    for (int v = 0; v < d->n_veh; ++v) {
        if (!(floor_of(SCPQP_DRIVE_TAU_A, v) >= 0.0))
            return fail_field("the smallest tau_a must be >= 0", SCPQP_DRIVE_TAU_A);
        for (int f : {SCPQP_DRIVE_GAIN_A, SCPQP_DRIVE_BIAS_A}) {
            if (fixed(f) ? !isfinite(d->mean[f][v])
                         : (d->field[f].lo == INFINITY || d->field[f].hi == -INFINITY))
                return fail_field("must stay finite", f);
        }
        if (!(floor_of(SCPQP_DRIVE_A_MAX, v) >= 0.0))
            return fail_field("the smallest a_max must be >= 0", SCPQP_DRIVE_A_MAX);
        if (!(floor_of(SCPQP_DRIVE_B_MAX, v) >= 0.0))
            return fail_field("the smallest b_max must be >= 0", SCPQP_DRIVE_B_MAX);
        const double h = d->mean[SCPQP_DRIVE_HOLD][v];
        if (!(h == 0.0 || h == 1.0)) return fail_field("must be fixed at 0 or 1", SCPQP_DRIVE_HOLD);
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

int scpqp_plant_step_drive(const scpqp_plant_params* p, int32_t B, int32_t n_ticks, double tick,
                           const double* x_start, const double* u_tick, const double* truth,
                           const double* noise, const scpqp_noise* nz, const double* a_cmd,
                           const double* drive, double* x_path, double h_max, void* stream) {
    if (!p) return scpqp_fail_(SCPQP_E_ARG, "null plant params");
    if (p->n_veh < 1 || p->n_veh > SCPQP_MAX_VEH) return scpqp_fail_(SCPQP_E_ARG, "n_veh out of range");
    if (noise && nz)
        return scpqp_fail_(SCPQP_E_ARG, "pass either noise (constant terms) or nz, not both");
    if (nz)
        if (int rc = check_noise(nz)) return rc;
    if (B < 0 || n_ticks < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size / n_ticks < 0");
    if (nz && n_ticks >= SCPQP_NOISE_MAX_TICKS)
        return scpqp_fail_(SCPQP_E_SIZE, "n_ticks must be < 65536 (16 bits of the counter)");
    if (!(tick > 0.0) || !(h_max > 0.0)) return scpqp_fail_(SCPQP_E_ARG, "bad tick / h_max");
    if (B == 0) return 0;
    if (!truth) return scpqp_fail_(SCPQP_E_ARG, "null truth array");
    if (!a_cmd) return scpqp_fail_(SCPQP_E_ARG, "null a_cmd array");
    if (!drive) return scpqp_fail_(SCPQP_E_ARG, "null drive array");
    if (!x_start || !u_tick || !x_path) return scpqp_fail_(SCPQP_E_ARG, "null array");
    const long long n = (long long)B * p->n_veh * (n_ticks + 1);
    if (n > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_veh * (n_ticks + 1) too large");
    const dim3 grid((unsigned)((n + PT - 1) / PT));
    if (nz)
        hipLaunchKernelGGL(plant_kernel_drive_noisy, grid, dim3(PT), 0,
                           static_cast<hipStream_t>(stream), (int)p->n_veh, B, n_ticks, tick,
                           h_max, x_start, u_tick, truth, *nz, a_cmd, drive, x_path);
    else
        hipLaunchKernelGGL(plant_kernel_drive, grid, dim3(PT), 0,
                           static_cast<hipStream_t>(stream), (int)p->n_veh, B, n_ticks, tick,
                           h_max, x_start, u_tick, truth, noise, a_cmd, drive, x_path);
    return launched();
}

int scpqp_drive_fill_ideal(int32_t n_veh, int32_t B, double* drive, void* stream) {
    if (n_veh < 1 || n_veh > SCPQP_MAX_VEH) return scpqp_fail_(SCPQP_E_ARG, "n_veh out of range");
    if (B < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size < 0");
    if (B == 0) return 0;
    if (!drive) return scpqp_fail_(SCPQP_E_ARG, "null drive array");
    const long long n = (long long)B * n_veh;
    if (n * SCPQP_DRIVE_NP > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_veh too large");
    hipLaunchKernelGGL(drive_ideal_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), (int)n, drive);
    return launched();
}

int scpqp_drive_sample(const scpqp_drive_dist* d, int32_t B, double* drive, void* stream) {
    if (int rc = check_drive_dist(d)) return rc;
    if (B < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size < 0");
    if (B == 0) return 0;
    if (!drive) return scpqp_fail_(SCPQP_E_ARG, "null drive array");
    const long long n = (long long)B * d->n_veh;
    if (n * SCPQP_DRIVE_NP > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_veh too large");
    hipLaunchKernelGGL(drive_sample_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), *d, B, drive);
    return launched();
}

}  // extern "C"
