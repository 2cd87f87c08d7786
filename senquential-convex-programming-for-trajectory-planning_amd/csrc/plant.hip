// plant.hip — the bicycle plant around the SCP solve, batched on MI355X (fp64).
//
//   scpqp_delay_compensate  IterClass delay compensation: every vehicle of every
//                           problem integrated over delay_x + dt + delay_u with
//                           its last commanded steering (MPC_Iter.py:24-33)
//   scpqp_plant_step        closed-loop plant simulation over one MPC step
//                           (main.py:176-191)
//   scpqp_clip_controls     steering-limit enforcement of the controller output
//                           (main.py:164-174)
//   scpqp_delay_compensate_noisy, scpqp_plant_step_noisy, scpqp_noise_fill
//                           the same integrators with the reference's model noise
//                           drawn anew per right-hand-side evaluation
//                           (include/scpqp_noise.h, Model.py:84-86)
//   scpqp_plant_step_truth, scpqp_truth_fill_nominal, scpqp_truth_sample
//                           the plant step with per-(realisation, vehicle) plant
//                           parameters the controller does not know, and their
//                           sampler (include/scpqp_truth.h)
//
// The reference integrates with scipy (odeint = LSODA at rtol = atol = 1.49e-8
// for the delay compensation, dopri5 at rtol = atol = 1e-8 for the plant).
// Here every trajectory is one lane running the classical fourth-order
// Runge-Kutta method with a fixed step (default 2.5 ms, a quarter tick): the
// right-hand side is smooth, so the fixed step is ~1e-11 from the exact flow —
// three orders below the reference's own integration tolerance — and the
// lanes of a wave stay in lockstep (no adaptive step control to diverge on).
// The integration is compute-bound and tiny next to the SCP solve; the lanes
// read and write their 6-state rows directly (48 B per lane).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>

#include "scpqp_bicycle.h"
#include "scpqp_noise.h"
#include "scpqp_philox.h"
#include "scpqp_rounding.h"
#include "scpqp_truth.h"

int scpqp_fail_(int code, const char* msg);   // scpqp.hip: sets scpqp_last_error()

namespace {

using namespace scpqp_plant_dev;   // scpqp_bicycle.h: NX, Veh, VehT, bicycle, rk4, flow, steps_for

constexpr int PT = 256;   // threads per workgroup

using scpqp_round_dev::mul_add_2r;   // the __dadd_rn(__dmul_rn(a, b), c) of include/scpqp_truth.h

// one lane per (problem, vehicle): linspace(0, horizon, n_out) outputs.  kNoisy:
// site 0 stream of (b_offset + b, v), counting on across the n_out - 1 spans.
template <bool kNoisy>
__device__ __forceinline__ void delay_lane(const scpqp_plant_params& p, int B, double horizon,
                                           int n_out, double hmax, const double* x_meas,
                                           const double* u_hold, const double* noise,
                                           const scpqp_noise& nz, double* x0_out,
                                           double* traj_out) {
    const int V = p.n_veh;
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= B * V) return;
    const int b = g / V, v = g % V;
    Veh q{p.lf[v], p.lr[v], u_hold[g], noise ? noise[2 * g] : 0.0, noise ? noise[2 * g + 1] : 0.0};
    Stream ns{};
    if constexpr (kNoisy)
        ns = scpqp_noise_dev::make_stream(nz.seed, nz.sigma, nz.epoch, SCPQP_NOISE_SITE_DELAY, 0u,
                                          (uint32_t)v, nz.b_offset + (uint32_t)b);
    double x[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = x_meas[(size_t)g * NX + i];
    const double span = horizon / (n_out - 1);
    const int n = steps_for(span, hmax);
    for (int j = 0; j < n_out; ++j) {
        if (j > 0) flow<kNoisy>(x, q, span, n, ns);
        if (traj_out) {
            // MPC_delay_compensation_trajectory layout [n_out][nx][nVeh] per problem
#pragma unroll
            for (int i = 0; i < NX; ++i)
                traj_out[(((size_t)b * n_out + j) * NX + i) * V + v] = x[i];
        }
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) x0_out[(size_t)g * NX + i] = x[i];
}

__global__ __launch_bounds__(PT) void delay_kernel(scpqp_plant_params p, int B, double horizon,
                                                   int n_out, double hmax, const double* x_meas,
                                                   const double* u_hold, const double* noise,
                                                   double* x0_out, double* traj_out) {
    delay_lane<false>(p, B, horizon, n_out, hmax, x_meas, u_hold, noise, scpqp_noise{}, x0_out,
                      traj_out);
}

__global__ __launch_bounds__(PT) void delay_kernel_noisy(scpqp_plant_params p, int B,
                                                         double horizon, int n_out, double hmax,
                                                         const double* x_meas,
                                                         const double* u_hold, scpqp_noise nz,
                                                         double* x0_out, double* traj_out) {
    delay_lane<true>(p, B, horizon, n_out, hmax, x_meas, u_hold, nullptr, nz, x0_out, traj_out);
}

// one lane per (problem, vehicle, output tick k): main.py:186-190 restarts the
// integration at t0 for every output time t_k, with the control value of tick k.
// kNoisy: site 1 stream of (b_offset + b, v, k): every restart has its own noise,
// as every restart of the reference consumes fresh draws.
template <bool kNoisy>
__device__ __forceinline__ void plant_lane(const scpqp_plant_params& p, int B, int n_ticks,
                                           double tick, double hmax, const double* x_start,
                                           const double* u_tick, const double* noise,
                                           const scpqp_noise& nz, double* x_path) {
    const int V = p.n_veh, K = n_ticks + 1;
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= B * V * K) return;
    const int k = g % K, bv = g / K, v = bv % V;
    Veh q{p.lf[v], p.lr[v], u_tick[g], noise ? noise[2 * bv] : 0.0,
          noise ? noise[2 * bv + 1] : 0.0};
    Stream ns{};
    if constexpr (kNoisy)
        ns = scpqp_noise_dev::make_stream(nz.seed, nz.sigma, nz.epoch, SCPQP_NOISE_SITE_PLANT,
                                          (uint32_t)k, (uint32_t)v, nz.b_offset + (uint32_t)(bv / V));
    double x[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = x_start[(size_t)bv * NX + i];
    if (k > 0) {
        const double T = k * tick;
        flow<kNoisy>(x, q, T, steps_for(T, hmax), ns);
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) x_path[(size_t)g * NX + i] = x[i];
}

__global__ __launch_bounds__(PT) void plant_kernel(scpqp_plant_params p, int B, int n_ticks,
                                                   double tick, double hmax, const double* x_start,
                                                   const double* u_tick, const double* noise,
                                                   double* x_path) {
    plant_lane<false>(p, B, n_ticks, tick, hmax, x_start, u_tick, noise, scpqp_noise{}, x_path);
}

__global__ __launch_bounds__(PT) void plant_kernel_noisy(scpqp_plant_params p, int B, int n_ticks,
                                                         double tick, double hmax,
                                                         const double* x_start,
                                                         const double* u_tick, scpqp_noise nz,
                                                         double* x_path) {
    plant_lane<true>(p, B, n_ticks, tick, hmax, x_start, u_tick, nullptr, nz, x_path);
}

// plant_lane with the lane's truth row (include/scpqp_truth.h): five loads, the
// validity guard, u_eff, then the same integration with the same step count.  A bad
// row makes its own outputs NaN and integrates nothing.
template <bool kNoisy>
__device__ __forceinline__ void plant_lane_truth(int V, int B, int n_ticks, double tick,
                                                 double hmax, const double* x_start,
                                                 const double* u_tick, const double* truth,
                                                 const double* noise, const scpqp_noise& nz,
                                                 double* x_path) {
    const int K = n_ticks + 1;
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= B * V * K) return;
    const int k = g % K, bv = g / K, v = bv % V;
    const double* row = truth + (size_t)bv * SCPQP_TRUTH_NP;
    const double lf = row[SCPQP_TRUTH_LF], lr = row[SCPQP_TRUTH_LR], tau = row[SCPQP_TRUTH_TAU];
    const double gain = row[SCPQP_TRUTH_GAIN], bias = row[SCPQP_TRUTH_BIAS];
    if (!(lf + lr > 0.0) || !(tau > 0.0)) {
#pragma unroll
        for (int i = 0; i < NX; ++i) x_path[(size_t)g * NX + i] = __builtin_nan("");
        return;
    }
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
    if (k > 0) {
        const double T = k * tick;
        flow<kNoisy>(x, q, T, steps_for(T, hmax), ns);
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) x_path[(size_t)g * NX + i] = x[i];
}

__global__ __launch_bounds__(PT) void plant_kernel_truth(int V, int B, int n_ticks, double tick,
                                                         double hmax, const double* x_start,
                                                         const double* u_tick,
                                                         const double* truth,
                                                         const double* noise, double* x_path) {
    plant_lane_truth<false>(V, B, n_ticks, tick, hmax, x_start, u_tick, truth, noise,
                            scpqp_noise{}, x_path);
}

__global__ __launch_bounds__(PT) void plant_kernel_truth_noisy(int V, int B, int n_ticks,
                                                               double tick, double hmax,
                                                               const double* x_start,
                                                               const double* u_tick,
                                                               const double* truth, scpqp_noise nz,
                                                               double* x_path) {
    plant_lane_truth<true>(V, B, n_ticks, tick, hmax, x_start, u_tick, truth, nullptr, nz,
                           x_path);
}

// one lane per (problem, vehicle): the nominal row of include/scpqp_truth.h
__global__ __launch_bounds__(PT) void truth_nominal_kernel(scpqp_plant_params p, int B,
                                                           double* truth) {
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= B * p.n_veh) return;
    const int v = g % p.n_veh;
    double* row = truth + (size_t)g * SCPQP_TRUTH_NP;
    row[SCPQP_TRUTH_LF] = p.lf[v];
    row[SCPQP_TRUTH_LR] = p.lr[v];
    row[SCPQP_TRUTH_TAU] = SCPQP_TRUTH_TAU_NOMINAL;
    row[SCPQP_TRUTH_GAIN] = 1.0;
    row[SCPQP_TRUTH_BIAS] = 0.0;
}

// one lane per (problem, vehicle): field f from the one Philox call of counter
// (f, 0, (site 3 << 24) | v, b_offset + b)
__global__ __launch_bounds__(PT) void truth_sample_kernel(scpqp_truth_dist d, int B,
                                                          double* truth) {
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= B * d.n_veh) return;
    const int b = g / d.n_veh, v = g % d.n_veh;
    double* row = truth + (size_t)g * SCPQP_TRUTH_NP;
    for (int f = 0; f < SCPQP_TRUTH_NP; ++f) {
        const scpqp_truth_field& fd = d.field[f];
        const double mean = d.mean[f][v];
        if (fd.kind == SCPQP_TRUTH_FIXED) {
            row[f] = mean;
            continue;
        }
        uint32_t c[4] = {(uint32_t)f, 0u, ((uint32_t)SCPQP_NOISE_SITE_TRUTH << 24) | (uint32_t)v,
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

// one lane per (problem, vehicle): the first n_eval draws of the (site, k) stream
__global__ __launch_bounds__(PT) void fill_kernel(scpqp_noise nz, int B, int V, int site, int k,
                                                  int n_eval, double* out) {
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= B * V) return;
    Stream ns = scpqp_noise_dev::make_stream(nz.seed, nz.sigma, nz.epoch, (uint32_t)site,
                                             (uint32_t)k, (uint32_t)(g % V),
                                             nz.b_offset + (uint32_t)(g / V));
    double* o = out + (size_t)g * n_eval * 2;
    for (int e = 0; e < n_eval; ++e) scpqp_noise_dev::draw(ns, o[2 * e], o[2 * e + 1]);
}

// one lane per (problem, vehicle): U[0] within +-umax and u0 +- du_lim, then
// U[j] within +-umax and U[j-1] +- du_lim (main.py:164-174), in place on the
// solver's vehicle-major layout u[v * hp + j]
__global__ __launch_bounds__(PT) void clip_kernel(int B, int V, int hp, int ld, double du_lim,
                                                  double* u, const double* u0, const double* umax) {
    const int g = blockIdx.x * PT + threadIdx.x;
    if (g >= B * V) return;
    const int b = g / V, v = g % V;
    double* uv = u + (size_t)b * ld + (size_t)v * hp;
    const double um = umax[g];
    double prev = u0[g];
    for (int j = 0; j < hp; ++j) {
        double w = uv[j];
        w = fmin(w, um);
        w = fmax(w, -um);
        w = fmin(w, prev + du_lim);
        w = fmax(w, prev - du_lim);
        uv[j] = w;
        prev = w;
    }
}

int check_params(const scpqp_plant_params* p) {
    if (!p) return scpqp_fail_(SCPQP_E_ARG, "null plant params");
    if (p->n_veh < 1 || p->n_veh > SCPQP_MAX_VEH) return scpqp_fail_(SCPQP_E_ARG, "n_veh out of range");
    for (int v = 0; v < p->n_veh; ++v)
        if (!(p->lf[v] + p->lr[v] > 0.0)) return scpqp_fail_(SCPQP_E_ARG, "lf + lr must be > 0");
    return 0;
}

int check_noise(const scpqp_noise* nz) {
    if (!nz) return scpqp_fail_(SCPQP_E_ARG, "null noise parameters");
    if (!(nz->sigma >= 0.0) || isinf(nz->sigma))
        return scpqp_fail_(SCPQP_E_ARG, "sigma must be finite and >= 0");
    return 0;
}

const char* const TRUTH_FIELD[SCPQP_TRUTH_NP] = {"lf", "lr", "tau", "gain", "bias"};

int fail_field(const char* what, int f) {
    static thread_local char msg[96];
    snprintf(msg, sizeof msg, "truth field %s: %s", TRUTH_FIELD[f], what);
    return scpqp_fail_(SCPQP_E_ARG, msg);
}

int check_truth_dist(const scpqp_truth_dist* d) {
    if (!d) return scpqp_fail_(SCPQP_E_ARG, "null truth distribution");
    if (d->n_veh < 1 || d->n_veh > SCPQP_MAX_VEH) return scpqp_fail_(SCPQP_E_ARG, "n_veh out of range");
    for (int f = 0; f < SCPQP_TRUTH_NP; ++f) {
        const scpqp_truth_field& fd = d->field[f];
        if (fd.kind < SCPQP_TRUTH_FIXED || fd.kind > SCPQP_TRUTH_NORMAL)
            return fail_field("kind must be 0 (fixed), 1 (uniform) or 2 (normal)", f);
        if (fd.kind == SCPQP_TRUTH_FIXED) continue;
        if (!(fd.spread >= 0.0) || isinf(fd.spread))
            return fail_field("spread must be finite and >= 0", f);
        if (!(fd.lo <= fd.hi)) return fail_field("lo must be <= hi", f);
    }
    // the smallest value the sampler can emit: never a row the plant would NaN
    auto floor_of = [d](int f, int v) {
        return d->field[f].kind == SCPQP_TRUTH_FIXED ? d->mean[f][v] : d->field[f].lo;
    };
    for (int v = 0; v < d->n_veh; ++v) {
        if (!(floor_of(SCPQP_TRUTH_LF, v) + floor_of(SCPQP_TRUTH_LR, v) > 0.0))
            return fail_field("the smallest lf + lr must be > 0", SCPQP_TRUTH_LF);
        if (!(floor_of(SCPQP_TRUTH_TAU, v) > 0.0))
            return fail_field("the smallest tau must be > 0", SCPQP_TRUTH_TAU);
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

int scpqp_delay_compensate(const scpqp_plant_params* p, int32_t B, double horizon, int32_t n_out,
                           const double* x_meas, const double* u_hold, const double* noise,
                           double* x0_out, double* traj_out, double h_max, void* stream) {
    if (int rc = check_params(p)) return rc;
    if (B < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size < 0");
    if (n_out < 2) return scpqp_fail_(SCPQP_E_ARG, "n_out must be >= 2");
    if (!(horizon >= 0.0) || !(h_max > 0.0)) return scpqp_fail_(SCPQP_E_ARG, "bad horizon / h_max");
    if (B == 0) return 0;
    if (!x_meas || !u_hold || !x0_out) return scpqp_fail_(SCPQP_E_ARG, "null array");
    const int n = B * p->n_veh;
    hipLaunchKernelGGL(delay_kernel, dim3((n + PT - 1) / PT), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), *p, B, horizon, n_out, h_max, x_meas,
                       u_hold, noise, x0_out, traj_out);
    return launched();
}

int scpqp_plant_step(const scpqp_plant_params* p, int32_t B, int32_t n_ticks, double tick,
                     const double* x_start, const double* u_tick, const double* noise,
                     double* x_path, double h_max, void* stream) {
    if (int rc = check_params(p)) return rc;
    if (B < 0 || n_ticks < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size / n_ticks < 0");
    if (!(tick > 0.0) || !(h_max > 0.0)) return scpqp_fail_(SCPQP_E_ARG, "bad tick / h_max");
    if (B == 0) return 0;
    if (!x_start || !u_tick || !x_path) return scpqp_fail_(SCPQP_E_ARG, "null array");
    const long long n = (long long)B * p->n_veh * (n_ticks + 1);
    if (n > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_veh * (n_ticks + 1) too large");
    hipLaunchKernelGGL(plant_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), *p, B, n_ticks, tick, h_max, x_start,
                       u_tick, noise, x_path);
    return launched();
}

int scpqp_delay_compensate_noisy(const scpqp_plant_params* p, int32_t B, double horizon,
                                 int32_t n_out, const double* x_meas, const double* u_hold,
                                 const scpqp_noise* nz, double* x0_out, double* traj_out,
                                 double h_max, void* stream) {
    if (int rc = check_params(p)) return rc;
    if (int rc = check_noise(nz)) return rc;
    if (B < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size < 0");
    if (n_out < 2) return scpqp_fail_(SCPQP_E_ARG, "n_out must be >= 2");
    if (!(horizon >= 0.0) || !(h_max > 0.0)) return scpqp_fail_(SCPQP_E_ARG, "bad horizon / h_max");
    if (B == 0) return 0;
    if (!x_meas || !u_hold || !x0_out) return scpqp_fail_(SCPQP_E_ARG, "null array");
    const long long n = (long long)B * p->n_veh;
    if (n > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_veh too large");
    hipLaunchKernelGGL(delay_kernel_noisy, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), *p, B, horizon, n_out, h_max, x_meas,
                       u_hold, *nz, x0_out, traj_out);
    return launched();
}

int scpqp_plant_step_noisy(const scpqp_plant_params* p, int32_t B, int32_t n_ticks, double tick,
                           const double* x_start, const double* u_tick, const scpqp_noise* nz,
                           double* x_path, double h_max, void* stream) {
    if (int rc = check_params(p)) return rc;
    if (int rc = check_noise(nz)) return rc;
    if (B < 0 || n_ticks < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size / n_ticks < 0");
    if (n_ticks >= SCPQP_NOISE_MAX_TICKS)
        return scpqp_fail_(SCPQP_E_SIZE, "n_ticks must be < 65536 (16 bits of the counter)");
    if (!(tick > 0.0) || !(h_max > 0.0)) return scpqp_fail_(SCPQP_E_ARG, "bad tick / h_max");
    if (B == 0) return 0;
    if (!x_start || !u_tick || !x_path) return scpqp_fail_(SCPQP_E_ARG, "null array");
    const long long n = (long long)B * p->n_veh * (n_ticks + 1);
    if (n > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_veh * (n_ticks + 1) too large");
    hipLaunchKernelGGL(plant_kernel_noisy, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), *p, B, n_ticks, tick, h_max, x_start,
                       u_tick, *nz, x_path);
    return launched();
}

int scpqp_noise_fill(const scpqp_noise* nz, int32_t B, int32_t n_veh, int32_t site, int32_t k,
                     int32_t n_eval, double* out, void* stream) {
    if (int rc = check_noise(nz)) return rc;
    if (B < 0 || n_eval < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size / n_eval < 0");
    if (n_veh < 1 || n_veh > SCPQP_MAX_VEH) return scpqp_fail_(SCPQP_E_ARG, "n_veh out of range");
    if (site < SCPQP_NOISE_SITE_DELAY || site > SCPQP_NOISE_SITE_LINEARIZE)
        return scpqp_fail_(SCPQP_E_ARG, "site must be 0, 1 or 2");
    if (k < 0) return scpqp_fail_(SCPQP_E_ARG, "k < 0");
    if (k >= SCPQP_NOISE_MAX_TICKS)
        return scpqp_fail_(SCPQP_E_SIZE, "k must be < 65536 (16 bits of the counter)");
    const long long n = (long long)B * n_veh;
    if (n * n_eval * 2 > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_veh * n_eval too large");
    if (B == 0 || n_eval == 0) return 0;
    if (!out) return scpqp_fail_(SCPQP_E_ARG, "null array");
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), *nz, B, n_veh, site, k, n_eval, out);
    return launched();
}

int scpqp_plant_step_truth(const scpqp_plant_params* p, int32_t B, int32_t n_ticks, double tick,
                           const double* x_start, const double* u_tick, const double* truth,
                           const double* noise, const scpqp_noise* nz,
                           double* x_path, double h_max, void* stream) {
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
    if (!x_start || !u_tick || !x_path) return scpqp_fail_(SCPQP_E_ARG, "null array");
    const long long n = (long long)B * p->n_veh * (n_ticks + 1);
    if (n > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_veh * (n_ticks + 1) too large");
    const dim3 grid((unsigned)((n + PT - 1) / PT));
    if (nz)
        hipLaunchKernelGGL(plant_kernel_truth_noisy, grid, dim3(PT), 0,
                           static_cast<hipStream_t>(stream), (int)p->n_veh, B, n_ticks, tick,
                           h_max, x_start, u_tick, truth, *nz, x_path);
    else
        hipLaunchKernelGGL(plant_kernel_truth, grid, dim3(PT), 0,
                           static_cast<hipStream_t>(stream), (int)p->n_veh, B, n_ticks, tick,
                           h_max, x_start, u_tick, truth, noise, x_path);
    return launched();
}

int scpqp_truth_fill_nominal(const scpqp_plant_params* p, int32_t B, double* truth, void* stream) {
    if (int rc = check_params(p)) return rc;
    if (B < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size < 0");
    if (B == 0) return 0;
    if (!truth) return scpqp_fail_(SCPQP_E_ARG, "null truth array");
    const long long n = (long long)B * p->n_veh;
    if (n * SCPQP_TRUTH_NP > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_veh too large");
    hipLaunchKernelGGL(truth_nominal_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), *p, B, truth);
    return launched();
}

int scpqp_truth_sample(const scpqp_truth_dist* d, int32_t B, double* truth, void* stream) {
    if (int rc = check_truth_dist(d)) return rc;
    if (B < 0) return scpqp_fail_(SCPQP_E_ARG, "batch size < 0");
    if (B == 0) return 0;
    if (!truth) return scpqp_fail_(SCPQP_E_ARG, "null truth array");
    const long long n = (long long)B * d->n_veh;
    if (n * SCPQP_TRUTH_NP > 0x7fffffffLL) return scpqp_fail_(SCPQP_E_SIZE, "B * n_veh too large");
    hipLaunchKernelGGL(truth_sample_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), *d, B, truth);
    return launched();
}

int scpqp_clip_controls(int32_t B, int32_t n_veh, int32_t hp, int32_t ld, double du_lim, double* u,
                        const double* u0, const double* umax, void* stream) {
    if (B < 0 || n_veh < 1 || hp < 1 || ld < n_veh * hp) return scpqp_fail_(SCPQP_E_ARG, "bad sizes");
    if (B == 0) return 0;
    if (!u || !u0 || !umax) return scpqp_fail_(SCPQP_E_ARG, "null array");
    const int n = B * n_veh;
    hipLaunchKernelGGL(clip_kernel, dim3((n + PT - 1) / PT), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), B, n_veh, hp, ld, du_lim, u, u0, umax);
    return launched();
}

}  // extern "C"
