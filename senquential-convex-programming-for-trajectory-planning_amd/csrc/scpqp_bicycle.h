// scpqp_bicycle.h — the bicycle right-hand side and its fixed-step RK4 flow (device
// side of the plant: Model.py:61-87), shared by plant.hip (delay compensation, plant
// step), estimator.hip (the filter's prediction) and drive.hip (the plant step behind a
// longitudinal actuator): one integrator, stated once.
#ifndef SCPQP_BICYCLE_H
#define SCPQP_BICYCLE_H

#include <hip/hip_runtime.h>

#include <math.h>

#include "scpqp_philox.h"

namespace scpqp_plant_dev {

constexpr int NX = 6;

struct Veh {
    double lf, lr, uref, n0, n1;
};

// Model.py:61-87 (BicyleModel.ode / odes_): dx for state
// [x, y, heading, speed (rear axle), acceleration, steering angle].
// n0, n1: the additive noise of dx[0], dx[1] (Model.py:84-86).  The reference
// draws it anew per right-hand-side evaluation: the kNoisy integrators below do
// the same from the lane's Philox stream (include/scpqp_noise.h) before every
// call.  The entry points of scpqp.h hold the caller's pair constant over the
// call instead (zero when noise is NULL; is_noise is False in main.py:235).
__device__ __forceinline__ void bicycle(const double (&x)[NX], const Veh& p, double (&dx)[NX]) {
    const double L = p.lf + p.lr, R = p.lr / L;
    const double tu = tan(x[5]);
    const double vc = x[3] * sqrt(1.0 + (R * tu) * (R * tu));
    const double beta = atan(R * tu);
    dx[0] = vc * cos(x[2] + beta) + p.n0;
    dx[1] = vc * sin(x[2] + beta) + p.n1;
    dx[2] = vc * tu * cos(beta) / L;
    dx[3] = x[4];
    dx[4] = 0.0;
    dx[5] = (p.uref - x[5]) / 0.1;
}

// a vehicle of the plant truth (include/scpqp_truth.h): uref holds u_eff, formed once
// per lane, and tau divides where 0.1 does; the right-hand side is otherwise bicycle()'s
struct VehT : Veh {
    double tau;
};

__device__ __forceinline__ void bicycle(const double (&x)[NX], const VehT& p, double (&dx)[NX]) {
    const double L = p.lf + p.lr, R = p.lr / L;
    const double tu = tan(x[5]);
    const double vc = x[3] * sqrt(1.0 + (R * tu) * (R * tu));
    const double beta = atan(R * tu);
    dx[0] = vc * cos(x[2] + beta) + p.n0;
    dx[1] = vc * sin(x[2] + beta) + p.n1;
    dx[2] = vc * tu * cos(beta) / L;
    dx[3] = x[4];
    dx[4] = 0.0;
    dx[5] = (p.uref - x[5]) / p.tau;
}

// a vehicle of the drive truth (include/scpqp_drive.h) with a lag or the hold rule: the
// acceleration x[4] answers a_eff with the lag tau_a (lag == false: it is constant), and with
// hold the brakes do not push a standing vehicle backwards.  A lane with neither is a VehT.
struct VehD : VehT {
    double a_eff, tau_a;
    bool lag, hold;
};

__device__ __forceinline__ void bicycle(const double (&x)[NX], const VehD& p, double (&dx)[NX]) {
    const double L = p.lf + p.lr, R = p.lr / L;
    const double tu = tan(x[5]);
    const double vc = x[3] * sqrt(1.0 + (R * tu) * (R * tu));
    const double beta = atan(R * tu);
    dx[0] = vc * cos(x[2] + beta) + p.n0;
    dx[1] = vc * sin(x[2] + beta) + p.n1;
    dx[2] = vc * tu * cos(beta) / L;
    dx[3] = (p.hold && !(x[3] > 0.0) && x[4] < 0.0) ? 0.0 : x[4];
    dx[4] = p.lag ? (p.a_eff - x[4]) / p.tau_a : 0.0;
    dx[5] = (p.uref - x[5]) / p.tau;
}

using scpqp_noise_dev::Stream;

// kNoisy: p.n0, p.n1 are redrawn before each of the four evaluations (c0 order
// k1, k2, k3, k4); else p is left as it is and ns is unused
template <bool kNoisy, class VehX>
__device__ __forceinline__ void rk4(double (&x)[NX], VehX& p, double h, Stream& ns) {
    double k1[NX], k2[NX], k3[NX], k4[NX], y[NX];
    if constexpr (kNoisy) scpqp_noise_dev::draw(ns, p.n0, p.n1);
    bicycle(x, p, k1);
#pragma unroll
    for (int i = 0; i < NX; ++i) y[i] = x[i] + 0.5 * h * k1[i];
    if constexpr (kNoisy) scpqp_noise_dev::draw(ns, p.n0, p.n1);
    bicycle(y, p, k2);
#pragma unroll
    for (int i = 0; i < NX; ++i) y[i] = x[i] + 0.5 * h * k2[i];
    if constexpr (kNoisy) scpqp_noise_dev::draw(ns, p.n0, p.n1);
    bicycle(y, p, k3);
#pragma unroll
    for (int i = 0; i < NX; ++i) y[i] = x[i] + h * k3[i];
    if constexpr (kNoisy) scpqp_noise_dev::draw(ns, p.n0, p.n1);
    bicycle(y, p, k4);
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] += h / 6.0 * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
}

// integrate x over a span of length T with n equal RK4 steps
template <bool kNoisy, class VehX>
__device__ __forceinline__ void flow(double (&x)[NX], VehX& p, double T, int n, Stream& ns) {
    const double h = T / n;
    for (int s = 0; s < n; ++s) rk4<kNoisy>(x, p, h, ns);
}

// flow() of a VehD: with hold, a speed that was >= 0 before an RK4 step and is < 0 after it
// is set to exactly 0 (include/scpqp_drive.h)
template <bool kNoisy>
__device__ __forceinline__ void flow_drive(double (&x)[NX], VehD& p, double T, int n, Stream& ns) {
    const double h = T / n;
    for (int s = 0; s < n; ++s) {
        const double s0 = x[3];
        rk4<kNoisy>(x, p, h, ns);
        if (p.hold && s0 >= 0.0 && x[3] < 0.0) x[3] = 0.0;
    }
}

__device__ __forceinline__ int steps_for(double T, double hmax) {
    const int n = (int)ceil(fabs(T) / hmax - 1e-9);
    return n < 1 ? 1 : n;
}

}  // namespace scpqp_plant_dev

#endif  // SCPQP_BICYCLE_H
