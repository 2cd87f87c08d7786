// governor.hip — speed governor on MI355X (fp64): a longitudinal command per (realisation,
// vehicle) from the plan the solve returned (include/scpqp_governor.h).
//
//   scpqp_governor_step   per (b, v) the smallest clearance of the plan's first LOOK points to
//                         the told obstacle points and to the other vehicles' plans, the first
//                         conflicting step, and the acceleration command: brake on a conflict,
//                         else the speed loop; slew limit; stop rule
//
// Sixteen threads per (b, v), so four lanes share a wave and sixteen a workgroup of 256.  The
// (step, other) pairs of a lane, other = an obstacle or another vehicle, are strided over its
// sixteen threads; the two minima (the clearance, and the first step with a negative one) are
// reduced by a __shfl butterfly of width 16, and thread 0 of the group runs steps 2 to 4 of the
// header and writes the outputs.  No LDS, no scratch.  Minima are free of order, so k_conf and
// clear do not depend on this mapping.
//
// No thread leaves before the last exchange (the rule at the top of imm.hip): groups past the
// batch run on clamped addresses with an empty pair loop and store nothing, off and bad lanes
// have an empty pair loop too, and the loop, whose trip count differs between the groups of a
// wave, holds no exchange: the butterfly comes after it, where the wave has converged.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>

#include "scpqp_entry_checks.h"
#include "scpqp_governor.h"

namespace {

constexpr int NP = SCPQP_GOV_NP;
constexpr int GW = 16;    // threads per (b, v)
constexpr int PT = 256;   // threads per workgroup: PT / GW lanes (b, v)

__global__ __launch_bounds__(PT) void governor_kernel(
    int n, int nV, int nO, int hp_max, double t_hold, double t_back,
    const double* __restrict__ x0, const double* __restrict__ traj,
    const double* __restrict__ obst, const double* __restrict__ margin,
    const int* __restrict__ hp, const double* __restrict__ dreq_obs,
    const double* __restrict__ dreq_veh, const double* __restrict__ gov,
    double* __restrict__ a_cmd, int* __restrict__ k_conf, double* __restrict__ clear) {
    const long long lane = (long long)blockIdx.x * (PT / GW) + (threadIdx.x >> 4);
    const int sub = threadIdx.x & (GW - 1);
    const bool in = lane < n;                     // the same for the whole group
    const int g = in ? (int)lane : n - 1;         // clamped: the reads stay inside the arrays
    const int b = g / nV, v = g - b * nV;

    double row[NP];
#pragma unroll
    for (int f = 0; f < NP; ++f) row[f] = gov[(size_t)g * NP + f];
    bool off = true, bad = false;
#pragma unroll
    for (int f = 0; f < NP; ++f) {
        off &= row[f] == 0.0;
        bad |= row[f] < 0.0 || !(isfinite(row[f]) || (f == SCPQP_GOV_J_MAX && row[f] > 0.0));
    }
    const double look = row[SCPQP_GOV_LOOK], band = row[SCPQP_GOV_BAND];
    bad |= !(look <= (double)SCPQP_MAX_HP) || look != floor(look);
    const double a_now = x0[(size_t)g * 6 + 4];
    const double s = off ? 0.0 : x0[(size_t)g * 6 + 3];
    const int hb = (hp && !off) ? hp[b] : hp_max;
    bad |= !isfinite(s) || !isfinite(a_now) || hb < 1 || hb > hp_max;
    bad &= !off;                                  // an off row is off whatever its state holds

    // 1. the pairs (k, j) of this lane, j < nO an obstacle, else vehicle j - nO
    const int K = (in && !off && !bad) ? min((int)look, hb) : 0;
    const int no = nO + nV, total = K * no;
    const double* tb = traj + (size_t)b * hp_max * 2 * nV;
    const double* ob = obst ? obst + (size_t)b * nO * 2 * hp_max : nullptr;
    const double* mb = margin ? margin + (size_t)b * nO * hp_max : nullptr;
    const double* dob = dreq_obs ? dreq_obs + (size_t)g * nO : nullptr;
    const double* dvb = dreq_veh + (size_t)g * nV;
    double cmin = INFINITY;
    int kmin = INT_MAX;
    for (int idx = sub; idx < total; idx += GW) {
        const int k = idx / no, j = idx - k * no;
        const int w = j - nO;
        if (w == v) continue;
        const double px = tb[(size_t)k * 2 * nV + v], py = tb[(size_t)k * 2 * nV + nV + v];
        double qx, qy, need;
        if (j < nO) {
            qx = ob[(size_t)(2 * j) * hb + k];
            qy = ob[(size_t)(2 * j + 1) * hb + k];
            need = dob[j] + (mb ? mb[(size_t)j * hb + k] : 0.0);
        } else {
            qx = tb[(size_t)k * 2 * nV + w];
            qy = tb[(size_t)k * 2 * nV + nV + w];
            need = dvb[w];
        }
        const bool fin = isfinite(px) && isfinite(py) && isfinite(qx) && isfinite(qy) &&
                         isfinite(need);
        const double dx = px - qx, dy = py - qy;
        double c = sqrt(dx * dx + dy * dy) - (need + band);
        c = (fin && c == c) ? c : -INFINITY;
        cmin = fmin(cmin, c);
        kmin = c < 0.0 ? min(kmin, k) : kmin;
    }
#pragma unroll
    for (int d = GW / 2; d >= 1; d >>= 1) {
        const double oc = __shfl_xor(cmin, d, GW);
        const int ok = __shfl_xor(kmin, d, GW);
        cmin = fmin(cmin, oc);
        kmin = min(kmin, ok);
    }

    if (in && sub == 0) {
        const bool conflict = kmin != INT_MAX;
        const double a_brake = row[SCPQP_GOV_A_BRAKE], j_max = row[SCPQP_GOV_J_MAX];
        // 2. the wish
        double a = fmin(fmax(row[SCPQP_GOV_K_V] * (row[SCPQP_GOV_V_REF] - s), -a_brake),
                        row[SCPQP_GOV_A_ACC]);
        a = conflict ? -a_brake : a;
        // 3. the slew limit
        if (isfinite(j_max)) {
            const double d = j_max * t_hold;
            a = fmin(fmax(a, a_now - d), a_now + d);
        }
        // 4. the stop rule
        const double s_app = fmax(s - a_now * t_back, 0.0);
        a = fmax(a, -s_app / t_hold);
        a_cmd[g] = off ? a_now : (bad ? NAN : a);
        if (k_conf) k_conf[g] = off ? -1 : (bad ? -2 : (conflict ? kmin : -1));
        if (clear) clear[g] = (off || bad) ? NAN : cmin;
    }
}

}  // namespace

extern "C" {

int scpqp_governor_step(int32_t n_veh, int32_t n_obst, int32_t hp_max, int32_t B, double t_hold,
                        double t_back, const double* x0, const double* traj, const double* obst,
                        const double* obst_margin, const int32_t* hp, const double* dreq_obs,
                        const double* dreq_veh, const double* gov, double* a_cmd,
                        int32_t* k_conf, double* clear, void* stream) {
    if (int rc = scpqp_host::conflict_step_checks(n_veh, n_obst, hp_max, B, t_hold, t_back, x0, traj,
                                                  obst, dreq_obs, dreq_veh, gov, NP,
                                                  "null gov rows array", a_cmd))
        return rc < 0 ? rc : 0;
    const long long n = (long long)B * n_veh;
    constexpr int per = PT / GW;
    // with no obstacle the obstacle arrays are not the kernel's to look at
    hipLaunchKernelGGL(governor_kernel, dim3((unsigned)((n + per - 1) / per)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), (int)n, (int)n_veh, (int)n_obst,
                       (int)hp_max, t_hold, t_back, x0, traj, n_obst ? obst : nullptr,
                       n_obst ? obst_margin : nullptr, hp, n_obst ? dreq_obs : nullptr, dreq_veh,
                       gov, a_cmd, k_conf, clear);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return scpqp_fail_(SCPQP_E_HIP, hipGetErrorString(e));
    return 0;
}

}  // extern "C"
