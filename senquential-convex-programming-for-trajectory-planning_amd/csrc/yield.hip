// yield.hip — right of way and graded braking on MI355X (fp64): a longitudinal command per
// (realisation, vehicle) from the plan the solve returned (include/scpqp_yield.h).
//
//   scpqp_yield_step   per (b, v) which of the other vehicles count (rank, standing, a row of
//                      their own), the smallest clearance of the plan's first LOOK points, the
//                      first step with any conflict and with a conflict that counts, whom the
//                      lane yields to, the length of the plan before that conflict, and the
//                      acceleration command: a deceleration sized to stop there, else the speed
//                      loop; slew limit; stop rule
//
// The governor's shape (governor.hip): sixteen threads per (b, v), four lanes per wave, sixteen
// per workgroup of 256.  SCPQP_MAX_VEH is 16, so thread `sub` of a group classifies vehicle
// w = sub once (rule 2 of the header) and a ballot hands every thread of the group the sixteen
// "counts" bits: the rows of the other vehicles are not read again per pair.  The (step, other)
// pairs are strided over the sixteen threads with three running minima: the clearance, the step
// of any conflict, and the key k (n_obst + n_veh) + j of a conflict that counts, whose halves are
// k_conf and who.  A __shfl_xor butterfly of width 16 reduces them; then the segments
// j < k_conf of d_stop are strided over the same threads and added by a second butterfly, and
// thread 0 of the group runs steps 4 and 5 of the header and writes.  No LDS, no scratch.
//
// The clearance is the expression of governor.hip, restated token for token, so that it
// compiles to the same operations (the fused multiply-add of the squared distance included):
// the reduction to scpqp_governor_step is bitwise.
//
// No thread leaves before the last exchange (the rule at the top of imm.hip): groups past the
// batch run on clamped addresses with empty loops and store nothing, off and bad lanes have empty
// loops too, and the loops, whose trip counts differ between the groups of a wave, hold no
// exchange: the ballot comes before them and the butterflies after, where the wave has converged.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>

#include "scpqp_entry_checks.h"
#include "scpqp_yield.h"

namespace {

constexpr int NP = SCPQP_YLD_NP;
constexpr int GW = 16;    // threads per (b, v)
constexpr int PT = 256;   // threads per workgroup: PT / GW lanes (b, v)

static_assert(SCPQP_MAX_VEH <= GW, "one thread of a group per other vehicle");

// the header's rules on the fields of a row alone
__device__ __forceinline__ void classify_row(const double (&row)[NP], bool& off, bool& bad) {
    off = true;
    bad = false;
#pragma unroll
    for (int f = 0; f < NP; ++f) {
        off &= row[f] == 0.0;
        bad |= row[f] < 0.0 || !(isfinite(row[f]) || (f == SCPQP_GOV_J_MAX && row[f] > 0.0));
    }
    const double look = row[SCPQP_GOV_LOOK], prio = row[SCPQP_YLD_PRIO];
    bad |= !(look <= (double)SCPQP_MAX_HP) || look != floor(look);
    bad |= !(prio <= (double)SCPQP_YLD_PRIO_MAX) || prio != floor(prio);
    bad |= !(row[SCPQP_YLD_A_EASE] <= row[SCPQP_GOV_A_BRAKE]);
    bad &= !off;
}

__global__ __launch_bounds__(PT) void yield_kernel(
    int n, int nV, int nO, int hp_max, double t_hold, double t_back,
    const double* __restrict__ x0, const double* __restrict__ traj,
    const double* __restrict__ obst, const double* __restrict__ margin,
    const int* __restrict__ hp, const double* __restrict__ dreq_obs,
    const double* __restrict__ dreq_veh, const double* __restrict__ yld,
    double* __restrict__ a_cmd, int* __restrict__ k_conf, int* __restrict__ k_any,
    int* __restrict__ who, double* __restrict__ clear, double* __restrict__ d_stop) {
    const long long lane = (long long)blockIdx.x * (PT / GW) + (threadIdx.x >> 4);
    const int sub = threadIdx.x & (GW - 1);
    const bool in = lane < n;                     // the same for the whole group
    const int g = in ? (int)lane : n - 1;         // clamped: the reads stay inside the arrays
    const int b = g / nV, v = g - b * nV;

    // 1. the own row
    double row[NP];
#pragma unroll
    for (int f = 0; f < NP; ++f) row[f] = yld[(size_t)g * NP + f];
    bool off, bad;
    classify_row(row, off, bad);
    const double look = row[SCPQP_GOV_LOOK], band = row[SCPQP_GOV_BAND];
    const double a_now = x0[(size_t)g * 6 + 4];
    const double s = off ? 0.0 : x0[(size_t)g * 6 + 3];
    const int hb = (hp && !off) ? hp[b] : hp_max;
    bad |= !isfinite(s) || !isfinite(a_now) || hb < 1 || hb > hp_max;
    bad &= !off;                                  // an off row is off whatever its state holds
    const bool live = in && !off && !bad;

    // 2. who counts: thread sub asks vehicle w = sub, the ballot collects the group's bits
    bool counts = true;
    if (live && sub < nV && sub != v) {
        const size_t gw = (size_t)b * nV + sub;
        double other[NP];
#pragma unroll
        for (int f = 0; f < NP; ++f) other[f] = yld[gw * NP + f];
        bool w_off, w_bad;
        classify_row(other, w_off, w_bad);
        const double s_stand = row[SCPQP_YLD_S_STAND];
        const bool standing = s_stand > 0.0 && !(x0[gw * 6 + 3] > s_stand);
        counts = !(!w_off && !w_bad && row[SCPQP_YLD_PRIO] > other[SCPQP_YLD_PRIO] && !standing);
    }
    const unsigned long long votes = __ballot(counts);
    const unsigned mask = (unsigned)(votes >> (threadIdx.x & 48)) & 0xffffu;

    // 3. the pairs (k, j) of this lane, j < nO an obstacle, else vehicle j - nO
    const int K = live ? min((int)look, hb) : 0;
    const int no = nO + nV, total = K * no;
    const double* tb = traj + (size_t)b * hp_max * 2 * nV;
    const double* ob = obst ? obst + (size_t)b * nO * 2 * hp_max : nullptr;
    const double* mb = margin ? margin + (size_t)b * nO * hp_max : nullptr;
    const double* dob = dreq_obs ? dreq_obs + (size_t)g * nO : nullptr;
    const double* dvb = dreq_veh + (size_t)g * nV;
    double cmin = INFINITY;
    int kmin = INT_MAX, key = INT_MAX;
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
        const bool num = fin && c == c;
        c = num ? c : -INFINITY;
        cmin = fmin(cmin, c);
        kmin = c < 0.0 ? min(kmin, k) : kmin;
        // an obstacle counts, a vehicle by its bit, what is not a number whatever the ranks
        const bool counted = j < nO || ((mask >> w) & 1u) || !num;
        key = (c < 0.0 && counted) ? min(key, idx) : key;
    }
#pragma unroll
    for (int d = GW / 2; d >= 1; d >>= 1) {
        const double oc = __shfl_xor(cmin, d, GW);
        const int ok = __shfl_xor(kmin, d, GW);
        const int oy = __shfl_xor(key, d, GW);
        cmin = fmin(cmin, oc);
        kmin = min(kmin, ok);
        key = min(key, oy);
    }

    // 4. the length of the plan before the conflict: segments j < k_conf, every thread of the
    //    group holds the same key
    const bool conflict = key != INT_MAX;
    const int kc = conflict ? key / no : 0;       // kc < K <= hb
    double ds = 0.0;
    for (int j = sub; j < kc; j += GW) {
        const double ax = j ? tb[(size_t)(j - 1) * 2 * nV + v] : x0[(size_t)g * 6 + 0];
        const double ay = j ? tb[(size_t)(j - 1) * 2 * nV + nV + v] : x0[(size_t)g * 6 + 1];
        const double ex = tb[(size_t)j * 2 * nV + v] - ax, ey = tb[(size_t)j * 2 * nV + nV + v] - ay;
        ds += sqrt(ex * ex + ey * ey);
    }
#pragma unroll
    for (int d = GW / 2; d >= 1; d >>= 1) ds += __shfl_xor(ds, d, GW);

    if (in && sub == 0) {
        const double a_brake = row[SCPQP_GOV_A_BRAKE], j_max = row[SCPQP_GOV_J_MAX];
        // the wish
        double a = fmin(fmax(row[SCPQP_GOV_K_V] * (row[SCPQP_GOV_V_REF] - s), -a_brake),
                        row[SCPQP_GOV_A_ACC]);
        const double sp = fmax(s, 0.0);
        const double a_need = (ds > 0.0 && isfinite(ds)) ? sp * sp / (2.0 * ds) : INFINITY;
        a = conflict ? -fmin(a_brake, fmax(row[SCPQP_YLD_A_EASE], a_need)) : a;
        // the slew limit
        if (isfinite(j_max)) {
            const double d = j_max * t_hold;
            a = fmin(fmax(a, a_now - d), a_now + d);
        }
        // the stop rule
        const double s_app = fmax(s - a_now * t_back, 0.0);
        a = fmax(a, -s_app / t_hold);
        const int none = off ? -1 : -2;
        const bool dead = off || bad;
        a_cmd[g] = off ? a_now : (bad ? NAN : a);
        if (k_conf) k_conf[g] = dead ? none : (conflict ? kc : -1);
        if (k_any) k_any[g] = dead ? none : (kmin != INT_MAX ? kmin : -1);
        if (who) who[g] = dead ? none : (conflict ? key - kc * no : -1);
        if (clear) clear[g] = dead ? NAN : cmin;
        if (d_stop) d_stop[g] = dead ? NAN : (conflict ? ds : INFINITY);
    }
}

}  // namespace

extern "C" {

int scpqp_yield_step(int32_t n_veh, int32_t n_obst, int32_t hp_max, int32_t B, double t_hold,
                     double t_back, const double* x0, const double* traj, const double* obst,
                     const double* obst_margin, const int32_t* hp, const double* dreq_obs,
                     const double* dreq_veh, const double* yld, double* a_cmd, int32_t* k_conf,
                     int32_t* k_any, int32_t* who, double* clear, double* d_stop, void* stream) {
    if (int rc = scpqp_host::conflict_step_checks(n_veh, n_obst, hp_max, B, t_hold, t_back, x0, traj,
                                                  obst, dreq_obs, dreq_veh, yld, NP,
                                                  "null yld rows array", a_cmd))
        return rc < 0 ? rc : 0;
    const long long n = (long long)B * n_veh;
    constexpr int per = PT / GW;
    // with no obstacle the obstacle arrays are not the kernel's to look at
    hipLaunchKernelGGL(yield_kernel, dim3((unsigned)((n + per - 1) / per)), dim3(PT), 0,
                       static_cast<hipStream_t>(stream), (int)n, (int)n_veh, (int)n_obst,
                       (int)hp_max, t_hold, t_back, x0, traj, n_obst ? obst : nullptr,
                       n_obst ? obst_margin : nullptr, hp, n_obst ? dreq_obs : nullptr, dreq_veh,
                       yld, a_cmd, k_conf, k_any, who, clear, d_stop);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return scpqp_fail_(SCPQP_E_HIP, hipGetErrorString(e));
    return 0;
}

}  // extern "C"
