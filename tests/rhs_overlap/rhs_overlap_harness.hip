// Test harness (not linked into libscpqp.so): the three assemble-and-factor phases of
// csrc/scpqp_kernel.h, each run on the same problem state with its right-hand side formed in
// front of the factorisation (all four waves) and beside it (the factorisation's side job on
// the non-lead waves), so that tests/test_gpu_rhs_overlap.py can demand that the two orders
// leave the same bits behind and write nothing they do not own.
//
// One translation unit per kernel instantiation under test, -DRO_UNIT=1..4, and one with
// -DRO_UNIT=0 for the C entry points (tests/rhs_overlap_harness.py builds and binds them).
//
// Per case (RoCase) a workgroup of 256 threads
//   * fills its whole dynamic LDS and its workspace slice with a canary pattern;
//   * loads the problem state (g, the constraint rows, d, tv, the polish mask and
//     multipliers, rd, q, dz) from the host's arrays into the plan's own layout;
//   * copies the LDS and the workspace out ("before");
//   * runs the site in the order asked for:
//       site 0  ph_scale_assemble_rhs_factor                      (IPM iteration)
//       site 1  ph_assemble_factor (+ ph_polish_rhs in front)     (polish round that refactors)
//       site 2  ph_init_a, ph_init_assemble_factor (+ ph_rhs_from_tv in front)   (cold start)
//       site 3  a given matrix K in place of the assembly, then site 0's right-hand side and
//               the factorisation (the failure path: K need not be positive definite)
//   * copies the LDS and the workspace out again ("after") and the phase's return value.
#include "../../senquential-convex-programming-for-trajectory-planning_amd/csrc/scpqp_kernel.h"

#include <cstdint>

#ifndef RO_UNIT
#define RO_UNIT 0
#endif

struct RoCase {
    int Hb, lead, site, order, inoff, ooff, koff, pad;
};
constexpr int kRoHdr = 8;   // doubles in front of a case's output: [0] the phase's return value
constexpr int kRoUnits = 4;
constexpr size_t kRoLdsLimit = 163840;

// (HG, VG, RM, OCC, SH of the layout) of a unit; unit 4 (c5's kernel) runs the phases of the
// horizon's class (shapes 4-6), as the kernel's own dispatch does
__host__ __device__ constexpr bool ro_vg(int u) { return u >= 3; }
__host__ __device__ constexpr int ro_rm(int u) { return u == 1 ? 1 : 2; }
__host__ __device__ constexpr int ro_occ(int u) { return u == 4 ? 2 : 3; }
__host__ __device__ constexpr int ro_sh(int u) { return u == 3 ? 1 : (u == 4 ? 2 : 0); }

// doubles of a case's input: g rowE rowW rowH dd tv sa la rd qs dz
__host__ __device__ inline int ro_in_doubles(int V, int O, int Hb) {
    const int N = V * Hb, n = N + 1, m = V * (V - 1) / 2 * Hb + V * O * Hb, mc = m + 2 * N + 1;
    return 2 * N + 2 * m + m + m + 4 * mc + n + N + n;
}

typedef int (*RoLaunch)(int, const RoCase*, const DevParams*, const double*, double*, double*, int, int, int);

#if RO_UNIT != 0
namespace {
__device__ __forceinline__ double ro_canary(int region, int e) {
    return __longlong_as_double(0x7ff8c0de00000000ll | ((long long)region << 24) | (long long)e);
}

template <bool HG, bool VG, int RM, int OCC, int SH>
__device__ __noinline__ int ro_site(const RoCase& d, Ctx c, const double* in) {
    const Lay<HG, VG, RM, OCC> L = lay_of<HG, VG, RM, OCC, SH>(c);
    const cParams& P = *c.P;
    const bool ovl = d.order != 0;
    int ret = 1;
    if (d.site == 0) {
        ret = ovl ? ph_scale_assemble_rhs_factor<HG, VG, RM, OCC, SH, true>(c)
                  : ph_scale_assemble_rhs_factor<HG, VG, RM, OCC, SH, false>(c);
    } else if (d.site == 1) {
        if (ovl) {
            ret = ph_assemble_factor<HG, VG, RM, OCC, SH, true>(c, P.polRho);
        } else {
            ret = ph_assemble_factor<HG, VG, RM, OCC, SH, false>(c, P.polRho);
            if (ret) ph_polish_rhs<HG, VG, RM, OCC, SH>(c);
        }
    } else if (d.site == 2) {
        ph_init_a<HG, VG, RM, OCC, SH>(c);
        if (ovl) {
            ph_init_assemble_factor<HG, VG, RM, OCC, SH, true>(c);
        } else {
            ph_init_assemble_factor<HG, VG, RM, OCC, SH, false>(c);
            ph_rhs_from_tv<HG, VG, RM, OCC, SH>(c, 0.0);
        }
    } else {
        const int n = L.n, F = n * (n + 1) / 2;
        for (int e = threadIdx.x; e < F; e += NT) {
            int i, j;
            tri_decode(e, i, j);
            L.H[roff(i) + j] = in[d.koff + e];
        }
        __syncthreads();
        if (ovl && side_fits<2>(L)) {
            ret = cholesky(L, newton_rhs_side(L)) ? 1 : 0;
        } else {
            RowsMem<Lay<HG, VG, RM, OCC>> A{L};
            newton_rhs_body<false>(L, A, 0, 0.0);
            ret = cholesky(L) ? 1 : 0;
        }
    }
    return ret;
}

template <bool HG, bool VG, int RM, int OCC, int SHL>
__global__ __launch_bounds__(NT, OCC) void ro_kernel(const RoCase* cases, const DevParams* Pd, const double* in,
                                                     double* out, double* wsAll, int ldsN, int wsN) {
    const RoCase d = cases[blockIdx.x];
    const int tid = threadIdx.x;
    const cParams* Pp = (const cParams*)Pd;
    const cParams& P = *Pp;
    ldouble* lds = (ldouble*)smem_;
    gdouble* ws = (gdouble*)(wsAll + (size_t)blockIdx.x * wsN);
    const Ctx c{Pp, ws, d.Hb, d.lead};
    const Lay<HG, VG, RM, OCC> L = lay_of<HG, VG, RM, OCC, SHL>(c);
    for (int e = tid; e < ldsN; e += NT) lds[e] = ro_canary(1, e);
    for (int e = tid; e < wsN; e += NT) ws[e] = ro_canary(2, e);
    __syncthreads();
    const int N = L.N, n = L.n, m = L.m, mc = L.mc;
    const double* p = in + d.inoff;
    for (int e = tid; e < 2 * N; e += NT) L.g[e] = p[e];
    p += 2 * N;
    for (int e = tid; e < 2 * m; e += NT) L.rowE[e] = p[e];
    p += 2 * m;
    for (int e = tid; e < m; e += NT) L.rowW[e] = p[e];
    p += m;
    for (int e = tid; e < m; e += NT) L.rowH[e] = p[e];
    p += m;
    for (int e = tid; e < mc; e += NT) {
        L.dd[e] = p[e];
        L.tv[e] = p[mc + e];
        L.sa[e] = p[2 * mc + e];
        L.la[e] = p[3 * mc + e];
    }
    p += 4 * mc;
    for (int e = tid; e < n; e += NT) L.rd[e] = p[e];
    p += n;
    for (int e = tid; e < N; e += NT) L.qs[e] = p[e];
    p += N;
    for (int e = tid; e < n; e += NT) L.dz[e] = p[e];
    if (tid == 0) L.red[kIdlSlot] = 1.0 / P.polDelta;
    __syncthreads();
    double* o = out + d.ooff;
    for (int e = tid; e < ldsN; e += NT) o[kRoHdr + e] = lds[e];
    for (int e = tid; e < wsN; e += NT) o[kRoHdr + ldsN + e] = ws[e];
    __syncthreads();
    int ret;
    if constexpr (SHL == 2) {   // c5's kernel: the phases of the horizon's class
        if (d.Hb == 30) ret = ro_site<HG, VG, RM, OCC, 6>(d, c, in);
        else if (d.Hb == 20) ret = ro_site<HG, VG, RM, OCC, 5>(d, c, in);
        else if (d.Hb == 10) ret = ro_site<HG, VG, RM, OCC, 4>(d, c, in);
        else ret = ro_site<HG, VG, RM, OCC, SHL>(d, c, in);
    } else {
        ret = ro_site<HG, VG, RM, OCC, SHL>(d, c, in);
    }
    __syncthreads();
    o += kRoHdr + ldsN + wsN;
    for (int e = tid; e < ldsN; e += NT) o[e] = lds[e];
    for (int e = tid; e < wsN; e += NT) o[ldsN + e] = ws[e];
    if (tid == 0) out[d.ooff] = ret;
}
}  // namespace

#define RO_CAT2(a, b) a##b
#define RO_CAT(a, b) RO_CAT2(a, b)
extern "C" int RO_CAT(ro_launch_, RO_UNIT)(int ncase, const RoCase* cases, const DevParams* P, const double* in,
                                           double* out, double* ws, int ldsN, int wsN, int) {
    auto k = ro_kernel<false, ro_vg(RO_UNIT), ro_rm(RO_UNIT), ro_occ(RO_UNIT), ro_sh(RO_UNIT)>;
    const size_t lds = (size_t)ldsN * sizeof(double);
    if (lds > kRoLdsLimit) return -1;
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k, dim3(ncase), dim3(NT), lds, 0, cases, P, in, out, ws, ldsN, wsN);
    return (int)hipGetLastError();
}

#else   // RO_UNIT == 0: the C entry points

extern "C" {
int ro_launch_1(int, const RoCase*, const DevParams*, const double*, double*, double*, int, int, int);
int ro_launch_2(int, const RoCase*, const DevParams*, const double*, double*, double*, int, int, int);
int ro_launch_3(int, const RoCase*, const DevParams*, const double*, double*, double*, int, int, int);
int ro_launch_4(int, const RoCase*, const DevParams*, const double*, double*, double*, int, int, int);

static bool ro_shape_ok(int unit, int V, int O, int HM) {
    if (unit < 1 || unit > kRoUnits || V < 1 || V > SCPQP_MAX_VEH || O < 0 || O > SCPQP_MAX_OBST || HM < 1) return false;
    if (V * HM + 1 > 64 * ro_rm(unit)) return false;
    if (unit == 3 && (V != 4 || O != 0 || HM != 20)) return false;
    if (unit == 4 && (V != 4 || O != 0)) return false;
    return true;
}
static Off ro_off(int unit, int V, int O, int HM) {
    return plan_offsets(V, O, HM, false, ro_vg(unit), lean_plan(false, ro_vg(unit), ro_occ(unit)));
}

// The plan of a unit at a shape, for the host's masks: out[0..15] = LDS doubles, workspace
// doubles, then the offsets yb rhs dinv red H Wt vec mcAlloc pb dz rd qs, then whether the
// vectors, W~ and tv live in the workspace / the workspace / LDS.  0, or -1 for a shape the
// unit does not run.
int ro_plan(int unit, int V, int O, int HM, int* out) {
    if (!ro_shape_ok(unit, V, O, HM)) return -1;
    const Off f = ro_off(unit, V, O, HM);
    const bool vg = ro_vg(unit), lean = lean_plan(false, vg, ro_occ(unit));
    const int v[17] = {f.persist + f.uni, f.ws, f.yb, f.rhs, f.dinv, f.red, f.H, f.Wt, f.vec, f.mcAlloc,
                       f.pb, f.dz, f.rd, f.qs, vg ? 1 : 0, lean ? 1 : 0, tv_in_lds(false, vg, lean) ? 1 : 0};
    for (int i = 0; i < 17; ++i) out[i] = v[i];
    return 0;
}
int ro_red_size(void) { return red_size(false); }
int ro_side_slot(void) { return kSidePart; }
int ro_in_size(int V, int O, int Hb) { return ro_in_doubles(V, O, Hb); }
// the panel step of stage k of a two-stage side job in a factorisation of nsteps steps
int ro_side_step(int k, int nsteps) { return side_step<2>(k, nsteps); }

// Run ncase cases on unit's kernel at the shape (V, O, HM); every case's own horizon Hb <= HM
// (unit 4 only: else Hb == HM).  Output per case at ooff: kRoHdr doubles, then the "before"
// and the "after" image, each the LDS then the workspace slice.
int ro_run(int unit, int V, int O, int HM, int ncase, const RoCase* cases, const double* in, long long nin,
           double* out, long long nout) {
    static const RoLaunch table[kRoUnits] = {ro_launch_1, ro_launch_2, ro_launch_3, ro_launch_4};
    if (!ro_shape_ok(unit, V, O, HM) || ncase < 1) return -2;
    const Off f = ro_off(unit, V, O, HM);
    const int ldsN = f.persist + f.uni, wsN = f.ws;
    if ((size_t)ldsN * sizeof(double) > kRoLdsLimit) return -6;
    for (int c = 0; c < ncase; ++c) {
        const RoCase& d = cases[c];
        if (d.Hb < 1 || d.Hb > HM || (unit != 4 && d.Hb != HM)) return -3;
        if (d.lead < 0 || d.lead >= NWAVE || d.site < 0 || d.site > 3 || d.order < 0 || d.order > 1) return -3;
        const long long n = (long long)V * d.Hb + 1;
        if (d.inoff < 0 || d.inoff + (long long)ro_in_doubles(V, O, d.Hb) > nin) return -5;
        if (d.site == 3 && (d.koff < 0 || d.koff + n * (n + 1) / 2 > nin)) return -5;
        if (d.ooff < 0 || d.ooff + (long long)kRoHdr + 2ll * (ldsN + wsN) > nout) return -5;
    }
    DevParams hp;
    memset(&hp, 0, sizeof(hp));
    hp.nV = V; hp.hpMax = HM; hp.nO = O;
    hp.uLim = 0.5; hp.slackW = 1e5; hp.polDelta = 1e-6; hp.polRho = 1e-6;
    for (int v = 0; v < SCPQP_MAX_VEH; ++v) {
        hp.Q[v] = 1.0 + 0.125 * v; hp.Qf[v] = 2.0 + 0.25 * v; hp.R[v] = 0.5 + 0.0625 * v;
    }
    RoCase* dc = nullptr;
    DevParams* dp = nullptr;
    double *din = nullptr, *dout = nullptr, *dws = nullptr;
    hipError_t e = hipSuccess;
    auto chk = [&](hipError_t r) { if (e == hipSuccess) e = r; return r == hipSuccess; };
    const size_t wsBytes = (size_t)(wsN > 0 ? wsN : 1) * ncase * sizeof(double);
    if (chk(hipMalloc(&dc, ncase * sizeof(RoCase))) && chk(hipMalloc(&dp, sizeof(DevParams))) &&
        chk(hipMalloc(&din, nin * sizeof(double))) && chk(hipMalloc(&dout, nout * sizeof(double))) &&
        chk(hipMalloc(&dws, wsBytes)) &&
        chk(hipMemcpy(dc, cases, ncase * sizeof(RoCase), hipMemcpyHostToDevice)) &&
        chk(hipMemcpy(dp, &hp, sizeof(DevParams), hipMemcpyHostToDevice)) &&
        chk(hipMemcpy(din, in, nin * sizeof(double), hipMemcpyHostToDevice)) &&
        chk(hipMemset(dout, 0, nout * sizeof(double)))) {
        const int rc = table[unit - 1](ncase, dc, dp, din, dout, dws, ldsN, wsN, 0);
        if (rc != 0) e = rc > 0 ? (hipError_t)rc : hipErrorInvalidValue;
        else if (chk(hipDeviceSynchronize())) chk(hipMemcpy(out, dout, nout * sizeof(double), hipMemcpyDeviceToHost));
    }
    (void)hipFree(dc); (void)hipFree(dp); (void)hipFree(din); (void)hipFree(dout); (void)hipFree(dws);
    return (int)e;
}
}
#endif
