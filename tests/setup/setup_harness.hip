// Test harness (not linked into libscpqp.so): the squaring count and the 8x8 matrix
// exponential of csrc/scpqp_kernel.h on their own (tests/setup_harness.py builds and binds
// it; tests/test_setup_host.py and tests/test_gpu_setup.py use it).
//
//   sh_squarings(nrm)   expm_squarings on the host: needs no GPU
//   sh_expm(...)        one workgroup of 256 threads runs expm8 on four given 8x8 matrices,
//                       one per wave, wave w taking part iff bit w of actmask is set
//
// The kernel fills its whole dynamic LDS with a canary pattern, places each wave's 576
// doubles of scratch between two guards of kShGuard doubles and the four doubles of the
// squaring-count exchange between two more, and counts what is no longer the pattern:
//   bad[0]  disturbed guard doubles
//   bad[1]  disturbed scratch doubles of the waves that take no part
#include "../../senquential-convex-programming-for-trajectory-planning_amd/csrc/scpqp_kernel.h"

#include <cstdint>

constexpr int kShGuard = 16;
constexpr int kShScr = 576;                      // what expm8 uses of a wave's SCR_PER_WAVE
constexpr int kShStride = kShScr + 2 * kShGuard;
constexpr int kShRed = NWAVE * kShStride + kShGuard;
constexpr int kShLds = kShRed + NWAVE + kShGuard;
static_assert(kShScr <= SCR_PER_WAVE, "expm8's scratch outgrew the plan's");

namespace {
__device__ __forceinline__ double sh_canary(int e) {
    return __longlong_as_double(0x7ff8c0de00000000ll | (long long)e);
}
__device__ __forceinline__ bool sh_is_canary(double v, int e) {
    return __double_as_longlong(v) == (0x7ff8c0de00000000ll | (long long)e);
}

__global__ __launch_bounds__(NT) void sh_kernel(const double* in, int actmask, double* out, int* bad) {
    ldouble* lds = (ldouble*)smem_;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const bool act = (actmask >> w) & 1;
    for (int e = tid; e < kShLds; e += NT) lds[e] = sh_canary(e);
    __syncthreads();
    ldouble* scr = lds + w * kShStride + kShGuard;
    if (act) scr[lane] = in[w * 64 + lane];
    __syncthreads();
    expm8(scr, act, lds + kShRed);
    __syncthreads();
    out[w * 64 + lane] = act ? scr[64 + lane] : 0.0;
    int guard = 0, idle = 0;
    for (int e = tid; e < kShLds; e += NT) {
        if (sh_is_canary(lds[e], e)) continue;
        if (e >= NWAVE * kShStride) {   // guard, the exchange's four doubles, guard
            guard += (e < kShRed || e >= kShRed + NWAVE) ? 1 : 0;
            continue;
        }
        const int ww = e / kShStride, r = e - ww * kShStride;
        if (r < kShGuard || r >= kShGuard + kShScr) ++guard;
        else if (!((actmask >> ww) & 1)) ++idle;
    }
    if (guard) atomicAdd(&bad[0], guard);
    if (idle) atomicAdd(&bad[1], idle);
}
}  // namespace

extern "C" {
int sh_squarings(double nrm) { return expm_squarings(nrm); }
int sh_max_squarings(void) { return kExpmMaxSquarings; }
int sh_scratch_doubles(void) { return kShScr; }

// in: four 8x8 matrices, row-major; out: their exponentials (zeros for a wave outside
// actmask); bad: the two counts above.  0, or a HIP error code.
int sh_expm(const double* in, int actmask, double* out, int* bad) {
    double *din = nullptr, *dout = nullptr;
    int* dbad = nullptr;
    hipError_t e = hipSuccess;
    auto chk = [&](hipError_t r) { if (e == hipSuccess) e = r; return r == hipSuccess; };
    const size_t nb = NWAVE * 64 * sizeof(double), lds = kShLds * sizeof(double);
    if (chk(hipMalloc(&din, nb)) && chk(hipMalloc(&dout, nb)) && chk(hipMalloc(&dbad, 2 * sizeof(int))) &&
        chk(hipMemcpy(din, in, nb, hipMemcpyHostToDevice)) && chk(hipMemset(dout, 0, nb)) &&
        chk(hipMemset(dbad, 0, 2 * sizeof(int)))) {
        hipLaunchKernelGGL(sh_kernel, dim3(1), dim3(NT), lds, 0, din, actmask & 15, dout, dbad);
        if (chk(hipGetLastError()) && chk(hipDeviceSynchronize()) &&
            chk(hipMemcpy(out, dout, nb, hipMemcpyDeviceToHost)))
            chk(hipMemcpy(bad, dbad, 2 * sizeof(int), hipMemcpyDeviceToHost));
    }
    (void)hipFree(din); (void)hipFree(dout); (void)hipFree(dbad);
    return (int)e;
}
}
