// scpqp_rounding.h — products and sums that are each their own rounding: the
// __dadd_rn(__dmul_rn(a, b), c) that include/scpqp_truth.h, scpqp_obstacles.h,
// scpqp_manoeuvres.h and scpqp_sensing.h fix for a drawn value.  Spelled with the operators
// under contract(off): the two intrinsics are plain * and + to the compiler, which would fuse
// them into one fma (one rounding) once inlined.
#ifndef SCPQP_ROUNDING_H
#define SCPQP_ROUNDING_H

#include <hip/hip_runtime.h>

namespace scpqp_round_dev {

// a * b + c in two roundings
__device__ __forceinline__ double mul_add_2r(double a, double b, double c) {
#pragma clang fp contract(off)
    const double ab = a * b;
    return ab + c;
}

__device__ __forceinline__ double add_1r(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}

__device__ __forceinline__ double mul_1r(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}

}  // namespace scpqp_round_dev

#endif  // SCPQP_ROUNDING_H
