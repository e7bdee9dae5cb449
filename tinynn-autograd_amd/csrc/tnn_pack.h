// What the float32 / float64 kernel families (bmm, conv, attn, norm, token, decode, dropout) share: the vector types
// of their wide accesses, the "16 bytes of T" trait, the float / double spelling of the math functions, and the dtype and
// workspace preconditions of their entry points.  The dispatch helper and the byte arithmetic are in tnn_dispatch.h.
// Internal: not installed under include/.
#pragma once
#include <math.h>

#include "tnn_internal.h"
#include "tnn_dispatch.h"

namespace tnn {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));      // the accumulator of a 32 x 32 MFMA tile

// what one lane moves per access: kVecBytes of T when VECTOR, one element otherwise
template <typename T, bool VECTOR> struct Pack { typedef T type; static constexpr int N = 1; };
template <> struct Pack<float, true> { typedef f32x4 type; static constexpr int N = 4; };
template <> struct Pack<double, true> { typedef f64x2 type; static constexpr int N = 2; };
static_assert(sizeof(Pack<float, true>::type) == kVecBytes && sizeof(Pack<double, true>::type) == kVecBytes, "one wide access");

template <typename T> struct Math;
template <> struct Math<float> {
    static __device__ __forceinline__ float exp_(float v) { return expf(v); }
    static __device__ __forceinline__ float log_(float v) { return logf(v); }
    static __device__ __forceinline__ float erf_(float v) { return erff(v); }
    static __device__ __forceinline__ float tanh_(float v) { return tanhf(v); }
    static __device__ __forceinline__ float rsqrt_(float v) { return 1.0f / sqrtf(v); }     // (correctly rounded, not rsqrtf)
};
template <> struct Math<double> {
    static __device__ __forceinline__ double exp_(double v) { return exp(v); }
    static __device__ __forceinline__ double log_(double v) { return log(v); }
    static __device__ __forceinline__ double erf_(double v) { return erf(v); }
    static __device__ __forceinline__ double tanh_(double v) { return tanh(v); }
    static __device__ __forceinline__ double rsqrt_(double v) { return 1.0 / sqrt(v); }
};

}  // namespace tnn

// `name` is the entry point: a string literal or a const char*; `dtype` is the entry point's own parameter
#define TNN_REQUIRE_FLOAT(name) \
    TNN_REQUIRE(dtype == TNN_F32 || dtype == TNN_F64, "%s: dtype %d (float32 and float64 only)", name, dtype)

#define TNN_REQUIRE_WORKSPACE(name, ws, bytes, need)                                  \
    TNN_REQUIRE((ws) != nullptr && (bytes) >= (need) && tnn::aligned16(ws),           \
                "%s: workspace of %lld bytes, %lld needed (16-byte aligned)", name, (long long)(bytes), (long long)(need))
