// The value and slope functions of GELU, shared by tnn_norm.hip (tnn_gelu_fwd / tnn_gelu_bwd) and tnn_gated.hip (the GEGLU
// forms of tnn_gated_fwd / tnn_gated_bwd): ONE copy, so both families evaluate the same expressions.
// Internal: not installed under include/.
#pragma once
#include "tnn_pack.h"

namespace tnn {

constexpr double kSqrtHalf = 0.70710678118654752440;        // 1 / sqrt(2)
constexpr double kSqrt2OverPi = 0.79788456080286535588;     // sqrt(2 / pi)
constexpr double kInvSqrt2Pi = 0.39894228040143267794;      // 1 / sqrt(2 pi)
constexpr double kCubic = 0.044715;

template <typename T, bool APPROX>
__device__ __forceinline__ T gelu_value(T x) {
    if constexpr (APPROX) {
        const T u = (T)kSqrt2OverPi * (x + (T)kCubic * x * x * x);
        return T(0.5) * x * (T(1) + Math<T>::tanh_(u));
    } else {
        return T(0.5) * x * (T(1) + Math<T>::erf_(x * (T)kSqrtHalf));
    }
}

template <typename T, bool APPROX>
__device__ __forceinline__ T gelu_slope(T x) {
    if constexpr (APPROX) {
        const T u = (T)kSqrt2OverPi * (x + (T)kCubic * x * x * x);
        const T th = Math<T>::tanh_(u);
        const T du = (T)kSqrt2OverPi * (T(1) + T(3) * (T)kCubic * x * x);
        return T(0.5) * (T(1) + th) + T(0.5) * x * (T(1) - th * th) * du;
    } else {
        const T cdf = T(0.5) * (T(1) + Math<T>::erf_(x * (T)kSqrtHalf));
        const T pdf = (T)kInvSqrt2Pi * Math<T>::exp_(T(-0.5) * x * x);
        return cdf + x * pdf;
    }
}

}  // namespace tnn
