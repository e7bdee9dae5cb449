// The HIP-free half of tnn_pack.h: how the float32 / float64 kernel families turn the runtime (dtype, vec) of an entry point
// into the compile-time (T, VECTOR) of a kernel template, and the byte arithmetic of their wide accesses.  Plain C++17: a
// host compiler checks the selection without a GPU (tests/float_dispatch_check.cpp).
#pragma once
#include <stdint.h>
#include <type_traits>
#include "tnn_hip.h"

namespace tnn {

constexpr int kVecBytes = 16;      // one wide access: global_load / store_dwordx4 (the families' TNN_<FAMILY>_VEC)

// a null pointer counts as aligned: an absent optional operand never rules out the wide form
inline bool aligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }
inline bool aligned16(const void* p) { return aligned(p, kVecBytes); }
inline int64_t round16(int64_t bytes) { return (bytes + 15) / 16 * 16; }
inline int64_t item_of(int dtype) { return dtype == TNN_F32 ? 4 : 8; }

// f(T()) with T = float for TNN_F32 and double otherwise (the entry point has required one of the two):
//     tnn::with_float(dtype, [&](auto t) { typedef decltype(t) T; hipLaunchKernelGGL(kernel<T>, ...); });
template <typename F>
inline auto with_float(int dtype, F&& f) {
    if (dtype == TNN_F32) return f(float());
    else return f(double());
}

// f(std::bool_constant<flag>()): a runtime yes / no as a template argument (decltype(v)::value)
template <typename F>
inline auto with_flag(bool flag, F&& f) {
    if (flag) return f(std::true_type());
    else return f(std::false_type());
}

// f(T(), std::bool_constant<vec>()): the four (T, VECTOR) instances of a kernel template
//     tnn::with_float(dtype, vec, [&](auto t, auto v) { ... kernel<decltype(t), decltype(v)::value> ... });
template <typename F>
inline auto with_float(int dtype, bool vec, F&& f) {
    return with_float(dtype, [&](auto t) { return with_flag(vec, [&](auto v) { return f(t, v); }); });
}

}  // namespace tnn
