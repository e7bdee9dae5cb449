// Host-only check of csrc/tnn_dispatch.h (tests/test_float_dispatch.py compiles this with g++ -std=c++17 and runs it): every
// runtime (dtype, vec) must reach the lambda as exactly its own compile-time (T, VECTOR).  Identical kernels cannot show
// that: with two arms swapped every numeric test still passes, because element accesses are always right and the wide
// accesses tolerate the addresses the tests use.
#include <stdio.h>
#include <string>
#include <type_traits>

#include "tnn_hip.h"
#include "tnn_dispatch.h"

static int failures = 0;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("FAILED line %d: %s\n", __LINE__, #cond);             \
            ++failures;                                                  \
        }                                                                \
    } while (0)

template <typename T> const char* name_of();
template <> const char* name_of<float>() { return "float"; }
template <> const char* name_of<double>() { return "double"; }

static std::string typed(int dtype) {
    return tnn::with_float(dtype, [](auto t) { return std::string(name_of<decltype(t)>()); });
}

static std::string flagged(bool flag) {
    return tnn::with_flag(flag, [](auto v) { return std::string(decltype(v)::value ? "true" : "false"); });
}

static std::string packed(int dtype, bool vec) {
    return tnn::with_float(dtype, vec, [](auto t, auto v) {
        static_assert(std::is_same<decltype(v), std::true_type>::value || std::is_same<decltype(v), std::false_type>::value,
                      "the vec argument is a std::bool_constant");
        return std::string(name_of<decltype(t)>()) + (decltype(v)::value ? ", true" : ", false");
    });
}

int main() {
    CHECK(typed(TNN_F32) == "float");
    CHECK(typed(TNN_F64) == "double");
    CHECK(flagged(true) == "true");
    CHECK(flagged(false) == "false");
    CHECK(packed(TNN_F32, true) == "float, true");
    CHECK(packed(TNN_F32, false) == "float, false");
    CHECK(packed(TNN_F64, true) == "double, true");
    CHECK(packed(TNN_F64, false) == "double, false");

    // a lambda without a result: the form every launch uses; each call runs exactly one arm
    int calls = 0, wide_floats = 0;
    tnn::with_float(TNN_F32, true, [&](auto t, auto v) {
        ++calls;
        if (std::is_same<decltype(t), float>::value && decltype(v)::value) ++wide_floats;
    });
    CHECK(calls == 1 && wide_floats == 1);

    CHECK(tnn::kVecBytes == 16);
    CHECK(tnn::item_of(TNN_F32) == 4);
    CHECK(tnn::item_of(TNN_F64) == 8);

    CHECK(tnn::round16(0) == 0);
    CHECK(tnn::round16(1) == 16);
    CHECK(tnn::round16(15) == 16);
    CHECK(tnn::round16(16) == 16);
    CHECK(tnn::round16(17) == 32);

    const auto at = [](uintptr_t address) { return reinterpret_cast<const void*>(address); };
    CHECK(tnn::aligned16(nullptr));          // an absent optional operand counts as aligned
    CHECK(tnn::aligned16(at(16)));
    CHECK(!tnn::aligned16(at(20)));
    CHECK(!tnn::aligned16(at(24)));
    CHECK(tnn::aligned16(at(32)));
    CHECK(tnn::aligned(at(24), 8) && !tnn::aligned(at(20), 8));      // dropout's state and ticket words

    if (failures == 0) printf("float dispatch ok\n");
    return failures == 0 ? 0 : 1;
}
