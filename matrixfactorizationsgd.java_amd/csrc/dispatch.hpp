// dispatch.hpp -- from the run-time lane-group size L (lanes per rating: kp / 4) and wave count W of a model to the
// kernel instantiation for them.  The one list of supported values of each: every launcher goes through it.
//     return with_L(L, [&](auto l) { return with_W(W, [&](auto w) { return launch_LW<l(), w()>(...); }); });
#pragma once

#include <hip/hip_runtime_api.h>

#include <type_traits>

namespace mfsgd {

// f(std::integral_constant<int, L>) -> hipError_t for a supported L, hipErrorInvalidValue for any other.
template <class F>
hipError_t with_L(const int L, F&& f) {
    switch (L) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 16: return f(std::integral_constant<int, 16>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        default: return hipErrorInvalidValue;
    }
}

template <class F>
hipError_t with_W(const int W, F&& f) {
    switch (W) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 8: return f(std::integral_constant<int, 8>{});
        default: return hipErrorInvalidValue;
    }
}

}  // namespace mfsgd
