// dispatch.hpp -- run-time value -> compile-time template argument, for the launchers of gridder.hip and gridder_wd.hip.
// f is called with std::integral_constant<int, V>: a generic lambda reads the value as decltype(v)::value.  Only the
// values of the range are instantiated; any other value throws.
#pragma once
#include <stdexcept>
#include <type_traits>

namespace pfbhip {

template <int V, int Hi, class F>
void with_int(int v, F &&f, const char *what)
{
    if constexpr (V > Hi) {
        throw std::runtime_error(what);
    } else {
        if (v == V) return (void)f(std::integral_constant<int, V>{});
        with_int<V + 1, Hi>(v, f, what);
    }
}

// kernel support W = 4..16
template <class F>
void with_W(int W, F &&f)
{
    with_int<4, 16>(W, f, "unsupported kernel support");
}
// planes per pass of the multi-plane kernels, 1..KP_MAX (4)
template <class F>
void with_KP(int kp, F &&f)
{
    with_int<1, 4>(kp, f, "unsupported planes per pass");
}
// kernel functions per axis of the one-plane w-scheme, 2..4
template <class F>
void with_K(int K, F &&f)
{
    with_int<2, 4>(K, f, "one-plane w-scheme: 2..4 kernel functions");
}
// block edge of the register-footprint scatters' frame: 2 exists at W = 14, 15 only, 4 everywhere
template <int W, class F>
void with_BC(int bc, F &&f)
{
    if constexpr (W == 14 || W == 15) {
        if (bc == 2) return (void)f(std::integral_constant<int, 2>{});
    }
    f(std::integral_constant<int, 4>{});
}

}  // namespace pfbhip
