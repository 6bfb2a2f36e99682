// launch_util.hpp — what the launchers of every kernel file share: the HIP status of a launch, the rank count as a
// template argument, the grid of a persistent pass.  Host code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "internal.hpp"

namespace tsa {

inline int last_error() { return hip_status((int)hipGetLastError()); }

// a bool template argument as the launch trace spells it
constexpr const char* tf(bool b) { return b ? "true" : "false"; }

// The rank count as a template argument: f(std::integral_constant<int, total>{}) for a power of
// two total in [LO, HI]; false (nothing launched) when the kernels have no instance for it.
template <int LO, int HI, class F>
bool for_ranks(int total, F&& f) {
    if (total == LO) {
        f(std::integral_constant<int, LO>{});
        return true;
    }
    if constexpr (LO < HI) return for_ranks<2 * LO, HI>(total, f);
    return false;
}

// workgroups of a persistent pass over `tiles` tiles: the pass's default, or what tune pipe_grid says
inline unsigned persistent_grid(uint64_t tiles, uint64_t dflt) {
    const int64_t g = tune(Tune::pipe_grid);
    const uint64_t cap = g > 0 ? (uint64_t)g : dflt;
    return (unsigned)(tiles < cap ? tiles : cap);
}

}  // namespace tsa
