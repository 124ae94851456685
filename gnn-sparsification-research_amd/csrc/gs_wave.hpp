// gs_wave.hpp -- what the lanes of one wave (64) do together: places at a shared cursor
// with one atomic per wave, and integer reductions.  Device code only; the workgroups are
// one-dimensional, so a thread's lane is threadIdx.x & 63.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

namespace gs {

// the set bits of mask below the calling lane
__device__ __forceinline__ unsigned int lanes_below(unsigned long long mask) {
    const int lane = threadIdx.x & 63;
    return (unsigned int)__popcll(mask & ((1ull << lane) - 1ull));
}

// n (the same in every active lane) places at *cursor, in LDS or global memory: one atomic,
// by the lowest active lane -- lane 0 of a whole wave, and still a lane that runs where the
// caller has diverged -- and every active lane gets the old value
template <class C>
__device__ __forceinline__ C wave_reserve(C n, C *cursor) {
    static_assert(std::is_same<C, unsigned int>::value || std::is_same<C, unsigned long long>::value,
                  "a cursor is an unsigned int or an unsigned long long");
    const int leader = __builtin_ctzll(__ballot(true));
    C base = 0;
    if ((int)(threadIdx.x & 63) == leader) base = atomicAdd(cursor, n);
    return __shfl(base, leader, 64);
}

// a place at *cursor for every lane that takes one, in lane order; no atomic when none does.
// Every active lane calls it; the value means something in the takers only.
template <class C>
__device__ __forceinline__ C wave_append(bool take, C *cursor) {
    const unsigned long long m = __ballot(take);
    if (!m) return 0;
    return wave_reserve((C)__popcll(m), cursor) + lanes_below(m);
}

// Reductions over a whole wave: lane 0 holds the result.  Integers only -- a floating-point
// sum depends on the order, and the kernels that need one spell their order out.
template <class T, class Op>
__device__ __forceinline__ T wave_fold(T x, Op op) {
    static_assert(std::is_integral<T>::value, "integer reductions only");
    for (int off = 32; off > 0; off >>= 1) x = op(x, (T)__shfl_down(x, off, 64));
    return x;
}
template <class T>
__device__ __forceinline__ T wave_sum(T x) {
    return wave_fold(x, [](T a, T b) { return (T)(a + b); });
}
template <class T>
__device__ __forceinline__ T wave_min(T x) {
    return wave_fold(x, [](T a, T b) { return b < a ? b : a; });
}
template <class T>
__device__ __forceinline__ T wave_max(T x) {
    return wave_fold(x, [](T a, T b) { return b > a ? b : a; });
}

}  // namespace gs
