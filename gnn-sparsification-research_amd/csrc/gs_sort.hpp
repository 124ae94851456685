// gs_sort.hpp -- rocPRIM's radix sort as the units call it: the size query, the temporary
// storage, the sort over a double buffer and the buffer that holds the result.  Host code;
// only the units that sort include it (it includes rocPRIM).
//
// Both helpers sort n items stably by bits [begin_bit, end_bit) of the keys on stream st,
// take their temporary storage from tmp (grown as needed) and return where the sorted data
// is: the caller's buffer or its alternate, whose other copy is then scratch.  n <= 1
// launches and allocates nothing and returns the caller's buffers.
#pragma once

#include <rocprim/device/device_radix_sort.hpp>

#include "gs_internal.hpp"

namespace gs {

template <class K>
static K *radix_sort_keys(gs_ctx *, DevBuf &tmp, K *keys, K *keys_alt, int64_t n, int begin_bit, int end_bit,
                          hipStream_t st) {
    if (n <= 1) return keys;
    rocprim::double_buffer<K> dk(keys, keys_alt);
    size_t bytes = 0;
    GS_HIP(rocprim::radix_sort_keys(nullptr, bytes, dk, (size_t)n, begin_bit, end_bit, st));
    void *t = tmp.ensure(bytes + 16);
    GS_HIP(rocprim::radix_sort_keys(t, bytes, dk, (size_t)n, begin_bit, end_bit, st));
    return dk.current();
}

template <class K, class V>
struct SortedPairs {
    K *keys;
    V *vals;
};

template <class K, class V>
static SortedPairs<K, V> radix_sort_pairs(gs_ctx *, DevBuf &tmp, K *keys, K *keys_alt, V *vals, V *vals_alt,
                                          int64_t n, int begin_bit, int end_bit, hipStream_t st) {
    if (n <= 1) return {keys, vals};
    rocprim::double_buffer<K> dk(keys, keys_alt);
    rocprim::double_buffer<V> dv(vals, vals_alt);
    size_t bytes = 0;
    GS_HIP(rocprim::radix_sort_pairs(nullptr, bytes, dk, dv, (size_t)n, begin_bit, end_bit, st));
    void *t = tmp.ensure(bytes + 16);
    GS_HIP(rocprim::radix_sort_pairs(t, bytes, dk, dv, (size_t)n, begin_bit, end_bit, st));
    return {dk.current(), dv.current()};
}

}  // namespace gs
