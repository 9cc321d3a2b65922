// mnv_points_probe.hip -- the yardstick of tools/points_bench.py (test-hook build only): rocprim::radix_sort_pairs alone over 64-bit keys and
// 32-bit payloads, the sort that mnv_point_tree_add runs between its key and reduce passes (csrc/mnv_points.hip).
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "mnv_internal.h"

extern "C" {

// tmp == NULL: *tmp_bytes receives the sort's temporary size.  Otherwise sorts keys / vals (device [n]) by key bits [0, bits), asynchronously
// on hip_stream, between the arrays and their spares as mnv_point_tree_add does (a double buffer: both halves are overwritten);
// *result_in_spare says which half holds the result.
int mnv_hook_points_sort_pairs(uint64_t *keys, uint64_t *keys_spare, uint32_t *vals, uint32_t *vals_spare, int64_t n, int32_t bits, void *tmp, size_t *tmp_bytes,
                               int32_t *result_in_spare, void *hip_stream) {
    if (!tmp_bytes || n < 1 || bits < 1 || bits > 64) return mnv::set_error(MNV_E_INVALID, "mnv_hook_points_sort_pairs: invalid arguments");
    if (tmp && (!keys || !keys_spare || !vals || !vals_spare)) return mnv::set_error(MNV_E_INVALID, "mnv_hook_points_sort_pairs: null array");
    rocprim::double_buffer<uint64_t> k(keys, keys_spare);
    rocprim::double_buffer<uint32_t> v(vals, vals_spare);
    const int rc = mnv::check_hip(rocprim::radix_sort_pairs(tmp, *tmp_bytes, k, v, (size_t)n, 0, bits, (hipStream_t)hip_stream), "radix_sort_pairs");
    if (result_in_spare) *result_in_spare = k.current() == keys_spare ? 1 : 0;
    return rc;
}

}  // extern "C"
