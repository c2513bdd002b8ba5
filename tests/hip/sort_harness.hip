// sort_harness.hip -- csrc/radix_sort.h behind a C ABI, for tests/test_radix_sort.py only. No logic of its own: every
// entry forwards to the header with the two instantiations the product has (depth sort / knn grid: <kItemsSmall,
// kOsItemsSmall>; tile sort: <kItemsLarge, kItemsLarge>) and launches the scans as binning.hip does. Built by the test
// into a temporary directory; not part of libgsrast.so, not declared in include/gsrast.h.
#include "radix_sort.h"

extern "C" {

// form 0: radix_sort_u32 (one-sweep below 2^28 keys, state_cleared = false), form 1: radix_sort_u32_legacy (three
// kernels per pass; takes neither may_skip nor rects / early_out). Returns the sort's own return value (0: result in
// (k0, v0), 1: in (k1, v1)); -1 for cap == 0, which would be an empty grid.
int th_sort(int form, int small, uint32_t* k0, uint32_t* v0, uint32_t* k1, uint32_t* v1, const uint64_t* n_dev, uint64_t cap,
            int bits, int iota, uint64_t* n_compact, uint32_t* hist, uint32_t* totals, void* stream, int batch, size_t bstride,
            int may_skip, const uint32_t* rects, uint64_t* early_out) {
  if (cap == 0) return -1;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (form == 0) {
    if (small)
      return radix_sort_u32<kItemsSmall, kOsItemsSmall>(k0, v0, k1, v1, n_dev, cap, bits, iota != 0, n_compact, hist, totals, s,
                                                        batch, bstride, /*state_cleared=*/false, may_skip != 0, rects, early_out);
    return radix_sort_u32<kItemsLarge, kItemsLarge>(k0, v0, k1, v1, n_dev, cap, bits, iota != 0, n_compact, hist, totals, s, batch,
                                                    bstride, /*state_cleared=*/false, may_skip != 0, rects, early_out);
  }
  if (small)
    return radix_sort_u32_legacy<kItemsSmall>(k0, v0, k1, v1, n_dev, cap, bits, iota != 0, n_compact, hist, totals, s, batch,
                                              bstride);
  return radix_sort_u32_legacy<kItemsLarge>(k0, v0, k1, v1, n_dev, cap, bits, iota != 0, n_compact, hist, totals, s, batch, bstride);
}

// one workgroup per row, blockIdx.y = view: binning.hip's launch of the column counts' scan
void th_scan(int wide, uint32_t* hist, uint32_t nblk_stride, uint32_t* totals, const uint64_t* n_items, uint32_t per_block,
             uint32_t rows, uint32_t batch, size_t bstride, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (wide)
    hipLaunchKernelGGL(k_radix_scan_wide, dim3(rows, batch), dim3(1024), 0, s, hist, nblk_stride, totals, n_items, per_block,
                       bstride);
  else
    hipLaunchKernelGGL(k_radix_scan, dim3(rows, batch), dim3(256), 0, s, hist, nblk_stride, totals, n_items, per_block, bstride);
}

size_t th_hist_bytes(uint64_t cap) {
  const size_t a = sort_hist_bytes(cap, kItemsSmall, kOsItemsSmall), b = sort_hist_bytes(cap, kItemsLarge, kItemsLarge);
  return a > b ? a : b;
}

uint32_t th_skip_flag_word() { return kOsSkipFlag; }

uint32_t th_tile_keys() { return (uint32_t)(kSortThreads * kItemsLarge); }

}  // extern "C"
