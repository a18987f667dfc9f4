// Key-value sort on the context's stream with the context's scratch (rocPRIM).
// rocPRIM's default sorts up to 2^20 items with a MERGE sort (block sort + log2(n / 1024) merge passes of two launches each) whatever the
// key width, larger inputs with its onesweep radix sort.  Forcing the radix sort for smaller inputs was measured in round 6 and lost
// (docs/experiments.md): a LiDAR scan's 115k keys 115 us against 54 us (five passes + seven state fills against ten launches).
#pragma once
#include <rocprim/rocprim.hpp>

#include "common.hpp"

namespace sga {
int ensure_temp(sga_context* ctx, size_t bytes);

// The branch sort_pairs takes for n items: 0 = up to 2048 items, rocPRIM's default (one block sort); 1 = up to 200 000, the 512 x 4 merge
// configuration below; 2 = above, rocPRIM's default again (a merge sort up to 2^20 items, its onesweep radix sort beyond).
inline int sort_path(size_t n) { return n <= 2048 ? 0 : n <= 200000 ? 1 : 2; }

template <typename Key, typename Val>
int sort_pairs(sga_context* ctx, Key* keys_in, Key* keys_out, Val* vals_in, Val* vals_out, size_t n, unsigned begin_bit, unsigned end_bit) {
  // a LiDAR scan's keys: block sorts of 2048 items (512 x 4) instead of the default 1024 — one merge pass less; same (stable) result
  // (scripts/ubench/sort_small.hip: 115k pairs 55.0 -> 48.7 us, 30k 38.2 -> 34.1; at 262k the default wins again)
  using Small = rocprim::radix_sort_config<rocprim::default_config, rocprim::merge_sort_config<512, 512, 4>, rocprim::default_config, 1 << 20>;
  size_t tb = 0;
  if (sort_path(n) == 1) {
    SGA_HIP(rocprim::radix_sort_pairs<Small>(nullptr, tb, keys_in, keys_out, vals_in, vals_out, n, begin_bit, end_bit, ctx->stream));
    SGA_TRY(ensure_temp(ctx, tb));
    SGA_HIP(rocprim::radix_sort_pairs<Small>(ctx->d_temp.p, tb, keys_in, keys_out, vals_in, vals_out, n, begin_bit, end_bit, ctx->stream));
  } else {
    SGA_HIP(rocprim::radix_sort_pairs(nullptr, tb, keys_in, keys_out, vals_in, vals_out, n, begin_bit, end_bit, ctx->stream));
    SGA_TRY(ensure_temp(ctx, tb));
    SGA_HIP(rocprim::radix_sort_pairs(ctx->d_temp.p, tb, keys_in, keys_out, vals_in, vals_out, n, begin_bit, end_bit, ctx->stream));
  }
  return SGA_OK;
}

// out[i] = in[0] + .. + in[i - 1] on the context's stream with the context's scratch (rocPRIM: the size query, then the scan).
// (A template, so that the scan's kernels are instantiated only in the translation units that call it.)
template <typename T>
int exclusive_scan(sga_context* ctx, T* in, T* out, size_t n) {
  size_t tb = 0;
  SGA_HIP(rocprim::exclusive_scan(nullptr, tb, in, out, T(0), n, rocprim::plus<T>(), ctx->stream));
  SGA_TRY(ensure_temp(ctx, tb));
  SGA_HIP(rocprim::exclusive_scan(ctx->d_temp.p, tb, in, out, T(0), n, rocprim::plus<T>(), ctx->stream));
  return SGA_OK;
}
}  // namespace sga
