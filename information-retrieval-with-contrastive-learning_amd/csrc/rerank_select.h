// The exact per-query select over a key workspace (rerank_select_kernel, rerank.hip), for
// every pass that fills one: the candidate top-k, the grouped scan, the grouped merge, and the
// cluster-pruned search (ivf.hip).  The kernel exists once; this is its host entry.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace irc {
namespace rerank {

constexpr int RR_MAXK = 1024;  // the largest k of the select

// Query q ranks keys[off[q] .. min(off[q + 1], n_keys)) (make_key keys; 0 = not eligible):
// the min(k, eligible) largest, descending, decoded into out_score / out_idx [Q, k] with
// (-inf, -1) padding, and out_n[q] their count.  Launches on st under the profiling hooks
// ("rerank_select"); returns check_launch's code.
int select_topk(const uint64_t* keys, const int64_t* off, int64_t n_keys, int64_t Q, int k,
                float* out_score, int64_t* out_idx, int32_t* out_n, hipStream_t st);

}  // namespace rerank
}  // namespace irc
