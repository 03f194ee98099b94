// Candidate-restricted dense top-k for gfx950 (MI355X): sparse filter, dense rerank.
//
// Joins the two stages of the reference's predict(): the hashed n-gram filter
// documents_filtering (src/evaluation.py:57-83) leaves each claim's candidate docs as a
// CSR pair, and the dense scoring its tail sketches (:110-112) ranks exactly those docs --
// a doc the filter excluded can never enter the top-k, unlike a scan of the whole shard.
//
// Design:
//  * rerank_score_kernel walks the FLATTENED candidate array in chunks of RR_CHUNK, one
//    workgroup per chunk, whatever the list lengths: one 200k-candidate list spreads over
//    800 workgroups instead of serialising on one while the short lists finish early.  A
//    chunk may span several lists; every thread finds the owner of its own candidate by
//    binary search in cand_off (narrowed first to the chunk's first / last owner).
//  * Rows are gathered whole: 8 lanes share a row, lane s reads the 16-byte pieces s,
//    s + 8, ... (8 x 16 B = one 128-byte granule per step, every D % 64 == 0), 8 rows in
//    flight per wave, 4 waves per workgroup, up to 4 workgroups per CU.  The query slice of
//    the 8-lane group stays in registers while consecutive rows belong to one query.
//  * The sum over D has ONE order per (query, doc): each lane accumulates its pieces in
//    ascending order in one fp32 chain, then lanes combine by xor-shuffles 1, 2, 4.  It
//    does not depend on the doc's place in the list or on the workgroup (bf16 products are
//    exact in fp32).  No atomics on scores.
//  * Every candidate gets a 64-bit key (make_key: score, ~global id) in the workspace,
//    8 B written against D * 2 read; ids of other shards get key 0 and are never read.
//  * rerank_select_kernel: one workgroup per query, exact radix select of the k-th key
//    below the keys' common prefix, then a bitonic sort of the winners.  A list of up to
//    S_STAGE keys is read from global memory once and selected in LDS; a longer one is
//    re-read per digit until the selected bucket fits, and the pass that moves the bucket
//    to LDS also collects the keys above it, so nothing is read after that.  Keys are
//    distinct (unique ids), so exactly min(k, eligible) keys reach the k-th.
//  * irc_rerank_topk_stream fills the same keys[] another way, for dense lists: the shard
//    streams once per 256-query tile through the ping-pong MFMA GEMM loop and each
//    query's candidates are picked out of the score tile (gemm_pp.hip, EPI_PICK; lists
//    ascending in global id).  rerank_foreign_kernel zeroes the keys of the ids outside
//    the shard, a prefix and a suffix of every list; the select is the same kernel.
//  * irc_rerank_topk_fp8 / irc_rerank_topk_stream_fp8 do both on e4m3 shards (rows of D
//    bytes): rerank_score_fp8_kernel decodes with v_cvt_pk_f32_fp8, the stream runs the
//    unit-scale e4m3 MFMA loop (gemm_pp.hip, F8 = 1).  Scores are the fp32 sums of the exact
//    products times a power-of-two score_scale; keys, foreign ids and select as above.
//  * irc_rerank_topk_grouped ranks groups of rows (pages) instead of rows: after any of the
//    four scoring passes rerank_collapse_kernel zeroes every key that is not the maximum of
//    its (query, group) run, and the unchanged select returns the top-k distinct groups.
//  * irc_rerank_biased_topk ranks by score + bias[i] (hybrid retrieval's fused score: the
//    sparse stage's per-candidate prior): the same four scoring passes with the addition as a
//    compile-time variant -- score_chunk<E4M3, D, BIAS>, and EPI_PICK_BIAS in gemm_pp.hip --
//    one fp32 add after the e4m3 scale, before the collapse when grouped.
//  * irc_topk_merge_grouped is the reduce step of that call over several shards: the
//    per-shard lists of a query hold one page twice when its best lines lie in two shards,
//    so merge_collapse_kernel sorts the query's P * kin entries by row id (a group is a run
//    of the sorted ids), keeps the maximum key of every group, and the same select returns
//    the top-k distinct groups.
//  * irc_scan_topk_grouped is the grouped top-k with EVERY row of the shard a candidate of
//    every query: no list, no scoring kernel of this file, no collapse -- the ping-pong GEMM
//    loop's group epilogue (gemm_pp.hip, EPI_GROUP) writes one key per (query, group) and the
//    same select ranks each query's n_groups keys.  Its own check sequence (no candidates).
//
// Layout: each thing exists once.  Device: score_chunk<E4M3, D> is the scoring body of both
// gathered kernels (Operand<E4M3, D> holds what differs: piece type, pieces per lane, row
// bytes, the dot product of a piece); chunk_owners is the owner search of the scoring and
// the collapse kernels.  Host: the six extern "C" entries are one call of rerank_run each,
// which holds the argument checks (their order is part of the interface), then runs
// score_gather (the D switch) or score_stream (the pick GEMM's arguments), the collapse if
// grouped, and the select.  A new operand type is one more Operand; a new entry one more Form.
// The select has one launch site, select_topk (rerank_select.h), which the cluster-pruned
// search (ivf.hip) ends in too.
#include <stdint.h>

#include <cmath>

#include "gemm_pp.h"
#include "irc_common.h"
#include "rerank_select.h"

namespace irc {
namespace rerank {

constexpr int RR_CHUNK = 256;  // candidates per scoring workgroup (= its threads)
constexpr int RR_LPR = 8;      // lanes sharing one row
constexpr int SNT = 1024;      // select: threads per query
constexpr int S_STAGE = 8192;  // keys staged in LDS (64 KB)
constexpr int S_U = 16;        // key loads in flight per thread
constexpr int S_NH = 4;        // histogram copies (waves w, w + 4, ... share one)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// number of q in [lo, hi) with cand_off[q + 1] <= i, plus lo: the owner of flat
// candidate i when it lies in [lo, hi]
__device__ __forceinline__ int owner_of(const int64_t* __restrict__ cand_off, int lo, int hi,
                                        int64_t i) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cand_off[mid + 1] <= i) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The owners qa, qb of a chunk's first and last flat candidate i0, ilast: owner_of twice over
// [0, Q), as two independent searches in one loop (one latency, not two).  A thread's own
// owner then lies in [qa, qb]: nothing left to search inside one long list.
__device__ __forceinline__ void chunk_owners(const int64_t* __restrict__ cand_off, int Q,
                                             int64_t i0, int64_t ilast, int& qa, int& qb) {
  int lo_a = 0, hi_a = Q, lo_b = 0, hi_b = Q;
  while (lo_a < hi_a || lo_b < hi_b) {
    if (lo_a < hi_a) {
      const int mid = (lo_a + hi_a) >> 1;
      if (cand_off[mid + 1] <= i0) lo_a = mid + 1;
      else hi_a = mid;
    }
    if (lo_b < hi_b) {
      const int mid = (lo_b + hi_b) >> 1;
      if (cand_off[mid + 1] <= ilast) lo_b = mid + 1;
      else hi_b = mid;
    }
  }
  qa = lo_a;
  qb = lo_b;
}

// acc += <a, b> over the 4 e4m3 pairs of one 32-bit word, element order 0..3
// (v_cvt_pk_f32_fp8 on each word half; an e4m3 product is exact in fp32)
__device__ __forceinline__ float dot4_e4m3(uint32_t a, uint32_t b, float acc) {
  const auto a0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)a, false);
  const auto b0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)b, false);
  const auto a1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)a, true);
  const auto b1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)b, true);
  acc = fmaf(a0[0], b0[0], acc);
  acc = fmaf(a0[1], b0[1], acc);
  acc = fmaf(a1[0], b1[0], acc);
  acc = fmaf(a1[1], b1[1], acc);
  return acc;
}

// What the scoring body needs to know of its operands.  A lane reads NC pieces of a row,
// piece c at piece index s + 8 c: 16-byte pieces (8 lanes x 16 B = one 128-byte granule per
// step), and 8-byte ones for e4m3 at D = 64, where a row is half a granule.  dot() adds a
// piece's products to acc in ascending element order, one fmaf chain.
template <bool E4M3, int D>
struct Operand;
template <int D>
struct Operand<false, D> {  // bf16
  typedef u32x4 piece_t;
  static constexpr int ROW_BYTES = D * 2;
  static constexpr int NC = D / 64;
  static __device__ __forceinline__ float dot(piece_t a, piece_t b, float acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc = fmaf(__uint_as_float(a[j] << 16), __uint_as_float(b[j] << 16), acc);
      acc = fmaf(__uint_as_float(a[j] & 0xffff0000u), __uint_as_float(b[j] & 0xffff0000u), acc);
    }
    return acc;
  }
};
template <int D>
struct Operand<true, D> {  // e4m3 codes
  static constexpr int PW = D >= 128 ? 4 : 2;  // 32-bit words per piece
  typedef uint32_t piece_t __attribute__((ext_vector_type(PW)));
  static constexpr int ROW_BYTES = D;
  static constexpr int NC = D / (RR_LPR * PW * 4);
  static __device__ __forceinline__ float dot(piece_t a, piece_t b, float acc) {
#pragma unroll
    for (int w = 0; w < PW; ++w) acc = dot4_e4m3(a[w], b[w], acc);
    return acc;
  }
};

// The scoring body of both gathered kernels: keys[i] of flat candidate i, one workgroup per
// chunk of RR_CHUNK.  score_scale (a power of two: exact) applies to e4m3 only.  BIAS
// (irc_rerank_biased_topk): the ranked score is the score plus bias[i], one fp32 addition
// after the scale; without it bias is not read.
template <bool E4M3, int D, bool BIAS = false>
__device__ __forceinline__ void score_chunk(
    const char* __restrict__ queries, const char* __restrict__ docs, int Q, int64_t N,
    const int32_t* __restrict__ cand, const int64_t* __restrict__ cand_off, int64_t n_cand,
    int64_t doc_offset, float score_scale, uint64_t* __restrict__ keys,
    const float* __restrict__ bias = nullptr) {
  typedef Operand<E4M3, D> Op;
  typedef typename Op::piece_t piece_t;
  constexpr int NC = Op::NC;  // pieces per lane per row
  static_assert(NC * RR_LPR * (int)sizeof(piece_t) == Op::ROW_BYTES,
                "a row is a whole number of 8-lane steps");
  const int tid = threadIdx.x;
  const int sub = tid & (RR_LPR - 1);
  const int64_t i0 = (int64_t)blockIdx.x * RR_CHUNK;
  const int64_t i = i0 + tid;
  const int64_t ilast = (i0 + RR_CHUNK <= n_cand ? i0 + RR_CHUNK : n_cand) - 1;

  int qa, qb;
  chunk_owners(cand_off, Q, i0, ilast, qa, qb);
  int myq = 0;
  int myrow = -1;  // row in this shard, -1: not scored (past the end / another shard)
  uint32_t gid = 0;
  if (i < n_cand) {
    myq = owner_of(cand_off, qa, qb, i);
    myq = myq < Q - 1 ? myq : Q - 1;  // cand_off[Q] < n_cand (caller's error): stay in bounds
    const int64_t id = (int64_t)cand[i];
    const int64_t r = id - doc_offset;
    if (r >= 0 && r < N) {
      myrow = (int)r;
      gid = (uint32_t)id;
    }
  }

  // group g = tid / 8 scores candidates 8 g .. 8 g + 7 one after the other, its 8 lanes
  // sharing each row; lane s keeps the score of candidate 8 g + s
  piece_t qv[NC];
  int qcur = -1;
  float myscore = 0.f;
#pragma unroll 1
  for (int r = 0; r < RR_LPR; ++r) {
    const int row = __shfl(myrow, r, RR_LPR);
    const int qq = __shfl(myq, r, RR_LPR);
    float acc = 0.f;
    if (row >= 0) {  // uniform over the 8-lane group
      if (qq != qcur) {
        const piece_t* qp =
            reinterpret_cast<const piece_t*>(queries + (int64_t)qq * Op::ROW_BYTES) + sub;
#pragma unroll
        for (int c = 0; c < NC; ++c) qv[c] = qp[c * RR_LPR];
        qcur = qq;
      }
      const piece_t* dp =
          reinterpret_cast<const piece_t*>(docs + (int64_t)row * Op::ROW_BYTES) + sub;
      piece_t dv[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) dv[c] = dp[c * RR_LPR];
#pragma unroll
      for (int c = 0; c < NC; ++c) acc = Op::dot(qv[c], dv[c], acc);
    }
    // every lane takes part (the exchange stays inside the 8-lane group)
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 4, 64);
    if (sub == r) myscore = acc;
  }
  if constexpr (E4M3) myscore *= score_scale;
  if constexpr (BIAS) {
    if (myrow >= 0) myscore = add_bias(myscore, bias[i]);
  }
  if (i < n_cand) keys[i] = myrow >= 0 ? make_key(myscore, gid) : 0ull;
}

template <int D>
__global__ __launch_bounds__(RR_CHUNK) void rerank_score_kernel(
    const unsigned short* __restrict__ queries, const unsigned short* __restrict__ docs, int Q,
    int64_t N, const int32_t* __restrict__ cand, const int64_t* __restrict__ cand_off,
    int64_t n_cand, int64_t doc_offset, uint64_t* __restrict__ keys) {
  score_chunk<false, D>(reinterpret_cast<const char*>(queries),
                        reinterpret_cast<const char*>(docs), Q, N, cand, cand_off, n_cand,
                        doc_offset, 1.f, keys);
}

// rerank_score_kernel for e4m3 shards (irc_rerank_topk_fp8): rows of D bytes
template <int D>
__global__ __launch_bounds__(RR_CHUNK) void rerank_score_fp8_kernel(
    const unsigned char* __restrict__ queries, const unsigned char* __restrict__ docs, int Q,
    int64_t N, const int32_t* __restrict__ cand, const int64_t* __restrict__ cand_off,
    int64_t n_cand, int64_t doc_offset, float score_scale, uint64_t* __restrict__ keys) {
  score_chunk<true, D>(reinterpret_cast<const char*>(queries),
                       reinterpret_cast<const char*>(docs), Q, N, cand, cand_off, n_cand,
                       doc_offset, score_scale, keys);
}

// The two gathered kernels with the per-candidate bias (irc_rerank_biased_topk): bias[i]
// belongs to flat candidate i, as keys[i] does.
template <int D>
__global__ __launch_bounds__(RR_CHUNK) void rerank_score_bias_kernel(
    const unsigned short* __restrict__ queries, const unsigned short* __restrict__ docs, int Q,
    int64_t N, const int32_t* __restrict__ cand, const int64_t* __restrict__ cand_off,
    int64_t n_cand, int64_t doc_offset, const float* __restrict__ bias,
    uint64_t* __restrict__ keys) {
  score_chunk<false, D, true>(reinterpret_cast<const char*>(queries),
                              reinterpret_cast<const char*>(docs), Q, N, cand, cand_off, n_cand,
                              doc_offset, 1.f, keys, bias);
}

template <int D>
__global__ __launch_bounds__(RR_CHUNK) void rerank_score_fp8_bias_kernel(
    const unsigned char* __restrict__ queries, const unsigned char* __restrict__ docs, int Q,
    int64_t N, const int32_t* __restrict__ cand, const int64_t* __restrict__ cand_off,
    int64_t n_cand, int64_t doc_offset, float score_scale, const float* __restrict__ bias,
    uint64_t* __restrict__ keys) {
  score_chunk<true, D, true>(reinterpret_cast<const char*>(queries),
                             reinterpret_cast<const char*>(docs), Q, N, cand, cand_off, n_cand,
                             doc_offset, score_scale, keys, bias);
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t t = __shfl_xor(v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

// One workgroup per query over keys[cand_off[q] .. cand_off[q + 1]) (0 = not eligible):
// the min(k, eligible) largest keys, sorted descending, decoded into the outputs.
__global__ __launch_bounds__(SNT) void rerank_select_kernel(
    const uint64_t* __restrict__ keys, const int64_t* __restrict__ cand_off, int64_t n_cand,
    int k, float* __restrict__ out_score, int64_t* __restrict__ out_idx,
    int32_t* __restrict__ out_n) {
  __shared__ uint32_t hist[S_NH][256];
  __shared__ uint64_t s_key[RR_MAXK];
  __shared__ uint64_t c_key[S_STAGE];
  __shared__ uint64_t s_mn[SNT / 64], s_mx[SNT / 64];
  // 0: eligible count, 1: kr, 2: digit, 3: collect counter, 4: selected bucket size,
  // 5: staged count
  __shared__ uint32_t s_misc[6];
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t c0 = cand_off[q], c1 = cand_off[q + 1];
  c1 = c1 < n_cand ? c1 : n_cand;  // keys[] holds n_cand entries whatever cand_off says
  c0 = c0 < 0 ? 0 : c0;
  c0 = c0 < c1 ? c0 : c1;
  // unordered pass over the list's eligible keys, S_U loads in flight per thread
  auto each_key = [&](auto&& f) {
    for (int64_t b = c0 + tid; b < c1; b += (int64_t)SNT * S_U) {
      uint64_t v[S_U];
#pragma unroll
      for (int u = 0; u < S_U; ++u) {
        const int64_t j = b + (int64_t)u * SNT;
        v[u] = j < c1 ? keys[j] : 0ull;
      }
#pragma unroll
      for (int u = 0; u < S_U; ++u)
        if (v[u] != 0ull) f(v[u]);
    }
  };
  if (tid < 6) s_misc[tid] = 0;
  __syncthreads();
  // A list that fits the stage is read from global memory once: the first pass copies it
  // to LDS as it stands (ineligible zeros included; every LDS pass skips them).
  const bool small = c1 - c0 <= (int64_t)S_STAGE;
  // first pass: eligible count, smallest and largest key
  {
    uint32_t nz = 0;
    uint64_t mn = ~0ull, mx = 0ull;
    if (small) {
      for (int64_t b = c0 + tid; b < c1; b += (int64_t)SNT * S_U) {
        uint64_t v[S_U];
#pragma unroll
        for (int u = 0; u < S_U; ++u) {
          const int64_t j = b + (int64_t)u * SNT;
          v[u] = j < c1 ? keys[j] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < S_U; ++u) {
          const int64_t j = b + (int64_t)u * SNT;
          if (j < c1) c_key[j - c0] = v[u];
          if (v[u] != 0ull) {
            ++nz;
            mn = v[u] < mn ? v[u] : mn;
            mx = v[u] > mx ? v[u] : mx;
          }
        }
      }
    } else {
      each_key([&](uint64_t key) {
        ++nz;
        mn = key < mn ? key : mn;
        mx = key > mx ? key : mx;
      });
    }
    mn = wave_min_u64(mn);
    mx = wave_max_u64(mx);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nz += __shfl_xor(nz, o, 64);
    if (lane == 0) {
      s_mn[wave] = mn;
      s_mx[wave] = mx;
      if (nz) atomicAdd(&s_misc[0], nz);
    }
  }
  __syncthreads();
  const uint32_t M = s_misc[0];
  const int cnt = (int)(M < (uint32_t)k ? M : (uint32_t)k);
  uint64_t kth = 0;  // keep every eligible key
  // staged: c_key[0 .. ns) holds every key that matched the prefix when it was filled
  // (zeros to skip), and the keys above that prefix -- winners for sure -- are in s_key
  bool staged = small;
  uint32_t ns = small ? (uint32_t)(c1 - c0) : 0u;
  // distinct keys: exactly cnt winners (the slot test only guards the outputs against a
  // list that broke the unique-id contract)
  auto take = [&](uint64_t key) {
    const uint32_t slot = atomicAdd(&s_misc[3], 1u);
    if (slot < (uint32_t)cnt) s_key[slot] = key;
  };
  if (M > (uint32_t)k) {
    uint64_t mn = s_mn[0], mx = s_mx[0];
    for (int w = 1; w < SNT / 64; ++w) {
      mn = s_mn[w] < mn ? s_mn[w] : mn;
      mx = s_mx[w] > mx ? s_mx[w] : mx;
    }
    // 8-bit digits from the highest bit where the keys differ (distinct keys: mn != mx)
    int hi = 63 - __builtin_clzll((mn ^ mx) | 1ull);
    uint64_t pmask = hi >= 63 ? 0ull : (~0ull << (hi + 1));
    uint64_t prefix = mn & pmask;
    uint32_t kr = (uint32_t)k;
    uint32_t nsel = M;
    for (;;) {
      const int lo = hi >= 7 ? hi - 7 : 0;
      const uint32_t dm = (2u << (hi - lo)) - 1u;
      bool fill = false;
      if (!staged && nsel <= (uint32_t)S_STAGE) {
        // the selected bucket fits: the last pass over global memory moves it to LDS and
        // collects the keys above it
        each_key([&](uint64_t key) {
          const uint64_t kp = key & pmask;
          if (kp == prefix) {
            const uint32_t slot = atomicAdd(&s_misc[5], 1u);
            if (slot < (uint32_t)S_STAGE) c_key[slot] = key;
          } else if (kp > prefix) {
            take(key);
          }
        });
        staged = fill = true;
      }
      for (int j = tid; j < S_NH * 256; j += SNT) (&hist[0][0])[j] = 0;
      __syncthreads();
      if (fill) ns = s_misc[5] < (uint32_t)S_STAGE ? s_misc[5] : (uint32_t)S_STAGE;
      uint32_t* hw = hist[wave & (S_NH - 1)];
      if (staged) {
        for (uint32_t j = tid; j < ns; j += SNT) {
          const uint64_t key = c_key[j];
          if (key != 0ull && (key & pmask) == prefix)
            atomicAdd(&hw[(uint32_t)(key >> lo) & dm], 1u);
        }
      } else {
        each_key([&](uint64_t key) {
          if ((key & pmask) == prefix) atomicAdd(&hw[(uint32_t)(key >> lo) & dm], 1u);
        });
      }
      __syncthreads();
      if (wave == 0) {
        uint32_t bb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          uint32_t t = 0;
#pragma unroll
          for (int w = 0; w < S_NH; ++w) t += hist[w][4 * lane + j];
          bb[j] = t;
        }
        const uint32_t c4 = bb[0] + bb[1] + bb[2] + bb[3];
        uint32_t suf = c4;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const uint32_t t = __shfl_down(suf, o, 64);
          if (lane + o < 64) suf += t;
        }
        const uint32_t above = suf - c4;
        if (suf >= kr && above < kr) {
          uint32_t acc = above;
          int sel = 4 * lane;
          uint32_t bsz = bb[0];
          for (int j = 3; j >= 0; --j) {
            if (acc + bb[j] >= kr) {
              sel = 4 * lane + j;
              bsz = bb[j];
              break;
            }
            acc += bb[j];
          }
          s_misc[2] = (uint32_t)sel;
          s_misc[1] = kr - acc;
          s_misc[4] = bsz;
        }
      }
      __syncthreads();
      prefix |= (uint64_t)s_misc[2] << lo;
      pmask |= (uint64_t)dm << lo;
      kr = s_misc[1];
      nsel = s_misc[4];
      __syncthreads();  // s_misc and hist are rewritten by the next pass
      // the bucket holds exactly the keys still wanted: every key >= its lowest possible
      // member wins
      if (nsel == kr || lo == 0) break;
      hi = lo - 1;
    }
    kth = prefix;
  }
  // the winners: every key >= kth (those above the staged bucket are collected already)
  if (staged) {
    for (uint32_t j = tid; j < ns; j += SNT) {
      const uint64_t key = c_key[j];
      if (key != 0ull && key >= kth) take(key);
    }
  } else {
    each_key([&](uint64_t key) {
      if (key >= kth) take(key);
    });
  }
  __syncthreads();
  int npow = 1;
  while (npow < cnt) npow <<= 1;
  {
    uint32_t filled = s_misc[3];
    filled = filled < (uint32_t)cnt ? filled : (uint32_t)cnt;
    for (int j = (int)filled + tid; j < npow; j += SNT) s_key[j] = 0ull;
  }
  __syncthreads();
  for (int size = 2; size <= npow; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const int j = tid ^ stride;
      if (tid < npow && j > tid) {
        const bool desc = (tid & size) == 0;
        const uint64_t a = s_key[tid], b = s_key[j];
        if (desc ? (a < b) : (a > b)) {
          s_key[tid] = b;
          s_key[j] = a;
        }
      }
      __syncthreads();
    }
  }
  for (int j = tid; j < k; j += SNT) {
    float sc = -__builtin_huge_valf();
    int64_t id = -1;
    const uint64_t key = j < cnt ? s_key[j] : 0ull;
    if (key != 0ull) {
      sc = unorderable_f32((uint32_t)(key >> 32));
      id = (int64_t)(uint32_t)(~(uint32_t)key);
    }
    out_score[q * k + j] = sc;
    out_idx[q * k + j] = id;
  }
  if (tid == 0) out_n[q] = cnt;
}

// The one launch site of the select (rerank_select.h): every pass that fills a key workspace
// ends here, those of other files too.
int select_topk(const uint64_t* keys, const int64_t* off, int64_t n_keys, int64_t Q, int k,
                float* out_score, int64_t* out_idx, int32_t* out_n, hipStream_t st) {
  prof_begin(st);
  hipLaunchKernelGGL(rerank_select_kernel, dim3((unsigned)Q), dim3(SNT), 0, st, keys, off, n_keys,
                     k, out_score, out_idx, out_n);
  prof_end("rerank_select", st, (double)n_keys * 8.0);
  return check_launch("rerank_select_kernel");
}

// Stream method: keys of the candidates of other shards.  With ascending lists the ids
// below doc_offset are a prefix of each list and those from doc_offset + N on a suffix;
// the pick kernel writes every key between the two and none of these.  One query per
// blockIdx.x, its prefix and suffix spread over the gridDim.y workgroups.  Both bounds
// stay in [c0, c1] whatever the list holds.
constexpr int RF_NT = 256;
constexpr int RF_Y = 8;
__global__ __launch_bounds__(RF_NT) void rerank_foreign_kernel(
    const int32_t* __restrict__ cand, const int64_t* __restrict__ cand_off, int64_t n_cand,
    int64_t doc_offset, int64_t N, uint64_t* __restrict__ keys) {
  const int64_t q = blockIdx.x;
  int64_t c0 = cand_off[q], c1 = cand_off[q + 1];
  c1 = c1 < n_cand ? c1 : n_cand;
  c0 = c0 < 0 ? 0 : c0;
  c0 = c0 < c1 ? c0 : c1;
  const int64_t first = doc_offset, last = doc_offset + N;
  int64_t la = c0, ha = c1, lb = c0, hb = c1;
  while (la < ha || lb < hb) {
    if (la < ha) {
      const int64_t mid = la + ((ha - la) >> 1);
      if ((int64_t)cand[mid] < first) la = mid + 1;
      else ha = mid;
    }
    if (lb < hb) {
      const int64_t mid = lb + ((hb - lb) >> 1);
      if ((int64_t)cand[mid] < last) lb = mid + 1;
      else hb = mid;
    }
  }
  const int64_t pre = la - c0, total = pre + (c1 - lb);
  for (int64_t i = (int64_t)blockIdx.y * RF_NT + threadIdx.x; i < total;
       i += (int64_t)RF_Y * RF_NT)
    keys[i < pre ? c0 + i : lb + (i - pre)] = 0ull;
}

// group_of (irc_common.h, shared with the scan's group epilogue in gemm_pp.hip): the group of
// a global row id, searched from RC_NS samples of group_off the workgroup keeps in LDS.

// Grouped top-k (irc_rerank_topk_grouped): between scoring and select, every key that is
// not the maximum of its run becomes 0.  A run is a maximal stretch of consecutive
// candidates of one query in one group (lists ascending); rows of no group are zeroed.
// The same flat chunking as the scoring kernel, for any run length, in two phases:
//  PHASE 0.  Every thread finds its owner and group and reads its own key, no other; a
//    candidate whose left neighbour has another (owner, group) is a run head.  The kernel
//    is bound by the latency of its dependent loads, so the group search starts in LDS
//    (group_of) and the independent loads are issued before the owner search.  A max-scan
//    of the head positions and a segmented max-scan of the keys run inside each wave
//    (shuffles).  A run that begins and ends inside one wave -- nearly all of them at ten
//    rows a page -- is settled there: the last lane's maximum goes back to the run's lanes
//    and each zeroes its own key unless it is the maximum; head[i] = -1 marks it done.
//    The other pieces (a run cut by a wave or chunk boundary) go through memory: head[i]
//    keeps the flat index of the run's head -- from the earlier waves' tails through LDS,
//    and for the run the chunk opens in, which may have begun chunks earlier, from one
//    thread's binary search in the list for the first id of the group's row range -- and
//    the last lane of each piece folds its maximum into rmax[head] with one 64-bit integer
//    atomic max (rmax zeroed before the launch).  A run of any length, over any number of
//    waves and chunks, ends with its maximum in its head's slot, whatever the order.
//  PHASE 1 zeroes keys[i] unless head[i] < 0 or it equals rmax[head[i]].
// In both phases a thread writes its own key only, and reads no other thread's key.
// Keys are distinct (unique ids), so one key per run survives, and an all-zero run stays so.
template <int PHASE>
__global__ __launch_bounds__(RR_CHUNK) void rerank_collapse_kernel(
    const int32_t* __restrict__ cand, const int64_t* __restrict__ cand_off, int Q,
    int64_t n_cand, const int64_t* __restrict__ group_off, int n_groups,
    uint64_t* __restrict__ keys, unsigned long long* __restrict__ rmax,
    int64_t* __restrict__ head) {
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * RR_CHUNK;
  const int64_t i = i0 + tid;
  if constexpr (PHASE == 1) {
    if (i < n_cand) {
      const int64_t h = head[i];
      if (h >= 0) {
        const uint64_t key = keys[i];
        if (key != 0ull && key != (uint64_t)rmax[h]) keys[i] = 0ull;
      }
    }
    return;
  } else {
    __shared__ int s_q[RR_CHUNK], s_g[RR_CHUNK];
    __shared__ int s_wh[RR_CHUNK / 64];
    __shared__ int64_t s_open, s_first;
    __shared__ int64_t s_samp[RC_NS];
    static_assert(RC_NS == RR_CHUNK, "one sample of group_off per thread");
    const int lane = tid & 63, wave = tid >> 6;
    const int64_t ilast = (i0 + RR_CHUNK <= n_cand ? i0 + RR_CHUNK : n_cand) - 1;
    // every load that depends on nothing goes out first: the searches below are chains of
    // dependent loads, and their length is what this kernel's time is made of
    const bool valid = i < n_cand;
    const int64_t id = valid ? (int64_t)cand[i] : 0;
    const uint64_t own = valid ? keys[i] : 0ull;
    const int64_t stride = ((int64_t)n_groups + RC_NS - 1) / RC_NS;
    if (n_groups > 0) {
      const int64_t at = (tid + 1) * stride;
      s_samp[tid] = group_off[at < n_groups ? at : n_groups];
      if (tid == 0) s_first = group_off[0];
    }
    // the chunk's first and last owner, then this thread's own (score_chunk)
    int qa, qb;
    chunk_owners(cand_off, Q, i0, ilast, qa, qb);
    int myq = -1, myg = -1;  // past the end: a run of its own, no key
    if (valid) {
      myq = owner_of(cand_off, qa, qb, i);
      myq = myq < Q - 1 ? myq : Q - 1;  // cand_off[Q] < n_cand (caller's error): stay in bounds
    }
    __syncthreads();  // the samples
    if (valid) myg = group_of(group_off, n_groups, stride, s_first, s_samp, id);
    const uint64_t key = myg >= 0 ? own : 0ull;  // a row of no group never wins
    s_q[tid] = myq;
    s_g[tid] = myg;
    if (tid == 0) {
      // the head of the run the chunk opens in: the list's first candidate of this group
      // (its first id >= group_off[g]), searched in [list start, i0] only -- and no further
      // back than the ids between the group's first row and this one allow (unique ids)
      int64_t h = i0;
      if (myg >= 0) {
        const int64_t first = group_off[myg];
        int64_t lo = cand_off[myq];
        lo = lo < 0 ? 0 : lo;
        lo = lo < i0 - (id - first) ? i0 - (id - first) : lo;
        lo = lo < i0 ? lo : i0;
        while (lo < h) {
          const int64_t mid = lo + ((h - lo) >> 1);
          if ((int64_t)cand[mid] < first) lo = mid + 1;
          else h = mid;
        }
      }
      s_open = h;
    }
    __syncthreads();
    // a row of no group is a run of its own
    const bool flag = tid == 0 || myg < 0 || s_q[tid - 1] != myq || s_g[tid - 1] != myg;
    // the next candidate opens another run: known inside the chunk and at the end of keys[]
    const bool nflag = tid < RR_CHUNK - 1
                           ? (s_g[tid + 1] < 0 || s_q[tid + 1] != myq || s_g[tid + 1] != myg)
                           : i + 1 >= n_cand;
    const int64_t open = s_open;
    // hl: the run head's place in the chunk as far as this wave knows it, -1: before the wave
    int hl = flag ? tid : -1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(hl, o, 64);
      if (lane >= o) hl = t > hl ? t : hl;
    }
    // the run begins at that lane, not earlier (tid 0 only if the chunk opens a run)
    const bool begins = hl > 0 || (hl == 0 && open == i0);
    // segmented max inside the wave: lane - o is of this run while it is not before its head
    const int sl = hl >= 0 ? hl - wave * 64 : 0;
    uint64_t run = key;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t t = __shfl_up(run, o, 64);
      if (lane - o >= sl) run = t > run ? t : run;
    }
    const bool tail = lane == 63 || nflag;  // the last lane of this (run, wave) piece
    int tl = tail ? lane : 64;              // that lane, for every lane of the piece
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_down(tl, o, 64);
      if (lane + o < 64) tl = t < tl ? t : tl;
    }
    const uint64_t piece = __shfl(run, tl, 64);           // the piece's maximum
    const bool ends = __shfl((int)nflag, tl, 64) != 0;    // the run ends with the piece
    if (lane == 63) s_wh[wave] = hl;
    __syncthreads();
    if (begins && ends) {  // the whole run lies in this wave: settled here
      if (valid) {
        if (own != 0ull && own != piece) keys[i] = 0ull;
        head[i] = -1;
      }
    } else {
      if (hl < 0) {  // the run began in an earlier wave; wave 0 always knows (tid 0 is a head)
        for (int v = wave - 1; v >= 0; --v) {
          hl = s_wh[v];
          if (hl >= 0) break;
        }
      }
      const int64_t h = hl > 0 ? i0 + hl : open;  // in [0, i]
      if (valid) {
        head[i] = h;
        if (tail && run != 0ull) atomicMax(&rmax[h], (unsigned long long)run);
      }
    }
  }
}

// Grouped merge (irc_topk_merge_grouped): the keys of the P lists of one query, at most
// S_STAGE entries in all, with every key that is not the maximum of its group set to 0; the
// unchanged select then runs over keys[q L .. (q + 1) L), L = P * kin.  One workgroup per
// query, of one thread per pair of sort slots (64 to SNT threads), and everything in LDS:
//  1. every entry becomes v = id << 32 | orderable score; an empty slot (id < 0; its score
//     is not read), an id from 2^31 on and the padding up to a power of two are ~0;
//  2. a bitonic sort makes v ascending.  The group is a non-decreasing function of the row
//     id, so the entries of one group are one run of the sorted array, whatever list they
//     came from, and the ~0 entries are its tail;
//  3. every entry finds its group (group_of, from LDS samples) and the head of its run --
//     the first sorted position whose id reaches the group's first row, a binary search in
//     LDS -- and folds its key into s_rmax[head] with one 64-bit atomic max: the maximum
//     does not depend on the order the atomics land in;
//  4. the entry whose key equals its run's maximum keeps it, every other one writes 0.
// Keys of one group are distinct while the row ids are (the caller's contract), so one
// entry per group survives; a row id that appears twice may survive twice.  Every sorted
// position below L writes its slot of keys[], so the workspace needs no clearing, and
// workgroup q writes the select's offset q L (the last one also Q L).
__global__ __launch_bounds__(SNT) void merge_collapse_kernel(
    const float* __restrict__ in_score, const int64_t* __restrict__ in_idx, int P, int Q,
    int kin, const int64_t* __restrict__ group_off, int n_groups, uint64_t* __restrict__ keys,
    int64_t* __restrict__ list_off) {
  __shared__ uint64_t s_v[S_STAGE];
  __shared__ unsigned long long s_rmax[S_STAGE];
  __shared__ int16_t s_head[S_STAGE];
  __shared__ int64_t s_samp[RC_NS];
  __shared__ int64_t s_first;
  static_assert(S_STAGE <= 32768, "a run head fits int16");
  const int q = blockIdx.x;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int L = P * kin;  // <= S_STAGE
  int npow = 1;
  while (npow < L) npow <<= 1;
  if (tid == 0) {
    list_off[q] = (int64_t)q * L;
    if (q == Q - 1) list_off[Q] = (int64_t)Q * L;
  }
  const int64_t stride = ((int64_t)n_groups + RC_NS - 1) / RC_NS;
  if (n_groups > 0) {
    for (int t = tid; t < RC_NS; t += nt) {
      const int64_t at = (t + 1) * stride;
      s_samp[t] = group_off[at < n_groups ? at : n_groups];
    }
    if (tid == 0) s_first = group_off[0];
  }
  for (int j = tid; j < npow; j += nt) {
    uint64_t v = ~0ull;
    if (j < L) {
      const int p = j / kin;
      const int64_t src = ((int64_t)p * Q + q) * kin + (j - p * kin);
      const int64_t id = in_idx[src];
      if (id >= 0 && id < (1ll << 31))
        v = ((uint64_t)id << 32) | (uint64_t)orderable_f32(in_score[src]);
    }
    s_v[j] = v;
    s_rmax[j] = 0ull;
  }
  __syncthreads();
  for (int size = 2; size <= npow; size <<= 1) {
    for (int st = size >> 1; st > 0; st >>= 1) {
      for (int t = tid; t < (npow >> 1); t += nt) {
        const int i = 2 * t - (t & (st - 1));
        const int j = i + st;
        const bool asc = (i & size) == 0;
        const uint64_t a = s_v[i], b = s_v[j];
        if ((a > b) == asc) {
          s_v[i] = b;
          s_v[j] = a;
        }
      }
      __syncthreads();
    }
  }
  // the ranking key of a sorted entry (make_key of its score and id)
  auto key_of = [](uint64_t v) { return (v << 32) | (uint64_t)(uint32_t)(~(uint32_t)(v >> 32)); };
  // positions from L on hold padding only (at least npow - L entries are ~0, all at the end)
  for (int i = tid; i < L; i += nt) {
    const uint64_t v = s_v[i];
    int h = -1;  // an empty slot or a row of no group: never wins
    if (v != ~0ull) {
      const int g = group_of(group_off, n_groups, stride, s_first, s_samp, (int64_t)(v >> 32));
      if (g >= 0) {
        int64_t first = group_off[g];  // <= id
        first = first < 0 ? 0 : first;
        const uint64_t target = (uint64_t)first << 32;
        int lo = 0, hi = i;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s_v[mid] < target) lo = mid + 1;
          else hi = mid;
        }
        h = lo;
        atomicMax(&s_rmax[h], (unsigned long long)key_of(v));
      }
    }
    s_head[i] = (int16_t)h;
  }
  __syncthreads();
  for (int i = tid; i < L; i += nt) {
    const int h = s_head[i];
    uint64_t key = 0ull;
    if (h >= 0) {
      key = key_of(s_v[i]);
      if (key != (uint64_t)s_rmax[h]) key = 0ull;
    }
    keys[(int64_t)q * L + i] = key;
  }
}

// irc_topk_merge_grouped's workspace: the keys, then the Q + 1 list offsets of the select
static size_t merge_keys_bytes(int64_t Q, int64_t L) { return align256((size_t)(Q * L) * 8); }
static size_t merge_workspace_bytes(int64_t Q, int64_t L) {
  return merge_keys_bytes(Q, L) + align256((size_t)(Q + 1) * 8);
}
static bool merge_sizes_ok(int64_t P, int64_t Q, int64_t kin) {
  return P >= 1 && kin >= 1 && Q >= 0 && Q < (1ll << 31) - 1 && P <= S_STAGE &&
         kin <= S_STAGE && P * kin <= S_STAGE;
}

// irc_scan_topk_grouped's workspace: gmax [Q][n_groups], the keys the select ranks, then its
// Q + 1 list offsets q * n_groups
static size_t scan_group_keys_bytes(int64_t Q, int64_t n_groups) {
  return align256((size_t)(Q * n_groups) * 8);
}
static size_t scan_group_workspace_bytes(int64_t Q, int64_t n_groups) {
  return scan_group_keys_bytes(Q, n_groups) + align256((size_t)(Q + 1) * 8);
}
// the sizes the workspace formula is defined for (the call itself reports them)
static bool scan_group_sizes_ok(int64_t Q, int64_t n_groups) {
  return Q >= 0 && Q < (1ll << 31) - 1 && n_groups >= 0 && n_groups < (1ll << 31) - 1 &&
         Q * n_groups < (1ll << 31) * 256;
}

// list_off[q] = q * L for q <= Q: the select's offsets over Q lists of one length
__global__ __launch_bounds__(256) void list_off_kernel(int64_t* __restrict__ list_off, int64_t Q,
                                                       int64_t L) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q <= Q) list_off[q] = q * L;
}

// keys, and for the grouped form rmax and head after them: 8 bytes per candidate each, every
// region on a 256-byte boundary
static size_t region_bytes(int64_t n_cand) {
  return align256((size_t)(n_cand > 0 ? n_cand : 0) * 8);
}
static size_t workspace_bytes_for(int64_t n_cand, bool grouped) {
  return (grouped ? 3 : 1) * region_bytes(n_cand) + 256;
}

// What one of the extern "C" entries asks of rerank_run.
struct Form {
  const char* name;          // the prefix of its messages
  bool stream, e4m3;         // the scoring pass: gathered / streamed, bf16 / e4m3 operands
  bool grouped;              // top-k per group: the collapse between scoring and select
  const int64_t* group_off;  // grouped only (null is the caller's error)
  int64_t n_groups;
  bool biased = false;         // irc_rerank_biased_topk: the ranked score is score + bias[i]
  const float* bias = nullptr;  // biased only, [n_cand] (null is the caller's error)
};

}  // namespace rerank
}  // namespace irc

using namespace irc;
using namespace irc::rerank;

extern "C" int irc_rerank_chunk(void) { return RR_CHUNK; }

extern "C" int64_t irc_rerank_topk_workspace(int64_t Q, int64_t n_cand, int64_t k) {
  (void)Q;
  (void)k;
  return (int64_t)workspace_bytes_for(n_cand, false);
}

extern "C" int64_t irc_rerank_topk_grouped_workspace(int64_t Q, int64_t n_cand, int64_t k) {
  (void)Q;
  (void)k;
  return (int64_t)workspace_bytes_for(n_cand, true);
}

extern "C" int irc_rerank_stream_tile(void) { return gpp::PICK_TILE; }

// The gathered scoring pass: keys[0 .. n_cand) from the candidates' rows.
static int score_gather(const Form& f, const void* queries, const void* docs, int64_t Q,
                        int64_t N, int64_t D, const int32_t* cand, const int64_t* cand_off,
                        int64_t n_cand, int64_t doc_offset, float score_scale, uint64_t* keys,
                        hipStream_t st) {
  const unsigned blocks = (unsigned)((n_cand + RR_CHUNK - 1) / RR_CHUNK);
  const unsigned short* qp = static_cast<const unsigned short*>(queries);
  const unsigned short* dp = static_cast<const unsigned short*>(docs);
  const unsigned char* qp8 = static_cast<const unsigned char*>(queries);
  const unsigned char* dp8 = static_cast<const unsigned char*>(docs);
  prof_begin(st);
#define IRC_RR_CASE(DD)                                                                         \
  case DD:                                                                                      \
    if (f.biased && f.e4m3)                                                                     \
      hipLaunchKernelGGL((rerank_score_fp8_bias_kernel<DD>), dim3(blocks), dim3(RR_CHUNK), 0,   \
                         st, qp8, dp8, (int)Q, N, cand, cand_off, n_cand, doc_offset,           \
                         score_scale, f.bias, keys);                                            \
    else if (f.biased)                                                                          \
      hipLaunchKernelGGL((rerank_score_bias_kernel<DD>), dim3(blocks), dim3(RR_CHUNK), 0, st,   \
                         qp, dp, (int)Q, N, cand, cand_off, n_cand, doc_offset, f.bias, keys);  \
    else if (f.e4m3)                                                                            \
      hipLaunchKernelGGL((rerank_score_fp8_kernel<DD>), dim3(blocks), dim3(RR_CHUNK), 0, st,    \
                         qp8, dp8, (int)Q, N, cand, cand_off, n_cand, doc_offset, score_scale,  \
                         keys);                                                                 \
    else                                                                                        \
      hipLaunchKernelGGL((rerank_score_kernel<DD>), dim3(blocks), dim3(RR_CHUNK), 0, st, qp,    \
                         dp, (int)Q, N, cand, cand_off, n_cand, doc_offset, keys);              \
    break;
  switch (D) {
    IRC_RR_CASE(64)
    IRC_RR_CASE(128)
    IRC_RR_CASE(256)
    IRC_RR_CASE(384)
    IRC_RR_CASE(512)
    IRC_RR_CASE(768)
    default: IRC_RR_CASE(1024)
  }
#undef IRC_RR_CASE
  // the gathered row bytes
  prof_end(f.e4m3 ? "rerank_fp8_score" : "rerank_score", st,
           (double)n_cand * D * (f.e4m3 ? 1.0 : 2.0));
  return check_launch(f.e4m3 ? "rerank_score_fp8_kernel" : "rerank_score_kernel");
}

// The streamed scoring pass (lists ascending in global id): the keys of the ids outside the
// shard are zeroed, the others picked out of the score tiles of the ping-pong GEMM loop.
static int score_stream(const Form& f, const void* queries, const void* docs, int64_t Q,
                        int64_t N, int64_t D, const int32_t* cand, const int64_t* cand_off,
                        int64_t n_cand, int64_t doc_offset, float score_scale, uint64_t* keys,
                        hipStream_t st) {
  prof_begin(st);
  hipLaunchKernelGGL(rerank_foreign_kernel, dim3((unsigned)Q, RF_Y), dim3(RF_NT), 0, st, cand,
                     cand_off, n_cand, doc_offset, N, keys);
  if (N > 0) {
    gpp::PArgs a = gpp::qd_pass(queries, docs, Q, N, D, f.e4m3);
    a.keys = keys;
    a.cand = cand;
    a.cand_off = cand_off;
    a.n_cand = n_cand;
    a.doc_offset = doc_offset;
    if (f.e4m3) a.score_scale = score_scale;
    if (f.biased) a.bias = f.bias;
    gpp::run_pick(a, st, f.e4m3, f.biased);
  }
  // the bytes the pass streams: the shard once per query tile
  prof_end(f.e4m3 ? "rerank_fp8_stream_score" : "rerank_stream_score", st,
           (double)((Q + 255) / 256) * (double)N * D * (f.e4m3 ? 1.0 : 2.0));
  return check_launch(f.e4m3 ? "rerank_fp8_stream_score" : "rerank_stream_score");
}

// Every entry: the one sequence of argument checks, one scoring pass, the collapse if
// grouped, the select.  The order of the checks is part of the interface
// (tests/test_rerank_validation_cpu.py): a call that breaks two reports the earlier one.
static int rerank_run(const Form& f, const void* queries, const void* docs, int64_t Q, int64_t N,
                      int64_t D, const int32_t* cand, const int64_t* cand_off, int64_t n_cand,
                      int64_t k, int64_t doc_offset, float score_scale, void* workspace,
                      int64_t workspace_bytes, float* out_score, int64_t* out_idx,
                      int32_t* out_n, irc_stream_t stream) {
  IRC_REQUIRE(Q >= 0 && N >= 0 && n_cand >= 0, "%s: negative size", f.name);
  IRC_REQUIRE(k >= 1 && k <= RR_MAXK, "%s: k=%lld outside [1, %d]", f.name, (long long)k,
              RR_MAXK);
  IRC_REQUIRE(supported_d(D), "%s: unsupported D=%lld", f.name, (long long)D);
  IRC_REQUIRE(!(f.e4m3 && f.stream) || D % 128 == 0,
              "%s: unsupported D=%lld for the e4m3 stream method (D %% 128 == 0)", f.name,
              (long long)D);
  IRC_REQUIRE(!f.e4m3 || pow2_scale(score_scale), "%s: score_scale must be a power of two",
              f.name);
  IRC_REQUIRE(doc_offset >= 0 && doc_offset + N < (1ll << 31),
              "%s: global doc ids must fit int32 (doc_offset + N < 2^31)", f.name);
  IRC_REQUIRE(Q < (1ll << 31) - 1, "%s: Q too large", f.name);
  IRC_REQUIRE(n_cand < (1ll << 31) * RR_CHUNK, "%s: n_cand too large", f.name);
  // one workgroup per (query tile, doc tile): the grid and the kernel's int tile count
  IRC_REQUIRE(!f.stream || ((Q + 255) / 256) * ((N + 255) / 256) < (1ll << 31),
              "%s: Q x N too large for the stream method", f.name);
  const int64_t need = (int64_t)workspace_bytes_for(n_cand, f.grouped);
  if (workspace == nullptr || workspace_bytes < need) {
    set_error("%s: workspace %lld < required %lld bytes", f.name, (long long)workspace_bytes,
              (long long)need);
    return IRC_E_WORKSPACE;
  }
  if (Q == 0) return IRC_OK;
  IRC_REQUIRE(queries && cand_off && out_score && out_idx && out_n, "%s: null pointer", f.name);
  IRC_REQUIRE(n_cand == 0 || (cand && (N == 0 || docs)), "%s: null candidates / docs", f.name);
  IRC_REQUIRE(!f.biased || n_cand == 0 || f.bias != nullptr, "%s: null bias", f.name);
  IRC_REQUIRE(((uintptr_t)queries % 16) == 0 && ((uintptr_t)docs % 16) == 0,
              "%s: queries and docs must be 16-byte aligned", f.name);
  if (f.grouped) {
    IRC_REQUIRE(f.group_off != nullptr, "%s: null group_off", f.name);
    IRC_REQUIRE(f.n_groups >= 0 && f.n_groups < (1ll << 31) - 1,
                "%s: n_groups=%lld outside [0, 2^31 - 1)", f.name, (long long)f.n_groups);
  }
  hipStream_t st = as_stream(stream);
  uint64_t* keys = static_cast<uint64_t*>(workspace);
  if (n_cand > 0) {
    if (int rc = (f.stream ? score_stream : score_gather)(f, queries, docs, Q, N, D, cand,
                                                          cand_off, n_cand, doc_offset,
                                                          score_scale, keys, st))
      return rc;
  }
  if (f.grouped && n_cand > 0) {
    const size_t region = region_bytes(n_cand);
    unsigned long long* rmax =
        reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + region);
    int64_t* head = reinterpret_cast<int64_t*>(static_cast<char*>(workspace) + 2 * region);
    const unsigned blocks = (unsigned)((n_cand + RR_CHUNK - 1) / RR_CHUNK);
    if (hipMemsetAsync(rmax, 0, (size_t)n_cand * 8, st) != hipSuccess)
      return check_launch("rerank_collapse memset");
    prof_begin(st);
    hipLaunchKernelGGL((rerank_collapse_kernel<0>), dim3(blocks), dim3(RR_CHUNK), 0, st, cand,
                       cand_off, (int)Q, n_cand, f.group_off, (int)f.n_groups, keys, rmax, head);
    hipLaunchKernelGGL((rerank_collapse_kernel<1>), dim3(blocks), dim3(RR_CHUNK), 0, st, cand,
                       cand_off, (int)Q, n_cand, f.group_off, (int)f.n_groups, keys, rmax, head);
    // per key: key + id read, head written, then key + head + slot read
    prof_end("rerank_collapse", st, (double)n_cand * 44.0);
    if (int rc = check_launch("rerank_collapse_kernel")) return rc;
  }
  return select_topk(keys, cand_off, n_cand, Q, (int)k, out_score, out_idx, out_n, st);
}

extern "C" int irc_rerank_topk(const void* queries, const void* docs, int64_t Q, int64_t N,
                               int64_t D, const int32_t* cand, const int64_t* cand_off,
                               int64_t n_cand, int64_t k, int64_t doc_offset, void* workspace,
                               int64_t workspace_bytes, float* out_score, int64_t* out_idx,
                               int32_t* out_n, irc_stream_t stream) {
  return rerank_run({"rerank_topk", false, false, false, nullptr, 0}, queries, docs, Q, N, D,
                    cand, cand_off, n_cand, k, doc_offset, 1.f, workspace, workspace_bytes,
                    out_score, out_idx, out_n, stream);
}

extern "C" int irc_rerank_topk_stream(const void* queries, const void* docs, int64_t Q,
                                      int64_t N, int64_t D, const int32_t* cand,
                                      const int64_t* cand_off, int64_t n_cand, int64_t k,
                                      int64_t doc_offset, void* workspace,
                                      int64_t workspace_bytes, float* out_score,
                                      int64_t* out_idx, int32_t* out_n, irc_stream_t stream) {
  return rerank_run({"rerank_topk", true, false, false, nullptr, 0}, queries, docs, Q, N, D,
                    cand, cand_off, n_cand, k, doc_offset, 1.f, workspace, workspace_bytes,
                    out_score, out_idx, out_n, stream);
}

extern "C" int irc_rerank_topk_fp8(const void* queries, const void* docs, int64_t Q, int64_t N,
                                   int64_t D, const int32_t* cand, const int64_t* cand_off,
                                   int64_t n_cand, int64_t k, int64_t doc_offset,
                                   float score_scale, void* workspace, int64_t workspace_bytes,
                                   float* out_score, int64_t* out_idx, int32_t* out_n,
                                   irc_stream_t stream) {
  return rerank_run({"rerank_topk_fp8", false, true, false, nullptr, 0}, queries, docs, Q, N, D,
                    cand, cand_off, n_cand, k, doc_offset, score_scale, workspace,
                    workspace_bytes, out_score, out_idx, out_n, stream);
}

extern "C" int irc_rerank_topk_stream_fp8(const void* queries, const void* docs, int64_t Q,
                                          int64_t N, int64_t D, const int32_t* cand,
                                          const int64_t* cand_off, int64_t n_cand, int64_t k,
                                          int64_t doc_offset, float score_scale, void* workspace,
                                          int64_t workspace_bytes, float* out_score,
                                          int64_t* out_idx, int32_t* out_n,
                                          irc_stream_t stream) {
  return rerank_run({"rerank_topk_fp8", true, true, false, nullptr, 0}, queries, docs, Q, N, D,
                    cand, cand_off, n_cand, k, doc_offset, score_scale, workspace,
                    workspace_bytes, out_score, out_idx, out_n, stream);
}

// The top-k per group, over any of the four scoring passes (flags).
extern "C" int irc_rerank_topk_grouped(const void* queries, const void* docs, int64_t Q,
                                       int64_t N, int64_t D, const int32_t* cand,
                                       const int64_t* cand_off, int64_t n_cand, int64_t k,
                                       int64_t doc_offset, const int64_t* group_off,
                                       int64_t n_groups, uint32_t flags, float score_scale,
                                       void* workspace, int64_t workspace_bytes,
                                       float* out_score, int64_t* out_idx, int32_t* out_n,
                                       irc_stream_t stream) {
  return rerank_run({"rerank_topk_grouped", (flags & IRC_RERANK_STREAM) != 0,
                     (flags & IRC_RERANK_E4M3) != 0, true, group_off, n_groups},
                    queries, docs, Q, N, D, cand, cand_off, n_cand, k, doc_offset, score_scale,
                    workspace, workspace_bytes, out_score, out_idx, out_n, stream);
}

// The candidate top-k by score + bias[i], over any of the four scoring passes (flags), per row
// (group_off null) or per group: the addition happens in the scoring pass, before the collapse.
extern "C" int irc_rerank_biased_topk(const void* queries, const void* docs, int64_t Q,
                                      int64_t N, int64_t D, const int32_t* cand,
                                      const int64_t* cand_off, int64_t n_cand, int64_t k,
                                      int64_t doc_offset, const int64_t* group_off,
                                      int64_t n_groups, uint32_t flags, float score_scale,
                                      const float* bias, void* workspace,
                                      int64_t workspace_bytes, float* out_score,
                                      int64_t* out_idx, int32_t* out_n, irc_stream_t stream) {
  return rerank_run({"rerank_topk_biased", (flags & IRC_RERANK_STREAM) != 0,
                     (flags & IRC_RERANK_E4M3) != 0, group_off != nullptr, group_off, n_groups,
                     true, bias},
                    queries, docs, Q, N, D, cand, cand_off, n_cand, k, doc_offset, score_scale,
                    workspace, workspace_bytes, out_score, out_idx, out_n, stream);
}

extern "C" int64_t irc_scan_topk_grouped_workspace(int64_t Q, int64_t n_groups, int64_t k) {
  (void)k;
  if (!scan_group_sizes_ok(Q, n_groups)) return 0;  // the call itself reports the sizes
  return (int64_t)scan_group_workspace_bytes(Q, n_groups);
}

// The dense scan per group: every row of the shard is a candidate of every query, so there
// is no list.  The group epilogue of the ping-pong GEMM loop (gemm_pp.hip, EPI_GROUP) folds
// each score tile into gmax[q][g], one key per (query, group), and the select of rerank_run
// ranks each query's n_groups keys (0: the group has no row in this shard).  The order of
// the checks is part of the interface (tests/test_scan_group_cpu.py).
extern "C" int irc_scan_topk_grouped(const void* queries, const void* docs, int64_t Q, int64_t N,
                                     int64_t D, int64_t k, int64_t doc_offset,
                                     const int64_t* group_off, int64_t n_groups, uint32_t flags,
                                     float score_scale, void* workspace,
                                     int64_t workspace_bytes, float* out_score,
                                     int64_t* out_idx, int32_t* out_n, irc_stream_t stream) {
  const char* name = "scan_topk_grouped";
  const bool e4m3 = (flags & IRC_RERANK_E4M3) != 0;
  IRC_REQUIRE(Q >= 0 && N >= 0, "%s: negative size", name);
  IRC_REQUIRE(k >= 1 && k <= RR_MAXK, "%s: k=%lld outside [1, %d]", name, (long long)k, RR_MAXK);
  IRC_REQUIRE(supported_d(D), "%s: unsupported D=%lld", name, (long long)D);
  IRC_REQUIRE(!e4m3 || D % 128 == 0, "%s: unsupported D=%lld for e4m3 operands (D %% 128 == 0)",
              name, (long long)D);
  IRC_REQUIRE((flags & ~IRC_RERANK_E4M3) == 0, "%s: unsupported flags 0x%x (IRC_RERANK_E4M3 only)",
              name, (unsigned)flags);
  IRC_REQUIRE(!e4m3 || pow2_scale(score_scale), "%s: score_scale must be a power of two", name);
  IRC_REQUIRE(doc_offset >= 0 && doc_offset + N < (1ll << 31),
              "%s: global doc ids must fit int32 (doc_offset + N < 2^31)", name);
  IRC_REQUIRE(Q < (1ll << 31) - 1, "%s: Q too large", name);
  IRC_REQUIRE(n_groups >= 0 && n_groups < (1ll << 31) - 1,
              "%s: n_groups=%lld outside [0, 2^31 - 1)", name, (long long)n_groups);
  IRC_REQUIRE(Q * n_groups < (1ll << 31) * 256, "%s: Q x n_groups too large", name);
  // one workgroup per (query tile, doc tile): the grid and the kernel's int tile count
  IRC_REQUIRE(((Q + 255) / 256) * ((N + 255) / 256) < (1ll << 31), "%s: Q x N too large", name);
  const int64_t need = (int64_t)scan_group_workspace_bytes(Q, n_groups);
  if (workspace == nullptr || workspace_bytes < need) {
    set_error("%s: workspace %lld < required %lld bytes", name, (long long)workspace_bytes,
              (long long)need);
    return IRC_E_WORKSPACE;
  }
  if (Q == 0) return IRC_OK;
  IRC_REQUIRE(queries && group_off && out_score && out_idx && out_n && (N == 0 || docs),
              "%s: null pointer", name);
  IRC_REQUIRE(((uintptr_t)queries % 16) == 0 && ((uintptr_t)docs % 16) == 0,
              "%s: queries and docs must be 16-byte aligned", name);
  hipStream_t st = as_stream(stream);
  uint64_t* gmax = static_cast<uint64_t*>(workspace);
  int64_t* list_off = reinterpret_cast<int64_t*>(static_cast<char*>(workspace) +
                                                 scan_group_keys_bytes(Q, n_groups));
  const int64_t n_keys = Q * n_groups;
  prof_begin(st);
  // key 0: no row of the group in this shard (the select skips zeros)
  if (n_keys > 0 && hipMemsetAsync(gmax, 0, (size_t)n_keys * 8, st) != hipSuccess)
    return check_launch("scan_group memset");
  if (N > 0 && n_groups > 0) {
    gpp::PArgs a = gpp::qd_pass(queries, docs, Q, N, D, e4m3);
    a.doc_offset = doc_offset;
    if (e4m3) a.score_scale = score_scale;
    a.gmax = gmax;
    a.group_off = group_off;
    a.n_groups = (int)n_groups;
    gpp::run_group(a, st, e4m3);
  }
  // the bytes the pass streams: the shard once per query tile, and the zeroed keys
  prof_end(e4m3 ? "scan_group_fp8_score" : "scan_group_score", st,
           (double)((Q + 255) / 256) * (double)N * D * (e4m3 ? 1.0 : 2.0) + (double)n_keys * 8.0);
  if (int rc = check_launch(e4m3 ? "scan_group_fp8_score" : "scan_group_score")) return rc;
  hipLaunchKernelGGL(list_off_kernel, dim3((unsigned)(Q / 256 + 1)), dim3(256), 0, st, list_off, Q,
                     n_groups);
  return select_topk(gmax, list_off, n_keys, Q, (int)k, out_score, out_idx, out_n, st);
}

extern "C" int64_t irc_topk_merge_grouped_workspace(int64_t P, int64_t Q, int64_t kin) {
  if (!merge_sizes_ok(P, Q, kin)) return 0;  // the call itself reports the sizes
  return (int64_t)merge_workspace_bytes(Q, P * kin);
}

// The reduce step of the grouped candidate top-k over several shards: the collapse of each
// query's P lists to one entry per group, then the select of rerank_run.
extern "C" int irc_topk_merge_grouped(const float* in_score, const int64_t* in_idx, int64_t P,
                                      int64_t Q, int64_t kin, int64_t kout,
                                      const int64_t* group_off, int64_t n_groups,
                                      void* workspace, int64_t workspace_bytes,
                                      float* out_score, int64_t* out_idx, int32_t* out_n,
                                      irc_stream_t stream) {
  IRC_REQUIRE(P >= 1 && Q >= 0 && kin >= 1, "topk_merge_grouped: bad sizes");
  IRC_REQUIRE(kout >= 1 && kout <= RR_MAXK, "topk_merge_grouped: kout=%lld outside [1, %d]",
              (long long)kout, RR_MAXK);
  IRC_REQUIRE(P <= S_STAGE && kin <= S_STAGE && P * kin <= S_STAGE,
              "topk_merge_grouped: P * kin = %lld x %lld above %d entries per query",
              (long long)P, (long long)kin, S_STAGE);
  IRC_REQUIRE(Q < (1ll << 31) - 1, "topk_merge_grouped: Q too large");
  IRC_REQUIRE(n_groups >= 0 && n_groups < (1ll << 31) - 1,
              "topk_merge_grouped: n_groups=%lld outside [0, 2^31 - 1)", (long long)n_groups);
  if (Q == 0) return IRC_OK;
  IRC_REQUIRE(group_off != nullptr, "topk_merge_grouped: null group_off");
  const int64_t L = P * kin;
  const int64_t need = (int64_t)merge_workspace_bytes(Q, L);
  IRC_REQUIRE(workspace != nullptr && workspace_bytes >= need,
              "topk_merge_grouped: workspace %lld < required %lld bytes",
              (long long)workspace_bytes, (long long)need);
  IRC_REQUIRE(in_score && in_idx && out_score && out_idx && out_n,
              "topk_merge_grouped: null pointer");
  hipStream_t st = as_stream(stream);
  uint64_t* keys = static_cast<uint64_t*>(workspace);
  int64_t* list_off =
      reinterpret_cast<int64_t*>(static_cast<char*>(workspace) + merge_keys_bytes(Q, L));
  // one thread per pair of sort slots (the sort array is L rounded up to a power of two)
  int threads = 64;
  while (threads < SNT && 2 * threads < L) threads <<= 1;
  prof_begin(st);
  hipLaunchKernelGGL(merge_collapse_kernel, dim3((unsigned)Q), dim3(threads), 0, st, in_score,
                     in_idx, (int)P, (int)Q, (int)kin, group_off, (int)n_groups, keys, list_off);
  // per entry: score + id read, key written
  prof_end("topk_merge_collapse", st, (double)(Q * L) * 20.0);
  if (int rc = check_launch("merge_collapse_kernel")) return rc;
  return select_topk(keys, list_off, Q * L, Q, (int)kout, out_score, out_idx, out_n, st);
}
