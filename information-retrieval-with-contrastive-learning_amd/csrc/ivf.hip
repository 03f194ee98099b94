// Cluster-pruned dense top-k for gfx950 (MI355X): an inverted-file (IVF) index whose probed
// lists are scored on MFMA.
//
// The dense scoring src/evaluation.py:110-112 sketches, restricted to the rows of the lists
// nearest to each query (the reference reaches for faiss only to cluster,
// src/contrastor/utils.py:39-47).  The corpus is kept in LIST ORDER: list c owns the rows
// [list_off[c], list_off[c + 1]) of docs, row_id[row] is the row's global id.  A search probes
// nprobe lists per query; everything approximate is in that choice.  The ranking of the probed
// rows is exact: (score desc, global id asc), as irc_scan_topk ranks a whole shard.
//
// Design ("Cluster-pruned search"):
//  * A probed list is read ONCE per 32 of the queries that probe it.  The (query, probe slot)
//    pairs are sorted by list on the device (retrieval.ivf_plan) and cut into chunks of 32;
//    a work item is (list, chunk, segment of IVF_TILE_ROWS rows), so a long list is spread
//    over many workgroups and a short one costs one.  The launch is a 2-D grid over a host
//    bound on the chunk count and the longest list's segments; a workgroup finds its list by
//    binary search in chunk_off and leaves at once when it has no item.
//  * ivf_score_kernel: the chunk's 32 queries are stationary B fragments of
//    v_mfma_f32_32x32x16_bf16 (absent columns zero), the segment streams in 32-row tiles --
//    contiguous in memory, the rows being in list order -- through registers into an LDS
//    tile: tile t + 1 is in flight to the registers while tile t is multiplied, so the
//    registers are the second buffer and the LDS holds one tile (two workgroups per CU up to
//    D = 768).  The four waves are four k-slices of D / 4 each, on one tile:
//    the query fragments then fit the registers at every D with one kernel body.  The four
//    partial 32 x 32 sums meet in LDS and are added as (s0 + s1) + (s2 + s3).
//  * One accumulation order per (query, row): an MFMA column's result does not depend on the
//    other columns, a k-slice is one chain in ascending k, and the slices add in the order
//    above -- so a pair's score has the same bits whatever else the call holds.
//  * Each (pair, row) owns one slot of the key workspace: keys[slot_off[pair] + row - list
//    start] = make_key(score, row_id[row]).  Every slot of a query is written exactly once, so
//    the workspace is not cleared; no atomics, no waits between workgroups.
//  * The select is rerank_select_kernel, unchanged (rerank_select.h), over (keys, cand_off).
#include <stdint.h>

#include "irc_common.h"
#include "rerank_select.h"

namespace irc {
namespace ivf {

constexpr int IVF_TILE_ROWS = 256;  // rows of one work item's segment
constexpr int IVF_NT = 256;         // threads: four waves, one k-slice each
constexpr int IVF_KS = 4;
constexpr int IVF_CHUNK = 32;       // pairs per chunk: the MFMA's columns
constexpr int IVF_MT = 32;          // rows per tile: the MFMA's rows
constexpr int XCH_LD = 65;          // floats per register row of the exchange (64 lanes + 1)
constexpr int XCH_WAVE = 16 * XCH_LD;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// LDS of one workgroup: the row tile (rows padded by 16 bytes: the fragment reads of 32 rows
// then spread over the banks), the k-slice exchange, the chunk's 32 slot bases.
template <int D>
struct Lds {
  static constexpr int ROW_B = D * 2 + 16;
  static constexpr int TILE_B = IVF_MT * ROW_B;
  static constexpr int XCH_AT = TILE_B;
  static constexpr int SLOT_AT = XCH_AT + IVF_KS * XCH_WAVE * 4;
  static constexpr int BYTES = SLOT_AT + IVF_CHUNK * 8;
  static_assert(BYTES <= IRC_LDS_BYTES, "the tiles fit the CU's LDS");
  static_assert(SLOT_AT % 8 == 0 && XCH_AT % 16 == 0, "alignment");
};

template <int D>
__global__ __launch_bounds__(IVF_NT) void ivf_score_kernel(
    const unsigned short* __restrict__ queries, const unsigned short* __restrict__ docs,
    const int32_t* __restrict__ row_id, const int64_t* __restrict__ list_off, int nlist,
    const int64_t* __restrict__ slot_off, const int32_t* __restrict__ pair_order,
    const int64_t* __restrict__ seg_off, const int64_t* __restrict__ chunk_off, int nprobe,
    int64_t n_pairs, int64_t N, int64_t n_keys, uint64_t* __restrict__ keys) {
  typedef Lds<D> L;
  constexpr int PASSES = D / 64;  // 16-byte pieces per thread per tile
  constexpr int KSTEPS = D / 64;  // MFMAs per wave per tile (D / 4 over 16)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* xch = reinterpret_cast<float*>(smem + L::XCH_AT);
  int64_t* s_slot = reinterpret_cast<int64_t*>(smem + L::SLOT_AT);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // the item: list c by binary search over the chunk counts, then chunk and row segment
  const int64_t x = blockIdx.x;
  if (x >= chunk_off[nlist]) return;
  int c = 0;
  {
    int hi = nlist - 1;
    while (c < hi) {
      const int mid = (c + hi) >> 1;
      if (chunk_off[mid + 1] <= x) c = mid + 1;
      else hi = mid;
    }
  }
  const int64_t lstart = list_off[c];
  int64_t lend = list_off[c + 1];
  lend = lend < N ? lend : N;  // nothing is read at or past row N, whatever list_off says
  const int64_t r0 = lstart + (int64_t)blockIdx.y * IVF_TILE_ROWS;
  if (lstart < 0 || r0 >= lend) return;
  const int64_t rend = r0 + IVF_TILE_ROWS < lend ? r0 + IVF_TILE_ROWS : lend;
  const int64_t p0 = seg_off[c] + (x - chunk_off[c]) * IVF_CHUNK;
  int64_t pend = seg_off[c + 1];
  pend = pend < n_pairs ? pend : n_pairs;
  if (p0 < 0 || p0 >= pend) return;
  const int ncols = (int)(pend - p0 < IVF_CHUNK ? pend - p0 : IVF_CHUNK);

  // the chunk's queries, gathered by index into this wave's k-slice of B fragments
  const int col = lane & 31, half = lane >> 5;
  u16x8 bfr[KSTEPS];
  {
    int64_t pair = col < ncols ? (int64_t)pair_order[p0 + col] : -1;
    if (pair >= n_pairs) pair = -1;
    const unsigned short* qp =
        queries + (pair < 0 ? 0 : pair / nprobe) * D + wave * (D / IVF_KS) + 8 * half;
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      bfr[s] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (pair >= 0) bfr[s] = *reinterpret_cast<const u16x8*>(qp + 16 * s);
    }
    if (tid < IVF_CHUNK) {
      int64_t base = -1;
      if (tid < ncols) {
        const int64_t pr = (int64_t)pair_order[p0 + tid];
        if (pr >= 0 && pr < n_pairs) base = slot_off[pr];
      }
      s_slot[tid] = base;
    }
  }

  // tile t of the segment: 32 rows, contiguous in memory; thread piece p is bytes
  // [(p * 256 + tid) * 16, + 16) of it.  Rows past the segment's end are clamped to its last.
  u32x4 stage[PASSES];
  auto load_tile = [&](int t) {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int at = (p * IVF_NT + tid) * 16;
      int64_t row = r0 + (int64_t)t * IVF_MT + at / (D * 2);
      row = row < rend ? row : rend - 1;
      stage[p] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(docs) +
                                                 row * (D * 2) + at % (D * 2));
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int at = (p * IVF_NT + tid) * 16;
      *reinterpret_cast<u32x4*>(smem + (at / (D * 2)) * L::ROW_B + at % (D * 2)) = stage[p];
    }
  };

  const int nt = (int)((rend - r0 + IVF_MT - 1) / IVF_MT);
  load_tile(0);
  store_tile();
  __syncthreads();  // tile 0 and the slot bases
  // the (row, columns) this thread adds up and writes: keys of one pair are consecutive in
  // the row, so 32 lanes write 256 contiguous bytes
  const int orow = tid & 31, ocol0 = tid >> 5;
  const int oat = ((orow & 3) + 4 * (orow >> 3)) * XCH_LD + 32 * ((orow >> 2) & 1);
#pragma unroll 1
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) load_tile(t + 1);
    const char* tile = smem + col * L::ROW_B + (wave * (D / IVF_KS) + 8 * half) * 2;
    f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      const u16x8 av = *reinterpret_cast<const u16x8*>(tile + 32 * s);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av),
                                                    __builtin_bit_cast(bf16x8, bfr[s]), acc, 0,
                                                    0, 0);
    }
    // acc[r]: row (r & 3) + 8 (r >> 2) + 4 half, column col, over this wave's k-slice
#pragma unroll
    for (int r = 0; r < 16; ++r) xch[wave * XCH_WAVE + r * XCH_LD + lane] = acc[r];
    __syncthreads();  // the four partial sums; every wave has read tile t
    if (t + 1 < nt) store_tile();
    const int64_t row = r0 + (int64_t)t * IVF_MT + orow;
    if (row < rend) {
      const uint32_t gid = (uint32_t)row_id[row];
#pragma unroll
      for (int j = 0; j < IVF_CHUNK / 8; ++j) {
        const int oc = ocol0 + 8 * j;
        const float* xp = xch + oat + oc;
        const float sum = (xp[0] + xp[XCH_WAVE]) + (xp[2 * XCH_WAVE] + xp[3 * XCH_WAVE]);
        const int64_t base = s_slot[oc];
        const int64_t at = base + (row - lstart);
        if (base >= 0 && at < n_keys) keys[at] = make_key(sum, gid);
      }
    }
    __syncthreads();  // tile t + 1; the exchange is rewritten by the next tile
  }
}

static size_t workspace_bytes_for(int64_t total_rows) {
  return align256((size_t)(total_rows > 0 ? total_rows : 0) * 8) + 256;
}

}  // namespace ivf
}  // namespace irc

using namespace irc;
using namespace irc::ivf;

extern "C" int irc_ivf_tile_rows(void) { return IVF_TILE_ROWS; }

extern "C" int64_t irc_ivf_topk_workspace(int64_t Q, int64_t nprobe, int64_t total_rows,
                                          int64_t k) {
  (void)Q;
  (void)nprobe;
  (void)k;
  return (int64_t)workspace_bytes_for(total_rows);
}

// The order of the checks is part of the interface (tests/test_ivf_cpu.py): a call that breaks
// two reports the earlier one.
extern "C" int irc_ivf_topk(const void* queries, const void* docs, const int32_t* row_id,
                            const int64_t* list_off, int64_t nlist, const int32_t* probe,
                            const int64_t* slot_off, const int64_t* cand_off,
                            const int32_t* pair_order, const int64_t* seg_off,
                            const int64_t* chunk_off, int64_t Q, int64_t nprobe, int64_t N,
                            int64_t D, int64_t k, int64_t total_rows, int64_t max_list_rows,
                            void* workspace, int64_t workspace_bytes, float* out_score,
                            int64_t* out_idx, int32_t* out_n, irc_stream_t stream) {
  const char* name = "ivf_topk";
  IRC_REQUIRE(Q >= 0 && N >= 0 && nlist >= 0 && total_rows >= 0 && max_list_rows >= 0,
              "%s: negative size", name);
  IRC_REQUIRE(k >= 1 && k <= rerank::RR_MAXK, "%s: k=%lld outside [1, %d]", name, (long long)k,
              rerank::RR_MAXK);
  IRC_REQUIRE(supported_d(D), "%s: unsupported D=%lld", name, (long long)D);
  IRC_REQUIRE(nprobe >= 1 && nprobe <= nlist, "%s: nprobe=%lld outside [1, nlist=%lld]", name,
              (long long)nprobe, (long long)nlist);
  IRC_REQUIRE(N < (1ll << 31), "%s: global doc ids must fit int32 (N < 2^31)", name);
  // pairs are int32 in pair_order, and the grid: x over the chunk bound, y over the segments
  IRC_REQUIRE(Q < (1ll << 31) - 1 && nlist < (1ll << 31) - 1 && Q * nprobe < (1ll << 30),
              "%s: Q x nprobe too large", name);
  IRC_REQUIRE(max_list_rows <= N && max_list_rows <= 65535ll * IVF_TILE_ROWS,
              "%s: max_list_rows=%lld above N or %lld", name, (long long)max_list_rows,
              65535ll * IVF_TILE_ROWS);
  const int64_t need = (int64_t)workspace_bytes_for(total_rows);
  if (workspace == nullptr || workspace_bytes < need) {
    set_error("%s: workspace %lld < required %lld bytes", name, (long long)workspace_bytes,
              (long long)need);
    return IRC_E_WORKSPACE;
  }
  if (Q == 0) return IRC_OK;
  IRC_REQUIRE(queries && row_id && list_off && probe && slot_off && cand_off && pair_order &&
                  seg_off && chunk_off && out_score && out_idx && out_n && (N == 0 || docs),
              "%s: null pointer", name);
  IRC_REQUIRE(((uintptr_t)queries % 16) == 0 && ((uintptr_t)docs % 16) == 0,
              "%s: queries and docs must be 16-byte aligned", name);
  hipStream_t st = as_stream(stream);
  uint64_t* keys = static_cast<uint64_t*>(workspace);
  const int64_t n_pairs = Q * nprobe;
  if (total_rows > 0 && max_list_rows > 0) {
    // every list has at most one partly filled chunk
    const int64_t gx = n_pairs / IVF_CHUNK + (nlist < n_pairs ? nlist : n_pairs);
    const int64_t gy = (max_list_rows + IVF_TILE_ROWS - 1) / IVF_TILE_ROWS;
    const unsigned short* qp = static_cast<const unsigned short*>(queries);
    const unsigned short* dp = static_cast<const unsigned short*>(docs);
    prof_begin(st);
#define IRC_IVF_CASE(DD)                                                                       \
  case DD:                                                                                     \
    hipLaunchKernelGGL((ivf_score_kernel<DD>), dim3((unsigned)gx, (unsigned)gy), dim3(IVF_NT), \
                       Lds<DD>::BYTES, st, qp, dp, row_id, list_off, (int)nlist, slot_off,     \
                       pair_order, seg_off, chunk_off, (int)nprobe, n_pairs, N, total_rows,    \
                       keys);                                                                  \
    break;
    switch (D) {
      IRC_IVF_CASE(64)
      IRC_IVF_CASE(128)
      IRC_IVF_CASE(256)
      IRC_IVF_CASE(384)
      IRC_IVF_CASE(512)
      IRC_IVF_CASE(768)
      default: IRC_IVF_CASE(1024)
    }
#undef IRC_IVF_CASE
    // The rows streamed are the sum over lists of chunks x rows, which only the device knows;
    // the host's figure is its upper bound, every pair streaming its list alone.
    // tools/ivf_probe.py reports the exact count from the plan.
    prof_end("ivf_score", st, (double)total_rows * D * 2.0);
    if (int rc = check_launch("ivf_score_kernel")) return rc;
  }
  return rerank::select_topk(keys, cand_off, total_rows, Q, (int)k, out_score, out_idx, out_n,
                             st);
}
