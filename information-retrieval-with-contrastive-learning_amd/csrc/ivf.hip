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
//  * irc_ivf_topk takes the plan from its caller (retrieval.ivf_plan, torch); irc_ivf_search
//    issues the probe, the plan's own kernels (irc_ivf_plan, below the scoring kernel), the
//    scoring pass and the select on one stream with no host synchronisation, the key count
//    replaced by a host bound.
//  * e4m3 lists (irc_ivf_topk_fp8, irc_ivf_search_fp8): the same body on
//    v_mfma_f32_32x32x16_fp8_fp8 over rows of D bytes; the plan, the work item, the slots and
//    the select do not know the element.  irc_ivf_search_fp8 probes with the bf16 queries and
//    scores their e4m3 codes, quantised into the workspace on the same stream.
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
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// The element forms of the scoring kernel.  EB = 2: bf16 rows on v_mfma_f32_32x32x16_bf16, a
// lane's fragment of one k-step is 16 bytes.  EB = 1: e4m3fn bytes on
// v_mfma_f32_32x32x16_fp8_fp8 (the instruction of the fp8 scan, scan_topk.hip EB = 1), a
// lane's fragment is 8 bytes.  A k-step is 16 elements in both, so a wave's chain is D / 64
// MFMAs whatever the element.
template <int EB>
struct Elem;
template <>
struct Elem<2> {
  typedef u16x8 frag;
  static __device__ __forceinline__ frag zero() { return u16x8{0, 0, 0, 0, 0, 0, 0, 0}; }
  static __device__ __forceinline__ f32x16 mfma(frag a, frag b, f32x16 acc) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a),
                                                   __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
  }
};
template <>
struct Elem<1> {
  typedef long frag;
  static __device__ __forceinline__ frag zero() { return 0; }
  static __device__ __forceinline__ f32x16 mfma(frag a, frag b, f32x16 acc) {
    return __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a, b, acc, 0, 0, 0);
  }
};

// LDS of one workgroup: the row tile, the k-slice exchange, the chunk's 32 slot bases.  The
// rows are padded so that the fragment reads of 32 rows spread over the banks: by 16 bytes for
// the 16-byte bf16 fragments, by 8 for the 8-byte e4m3 ones (row stride 8 x odd: 32 rows x 2
// banks cover the 64 banks once).  The e4m3 tile is 32 rows too, half the bf16 tile's bytes: a
// 64-row tile (two MFMA blocks and two accumulators per wave, the bf16 tile's bytes per pair of
// barriers) was measured and lost -- its kernel ran at the bf16 kernel's time, not at half of
// it ("e4m3 lists"; profiles/ivf_fp8_probe_tile64.json).
template <int D, int EB = 2>
struct Lds {
  static constexpr int ROW_D = D * EB;  // bytes of a row in memory
  static constexpr int ROW_B = ROW_D + 8 * EB;
  static constexpr int TILE_B = IVF_MT * ROW_B;
  static constexpr int XCH_AT = TILE_B;
  static constexpr int SLOT_AT = XCH_AT + IVF_KS * XCH_WAVE * 4;
  static constexpr int BYTES = SLOT_AT + IVF_CHUNK * 8;
  static_assert(BYTES <= IRC_LDS_BYTES, "the tiles fit the CU's LDS");
  static_assert(SLOT_AT % 8 == 0 && XCH_AT % 16 == 0, "alignment");
};

// One body for both elements and all seven widths.  score_scale is the e4m3 form's descale
// (a power of two: the multiply is exact); the bf16 form does not read it.
template <int D, int EB = 2>
__global__ __launch_bounds__(IVF_NT) void ivf_score_kernel(
    const unsigned char* __restrict__ queries, const unsigned char* __restrict__ docs,
    const int32_t* __restrict__ row_id, const int64_t* __restrict__ list_off, int nlist,
    const int64_t* __restrict__ slot_off, const int32_t* __restrict__ pair_order,
    const int64_t* __restrict__ seg_off, const int64_t* __restrict__ chunk_off, int nprobe,
    int64_t n_pairs, int64_t N, int64_t n_keys, uint64_t* __restrict__ keys, float score_scale) {
  typedef Lds<D, EB> L;
  typedef Elem<EB> E;
  typedef typename E::frag frag;
  constexpr int TILE_D = IVF_MT * L::ROW_D;  // bytes of a tile in memory
  constexpr int PASSES = (TILE_D + IVF_NT * 16 - 1) / (IVF_NT * 16);  // 16-byte pieces per thread
  constexpr bool PART = TILE_D % (IVF_NT * 16) != 0;  // e4m3 at D = 64: half a pass
  constexpr int KSTEPS = D / 64;  // MFMAs per wave per tile (D / 4 over 16)
  constexpr int FB = 8 * EB;      // bytes of a lane's fragment
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
  frag bfr[KSTEPS];
  {
    int64_t pair = col < ncols ? (int64_t)pair_order[p0 + col] : -1;
    if (pair >= n_pairs) pair = -1;
    const unsigned char* qp = queries + (pair < 0 ? 0 : pair / nprobe) * L::ROW_D +
                              wave * (L::ROW_D / IVF_KS) + FB * half;
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      bfr[s] = E::zero();
      if (pair >= 0) bfr[s] = *reinterpret_cast<const frag*>(qp + 2 * FB * s);
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
      if (PART && at >= TILE_D) continue;
      int64_t row = r0 + (int64_t)t * IVF_MT + at / L::ROW_D;
      row = row < rend ? row : rend - 1;
      stage[p] = *reinterpret_cast<const u32x4*>(docs + row * L::ROW_D + at % L::ROW_D);
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int at = (p * IVF_NT + tid) * 16;
      if (PART && at >= TILE_D) continue;
      char* dst = smem + (at / L::ROW_D) * L::ROW_B + at % L::ROW_D;
      if constexpr (EB == 2) {
        *reinterpret_cast<u32x4*>(dst) = stage[p];
      } else {  // the e4m3 row stride is a multiple of 8, not of 16
        *reinterpret_cast<u32x2*>(dst) = u32x2{stage[p][0], stage[p][1]};
        *reinterpret_cast<u32x2*>(dst + 8) = u32x2{stage[p][2], stage[p][3]};
      }
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
    const char* tile = smem + col * L::ROW_B + wave * (L::ROW_D / IVF_KS) + FB * half;
    f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      const frag av = *reinterpret_cast<const frag*>(tile + 2 * FB * s);
      acc = E::mfma(av, bfr[s], acc);
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
        float sum = (xp[0] + xp[XCH_WAVE]) + (xp[2 * XCH_WAVE] + xp[3 * XCH_WAVE]);
        if constexpr (EB == 1) sum *= score_scale;
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

// ---------------------------------------------------------------------------------------
// The plan on the device (irc_ivf_plan): retrieval.ivf_plan's five arrays with no sort.
//
// Bit (c, q) of an nlist x W-word bitmap (W = ceil(Q / 32)) says that query q probes list c;
// rows being unique within a probe row, list c's pair count is the popcount of its row and the
// stable rank of pair (q, j) inside the list is the popcount of the row below bit q.  The bits
// are OR-ed in atomically -- the result does not depend on the order -- and everything else
// is integer prefix sums:
//   mark    pairs: set the bits; per workgroup the sums of the pairs' list lengths and of the
//           invalid pairs (the reduce pass of the pairs' scan)
//   rows    bitmap rows, a group of lanes each: the running popcount in front of every word
//           (wpre), so a list's count and a pair's rank are one word's popcount plus one load
//   count   lists: seg_off / chunk_off at once when one workgroup covers the lists, else the
//           workgroup's sums
//   bases   one workgroup per scan: the exclusive scan of the workgroup sums, in place
//   lists   (only past one workgroup) seg_off / chunk_off from the counts and the bases
//   pairs   slot_off, cand_off, and pair_order[seg_off[c] + rank] = pair; an invalid pair goes
//           to seg_off[nlist] + (invalid pairs before it)
// A workgroup covers PLAN_SPAN consecutive elements, PLAN_ITEMS per thread; the pairs' scan has
// Q * nprobe + 1 elements (the last is the total) and the lists' nlist + 1.  No workgroup waits
// on another, no float arithmetic, every index checked against its array.
constexpr int PLAN_NT = 1024;
constexpr int PLAN_ITEMS = 4;
constexpr int PLAN_SPAN = PLAN_NT * PLAN_ITEMS;
constexpr int PLAN_NW = PLAN_NT / 64;

// Exclusive prefix of (a, b) over the workgroup's threads and the workgroup's totals.
// s_w: 2 * PLAN_NW int64 of LDS, free again on return.
__device__ __forceinline__ void block_scan2(int64_t a, int64_t b, int64_t* s_w, int64_t& ea,
                                            int64_t& eb, int64_t& ta, int64_t& tb) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t ia = a, ib = b;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t xa = __shfl_up((long long)ia, d, 64), xb = __shfl_up((long long)ib, d, 64);
    if (lane >= d) {
      ia += xa;
      ib += xb;
    }
  }
  if (lane == 63) {
    s_w[wave] = ia;
    s_w[PLAN_NW + wave] = ib;
  }
  __syncthreads();
  ea = ia - a;
  eb = ib - b;
  ta = tb = 0;
#pragma unroll
  for (int w = 0; w < PLAN_NW; ++w) {
    const int64_t xa = s_w[w], xb = s_w[PLAN_NW + w];
    if (w < wave) {
      ea += xa;
      eb += xb;
    }
    ta += xa;
    tb += xb;
  }
  __syncthreads();
}

// the list of pair p, or -1 when its id names none
template <typename PT>
__device__ __forceinline__ int64_t pair_list(const PT* __restrict__ probe, int64_t p, int nlist) {
  const int64_t c = (int64_t)probe[p];
  return c >= 0 && c < nlist ? c : -1;
}

template <typename PT>
__global__ __launch_bounds__(PLAN_NT) void ivf_plan_mark_kernel(
    const PT* __restrict__ probe, const int64_t* __restrict__ list_off, int nlist, int nprobe,
    int W, int64_t n_pairs, uint32_t* __restrict__ bits, int64_t* __restrict__ blk_rows,
    int64_t* __restrict__ blk_inv, int32_t* __restrict__ out_probe) {
  __shared__ int64_t s_w[2 * PLAN_NW];
  const int64_t p0 = (int64_t)blockIdx.x * PLAN_SPAN + (int64_t)threadIdx.x * PLAN_ITEMS;
  int64_t rows = 0, inv = 0;
#pragma unroll
  for (int i = 0; i < PLAN_ITEMS; ++i) {
    const int64_t p = p0 + i;
    if (p >= n_pairs) break;
    const int64_t c = pair_list(probe, p, nlist);
    if (out_probe) {
      const int64_t id = (int64_t)probe[p];
      out_probe[p] = id >= 0 && id < (1ll << 31) ? (int32_t)id : -1;
    }
    if (c < 0) {
      ++inv;
      continue;
    }
    const uint32_t q = (uint32_t)p / (uint32_t)nprobe;
    atomicOr(&bits[c * W + (q >> 5)], 1u << (q & 31));
    rows += list_off[c + 1] - list_off[c];
  }
  int64_t ea, eb, ta, tb;
  block_scan2(rows, inv, s_w, ea, eb, ta, tb);
  if (threadIdx.x == 0) {
    blk_rows[blockIdx.x] = ta;
    blk_inv[blockIdx.x] = tb;
  }
}

// Elements [e0, e0 + PLAN_ITEMS) of the lists' scan: the pair count of list e (0 for the
// element nlist) from the running counts, and its chunk count.
__device__ __forceinline__ int64_t list_count(const uint32_t* __restrict__ bits,
                                              const uint32_t* __restrict__ wpre, int W, int64_t c) {
  const int64_t at = c * W + (W - 1);
  return (int64_t)wpre[at] + __popc(bits[at]);
}

__device__ __forceinline__ void write_list_offsets(const int64_t* n, int64_t e0, int nlist,
                                                   int64_t seg, int64_t chk,
                                                   int64_t* __restrict__ seg_off,
                                                   int64_t* __restrict__ chunk_off) {
#pragma unroll
  for (int i = 0; i < PLAN_ITEMS; ++i) {
    const int64_t e = e0 + i;
    if (e > nlist) break;
    seg_off[e] = seg;
    chunk_off[e] = chk;
    seg += n[i];
    chk += (n[i] + IVF_CHUNK - 1) / IVF_CHUNK;
  }
}

// wpre[c][w] = the bits of row c in the words before w.  g lanes (a power of two, at most a
// wave) share a row: its words in steps of g, a shuffle scan within the group, the carry in
// registers.  Every lane runs every step (the shuffles need them); only the loads and stores
// are guarded.
constexpr int ROWS_NT = 256;
__global__ __launch_bounds__(ROWS_NT) void ivf_plan_rows_kernel(const uint32_t* __restrict__ bits,
                                                                int nlist, int W, int g,
                                                                uint32_t* __restrict__ wpre) {
  const int64_t t = (int64_t)blockIdx.x * ROWS_NT + threadIdx.x;
  const int64_t c = t / g;
  const int l = (int)(threadIdx.x & (g - 1));
  uint32_t carry = 0;
  for (int w0 = 0; w0 < W; w0 += g) {
    const int w = w0 + l;
    const bool ok = c < nlist && w < W;
    const uint32_t n = ok ? __popc(bits[c * W + w]) : 0u;
    uint32_t inc = n;
    for (int d = 1; d < g; d <<= 1) {
      const uint32_t x = __shfl_up(inc, d, g);
      if (l >= d) inc += x;
    }
    if (ok) wpre[c * W + w] = carry + inc - n;
    carry += __shfl(inc, g - 1, g);
  }
}

__global__ __launch_bounds__(PLAN_NT) void ivf_plan_count_kernel(
    const uint32_t* __restrict__ bits, int nlist, int W, const uint32_t* __restrict__ wpre,
    int64_t* __restrict__ blk_cnt, int64_t* __restrict__ blk_chk, int64_t* __restrict__ seg_off,
    int64_t* __restrict__ chunk_off) {
  __shared__ int64_t s_w[2 * PLAN_NW];
  const int64_t e0 = (int64_t)blockIdx.x * PLAN_SPAN + (int64_t)threadIdx.x * PLAN_ITEMS;
  int64_t n[PLAN_ITEMS], cnt = 0, chk = 0;
#pragma unroll
  for (int i = 0; i < PLAN_ITEMS; ++i) {
    n[i] = e0 + i < nlist ? list_count(bits, wpre, W, e0 + i) : 0;
    cnt += n[i];
    chk += (n[i] + IVF_CHUNK - 1) / IVF_CHUNK;
  }
  int64_t ea, eb, ta, tb;
  block_scan2(cnt, chk, s_w, ea, eb, ta, tb);
  if (gridDim.x == 1) {
    write_list_offsets(n, e0, nlist, ea, eb, seg_off, chunk_off);
  } else if (threadIdx.x == 0) {
    blk_cnt[blockIdx.x] = ta;
    blk_chk[blockIdx.x] = tb;
  }
}

// Workgroup 0: the pairs' workgroup sums (a0, b0, n0 of them); workgroup 1: the lists'.  Each
// becomes its exclusive scan in place, PLAN_NT sums per step with the carry in registers.
__global__ __launch_bounds__(PLAN_NT) void ivf_plan_bases_kernel(int64_t* a0, int64_t* b0,
                                                                 int64_t n0, int64_t* a1,
                                                                 int64_t* b1, int64_t n1) {
  __shared__ int64_t s_w[2 * PLAN_NW];
  int64_t* a = blockIdx.x == 0 ? a0 : a1;
  int64_t* b = blockIdx.x == 0 ? b0 : b1;
  const int64_t n = blockIdx.x == 0 ? n0 : n1;
  int64_t ca = 0, cb = 0;
  for (int64_t at = 0; at < n; at += PLAN_NT) {
    const int64_t i = at + threadIdx.x;
    const int64_t va = i < n ? a[i] : 0, vb = i < n ? b[i] : 0;
    int64_t ea, eb, ta, tb;
    block_scan2(va, vb, s_w, ea, eb, ta, tb);
    if (i < n) {
      a[i] = ca + ea;
      b[i] = cb + eb;
    }
    ca += ta;
    cb += tb;
  }
}

__global__ __launch_bounds__(PLAN_NT) void ivf_plan_lists_kernel(
    const uint32_t* __restrict__ bits, const uint32_t* __restrict__ wpre, int nlist, int W,
    const int64_t* __restrict__ blk_cnt, const int64_t* __restrict__ blk_chk,
    int64_t* __restrict__ seg_off, int64_t* __restrict__ chunk_off) {
  __shared__ int64_t s_w[2 * PLAN_NW];
  const int64_t e0 = (int64_t)blockIdx.x * PLAN_SPAN + (int64_t)threadIdx.x * PLAN_ITEMS;
  int64_t n[PLAN_ITEMS], cnt = 0, chk = 0;
#pragma unroll
  for (int i = 0; i < PLAN_ITEMS; ++i) {
    n[i] = e0 + i < nlist ? list_count(bits, wpre, W, e0 + i) : 0;
    cnt += n[i];
    chk += (n[i] + IVF_CHUNK - 1) / IVF_CHUNK;
  }
  int64_t ea, eb, ta, tb;
  block_scan2(cnt, chk, s_w, ea, eb, ta, tb);
  write_list_offsets(n, e0, nlist, blk_cnt[blockIdx.x] + ea, blk_chk[blockIdx.x] + eb, seg_off,
                     chunk_off);
}

template <typename PT>
__global__ __launch_bounds__(PLAN_NT) void ivf_plan_pairs_kernel(
    const PT* __restrict__ probe, const int64_t* __restrict__ list_off, int nlist, int nprobe,
    int W, int64_t n_pairs, const uint32_t* __restrict__ bits, const uint32_t* __restrict__ wpre,
    const int64_t* __restrict__ blk_rows, const int64_t* __restrict__ blk_inv,
    const int64_t* __restrict__ seg_off, int64_t* __restrict__ slot_off,
    int64_t* __restrict__ cand_off, int32_t* __restrict__ pair_order) {
  __shared__ int64_t s_w[2 * PLAN_NW];
  const int64_t p0 = (int64_t)blockIdx.x * PLAN_SPAN + (int64_t)threadIdx.x * PLAN_ITEMS;
  int64_t c[PLAN_ITEMS], len[PLAN_ITEMS], rows = 0, inv = 0;
#pragma unroll
  for (int i = 0; i < PLAN_ITEMS; ++i) {
    const int64_t p = p0 + i;
    c[i] = p < n_pairs ? pair_list(probe, p, nlist) : -1;
    len[i] = c[i] >= 0 ? list_off[c[i] + 1] - list_off[c[i]] : 0;
    rows += len[i];
    inv += p < n_pairs && c[i] < 0;
  }
  int64_t slot, bad, ta, tb;
  block_scan2(rows, inv, s_w, slot, bad, ta, tb);
  if (gridDim.x > 1) {
    slot += blk_rows[blockIdx.x];
    bad += blk_inv[blockIdx.x];
  }
  const int64_t n_valid = seg_off[nlist];
#pragma unroll
  for (int i = 0; i < PLAN_ITEMS; ++i) {
    const int64_t p = p0 + i;
    if (p > n_pairs) break;
    slot_off[p] = slot;  // element n_pairs: the total
    const uint32_t q = (uint32_t)p / (uint32_t)nprobe;
    if (q * (uint32_t)nprobe == (uint32_t)p) cand_off[q] = slot;
    if (p == n_pairs) break;
    int64_t dst;
    if (c[i] >= 0) {
      const int64_t at = c[i] * W + (q >> 5);
      dst = seg_off[c[i]] + wpre[at] + __popc(bits[at] & ((1u << (q & 31)) - 1u));
    } else {
      dst = n_valid + bad++;
    }
    if (dst >= 0 && dst < n_pairs) pair_order[dst] = (int32_t)p;
    slot += len[i];
  }
}

static inline int64_t plan_words(int64_t Q) { return (Q + 31) / 32; }
static inline int64_t plan_blocks(int64_t elements) {
  return (elements + PLAN_SPAN - 1) / PLAN_SPAN;
}

// the plan's scratch inside a workspace
struct PlanScratch {
  size_t bits, wpre, blk_rows, blk_inv, blk_cnt, blk_chk, bytes;
};
static PlanScratch plan_scratch(int64_t Q, int64_t nprobe, int64_t nlist) {
  Q = Q > 0 ? Q : 0;
  nprobe = nprobe > 0 ? nprobe : 0;
  nlist = nlist > 0 ? nlist : 0;
  const size_t words = align256((size_t)nlist * (size_t)plan_words(Q) * 4);
  const size_t bp = align256((size_t)plan_blocks(Q * nprobe + 1) * 8);
  const size_t bl = align256((size_t)plan_blocks(nlist + 1) * 8);
  PlanScratch s;
  s.bits = 0;
  s.wpre = s.bits + words;
  s.blk_rows = s.wpre + words;
  s.blk_inv = s.blk_rows + bp;
  s.blk_cnt = s.blk_inv + bp;
  s.blk_chk = s.blk_cnt + bl;
  s.bytes = s.blk_chk + bl;
  return s;
}

// The plan's launches on st: validated sizes, Q >= 1, scratch of plan_scratch(...).bytes.
static int plan_launch(const void* probe, bool probe_i64, const int64_t* list_off, int64_t Q,
                       int64_t nprobe, int64_t nlist, char* scratch, int64_t* slot_off,
                       int64_t* cand_off, int32_t* pair_order, int64_t* seg_off,
                       int64_t* chunk_off, int32_t* out_probe, hipStream_t st) {
  const PlanScratch s = plan_scratch(Q, nprobe, nlist);
  const int64_t n_pairs = Q * nprobe;
  const int W = (int)plan_words(Q);
  const unsigned bp = (unsigned)plan_blocks(n_pairs + 1), bl = (unsigned)plan_blocks(nlist + 1);
  uint32_t* bits = reinterpret_cast<uint32_t*>(scratch + s.bits);
  uint32_t* wpre = reinterpret_cast<uint32_t*>(scratch + s.wpre);
  int64_t* blk_rows = reinterpret_cast<int64_t*>(scratch + s.blk_rows);
  int64_t* blk_inv = reinterpret_cast<int64_t*>(scratch + s.blk_inv);
  int64_t* blk_cnt = reinterpret_cast<int64_t*>(scratch + s.blk_cnt);
  int64_t* blk_chk = reinterpret_cast<int64_t*>(scratch + s.blk_chk);
  prof_begin(st);
  if (hipMemsetAsync(bits, 0, (size_t)nlist * W * 4, st) != hipSuccess)
    return check_launch("ivf_plan(clear)");
  if (probe_i64)
    hipLaunchKernelGGL((ivf_plan_mark_kernel<int64_t>), dim3(bp), dim3(PLAN_NT), 0, st,
                       static_cast<const int64_t*>(probe), list_off, (int)nlist, (int)nprobe, W,
                       n_pairs, bits, blk_rows, blk_inv, out_probe);
  else
    hipLaunchKernelGGL((ivf_plan_mark_kernel<int32_t>), dim3(bp), dim3(PLAN_NT), 0, st,
                       static_cast<const int32_t*>(probe), list_off, (int)nlist, (int)nprobe, W,
                       n_pairs, bits, blk_rows, blk_inv, out_probe);
  int g = 1;  // lanes per bitmap row: the words' next power of two, at most a wave
  while (g < W && g < 64) g <<= 1;
  hipLaunchKernelGGL(ivf_plan_rows_kernel,
                     dim3((unsigned)((nlist * g + ROWS_NT - 1) / ROWS_NT)), dim3(ROWS_NT), 0, st,
                     bits, (int)nlist, W, g, wpre);
  hipLaunchKernelGGL(ivf_plan_count_kernel, dim3(bl), dim3(PLAN_NT), 0, st, bits, (int)nlist, W,
                     wpre, blk_cnt, blk_chk, seg_off, chunk_off);
  if (bp > 1 || bl > 1)
    hipLaunchKernelGGL(ivf_plan_bases_kernel, dim3(2), dim3(PLAN_NT), 0, st, blk_rows, blk_inv,
                       (int64_t)bp, blk_cnt, blk_chk, (int64_t)(bl > 1 ? bl : 0));
  if (bl > 1)
    hipLaunchKernelGGL(ivf_plan_lists_kernel, dim3(bl), dim3(PLAN_NT), 0, st, bits, wpre,
                       (int)nlist, W, blk_cnt, blk_chk, seg_off, chunk_off);
  if (probe_i64)
    hipLaunchKernelGGL((ivf_plan_pairs_kernel<int64_t>), dim3(bp), dim3(PLAN_NT), 0, st,
                       static_cast<const int64_t*>(probe), list_off, (int)nlist, (int)nprobe, W,
                       n_pairs, bits, wpre, blk_rows, blk_inv, seg_off, slot_off, cand_off,
                       pair_order);
  else
    hipLaunchKernelGGL((ivf_plan_pairs_kernel<int32_t>), dim3(bp), dim3(PLAN_NT), 0, st,
                       static_cast<const int32_t*>(probe), list_off, (int)nlist, (int)nprobe, W,
                       n_pairs, bits, wpre, blk_rows, blk_inv, seg_off, slot_off, cand_off,
                       pair_order);
  prof_end("ivf_plan", st);
  return check_launch("ivf_plan kernels");
}

// The tail every entry ends in: the scoring pass over a plan and the select.  n_keys is the
// key region's size: the plan's own total (irc_ivf_topk) or a host bound on it
// (irc_ivf_search).  eb = 2: bf16 operands; eb = 1: e4m3 bytes, the sums times score_scale.
static int score_and_select(const void* queries, const void* docs, const int32_t* row_id,
                            const int64_t* list_off, int64_t nlist, const int64_t* slot_off,
                            const int64_t* cand_off, const int32_t* pair_order,
                            const int64_t* seg_off, const int64_t* chunk_off, int64_t Q,
                            int64_t nprobe, int64_t N, int64_t D, int64_t k, int64_t n_keys,
                            int64_t max_list_rows, uint64_t* keys, float* out_score,
                            int64_t* out_idx, int32_t* out_n, hipStream_t st, int eb = 2,
                            float score_scale = 1.0f) {
  const int64_t n_pairs = Q * nprobe;
  if (n_keys > 0 && max_list_rows > 0) {
    // every list has at most one partly filled chunk
    const int64_t gx = n_pairs / IVF_CHUNK + (nlist < n_pairs ? nlist : n_pairs);
    const int64_t gy = (max_list_rows + IVF_TILE_ROWS - 1) / IVF_TILE_ROWS;
    const unsigned char* qp = static_cast<const unsigned char*>(queries);
    const unsigned char* dp = static_cast<const unsigned char*>(docs);
    prof_begin(st);
#define IRC_IVF_LAUNCH(DD, EB)                                                                   \
  hipLaunchKernelGGL((ivf_score_kernel<DD, EB>), dim3((unsigned)gx, (unsigned)gy), dim3(IVF_NT), \
                     (Lds<DD, EB>::BYTES), st, qp, dp, row_id, list_off, (int)nlist, slot_off,   \
                     pair_order, seg_off, chunk_off, (int)nprobe, n_pairs, N, n_keys, keys,      \
                     score_scale)
#define IRC_IVF_CASE(DD)                   \
  case DD:                                 \
    if (eb == 2) IRC_IVF_LAUNCH(DD, 2);    \
    else IRC_IVF_LAUNCH(DD, 1);            \
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
#undef IRC_IVF_LAUNCH
    // The rows streamed are the sum over lists of chunks x rows, which only the device knows;
    // the host's figure is its upper bound, every pair streaming its list alone -- and from
    // irc_ivf_search a bound of that bound, n_keys being Q x the nprobe longest lists.
    // tools/ivf_probe.py reports the exact count from the plan.
    prof_end(eb == 2 ? "ivf_score" : "ivf_score_fp8", st, (double)n_keys * D * (double)eb);
    if (int rc = check_launch("ivf_score_kernel")) return rc;
  }
  return rerank::select_topk(keys, cand_off, n_keys, Q, (int)k, out_score, out_idx, out_n, st);
}

// the sizes both search entries check, in irc_ivf_topk's order
#define IRC_IVF_CHECK_SIZES(name, rows)                                                          \
  IRC_REQUIRE(Q >= 0 && N >= 0 && nlist >= 0 && (rows) >= 0 && max_list_rows >= 0,               \
              "%s: negative size", name);                                                        \
  IRC_REQUIRE(k >= 1 && k <= rerank::RR_MAXK, "%s: k=%lld outside [1, %d]", name, (long long)k,  \
              rerank::RR_MAXK);                                                                  \
  IRC_REQUIRE(supported_d(D), "%s: unsupported D=%lld", name, (long long)D);                     \
  IRC_REQUIRE(nprobe >= 1 && nprobe <= nlist, "%s: nprobe=%lld outside [1, nlist=%lld]", name,   \
              (long long)nprobe, (long long)nlist)

// pairs are int32 in pair_order, and the grid: x over the chunk bound, y over the segments
#define IRC_IVF_CHECK_RANGES(name)                                                               \
  IRC_REQUIRE(N < (1ll << 31), "%s: global doc ids must fit int32 (N < 2^31)", name);            \
  IRC_REQUIRE(Q < (1ll << 31) - 1 && nlist < (1ll << 31) - 1 && Q * nprobe < (1ll << 30),        \
              "%s: Q x nprobe too large", name);                                                 \
  IRC_REQUIRE(max_list_rows <= N && max_list_rows <= 65535ll * IVF_TILE_ROWS,                    \
              "%s: max_list_rows=%lld above N or %lld", name, (long long)max_list_rows,          \
              65535ll * IVF_TILE_ROWS)

// the e4m3 entries' scales, checked directly after nprobe
#define IRC_IVF_CHECK_SCORE_SCALE(name) \
  IRC_REQUIRE(pow2_scale(score_scale), "%s: score_scale must be a power of two", name)
#define IRC_IVF_CHECK_QUERY_SCALE(name)                                                       \
  IRC_REQUIRE(query_scale > 0.f && std::isfinite(query_scale),                                \
              "%s: query_scale=%g must be finite and positive", name, (double)query_scale)

constexpr int IVF_PROBE_MAX = 1024;  // the scan's largest k: the lists a call can probe itself

// irc_ivf_search's workspace: the keys, the plan, its scratch, the probe's outputs and scan.
struct SearchWs {
  size_t keys, slot_off, cand_off, pair_order, seg_off, chunk_off, scratch, probe_idx,
      probe_score, scan, scan_bytes, codes, bytes;
};
constexpr int64_t IVF_MAX_D = 1024;  // the widest row: the query codes' region does not know D
static SearchWs search_ws(int64_t Q, int64_t nprobe, int64_t nlist, int64_t key_rows, int64_t k,
                          bool fp8 = false) {
  (void)k;
  Q = Q > 0 ? Q : 0;
  nprobe = nprobe > 0 ? nprobe : 0;
  nlist = nlist > 0 ? nlist : 0;
  const size_t n_pairs = (size_t)Q * (size_t)nprobe;
  SearchWs w;
  w.keys = 0;
  w.slot_off = w.keys + workspace_bytes_for(key_rows);
  w.cand_off = w.slot_off + align256((n_pairs + 1) * 8);
  w.pair_order = w.cand_off + align256((size_t)(Q + 1) * 8);
  w.seg_off = w.pair_order + align256(n_pairs * 4);
  w.chunk_off = w.seg_off + align256((size_t)(nlist + 1) * 8);
  w.scratch = w.chunk_off + align256((size_t)(nlist + 1) * 8);
  w.probe_idx = w.scratch + plan_scratch(Q, nprobe, nlist).bytes;
  w.probe_score = w.probe_idx + align256(n_pairs * 8);
  w.scan = w.probe_score + align256(n_pairs * 4);
  // the search's workspace does not know D: the scan's largest over the widths it accepts
  w.scan_bytes = 0;
  if (nprobe <= IVF_PROBE_MAX)
    for (int64_t d : {64, 128, 256, 384, 512, 768, 1024}) {
      const int64_t b = irc_scan_topk_workspace(Q, nlist, d, nprobe);
      w.scan_bytes = (size_t)b > w.scan_bytes ? (size_t)b : w.scan_bytes;
    }
  // irc_ivf_search_fp8 only: the queries' e4m3 codes
  w.codes = w.scan + align256(w.scan_bytes);
  w.bytes = w.codes + (fp8 ? align256((size_t)Q * (size_t)IVF_MAX_D) : 0);
  return w;
}

}  // namespace ivf
}  // namespace irc

using namespace irc;
using namespace irc::ivf;

extern "C" int irc_ivf_tile_rows(void) { return IVF_TILE_ROWS; }

extern "C" int irc_ivf_plan_span(void) { return PLAN_SPAN; }

extern "C" int64_t irc_ivf_plan_workspace(int64_t Q, int64_t nprobe, int64_t nlist) {
  return (int64_t)plan_scratch(Q, nprobe, nlist).bytes + 256;
}

// The order of the checks is part of the interface (tests/test_ivf_native_cpu.py).
extern "C" int irc_ivf_plan(const void* probe, int probe_is_i64, const int64_t* list_off,
                            int64_t Q, int64_t nprobe, int64_t nlist, void* workspace,
                            int64_t workspace_bytes, int64_t* slot_off, int64_t* cand_off,
                            int32_t* pair_order, int64_t* seg_off, int64_t* chunk_off,
                            irc_stream_t stream) {
  const char* name = "ivf_plan";
  IRC_REQUIRE(Q >= 0 && nlist >= 0, "%s: negative size", name);
  IRC_REQUIRE(nprobe >= 1 && nprobe <= nlist, "%s: nprobe=%lld outside [1, nlist=%lld]", name,
              (long long)nprobe, (long long)nlist);
  IRC_REQUIRE(Q < (1ll << 31) - 1 && nlist < (1ll << 31) - 1 && Q * nprobe < (1ll << 30),
              "%s: Q x nprobe too large", name);
  const int64_t need = irc_ivf_plan_workspace(Q, nprobe, nlist);
  if (workspace == nullptr || workspace_bytes < need) {
    set_error("%s: workspace %lld < required %lld bytes", name, (long long)workspace_bytes,
              (long long)need);
    return IRC_E_WORKSPACE;
  }
  if (Q == 0) return IRC_OK;
  IRC_REQUIRE(probe && list_off && slot_off && cand_off && pair_order && seg_off && chunk_off,
              "%s: null pointer", name);
  return plan_launch(probe, probe_is_i64 != 0, list_off, Q, nprobe, nlist,
                     static_cast<char*>(workspace), slot_off, cand_off, pair_order, seg_off,
                     chunk_off, nullptr, as_stream(stream));
}

extern "C" int64_t irc_ivf_topk_workspace(int64_t Q, int64_t nprobe, int64_t total_rows,
                                          int64_t k) {
  (void)Q;
  (void)nprobe;
  (void)k;
  return (int64_t)workspace_bytes_for(total_rows);
}

// irc_ivf_topk (eb = 2) and irc_ivf_topk_fp8 (eb = 1) in one validated path.  The order of the
// checks is part of the interface (tests/test_ivf_cpu.py, tests/test_ivf_fp8_cpu.py): a call
// that breaks two reports the earlier one; the e4m3 form's scale comes directly after nprobe.
static int topk_impl(const char* name, int eb, float score_scale, const void* queries,
                     const void* docs, const int32_t* row_id, const int64_t* list_off,
                     int64_t nlist, const int32_t* probe, const int64_t* slot_off,
                     const int64_t* cand_off, const int32_t* pair_order, const int64_t* seg_off,
                     const int64_t* chunk_off, int64_t Q, int64_t nprobe, int64_t N, int64_t D,
                     int64_t k, int64_t total_rows, int64_t max_list_rows, void* workspace,
                     int64_t workspace_bytes, float* out_score, int64_t* out_idx, int32_t* out_n,
                     irc_stream_t stream) {
  IRC_IVF_CHECK_SIZES(name, total_rows);
  if (eb == 1) IRC_IVF_CHECK_SCORE_SCALE(name);
  IRC_IVF_CHECK_RANGES(name);
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
  return score_and_select(queries, docs, row_id, list_off, nlist, slot_off, cand_off, pair_order,
                          seg_off, chunk_off, Q, nprobe, N, D, k, total_rows, max_list_rows,
                          static_cast<uint64_t*>(workspace), out_score, out_idx, out_n,
                          as_stream(stream), eb, score_scale);
}

extern "C" int irc_ivf_topk(const void* queries, const void* docs, const int32_t* row_id,
                            const int64_t* list_off, int64_t nlist, const int32_t* probe,
                            const int64_t* slot_off, const int64_t* cand_off,
                            const int32_t* pair_order, const int64_t* seg_off,
                            const int64_t* chunk_off, int64_t Q, int64_t nprobe, int64_t N,
                            int64_t D, int64_t k, int64_t total_rows, int64_t max_list_rows,
                            void* workspace, int64_t workspace_bytes, float* out_score,
                            int64_t* out_idx, int32_t* out_n, irc_stream_t stream) {
  return topk_impl("ivf_topk", 2, 1.0f, queries, docs, row_id, list_off, nlist, probe, slot_off,
                   cand_off, pair_order, seg_off, chunk_off, Q, nprobe, N, D, k, total_rows,
                   max_list_rows, workspace, workspace_bytes, out_score, out_idx, out_n, stream);
}

extern "C" int irc_ivf_topk_fp8(const void* queries, const void* docs, const int32_t* row_id,
                                const int64_t* list_off, int64_t nlist, const int32_t* probe,
                                const int64_t* slot_off, const int64_t* cand_off,
                                const int32_t* pair_order, const int64_t* seg_off,
                                const int64_t* chunk_off, int64_t Q, int64_t nprobe, int64_t N,
                                int64_t D, int64_t k, int64_t total_rows, int64_t max_list_rows,
                                float score_scale, void* workspace, int64_t workspace_bytes,
                                float* out_score, int64_t* out_idx, int32_t* out_n,
                                irc_stream_t stream) {
  return topk_impl("ivf_topk_fp8", 1, score_scale, queries, docs, row_id, list_off, nlist, probe,
                   slot_off, cand_off, pair_order, seg_off, chunk_off, Q, nprobe, N, D, k,
                   total_rows, max_list_rows, workspace, workspace_bytes, out_score, out_idx,
                   out_n, stream);
}

extern "C" int64_t irc_ivf_search_workspace(int64_t Q, int64_t nprobe, int64_t nlist,
                                            int64_t key_rows, int64_t k) {
  return (int64_t)search_ws(Q, nprobe, nlist, key_rows, k).bytes;
}

extern "C" int64_t irc_ivf_search_fp8_workspace(int64_t Q, int64_t nprobe, int64_t nlist,
                                                int64_t key_rows, int64_t k) {
  return (int64_t)search_ws(Q, nprobe, nlist, key_rows, k, true).bytes;
}

// irc_ivf_search (eb = 2) and irc_ivf_search_fp8 (eb = 1) in one validated path.  The order of
// the checks is part of the interface (tests/test_ivf_native_cpu.py, tests/test_ivf_fp8_cpu.py):
// irc_ivf_topk's, with the probe's own limit after nprobe's, then the e4m3 form's two scales,
// and the centroids among the pointers.
static int search_impl(const char* name, int eb, float query_scale, float score_scale,
                       const void* queries, const void* docs, const int32_t* row_id,
                       const int64_t* list_off, int64_t nlist, const void* centroids,
                       const int32_t* probe, int64_t Q, int64_t nprobe, int64_t N, int64_t D,
                       int64_t k, int64_t key_rows, int64_t max_list_rows, void* workspace,
                       int64_t workspace_bytes, float* out_score, int64_t* out_idx,
                       int32_t* out_n, int32_t* out_probe, irc_stream_t stream) {
  IRC_IVF_CHECK_SIZES(name, key_rows);
  IRC_REQUIRE(probe != nullptr || nprobe <= IVF_PROBE_MAX,
              "%s: nprobe=%lld above %d, the most lists a call probes itself", name,
              (long long)nprobe, IVF_PROBE_MAX);
  if (eb == 1) {
    IRC_IVF_CHECK_SCORE_SCALE(name);
    IRC_IVF_CHECK_QUERY_SCALE(name);
  }
  IRC_IVF_CHECK_RANGES(name);
  const SearchWs w = search_ws(Q, nprobe, nlist, key_rows, k, eb == 1);
  if (workspace == nullptr || workspace_bytes < (int64_t)w.bytes) {
    set_error("%s: workspace %lld < required %lld bytes", name, (long long)workspace_bytes,
              (long long)w.bytes);
    return IRC_E_WORKSPACE;
  }
  if (Q == 0) return IRC_OK;
  IRC_REQUIRE(queries && row_id && list_off && (probe || centroids) && out_score && out_idx &&
                  out_n && (N == 0 || docs),
              "%s: null pointer", name);
  IRC_REQUIRE(((uintptr_t)queries % 16) == 0 && ((uintptr_t)docs % 16) == 0 &&
                  (probe != nullptr || ((uintptr_t)centroids % 16) == 0),
              "%s: queries, docs and centroids must be 16-byte aligned", name);
  hipStream_t st = as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  int64_t* slot_off = reinterpret_cast<int64_t*>(ws + w.slot_off);
  int64_t* cand_off = reinterpret_cast<int64_t*>(ws + w.cand_off);
  int32_t* pair_order = reinterpret_cast<int32_t*>(ws + w.pair_order);
  int64_t* seg_off = reinterpret_cast<int64_t*>(ws + w.seg_off);
  int64_t* chunk_off = reinterpret_cast<int64_t*>(ws + w.chunk_off);
  const void* pr = probe;
  if (probe == nullptr) {
    // IVFDenseIndex.probe's call: inner product desc, ties to the lower list id; the plan reads
    // the int64 ids where the scan leaves them
    int64_t* ids = reinterpret_cast<int64_t*>(ws + w.probe_idx);
    if (int rc = irc_scan_topk(queries, centroids, Q, nlist, D, nprobe, 0, ws + w.scan,
                               (int64_t)w.scan_bytes,
                               reinterpret_cast<float*>(ws + w.probe_score), ids, stream))
      return rc;
    pr = ids;
  }
  const void* scored = queries;
  if (eb == 1) {
    // the probe ranked the bf16 queries; the lists are scored against their e4m3 codes
    if (int rc = irc_quantize_fp8(0, queries, Q * D, query_scale, ws + w.codes, stream)) return rc;
    scored = ws + w.codes;
  }
  if (int rc = plan_launch(pr, probe == nullptr, list_off, Q, nprobe, nlist, ws + w.scratch,
                           slot_off, cand_off, pair_order, seg_off, chunk_off, out_probe, st))
    return rc;
  return score_and_select(scored, docs, row_id, list_off, nlist, slot_off, cand_off, pair_order,
                          seg_off, chunk_off, Q, nprobe, N, D, k, key_rows, max_list_rows,
                          reinterpret_cast<uint64_t*>(ws + w.keys), out_score, out_idx, out_n, st,
                          eb, score_scale);
}

extern "C" int irc_ivf_search(const void* queries, const void* docs, const int32_t* row_id,
                              const int64_t* list_off, int64_t nlist, const void* centroids,
                              const int32_t* probe, int64_t Q, int64_t nprobe, int64_t N,
                              int64_t D, int64_t k, int64_t key_rows, int64_t max_list_rows,
                              void* workspace, int64_t workspace_bytes, float* out_score,
                              int64_t* out_idx, int32_t* out_n, int32_t* out_probe,
                              irc_stream_t stream) {
  return search_impl("ivf_search", 2, 1.0f, 1.0f, queries, docs, row_id, list_off, nlist,
                     centroids, probe, Q, nprobe, N, D, k, key_rows, max_list_rows, workspace,
                     workspace_bytes, out_score, out_idx, out_n, out_probe, stream);
}

extern "C" int irc_ivf_search_fp8(const void* queries, const void* docs, const int32_t* row_id,
                                  const int64_t* list_off, int64_t nlist, const void* centroids,
                                  const int32_t* probe, int64_t Q, int64_t nprobe, int64_t N,
                                  int64_t D, int64_t k, int64_t key_rows, int64_t max_list_rows,
                                  float query_scale, float score_scale, void* workspace,
                                  int64_t workspace_bytes, float* out_score, int64_t* out_idx,
                                  int32_t* out_n, int32_t* out_probe, irc_stream_t stream) {
  return search_impl("ivf_search_fp8", 1, query_scale, score_scale, queries, docs, row_id,
                     list_off, nlist, centroids, probe, Q, nprobe, N, D, k, key_rows,
                     max_list_rows, workspace, workspace_bytes, out_score, out_idx, out_n,
                     out_probe, stream);
}
