// row_prims.h — the device pieces that the row kernels (k_take.hip, k_put.hip, k_where.hip, k_aggregate.hip) and k_getitem_gather
// (k_decode.hip) share, each defined once: the owner of a tile, the chunk of a row, one row moved by a group of lanes, a tile copied by a
// wave, a row's field, its predicate and a list of them.  A rule is stated here, at its helper; tests/test_wave_emu_row_prims.py and
// tests/test_wave_emu_clauses.py run them one by one.
#pragma once
#include "dev_types.h"
#include "mem_prims.h"

namespace bamd {

// ---- tiles: work cut into pieces that never straddle an owner (a range, a copy, a chunk); tile_first[i] tiles lie in front of owner i ----
// the owner of tile t, t < tile_first[n]: the last i with tile_first[i] <= t - of equal entries (owners without tiles) the last one
__device__ __forceinline__ uint32_t tile_owner(const uint32_t* __restrict__ tile_first, int n, uint32_t t) {
  uint32_t i = 0, hi = (uint32_t)n;
  while (hi - i > 1u) {
    const uint32_t mid = (i + hi) >> 1;
    if (tile_first[mid] <= t) i = mid; else hi = mid;
  }
  return i;
}

// where's and aggregate's tiles: WH_TILE rows of one chunk
constexpr int WH_THREADS = 256;
constexpr int WH_WAVES = WH_THREADS / 64;
constexpr int WH_STEPS = 4;                                  // steps of WH_THREADS rows per tile
constexpr uint32_t WH_TILE = WH_THREADS * WH_STEPS;          // rows of a tile
constexpr int WH_WORDS = WH_WAVES * WH_STEPS;                // mask words of a tile: word s * WH_WAVES + w holds rows [64 (s * WH_WAVES + w), + 64)
constexpr int WH_WAVES_PER_CU = 32;                          // the grid: a choice, not a residency

// ---- an index table over the rows of a call's chunks (dev_types.h: TakeChunk): take and put ----
constexpr int TK_THREADS = 256;
constexpr int TK_WAVES_PER_CU = 16;         // the grid, as k_getitem_gather's: a choice, not a residency
constexpr int TK_LDS_CHUNKS = 1024;

// The workgroup keeps row_first in LDS where the call has at most TK_LDS_CHUNKS chunks (8 KiB, four workgroups of four waves per CU); above
// that the bisection reads the table in global memory, which stays in L2.  (A macro: it declares the kernel's __shared__ array.)
#define TK_ROW_FIRST_IN_LDS(first, in_lds)                                                                               \
  __shared__ int64_t first[TK_LDS_CHUNKS];                                                                               \
  const bool in_lds = nchunks <= TK_LDS_CHUNKS;                                                                          \
  if (in_lds) {                                                                                                          \
    for (int i = (int)threadIdx.x; i < nchunks; i += TK_THREADS) first[i] = chunks[i].row_first;                         \
    __syncthreads();                                                                                                     \
  }

// the chunk of row r, 0 <= r < the call's rows: the last c with row_first <= r (chunks without rows share their successor's row_first)
__device__ __forceinline__ uint32_t take_chunk_of(const int64_t* first_lds, const TakeChunk* __restrict__ chunks, int nchunks, bool in_lds, int64_t r) {
  uint32_t c = 0, hi = (uint32_t)nchunks;
  while (hi - c > 1u) {
    const uint32_t mid = (c + hi) >> 1;
    const int64_t f = in_lds ? first_lds[mid] : chunks[mid].row_first;
    if (f <= r) c = mid; else hi = mid;
  }
  return c;
}

// The index prologue of all four kernels: r = index[k] names no row of any chunk (nrows = chunks[nchunks].row_first), or row r of the call
// in chunk take_chunk_of(r).  A predicate in front of the bisection, not one function that returns both: the caller leaves before the
// bisection's loop, and the compiler does not move that exit across the loop by itself (one more exec region per kernel when tried).
__device__ __forceinline__ bool take_no_row(int64_t r, int64_t nrows) { return r < 0 || r >= nrows; }
// index k fails with `code`: called by the first lane of its group, which counts it.  An index that names no row of any chunk is answered
// once, by the pass that has first_pass set.
__device__ __forceinline__ void take_fail(int32_t* __restrict__ status /*may be nullptr*/, size_t k, int32_t code, uint32_t& nfail) {
  if (status) status[k] = code;
  nfail++;
}

// One row of row_bytes bytes from s to d by a group of G = 2^lanes_log2 consecutive lanes, of which this one is number sub.  The host picks G
// from row_bytes and the alignment of d (engine.hip: row_lanes_log2), the same for every row of a call:
//   row_bytes <= 16: G = 1; one load and one store of the natural width where row_bytes is 2 / 4 / 8 / 16 and BOTH addresses are aligned for
//                    it, byte moves otherwise;
//   larger rows:     bytes up to the first 16-byte boundary of d, aligned 16-byte stores fed by unaligned dwordx4 loads (mem_prims.h), bytes
//                    behind them.  The boundary is always the STORE's: dest + k * row_bytes in take, the row's place in its slot in put.
__device__ __forceinline__ void move_row(gu8* d, const gu8* s, uint32_t row_bytes, uint32_t sub, uint32_t G) {
  if (row_bytes <= 16u) {
    const uint32_t a = (uint32_t)(uintptr_t)s | (uint32_t)(uintptr_t)d;
    if (row_bytes == 16u && !(a & 15u)) g_st16(d, g_ld16(s));
    else if (row_bytes == 8u && !(a & 7u)) g_st8(d, g_ld8(s));
    else if (row_bytes == 4u && !(a & 3u)) g_st4(d, g_ld4(s));
    else if (row_bytes == 2u && !(a & 1u)) g_st2(d, g_ld2(s));
    else for (uint32_t i = 0; i < row_bytes; i++) d[i] = s[i];
  } else {
    const uint32_t head = (16u - ((uint32_t)(uintptr_t)d & 15u)) & 15u;      // < row_bytes
    const uint32_t body = (row_bytes - head) & ~15u, tail = row_bytes - head - body;
    for (uint32_t i = sub; i < head; i += G) d[i] = s[i];
    for (uint32_t o = sub * 16u; o < body; o += G * 16u) g_st16(d + head + o, g_ld16(s + head + o));
    for (uint32_t i = sub; i < tail; i += G) d[head + body + i] = s[head + body + i];
  }
}

// One wave writes the n bytes of a tile at d (k_getitem_gather, k_put_assemble: n <= 16 KiB, 16 steps of 64 lanes x 16 bytes): bytes up to the
// first 16-byte boundary of the DESTINATION, aligned 16-byte stores over the middle, bytes behind it.  The loads are aligned as well where s
// and d are mutually aligned, and unaligned dwordx4 loads otherwise (mem_prims.h).  ZEROS: only the first `live` bytes come from s, zeros
// follow, and nothing beyond s + live is read; without it `live` is not looked at and all n bytes are copied.
constexpr uint32_t TILE_COPY_LANES = 64;
template <bool ZEROS>
__device__ __forceinline__ void wave_copy_tile(gu8* d, const gu8* s, uint32_t n, uint32_t live, uint32_t lane) {
  uint32_t head = (uint32_t)((16u - ((uint32_t)(uintptr_t)d & 15u)) & 15u);
  if (head > n) head = n;
  const uint32_t body = (n - head) & ~15u, tail = n - head - body;
  if (!ZEROS) {
    if (lane < head) d[lane] = s[lane];
    for (uint32_t k = lane * 16u; k < body; k += TILE_COPY_LANES * 16u) g_st16(d + head + k, g_ld16(s + head + k));
    if (lane < tail) d[head + body + lane] = s[head + body + lane];
    return;
  }
  if (lane < head) d[lane] = lane < live ? s[lane] : (uint8_t)0;
  for (uint32_t k = lane * 16u; k < body; k += TILE_COPY_LANES * 16u) {
    const uint32_t at = head + k;
    if (at + 16u <= live) g_st16(d + at, g_ld16(s + at));
    else if (at >= live) g_st16(d + at, make_uint4(0u, 0u, 0u, 0u));
    else for (uint32_t i = 0; i < 16u; i++) d[at + i] = at + i < live ? s[at + i] : (uint8_t)0;      // the last live bytes and the first zeros
  }
  if (lane < tail) { const uint32_t at = head + body + lane; d[at] = at < live ? s[at] : (uint8_t)0; }
}

// ---- a field of a row and a predicate on it (dev_types.h: WherePred, where_key): where and aggregate ----
// the field at p, whatever its address (mem_prims.h: unaligned loads)
__device__ __forceinline__ uint64_t where_field(const gu8* p, uint32_t bytes) {
  if (bytes == 1u) return (uint64_t)p[0];
  if (bytes == 2u) return (uint64_t)g_ld2(p);
  if (bytes == 4u) return (uint64_t)g_ld4(p);
  return g_ld8(p);
}

__device__ __forceinline__ bool where_test(const WherePred& q, uint64_t v) {
  bool nan;
  const int64_t k = where_key(v, q.kind, q.bytes, q.inf, &nan);
  if (nan || q.nan) return q.op == 1;
  switch (q.op) {
    case 0: return k == q.key;
    case 1: return k != q.key;
    case 2: return k < q.key;
    case 3: return k <= q.key;
    case 4: return k > q.key;
    default: return k >= q.key;
  }
}

// A term list on the row at `row` (dev_types.h: WhereTerms; include/blosc_gpu_clauses.h): true when every clause of the list has a true
// term.  The row's distinct fields go to v[0] ... v[nfields - 1], every one loaded once and all of them before the first comparison - the
// loads are independent, so a row that spans several sectors waits for them together.  q is read at indices that are the same in every
// lane: the fields at constant indices under the uniform bound nfields, the terms of a field under its uniform range.  No lane leaves early.
__device__ __forceinline__ bool where_terms_test(const WhereTerms* __restrict__ q, const gu8* row, uint64_t (&v)[WH_MAX_FIELDS]) {
  const uint32_t nfields = q->nfields;
  uint32_t lo[WH_MAX_FIELDS], hi[WH_MAX_FIELDS];      // where_field's loads, each into the register it stays in: nothing here waits for one of them
#pragma unroll
  for (int f = 0; f < WH_MAX_FIELDS; f++)
    if ((uint32_t)f < nfields) {
      const gu8* p = row + q->offset[f];
      const uint32_t b = q->bytes[f];
      hi[f] = 0u;
      if (b == 8u) { lo[f] = g_ld4(p); hi[f] = g_ld4(p + 4); }
      else if (b == 4u) lo[f] = g_ld4(p);
      else if (b == 2u) lo[f] = g_ld2(p);
      else lo[f] = (uint32_t)p[0];
    }
  uint32_t met = 0;      // the clauses that have a true term
#pragma unroll
  for (int f = 0; f < WH_MAX_FIELDS; f++)
    if ((uint32_t)f < nfields) {
      v[f] = (uint64_t)hi[f] << 32 | lo[f];
      for (uint32_t t = q->first[f], t1 = q->first[f + 1]; t < t1; t++) {
        const WherePred p = q->test[t];
        met |= where_test(p, v[f]) ? q->bit[t] : 0u;
      }
    }
  return met == q->clauses;
}

}  // namespace bamd
