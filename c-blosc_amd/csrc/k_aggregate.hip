// k_aggregate.hip — count, sum, min and max of a row field of compressed chunks (include/blosc_gpu_aggregate.h; engine.hip: engine_aggregate).
//
// The pass is where's (k_where.hip): the chunks decoded whole into plaintext slots (dev_types.h: WhereChunk), tiles of WH_TILE rows that never
// straddle a chunk, tile_first and tile_owner (row_prims.h).  Two kernels per pass, and no workgroup ever waits for another one:
//   k_aggregate_tiles    one lane per row: the filter's field against its constant (where_test) and the aggregated field's key (where_key);
//                        every lane accumulates its WH_STEPS rows in step order, the wave folds its lanes by a butterfly of __shfl_xor, the
//                        workgroup its waves through LDS in wave order: one AggPartial per tile;
//   k_aggregate_chunks   a workgroup per chunk: lane i folds tiles i, i + WH_THREADS, ... of the chunk in ascending order, then the same
//                        butterfly and the same wave order; the rows in chunk become the call's row numbers, the bytes of the two extremes are
//                        read from the slot, and the chunk's AggResult goes to the call's table.
// The order of the additions is fixed by the chunk's number of rows alone - tiles are numbered inside their chunk, the tree over a tile and the
// tree over the tiles are the same whatever the pass, the grid and the chunks around it - so the binary64 sum of a chunk is the same in every
// call; there is no atomic.  The extremes are (key, row) pairs in a total order: the lower row wins among equal keys in any order of folding.
// Bytes per row: the field (and the filter's, where it is another one); 40 bytes per tile and 64 per chunk are written.
#pragma once
#include "dev_types.h"
#include "mem_prims.h"
#include "row_prims.h"
#include "wave_prims.h"

namespace bamd {

// what the kernels fold: a tile's rows, a chunk's tiles
struct AggAcc {
  int64_t min_key, max_key;
  uint64_t sum;
  uint32_t min_row, max_row;
  uint32_t count, nans;
};

__device__ __forceinline__ AggAcc agg_none() {
  return AggAcc{INT64_MAX, INT64_MIN, 0ull, AGG_NO_ROW, AGG_NO_ROW, 0u, 0u};
}
__device__ __forceinline__ double agg_f64(uint64_t u) { double d; __builtin_memcpy(&d, &u, 8); return d; }
__device__ __forceinline__ uint64_t agg_u64(double d) { uint64_t u; __builtin_memcpy(&u, &d, 8); return u; }
__device__ __forceinline__ uint64_t agg_add(uint64_t a, uint64_t b, bool fp) { return fp ? agg_u64(agg_f64(a) + agg_f64(b)) : a + b; }

// a value into the extremes: the pairs (key, row) in their lexicographic order, AGG_NO_ROW behind every row
__device__ __forceinline__ void agg_extreme(AggAcc& a, int64_t key, uint32_t row) {
  if (key < a.min_key || (key == a.min_key && row < a.min_row)) { a.min_key = key; a.min_row = row; }
  if (key > a.max_key || (key == a.max_key && row < a.max_row)) { a.max_key = key; a.max_row = row; }
}
// a (in front) and b folded; the sum is a + b in this order
__device__ __forceinline__ AggAcc agg_fold(AggAcc a, const AggAcc& b, bool fp) {
  if (b.min_row != AGG_NO_ROW && (b.min_key < a.min_key || (b.min_key == a.min_key && b.min_row < a.min_row))) { a.min_key = b.min_key; a.min_row = b.min_row; }
  if (b.max_row != AGG_NO_ROW && (b.max_key > a.max_key || (b.max_key == a.max_key && b.max_row < a.max_row))) { a.max_key = b.max_key; a.max_row = b.max_row; }
  a.sum = agg_add(a.sum, b.sum, fp);
  a.count += b.count; a.nans += b.nans;
  return a;
}

__device__ __forceinline__ uint32_t agg_xor32(uint32_t v, int d) { return (uint32_t)__shfl_xor((int)v, d, 64); }
// the wave's lanes folded: lane l takes lane l ^ 32, then ^ 16, ... ^ 1.  Every lane runs the same tree over the same values (the lower
// lane's operand in front), so all 64 hold the result; the caller takes lane 0's.
__device__ __forceinline__ AggAcc agg_wave(AggAcc a, uint32_t lane, bool fp) {
  for (int d = 32; d >= 1; d >>= 1) {
    AggAcc o;
    o.min_key = (int64_t)wave_xor_u64((uint64_t)a.min_key, d); o.max_key = (int64_t)wave_xor_u64((uint64_t)a.max_key, d);
    o.sum = wave_xor_u64(a.sum, d);
    o.min_row = agg_xor32(a.min_row, d); o.max_row = agg_xor32(a.max_row, d);
    o.count = agg_xor32(a.count, d); o.nans = agg_xor32(a.nans, d);
    a = (lane & (uint32_t)d) ? agg_fold(o, a, fp) : agg_fold(a, o, fp);
  }
  return a;
}
// ... and the workgroup's waves, in wave order, by thread 0 (the others get their own wave's back).  Two barriers: `waves` may be written again behind it
__device__ __forceinline__ AggAcc agg_workgroup(AggAcc a, AggAcc* waves, uint32_t tid, bool fp) {
  const uint32_t wave = tid >> 6, lane = tid & 63u;
  a = agg_wave(a, lane, fp);
  if (lane == 0) waves[wave] = a;
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < WH_WAVES; w++) a = agg_fold(a, waves[w], fp);
  __syncthreads();
  return a;
}

// partials [ntiles]: of this pass, every entry written (a tile of a chunk that did not decode: nothing)
__global__ __launch_bounds__(WH_THREADS) void k_aggregate_tiles(const WhereChunk* __restrict__ chunks /*[nchunks]*/, const uint32_t* __restrict__ tile_first /*[nchunks + 1]*/,
                                                               int nchunks, uint32_t row_bytes, AggField f, WherePred q, int filtered,
                                                               AggPartial* __restrict__ partials) {
  __shared__ AggAcc waves[WH_WAVES];
  const uint32_t tid = threadIdx.x;
  const uint32_t ntiles = tile_first[nchunks];
  const bool fp = f.kind == 2;
  const bool one_load = filtered && q.offset == f.offset && q.bytes == f.bytes;      // the filter reads the aggregated bytes
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint32_t c = tile_owner(tile_first, nchunks, t);
    const WhereChunk ch = chunks[c];
    const uint32_t row0 = (t - tile_first[c]) * WH_TILE;
    const gu8* base = as_global(ch.slot);
    AggAcc a = agg_none();
#pragma unroll
    for (int s = 0; s < WH_STEPS; s++) {
      const uint32_t r = row0 + (uint32_t)s * WH_THREADS + tid;
      if (ch.status < 0 || r >= ch.rows) continue;
      const gu8* row = base + (size_t)r * row_bytes;
      const uint64_t v = where_field(row + f.offset, f.bytes);
      if (filtered && !where_test(q, one_load ? v : where_field(row + q.offset, q.bytes))) continue;
      bool nan;
      const int64_t key = where_key(v, f.kind, f.bytes, f.inf, &nan);
      a.count++;
      if (nan) { a.nans++; continue; }
      agg_extreme(a, key, r);
      a.sum = fp ? agg_u64(agg_f64(a.sum) + agg_f64(widen_to_f64(v, f.bytes, f.mant))) : a.sum + (f.kind == 1 ? (uint64_t)key : v);
    }
    a = agg_workgroup(a, waves, tid, fp);
    if (tid == 0) partials[t] = AggPartial{a.min_key, a.max_key, a.sum, a.min_row, a.max_row, a.count, a.nans};
  }
}

// k_aggregate_tiles for a term list (include/blosc_gpu_clauses.h; row_prims.h: where_terms_test): the same tiles, grid, order of additions
// and AggPartial, so k_aggregate_chunks runs behind it as it is.  Field 0 of the list is the aggregated one (dev_types.h: WhereTerms): the
// row's value is what where_terms_test loaded for it, whether a term tests it or not.  No terms: every row.
__global__ __launch_bounds__(WH_THREADS) void k_aggregate_tiles_terms(const WhereChunk* __restrict__ chunks /*[nchunks]*/, const uint32_t* __restrict__ tile_first /*[nchunks + 1]*/,
                                                                     int nchunks, uint32_t row_bytes, AggField f, const WhereTerms* __restrict__ terms,
                                                                     AggPartial* __restrict__ partials) {
  __shared__ AggAcc waves[WH_WAVES];
  const uint32_t tid = threadIdx.x;
  const uint32_t ntiles = tile_first[nchunks];
  const bool fp = f.kind == 2;
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint32_t c = tile_owner(tile_first, nchunks, t);
    const WhereChunk ch = chunks[c];
    const uint32_t row0 = (t - tile_first[c]) * WH_TILE;
    const gu8* base = as_global(ch.slot);
    AggAcc a = agg_none();
#pragma unroll 1
    for (int s = 0; s < WH_STEPS; s++) {
      const uint32_t r = row0 + (uint32_t)s * WH_THREADS + tid;
      if (ch.status < 0 || r >= ch.rows) continue;
      uint64_t v[WH_MAX_FIELDS];
      if (!where_terms_test(terms, base + (size_t)r * row_bytes, v)) continue;
      bool nan;
      const int64_t key = where_key(v[0], f.kind, f.bytes, f.inf, &nan);
      a.count++;
      if (nan) { a.nans++; continue; }
      agg_extreme(a, key, r);
      a.sum = fp ? agg_u64(agg_f64(a.sum) + agg_f64(widen_to_f64(v[0], f.bytes, f.mant))) : a.sum + (f.kind == 1 ? (uint64_t)key : v[0]);
    }
    a = agg_workgroup(a, waves, tid, fp);
    if (tid == 0) partials[t] = AggPartial{a.min_key, a.max_key, a.sum, a.min_row, a.max_row, a.count, a.nans};
  }
}

// results [nchunks]: the entries of the pass's chunks in the call's table, every one written
__global__ __launch_bounds__(WH_THREADS) void k_aggregate_chunks(const WhereChunk* __restrict__ chunks, const uint32_t* __restrict__ tile_first, int nchunks,
                                                                uint32_t row_bytes, AggField f, const AggPartial* __restrict__ partials,
                                                                AggResult* __restrict__ results) {
  __shared__ AggAcc waves[WH_WAVES];
  const uint32_t tid = threadIdx.x;
  const bool fp = f.kind == 2;
  for (uint32_t c = blockIdx.x; c < (uint32_t)nchunks; c += gridDim.x) {
    const WhereChunk ch = chunks[c];
    const uint32_t t1 = tile_first[c + 1];
    AggAcc a = agg_none();      // (a chunk has fewer than 2^32 rows: its counts stay in 32 bits)
    for (uint32_t t = tile_first[c] + tid; t < t1; t += WH_THREADS) {
      const AggPartial p = partials[t];
      a = agg_fold(a, AggAcc{p.min_key, p.max_key, p.sum, p.min_row, p.max_row, p.count, p.nans}, fp);
    }
    a = agg_workgroup(a, waves, tid, fp);
    if (tid == 0) {
      AggResult r{0, 0, 0, -1, -1, 0, 0, 0};
      if (ch.status >= 0) {
        const gu8* at = as_global(ch.slot) + f.offset;
        r.rows = ch.rows; r.count = a.count; r.nans = a.nans; r.sum = a.sum;
        if (a.min_row != AGG_NO_ROW) { r.min_row = ch.row_first + (int64_t)a.min_row; r.min = where_field(at + (size_t)a.min_row * row_bytes, f.bytes); }
        if (a.max_row != AGG_NO_ROW) { r.max_row = ch.row_first + (int64_t)a.max_row; r.max = where_field(at + (size_t)a.max_row * row_bytes, f.bytes); }
      }
      results[c] = r;
    }
  }
}

}  // namespace bamd
