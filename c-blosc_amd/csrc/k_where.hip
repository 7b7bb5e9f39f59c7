// k_where.hip — the rows of compressed chunks whose field satisfies a predicate (include/blosc_gpu_where.h; engine.hip: engine_where).
//
// The chunks of a pass are decoded whole into plaintext slots (dev_types.h: WhereChunk).  A pass is cut into tiles of WH_TILE rows that never
// straddle a chunk; tile_first[c] is the number of tiles in front of chunk c of the pass, and a tile finds its chunk by bisection
// (row_prims.h: tile_owner).  Three kernels per pass, and no workgroup ever waits for another one:
//   k_where_mark    one lane per row: the field's key against the constant's (dev_types.h: WherePred), one __ballot word per 64 rows, the
//                   tile's count, and that count added to its chunk's counter (an integer atomic at L2: the sum does not depend on the order);
//                   k_where_mark_terms is the same for a term list (include/blosc_gpu_clauses.h), with the same outputs;
//   k_where_scan    ONE workgroup: the exclusive prefix of the pass's tile counts, started at the call's running total, which lives in
//                   device memory and is carried to the next pass - the passes order themselves on the stream;
//   k_where_write   one lane per row again: tile base + the counts of the words in front of its own (LDS) + the set bits below its lane
//                   (mbcnt), and where that is below the capacity the row's number goes there - ascending, the same in every run.
// Bytes per row: mark reads the field (one sector of the row where rows are wider than a sector) and writes 1/8 byte of mask; write
// reads that 1/8 byte and writes 8 bytes per match.
#pragma once
#include "dev_types.h"
#include "mem_prims.h"
#include "row_prims.h"      // the WH_* tile constants, tile_owner, where_field, where_test

namespace bamd {

constexpr int WH_SCAN_THREADS = 1024;

// masks [ntiles * WH_WORDS], tile_count [ntiles]: of this pass, every word written.  chunk_count: the counters of the pass's chunks.
__global__ __launch_bounds__(WH_THREADS) void k_where_mark(const WhereChunk* __restrict__ chunks /*[nchunks]*/, const uint32_t* __restrict__ tile_first /*[nchunks + 1]*/,
                                                          int nchunks, uint32_t row_bytes, WherePred q, uint64_t* __restrict__ masks,
                                                          uint32_t* __restrict__ tile_count, uint32_t* __restrict__ chunk_count) {
  __shared__ uint32_t wave_count[WH_WAVES];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const uint32_t ntiles = tile_first[nchunks];
  uint32_t held = 0, held_chunk = 0;      // thread 0: matches of held_chunk not yet added to its counter - one atomic per chunk the workgroup meets, not per tile
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint32_t c = tile_owner(tile_first, nchunks, t);
    const WhereChunk ch = chunks[c];
    const uint32_t row0 = (t - tile_first[c]) * WH_TILE;
    const gu8* base = as_global(ch.slot) + q.offset;
    uint32_t count = 0;      // of this wave's words: the same in all its lanes
#pragma unroll
    for (int s = 0; s < WH_STEPS; s++) {
      const uint32_t r = row0 + (uint32_t)s * WH_THREADS + tid;
      bool hit = false;
      if (ch.status >= 0 && r < ch.rows) hit = where_test(q, where_field(base + (size_t)r * row_bytes, q.bytes));
      const uint64_t m = __ballot(hit);
      if (lane == 0) masks[(size_t)t * WH_WORDS + (uint32_t)s * WH_WAVES + wave] = m;
      count += (uint32_t)__builtin_popcountll(m);
    }
    if (lane == 0) wave_count[wave] = count;
    __syncthreads();
    if (tid == 0) {
      uint32_t total = 0;
      for (int w = 0; w < WH_WAVES; w++) total += wave_count[w];
      tile_count[t] = total;
      if (c != held_chunk) {
        if (held) atomicAdd(&chunk_count[held_chunk], held);
        held = 0; held_chunk = c;
      }
      held += total;
    }
    __syncthreads();      // wave_count is written again by the next tile
  }
  if (tid == 0 && held) atomicAdd(&chunk_count[held_chunk], held);
}

// k_where_mark for a term list (include/blosc_gpu_clauses.h; row_prims.h: where_terms_test): the same tiles, grid and outputs, so
// k_where_scan and k_where_write run behind it as they are.  terms: the list in device memory, read at lane-uniform indices.
__global__ __launch_bounds__(WH_THREADS) void k_where_mark_terms(const WhereChunk* __restrict__ chunks /*[nchunks]*/, const uint32_t* __restrict__ tile_first /*[nchunks + 1]*/,
                                                                int nchunks, uint32_t row_bytes, const WhereTerms* __restrict__ terms,
                                                                uint64_t* __restrict__ masks, uint32_t* __restrict__ tile_count,
                                                                uint32_t* __restrict__ chunk_count) {
  __shared__ uint32_t wave_count[WH_WAVES];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const uint32_t ntiles = tile_first[nchunks];
  uint32_t held = 0, held_chunk = 0;      // thread 0, as in k_where_mark: one atomic per chunk the workgroup meets
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint32_t c = tile_owner(tile_first, nchunks, t);
    const WhereChunk ch = chunks[c];
    const uint32_t row0 = (t - tile_first[c]) * WH_TILE;
    const gu8* base = as_global(ch.slot);
    uint32_t count = 0;      // of this wave's words: the same in all its lanes
#pragma unroll 1
    for (int s = 0; s < WH_STEPS; s++) {
      const uint32_t r = row0 + (uint32_t)s * WH_THREADS + tid;
      bool hit = false;
      if (ch.status >= 0 && r < ch.rows) {
        uint64_t v[WH_MAX_FIELDS];
        hit = where_terms_test(terms, base + (size_t)r * row_bytes, v);
      }
      const uint64_t m = __ballot(hit);
      if (lane == 0) masks[(size_t)t * WH_WORDS + (uint32_t)s * WH_WAVES + wave] = m;
      count += (uint32_t)__builtin_popcountll(m);
    }
    if (lane == 0) wave_count[wave] = count;
    __syncthreads();
    if (tid == 0) {
      uint32_t total = 0;
      for (int w = 0; w < WH_WAVES; w++) total += wave_count[w];
      tile_count[t] = total;
      if (c != held_chunk) {
        if (held) atomicAdd(&chunk_count[held_chunk], held);
        held = 0; held_chunk = c;
      }
      held += total;
    }
    __syncthreads();      // wave_count is written again by the next tile
  }
  if (tid == 0 && held) atomicAdd(&chunk_count[held_chunk], held);
}

// tile_base[t] = *running + the counts of the tiles in front of t; *running += all of them.  One workgroup: thread i owns the `per`
// consecutive tiles from i * per, the workgroup scans the threads' sums (a wave's by __shfl_up, the waves' through LDS).
__global__ __launch_bounds__(WH_SCAN_THREADS) void k_where_scan(const uint32_t* __restrict__ tile_count, uint32_t ntiles, uint64_t* __restrict__ tile_base,
                                                               uint64_t* __restrict__ running) {
  __shared__ uint32_t wave_sum[WH_SCAN_THREADS / 64];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const uint32_t per = (ntiles + WH_SCAN_THREADS - 1u) / WH_SCAN_THREADS;
  const uint32_t t0 = tid * per < ntiles ? tid * per : ntiles, t1 = t0 + per < ntiles ? t0 + per : ntiles;      // (a pass has fewer than 2^31 rows: no sum leaves 32 bits)
  uint32_t mine = 0;
  for (uint32_t t = t0; t < t1; t++) mine += tile_count[t];
  uint32_t incl = mine;      // inclusive scan inside the wave
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
    if ((int)lane >= d) incl += o;
  }
  if (lane == 63u) wave_sum[wave] = incl;
  __syncthreads();
  uint32_t front = 0, all = 0;
  for (uint32_t w = 0; w < WH_SCAN_THREADS / 64; w++) { if (w < wave) front += wave_sum[w]; all += wave_sum[w]; }
  const uint64_t start = *running;
  uint64_t at = start + front + (incl - mine);
  for (uint32_t t = t0; t < t1; t++) { tile_base[t] = at; at += tile_count[t]; }
  __syncthreads();          // every thread has read *running
  if (tid == 0) *running = start + all;
}

// index_out[p] = the call's number of the p-th matching row, for p < capacity
__global__ __launch_bounds__(WH_THREADS) void k_where_write(const WhereChunk* __restrict__ chunks, const uint32_t* __restrict__ tile_first, int nchunks,
                                                           const uint64_t* __restrict__ masks, const uint32_t* __restrict__ tile_count,
                                                           const uint64_t* __restrict__ tile_base, int64_t* __restrict__ index_out, uint64_t capacity) {
  __shared__ uint32_t word_count[WH_WORDS];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const uint32_t ntiles = tile_first[nchunks];
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t tile_at = tile_base[t];
    if (!tile_count[t] || tile_at >= capacity) continue;      // (the same for the whole workgroup: no barrier is left out by some)
    const uint32_t c = tile_owner(tile_first, nchunks, t);
    const int64_t row0 = chunks[c].row_first + (int64_t)(t - tile_first[c]) * WH_TILE;
    if (tid < (uint32_t)WH_WORDS) word_count[tid] = (uint32_t)__builtin_popcountll(masks[(size_t)t * WH_WORDS + tid]);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < WH_STEPS; s++) {
      const uint32_t w = (uint32_t)s * WH_WAVES + wave;
      const uint64_t m = masks[(size_t)t * WH_WORDS + w];
      uint32_t front = 0;
      for (uint32_t i = 0; i < w; i++) front += word_count[i];
      const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      const uint64_t at = tile_at + front + below;
      if (((m >> lane) & 1ull) && at < capacity) index_out[at] = row0 + (int64_t)(w * 64u + lane);
    }
    __syncthreads();      // word_count is written again by the next tile
  }
}

}  // namespace bamd
