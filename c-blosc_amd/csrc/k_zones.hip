// k_zones.hip — the aggregates of SEVERAL row fields of compressed chunks in one decode (include/blosc_gpu_zones.h; engine.hip:
// engine_aggregate_fields).  The pass, the tiles, the grid and the order of every addition are k_aggregate.hip's; AggAcc, agg_fold, agg_wave
// and agg_workgroup are used from there as they are.  Two kernels per pass:
//   k_aggregate_tiles_fields    the term list once per row (row_prims.h: where_terms_test); a lane keeps the verdicts of its WH_STEPS rows as
//                               bits.  Then a loop over the fields that is the same in every lane: the accumulation of k_aggregate_tiles_terms
//                               for ONE field over the rows whose bit is set, agg_workgroup, and AggPartial t * nfields + f.  One accumulator is
//                               live at a time.  The field table lies in device memory and is read at an index every lane shares, so a
//                               field's offset, width and kind are scalars as WhereTerms' are.  A row is read from HBM by the term list (or
//                               by the first field) and from cache by the fields behind it;
//   k_aggregate_chunks_fields   a workgroup per (chunk of the pass, field): k_aggregate_chunks' fold - lane l takes tiles l, l + WH_THREADS,
//                               ... of the chunk - over the partials of that field, into entry chunk * nfields + f of the call's table.
// What field f of a chunk answers is what k_aggregate_tiles_terms and k_aggregate_chunks answer for it alone, bit for bit: the same rows in
// the same lanes and steps, the same butterfly, the same wave order, the same tiles per lane.
#pragma once
#include "k_aggregate.hip"

namespace bamd {

// partials [ntiles * nfields]: of this pass, every entry written (a tile of a chunk that did not decode: nothing)
__global__ __launch_bounds__(WH_THREADS) void k_aggregate_tiles_fields(const WhereChunk* __restrict__ chunks /*[nchunks]*/, const uint32_t* __restrict__ tile_first /*[nchunks + 1]*/,
                                                                      int nchunks, uint32_t row_bytes, const AggField* __restrict__ fields /*[nfields]*/, int nfields,
                                                                      const WhereTerms* __restrict__ terms, AggPartial* __restrict__ partials) {
  __shared__ AggAcc waves[WH_WAVES];
  const uint32_t tid = threadIdx.x;
  const uint32_t ntiles = tile_first[nchunks];
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint32_t c = tile_owner(tile_first, nchunks, t);
    const WhereChunk ch = chunks[c];
    const uint32_t row0 = (t - tile_first[c]) * WH_TILE;
    const gu8* base = as_global(ch.slot);
    uint32_t passes = 0;      // bit s: the lane's row of step s exists and passes the list
#pragma unroll 1
    for (int s = 0; s < WH_STEPS; s++) {
      const uint32_t r = row0 + (uint32_t)s * WH_THREADS + tid;
      if (ch.status < 0 || r >= ch.rows) continue;
      uint64_t v[WH_MAX_FIELDS];
      if (where_terms_test(terms, base + (size_t)r * row_bytes, v)) passes |= 1u << s;
    }
    for (int k = 0; k < nfields; k++) {
      const AggField f = fields[k];
      const bool fp = f.kind == 2;
      AggAcc a = agg_none();
#pragma unroll
      for (int s = 0; s < WH_STEPS; s++) {
        if (!(passes >> s & 1u)) continue;
        const uint32_t r = row0 + (uint32_t)s * WH_THREADS + tid;
        const uint64_t v = where_field(base + (size_t)r * row_bytes + f.offset, f.bytes);
        bool nan;
        const int64_t key = where_key(v, f.kind, f.bytes, f.inf, &nan);
        a.count++;
        if (nan) { a.nans++; continue; }
        agg_extreme(a, key, r);
        a.sum = fp ? agg_u64(agg_f64(a.sum) + agg_f64(widen_to_f64(v, f.bytes, f.mant))) : a.sum + (f.kind == 1 ? (uint64_t)key : v);
      }
      a = agg_workgroup(a, waves, tid, fp);
      if (tid == 0) partials[(size_t)t * (uint32_t)nfields + (uint32_t)k] = AggPartial{a.min_key, a.max_key, a.sum, a.min_row, a.max_row, a.count, a.nans};
    }
  }
}

// results [nchunks * nfields]: the entries of the pass's chunks in the call's table, chunk-major, every one written
__global__ __launch_bounds__(WH_THREADS) void k_aggregate_chunks_fields(const WhereChunk* __restrict__ chunks, const uint32_t* __restrict__ tile_first, int nchunks,
                                                                       uint32_t row_bytes, const AggField* __restrict__ fields /*[nfields]*/, int nfields,
                                                                       const AggPartial* __restrict__ partials, AggResult* __restrict__ results) {
  __shared__ AggAcc waves[WH_WAVES];
  const uint32_t tid = threadIdx.x;
  const uint32_t nwork = (uint32_t)nchunks * (uint32_t)nfields;
  for (uint32_t w = blockIdx.x; w < nwork; w += gridDim.x) {
    const uint32_t c = w / (uint32_t)nfields, k = w % (uint32_t)nfields;
    const AggField f = fields[k];
    const bool fp = f.kind == 2;
    const WhereChunk ch = chunks[c];
    const uint32_t t1 = tile_first[c + 1];
    AggAcc a = agg_none();
    for (uint32_t t = tile_first[c] + tid; t < t1; t += WH_THREADS) {
      const AggPartial p = partials[(size_t)t * (uint32_t)nfields + k];
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
      results[w] = r;
    }
  }
}

}  // namespace bamd
