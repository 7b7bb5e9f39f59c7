// k_take.hip — rows of compressed chunks by a device index table (include/blosc_gpu_take.h; engine.hip: engine_take).
//
// The chunks of a call are one array of rows of row_bytes bytes (dev_types.h: TakeChunk).  Two kernels, neither persistent, both over all
// indices of the call:
//   k_take_mark    one lane per index: the blocks the row lies in get a byte 1 in `touched` (plain byte stores of one value: rows that share a
//                  block race for nothing), from which the host builds the runs to decode;
//   k_take_gather  per pass, once the runs are decoded: every row of the pass's chunks from its slot to dest + k * row_bytes.
// Both find a row's chunk by bisection over row_first, which the workgroup keeps in LDS where it fits (row_prims.h: take_chunk_of).
#pragma once
#include "dev_types.h"
#include "mem_prims.h"
#include "row_prims.h"

namespace bamd {

__global__ __launch_bounds__(TK_THREADS) void k_take_mark(const TakeChunk* __restrict__ chunks /*[nchunks + 1]*/, int nchunks,
                                                         const int64_t* __restrict__ index, size_t nidx, uint32_t row_bytes,
                                                         uint8_t* __restrict__ touched /*[chunks[nchunks].block_first]*/) {
  TK_ROW_FIRST_IN_LDS(first, in_lds)
  const int64_t nrows = chunks[nchunks].row_first;
  for (size_t k = (size_t)blockIdx.x * TK_THREADS + threadIdx.x; k < nidx; k += (size_t)gridDim.x * TK_THREADS) {
    const int64_t r = index[k];
    if (take_no_row(r, nrows)) continue;
    const TakeChunk t = chunks[take_chunk_of(first, chunks, nchunks, in_lds, r)];
    if (!t.blocksize) continue;      // MEMCPYED: nothing to decode
    const uint32_t lo = (uint32_t)(r - t.row_first) * row_bytes;      // (a chunk has fewer than 2^31 bytes)
    const uint32_t j0 = lo / (uint32_t)t.blocksize, j1 = (lo + row_bytes - 1u) / (uint32_t)t.blocksize;
    for (uint32_t j = j0; j <= j1; j++) touched[(uint32_t)t.block_first + j] = 1;
  }
}

// 2^lanes_log2 consecutive lanes serve one row (row_prims.h: move_row), consecutive groups consecutive k - the stores of a wave cover one
// contiguous piece of dest.
// A row is written only after the status words of all its blocks have been read; the first negative one is its answer and nothing is written.
__global__ __launch_bounds__(TK_THREADS) void k_take_gather(const TakeChunk* __restrict__ chunks /*[nchunks + 1]*/, int nchunks,
                                                           const TakeBlock* __restrict__ blocks, const int32_t* __restrict__ block_status,
                                                           const int64_t* __restrict__ index, size_t nidx, uint32_t row_bytes, int lanes_log2,
                                                           uint8_t* __restrict__ dest, int32_t* __restrict__ status /*may be nullptr*/,
                                                           uint32_t* __restrict__ failed, int first_pass) {
  TK_ROW_FIRST_IN_LDS(first, in_lds)
  const int64_t nrows = chunks[nchunks].row_first;
  const uint32_t G = 1u << lanes_log2, sub = threadIdx.x & (G - 1u);
  const size_t per_group = (size_t)(TK_THREADS >> lanes_log2);      // rows of one workgroup and step
  uint32_t nfail = 0;
  for (size_t k0 = (size_t)blockIdx.x * per_group; k0 < nidx; k0 += (size_t)gridDim.x * per_group) {
    const size_t k = k0 + (threadIdx.x >> lanes_log2);
    if (k >= nidx) continue;
    const int64_t r = index[k];
    if (take_no_row(r, nrows)) {
      if (first_pass && sub == 0) take_fail(status, k, -1, nfail);
      continue;
    }
    const TakeChunk t = chunks[take_chunk_of(first, chunks, nchunks, in_lds, r)];
    const uint32_t lo = (uint32_t)(r - t.row_first) * row_bytes;
    uint32_t j0 = 0, j1 = 0;
    if (t.blocksize) { j0 = lo / (uint32_t)t.blocksize; j1 = (lo + row_bytes - 1u) / (uint32_t)t.blocksize; }
    const TakeBlock b = blocks[(uint32_t)t.block_first + j0];
    if (!b.base) continue;          // a chunk of another pass
    int32_t code = 0;               // (the blocks of a row lie in one run: their status words are neighbours)
    if (b.status >= 0)
      for (uint32_t j = 0; j <= j1 - j0 && !code; j++) { const int32_t v = block_status[b.status + (int32_t)j]; if (v < 0) code = v; }
    if (code) {
      if (sub == 0) take_fail(status, k, code, nfail);
      continue;
    }
    move_row(as_global(dest) + k * (size_t)row_bytes, as_global(b.base) + (lo - j0 * (uint32_t)t.blocksize), row_bytes, sub, G);
    if (sub == 0 && status) status[k] = (int32_t)row_bytes;
  }
  if (nfail) atomicAdd(failed, nfail);
}

}  // namespace bamd
