// k_take.hip — rows of compressed chunks by a device index table (include/blosc_gpu_take.h; engine.hip: engine_take).
//
// The chunks of a call are one array of rows of row_bytes bytes (dev_types.h: TakeChunk).  Two kernels, neither persistent, both over all
// indices of the call:
//   k_take_mark    one lane per index: the blocks the row lies in get a byte 1 in `touched` (plain byte stores of one value: rows that share a
//                  block race for nothing), from which the host builds the runs to decode;
//   k_take_gather  per pass, once the runs are decoded: every row of the pass's chunks from its slot to dest + k * row_bytes.
// Both find a row's chunk by bisection over row_first.  The workgroup keeps row_first in LDS where the call has at most TK_LDS_CHUNKS chunks
// (8 KiB, four workgroups of four waves per CU); above that the bisection reads the table in global memory, which stays in L2.
#pragma once
#include "dev_types.h"
#include "mem_prims.h"

namespace bamd {

constexpr int TK_THREADS = 256;
constexpr int TK_WAVES_PER_CU = 16;         // the grid, as k_getitem_gather's: a choice, not a residency
constexpr int TK_LDS_CHUNKS = 1024;

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

#define TAKE_ROW_FIRST_IN_LDS(first, in_lds)                                                                             \
  __shared__ int64_t first[TK_LDS_CHUNKS];                                                                               \
  const bool in_lds = nchunks <= TK_LDS_CHUNKS;                                                                          \
  if (in_lds) {                                                                                                          \
    for (int i = (int)threadIdx.x; i < nchunks; i += TK_THREADS) first[i] = chunks[i].row_first;                         \
    __syncthreads();                                                                                                     \
  }

__global__ __launch_bounds__(TK_THREADS) void k_take_mark(const TakeChunk* __restrict__ chunks /*[nchunks + 1]*/, int nchunks,
                                                         const int64_t* __restrict__ index, size_t nidx, uint32_t row_bytes,
                                                         uint8_t* __restrict__ touched /*[chunks[nchunks].block_first]*/) {
  TAKE_ROW_FIRST_IN_LDS(first, in_lds)
  const int64_t nrows = chunks[nchunks].row_first;
  for (size_t k = (size_t)blockIdx.x * TK_THREADS + threadIdx.x; k < nidx; k += (size_t)gridDim.x * TK_THREADS) {
    const int64_t r = index[k];
    if (r < 0 || r >= nrows) continue;
    const TakeChunk t = chunks[take_chunk_of(first, chunks, nchunks, in_lds, r)];
    if (!t.blocksize) continue;      // MEMCPYED: nothing to decode
    const uint32_t lo = (uint32_t)(r - t.row_first) * row_bytes;      // (a chunk has fewer than 2^31 bytes)
    const uint32_t j0 = lo / (uint32_t)t.blocksize, j1 = (lo + row_bytes - 1u) / (uint32_t)t.blocksize;
    for (uint32_t j = j0; j <= j1; j++) touched[(uint32_t)t.block_first + j] = 1;
  }
}

// Lane mapping, chosen by the host from row_bytes (and dest's alignment), the same for every row: 2^lanes_log2 consecutive lanes serve one row,
// consecutive groups consecutive k - the stores of a wave cover one contiguous piece of dest.
//   row_bytes <= 16: one lane per row; one load and one store of the natural width where row_bytes is 2 / 4 / 8 / 16 and both addresses are
//                    aligned for it, byte moves otherwise;
//   larger rows:     k_getitem_gather's scheme inside the group - bytes up to the first 16-byte boundary of the DESTINATION, aligned 16-byte
//                    stores fed by unaligned dwordx4 loads (mem_prims.h), bytes behind them.
// A row is written only after the status words of all its blocks have been read; the first negative one is its answer and nothing is written.
__global__ __launch_bounds__(TK_THREADS) void k_take_gather(const TakeChunk* __restrict__ chunks /*[nchunks + 1]*/, int nchunks,
                                                           const TakeBlock* __restrict__ blocks, const int32_t* __restrict__ block_status,
                                                           const int64_t* __restrict__ index, size_t nidx, uint32_t row_bytes, int lanes_log2,
                                                           uint8_t* __restrict__ dest, int32_t* __restrict__ status /*may be nullptr*/,
                                                           uint32_t* __restrict__ failed, int first_pass) {
  TAKE_ROW_FIRST_IN_LDS(first, in_lds)
  const int64_t nrows = chunks[nchunks].row_first;
  const uint32_t G = 1u << lanes_log2, sub = threadIdx.x & (G - 1u);
  const size_t per_group = (size_t)(TK_THREADS >> lanes_log2);      // rows of one workgroup and step
  uint32_t nfail = 0;
  for (size_t k0 = (size_t)blockIdx.x * per_group; k0 < nidx; k0 += (size_t)gridDim.x * per_group) {
    const size_t k = k0 + (threadIdx.x >> lanes_log2);
    if (k >= nidx) continue;
    const int64_t r = index[k];
    if (r < 0 || r >= nrows) {      // no row of any chunk: answered once, by the first pass
      if (first_pass && sub == 0) { if (status) status[k] = -1; nfail++; }
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
      if (sub == 0) { if (status) status[k] = code; nfail++; }
      continue;
    }
    const gu8* s = as_global(b.base) + (lo - j0 * (uint32_t)t.blocksize);
    gu8* d = as_global(dest) + k * (size_t)row_bytes;
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
    if (sub == 0 && status) status[k] = (int32_t)row_bytes;
  }
  if (nfail) atomicAdd(failed, nfail);
}

#undef TAKE_ROW_FIRST_IN_LDS

}  // namespace bamd
