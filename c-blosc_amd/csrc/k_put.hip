// k_put.hip — rows written into compressed chunks by a device index table (include/blosc_gpu_put.h; engine.hip: engine_put).
//
// k_take.hip mirrored, over the same pieces (row_prims.h).  The chunks of a call are one array of rows (dev_types.h: TakeChunk); the chunks some
// valid index names are decoded whole into plaintext slots, pass by pass, and the chunks of a pass are a range [c0, c1) of the call's chunks
// (PutChunk[c1 - c0]).
// Three kernels, none persistent:
//   k_put_claim     one lane per index: the row's owner word takes the minimum of nidx - 1 - k over the indices k that name the row, so the
//                   LAST occurrence owns it (atomicMin at L2; the words are read by the next kernel only, behind the kernel boundary);
//   k_put_scatter   k_take_gather's lane mapping (move_row) with source and destination exchanged: index k stores rows + k * row_bytes into
//                   its row of the slot if it owns the row - whole rows, never a mix - and answers status[k];
//   k_put_assemble  every chunk of the pass to its place in the new container, from the source (carried over) or from the slot the encoder
//                   wrote (rewritten), and zeros up to the next offset: tiles of one wave (tile_owner, wave_copy_tile).
// The mark kernel of a put is k_take_mark, unchanged, over a table that gives every chunk ONE block of nbytes: a flag per touched chunk.
#pragma once
#include "dev_types.h"
#include "mem_prims.h"
#include "row_prims.h"

namespace bamd {

constexpr uint32_t PA_TILE = 16384;     // k_put_assemble: 16 steps of 64 lanes x 16 bytes
constexpr int PA_THREADS = 64;
constexpr int PA_WAVES_PER_CU = 16;

__global__ __launch_bounds__(TK_THREADS) void k_put_claim(const TakeChunk* __restrict__ chunks /*[nchunks + 1]*/, int nchunks,
                                                         const PutChunk* __restrict__ put /*[c1 - c0]*/, int c0, int c1,
                                                         const int64_t* __restrict__ index, size_t nidx, uint32_t* __restrict__ owner) {
  TK_ROW_FIRST_IN_LDS(first, in_lds)
  const int64_t nrows = chunks[nchunks].row_first;
  for (size_t k = (size_t)blockIdx.x * TK_THREADS + threadIdx.x; k < nidx; k += (size_t)gridDim.x * TK_THREADS) {
    const int64_t r = index[k];
    if (take_no_row(r, nrows)) continue;
    const int c = (int)take_chunk_of(first, chunks, nchunks, in_lds, r);
    if (c < c0 || c >= c1) continue;      // a chunk of another pass
    const PutChunk p = put[c - c0];
    if (!p.slot || p.status < 0) continue;
    atomicMin(&owner[p.owner_first + (uint64_t)(r - chunks[c].row_first)], (uint32_t)(nidx - 1 - k));      // (nidx <= UINT32_MAX - 1: never all ones)
  }
}

// 2^lanes_log2 consecutive lanes serve one index (row_prims.h: move_row, into the row's place in its slot), consecutive groups consecutive k -
// the loads of a wave cover one contiguous piece of `rows`.
// An index of a chunk that did not decode answers -1; an index outside the rows is answered where first_pass is set.
__global__ __launch_bounds__(TK_THREADS) void k_put_scatter(const TakeChunk* __restrict__ chunks /*[nchunks + 1]*/, int nchunks,
                                                           const PutChunk* __restrict__ put /*[c1 - c0]*/, int c0, int c1,
                                                           const uint32_t* __restrict__ owner, const int64_t* __restrict__ index, size_t nidx,
                                                           uint32_t row_bytes, int lanes_log2, const uint8_t* __restrict__ rows,
                                                           int32_t* __restrict__ status /*may be nullptr*/, uint32_t* __restrict__ failed, int first_pass) {
  TK_ROW_FIRST_IN_LDS(first, in_lds)
  const int64_t nrows = chunks[nchunks].row_first;
  const uint32_t G = 1u << lanes_log2, sub = threadIdx.x & (G - 1u);
  const size_t per_group = (size_t)(TK_THREADS >> lanes_log2);      // indices of one workgroup and step
  uint32_t nfail = 0;
  for (size_t k0 = (size_t)blockIdx.x * per_group; k0 < nidx; k0 += (size_t)gridDim.x * per_group) {
    const size_t k = k0 + (threadIdx.x >> lanes_log2);
    if (k >= nidx) continue;
    const int64_t r = index[k];
    if (take_no_row(r, nrows)) {
      if (first_pass && sub == 0) take_fail(status, k, -1, nfail);
      continue;
    }
    const int c = (int)take_chunk_of(first, chunks, nchunks, in_lds, r);
    if (c < c0 || c >= c1) continue;      // a chunk of another pass
    const PutChunk p = put[c - c0];
    if (!p.slot) continue;
    if (p.status < 0) {                   // the chunk did not decode: it is carried over as it is
      if (sub == 0) take_fail(status, k, -1, nfail);
      continue;
    }
    const uint64_t row = (uint64_t)(r - chunks[c].row_first);
    if (owner[p.owner_first + row] == (uint32_t)(nidx - 1 - k))
      move_row(as_global(p.slot) + row * row_bytes, as_global(rows) + k * (size_t)row_bytes, row_bytes, sub, G);
    if (sub == 0 && status) status[k] = (int32_t)row_bytes;      // winner or not: the row holds what the last occurrence brought
  }
  if (nfail) atomicAdd(failed, nfail);
}

// One-wave workgroups over tiles of PA_TILE bytes of the pass's chunks: copy c covers nbytes + pad bytes of the container - the chunk, then zeros -
// and tile_first[c] is the number of tiles in front of it (a chunk that ends behind the caller's destsize has none).
__global__ __launch_bounds__(PA_THREADS) void k_put_assemble(const PutCopy* __restrict__ copies, const uint32_t* __restrict__ tile_first /*[ncopies + 1]*/, int ncopies) {
  const uint32_t lane = threadIdx.x;
  const uint32_t ntiles = tile_first[ncopies];
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint32_t c = tile_owner(tile_first, ncopies, t);
    const PutCopy g = copies[c];
    const uint32_t total = g.nbytes + g.pad, off = (t - tile_first[c]) * PA_TILE;
    if (off >= total) continue;
    const uint32_t n = total - off < PA_TILE ? total - off : PA_TILE;
    const uint32_t live = off >= g.nbytes ? 0u : (g.nbytes - off < n ? g.nbytes - off : n);      // bytes of the tile that come from src
    wave_copy_tile<true>(as_global(g.dst) + off, as_global(g.src) + off, n, live, lane);
  }
}

}  // namespace bamd
