// k_checksum.hip — zlib's adler32 / crc32 of many byte runs in device memory (include/blosc_gpu_checksum.h).
//
// Every run is cut into tiles of `tile_bytes` (a multiple of 16) counted from the run's FIRST byte; tile0[] is the prefix sum of the runs' tile
// counts.  k_checksum_tiles: one wavefront per tile (a persistent grid strides over the tiles) writes one 32-bit partial that already
// carries the tile's place in its run, so that k_checksum_combine - one wavefront per run - only adds (adler32) or XORs (crc32) the run's
// partials and puts in the terms that depend on the length alone.  Both digests combine in any order, so every level is a reduction and
// the result does not depend on the grid.
//
//   adler32 = (B << 16) | A,  A = 1 + sum d_i,  B = n + sum (n - i) d_i  (mod 65521).  A tile of L bytes with `behind` bytes of the run after it
//   contributes  S1 = sum d  and  S2 + behind * S1,  S2 = sum (L - i) d_i  over its own bytes.
//
//   crc32: with raw(M) = M(x) x^32 mod P (register starts at 0, no final XOR; linear over GF(2)),
//   crc32(M) = raw(M) ^ 0xFFFFFFFF x^(8n) ^ 0xFFFFFFFF  and  raw(M1 M2) = raw(M1) x^(8 |M2|) ^ raw(M2).
//   All polynomials are in zlib's reflected form: bit 31 is x^0, a right shift multiplies by x, and a dword loaded little endian from four
//   message bytes IS the polynomial of those bytes.
//
// Reads: every load lies inside the run (whole 16-byte words from run offset `tile offset + L % 16 + 16 j`, and the tile's first L % 16
// bytes one by one), whatever the alignment of the run - nothing before its first or behind its last byte is touched.
#pragma once
#include "wave_prims.h"

namespace bamd {

constexpr int CK_ADLER32 = 1, CK_CRC32 = 2;
constexpr int CK_THREADS = 256, CK_WAVES = CK_THREADS / 64;
constexpr int CK_WGS_PER_CU = 4;        // 106 VGPRs: four waves per SIMD
constexpr uint32_t CK_TILE_DEFAULT = 256u << 10, CK_TILE_MAX = 1u << 20;      // a lane's byte sum of a tile stays below 2^22, its weighted sum below 2^42
constexpr uint32_t CK_MOD = 65521u;
constexpr uint32_t CK_POLY = 0xedb88320u;
constexpr uint32_t CK_STRIDE = 1024u;             // bytes between two words of one lane: 64 lanes x 16 bytes

struct CkRun { const uint8_t* src; uint64_t nbytes; };

// constants of the crc32 kernels, computed by the host once (ck_constants) and uploaded behind the run table
//   [0, 32)  x^(2^k) mod P          [32 + j], j = 0 .. 3: x^(32 (4 - j)) - what dword j of a 16-byte word is multiplied by        [36] x^(8 CK_STRIDE)
constexpr int CK_NCONST = 40, CK_C_WORD = 32, CK_C_STRIDE = 36;

// a(x) b(x) mod P (zlib's multmodp with a fixed trip count: no lane leaves early)
__host__ __device__ inline uint32_t ck_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    p ^= (a & (0x80000000u >> i)) ? b : 0u;
    b = (b >> 1) ^ ((b & 1u) ? CK_POLY : 0u);
  }
  return p;
}
inline void ck_constants(uint32_t* c) {
  c[0] = 0x40000000u;                                                        // x^1
  for (int k = 1; k < 32; k++) c[k] = ck_mulmod(c[k - 1], c[k - 1]);
  c[CK_C_WORD + 0] = c[7]; c[CK_C_WORD + 1] = ck_mulmod(c[6], c[5]); c[CK_C_WORD + 2] = c[6]; c[CK_C_WORD + 3] = c[5];
  c[CK_C_STRIDE] = c[13];                                                    // x^8192
  for (int k = CK_C_STRIDE + 1; k < CK_NCONST; k++) c[k] = 0;
}

__device__ __forceinline__ uint64_t uni64(uint64_t v) { return ((uint64_t)uni((uint32_t)(v >> 32)) << 32) | uni((uint32_t)v); }

// x^e mod P, the same in every lane: lane k holds x^(2^k) where bit k of e is set (x^(2^32) = x, so the table repeats after 32), and a
// butterfly multiplies the 64 factors
__device__ __forceinline__ uint32_t wave_xpow(const uint32_t* __restrict__ consts, uint64_t e, int lane) {
  uint32_t f = ((e >> lane) & 1u) ? consts[lane & 31] : 0x80000000u;
  for (int m = 1; m < 64; m <<= 1) f = ck_mulmod(f, (uint32_t)__shfl_xor((int)f, m, 64));
  return f;
}

// the run that tile t belongs to: the largest i with tile0[i] <= t (tile0[nruns] > t).  64 probes per round.
__device__ __forceinline__ uint32_t ck_find_run(const uint64_t* __restrict__ tile0, uint32_t nruns, uint64_t t, int lane) {
  uint32_t lo = 0, hi = nruns;
  while (hi - lo > 1u) {
    const uint32_t step = (hi - lo + 63u) >> 6;
    const uint64_t probe = (uint64_t)lo + (uint64_t)(lane + 1) * step;
    const bool le = probe < hi && tile0[probe] <= t;
    const uint32_t c = (uint32_t)__builtin_popcountll(__ballot(le));         // tile0 is sorted: the lanes that say yes are the first c
    const uint64_t nhi = (uint64_t)lo + (uint64_t)(c + 1u) * step;
    lo += c * step;
    if (nhi < hi) hi = (uint32_t)nhi;
  }
  return lo;
}

// ---- adler32 of one tile: (S2 << 16 | S1), S2 weighted towards the tile's end -----------------------------------------
__device__ __forceinline__ void ck_adler_tile(const gu8* p, uint32_t L, int lane, uint32_t* S1, uint32_t* S2) {
  uint32_t s1 = 0; uint64_t s2 = 0;
  const uint32_t r = L & 15u, nw = L >> 4;
  if ((uint32_t)lane < r) { const uint32_t d = p[lane]; s1 = d; s2 = (uint64_t)(L - (uint32_t)lane) * d; }
#pragma unroll 4
  for (uint32_t j = (uint32_t)lane; j < nw; j += 64u) {
    const uint32_t o = r + 16u * j;
    const uint4 v = g_ld16(p + o);
    const uint32_t wds[4] = {v.x, v.y, v.z, v.w};
    uint32_t t1 = 0, t2 = 0;             // t2 = sum k * d_(o+k), k = 0..15
#pragma unroll
    for (int k = 0; k < 16; k++) { const uint32_t d = (wds[k >> 2] >> (8 * (k & 3))) & 0xffu; t1 += d; t2 += (uint32_t)k * d; }
    s1 += t1; s2 += (uint64_t)((L - o) * t1 - t2);        // (L - o) t1 < 2^20 * 2^12
  }
  *S1 = wave_sum_u32(s1) % CK_MOD;
  *S2 = wave_sum_u32((uint32_t)(s2 % CK_MOD)) % CK_MOD;
}

// ---- crc32 ---------------------------------------------------------------------------------------------------------
// tab[op][k][b] = (b << 8 k)(x) * C_op: op 0 .. 3 the dwords of a word, op 4 the lane's register on its way over CK_STRIDE bytes.
// Twenty independent ds_read_b32 per 16 bytes; their indices are data, so the 32 lanes of a half wave fall on the 32 banks at random.
__device__ __forceinline__ uint32_t ck_mul4(const uint32_t* tab, int op, uint32_t v) {
  const uint32_t* t = tab + op * 1024;
  return t[v & 0xffu] ^ t[256u + ((v >> 8) & 0xffu)] ^ t[512u + ((v >> 16) & 0xffu)] ^ t[768u + (v >> 24)];
}
__device__ __forceinline__ uint32_t ck_raw16(const uint32_t* tab, const uint4& w) {
  return ck_mul4(tab, 0, w.x) ^ ck_mul4(tab, 1, w.y) ^ ck_mul4(tab, 2, w.z) ^ ck_mul4(tab, 3, w.w);
}
// raw() of one tile.  The tile is laid out in 16-byte slots that END at the tile's end: its first L % 16 bytes make a slot of their own,
// filled up with zeros in FRONT, and empty slots in front of that one fill the first row of 64 - zeros in front of a message do not change
// raw().  Slot q belongs to lane q % 64; a lane walks its slots with  s = s x^(8 CK_STRIDE) ^ raw(slot), and the 64 registers, 16 bytes
// apart, meet in a butterfly.
__device__ __forceinline__ uint32_t ck_crc_tile(const gu8* p, uint32_t L, int lane, const uint32_t* tab, const uint32_t* __restrict__ consts) {
  const uint32_t r = L & 15u, hr = r ? 1u : 0u, nslots = (L >> 4) + hr;
  const uint32_t rows = (nslots + 63u) >> 6, pad = rows * 64u - nslots;
  uint32_t s = 0;
  if ((uint32_t)lane >= pad) {
    uint4 w;
    if (hr && (uint32_t)lane == pad) {
      uint64_t lo = 0, hi = 0;
      for (uint32_t i = 0; i < r; i++) {
        const uint32_t pos = 16u - r + i; const uint64_t d = p[i];
        if (pos < 8u) lo |= d << (8u * pos); else hi |= d << (8u * (pos - 8u));
      }
      w = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    } else {
      w = g_ld16(p + r + 16u * ((uint32_t)lane - pad - hr));
    }
    s = ck_raw16(tab, w);
  }
  const gu8* q = p + r + 16u * (64u + (uint32_t)lane - pad - hr);
#pragma unroll 4
  for (uint32_t k = 1; k < rows; k++, q += CK_STRIDE) {
    const uint4 w = g_ld16(q);
    s = ck_mul4(tab, 4, s) ^ ck_raw16(tab, w);
  }
  for (int m = 0; m < 6; m++) {                     // level m: groups of 2^m lanes, 16 * 2^m bytes each; the lower group comes first in the message
    const uint32_t o = (uint32_t)__shfl_xor((int)s, 1 << m, 64);
    const bool upper = (lane >> m) & 1;
    s = ck_mulmod(upper ? o : s, consts[7 + m]) ^ (upper ? s : o);
  }
  return s;
}

__global__ __launch_bounds__(CK_THREADS) void k_checksum_tiles(int kind, const CkRun* __restrict__ runs, const uint64_t* __restrict__ tile0, uint32_t nruns,
                                                               uint64_t ntiles, uint32_t tile_bytes, const uint32_t* __restrict__ consts,
                                                               uint32_t* __restrict__ partials) {
  __shared__ uint32_t tab[5 * 1024];
  if (kind == CK_CRC32) {
    for (uint32_t i = threadIdx.x; i < 5u * 1024u; i += CK_THREADS)
      tab[i] = ck_mulmod((i & 255u) << (8u * ((i >> 8) & 3u)), consts[CK_C_WORD + (i >> 10)]);
    __syncthreads();
  }
  const int lane = (int)(threadIdx.x & 63u);
  const uint32_t wave = uni(threadIdx.x >> 6);
  for (uint64_t t = (uint64_t)blockIdx.x * CK_WAVES + wave; t < ntiles; t += (uint64_t)gridDim.x * CK_WAVES) {
    const uint32_t run = uni(ck_find_run(tile0, nruns, t, lane));
    const uint64_t n = uni64(runs[run].nbytes);
    const uint64_t off = (t - uni64(tile0[run])) * tile_bytes;
    const uint32_t L = n - off < tile_bytes ? (uint32_t)(n - off) : tile_bytes;
    const uint64_t behind = n - off - L;
    const gu8* p = uni_ptr(as_global(runs[run].src)) + off;
    uint32_t part;
    if (kind == CK_CRC32) {
      part = ck_mulmod(ck_crc_tile(p, L, lane, tab, consts), wave_xpow(consts, behind << 3, lane));
    } else {
      uint32_t s1, s2;
      ck_adler_tile(p, L, lane, &s1, &s2);
      part = ((uint32_t)((s2 + (behind % CK_MOD) * s1) % CK_MOD) << 16) | s1;
    }
    if (lane == 0) partials[t] = part;
  }
}

// one wavefront per run
__global__ __launch_bounds__(CK_THREADS) void k_checksum_combine(int kind, const CkRun* __restrict__ runs, const uint64_t* __restrict__ tile0, uint32_t nruns,
                                                                 const uint32_t* __restrict__ consts, const uint32_t* __restrict__ partials,
                                                                 uint32_t* __restrict__ digests) {
  const int lane = (int)(threadIdx.x & 63u);
  const uint64_t run = (uint64_t)blockIdx.x * CK_WAVES + (threadIdx.x >> 6);
  if (run >= nruns) return;
  const uint64_t t0 = tile0[run], t1 = tile0[run + 1], n = runs[run].nbytes;
  uint32_t digest;
  if (kind == CK_CRC32) {
    uint32_t x = 0;
    for (uint64_t t = t0 + (uint64_t)lane; t < t1; t += 64u) x ^= partials[t];
    for (int m = 1; m < 64; m <<= 1) x ^= (uint32_t)__shfl_xor((int)x, m, 64);
    digest = x ^ ck_mulmod(0xffffffffu, wave_xpow(consts, n << 3, lane)) ^ 0xffffffffu;
  } else {
    uint64_t a = 0, b = 0;
    for (uint64_t t = t0 + (uint64_t)lane; t < t1; t += 64u) { const uint32_t v = partials[t]; a += v & 0xffffu; b += v >> 16; }
    const uint32_t A = (1u + wave_sum_u32((uint32_t)(a % CK_MOD))) % CK_MOD;
    const uint32_t B = ((uint32_t)(n % CK_MOD) + wave_sum_u32((uint32_t)(b % CK_MOD))) % CK_MOD;
    digest = (B << 16) | A;
  }
  if (lane == 0) digests[run] = digest;
}

}  // namespace bamd
