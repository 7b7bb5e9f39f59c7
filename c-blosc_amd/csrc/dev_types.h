// dev_types.h — descriptor tables shared by the host engine and the HIP kernels.
//
// The reference walks chunk -> block -> split with nested loops on one thread
// (blosc/blosc.c:803-867 serial_blosc, :591-800 blosc_c/blosc_d).  On the GPU every level is
// flattened into a table so that one launch covers every block / stream of every chunk of a
// batch:  ChunkDesc[nchunks]  ->  BlockDesc[nblocks_total]  ->  StreamDesc[nstreams_total]
// ("stream" = one split of a block, or the whole block when it is not split: the unit a codec sees).
#pragma once
#include <stdint.h>

namespace bamd {

enum : int32_t {
  FMT_BLOSCLZ = 0,  // header flag bits 5-7 (blosc/blosc.h:93-99)
  FMT_LZ4 = 1,
  FMT_ZLIB = 3,     // k_zlib.hip (decode), deflate_enc.h (encode)
  FMT_ZSTD = 4,     // k_zstd.hip / k_zstd2.hip (decode), zstd_enc.h (encode)
};

enum : uint32_t {
  CH_SHUFFLE = 1u,     // byte shuffle active for this chunk's blocks (flag bit0 && typesize > 1)
  CH_BITSHUFFLE = 2u,  // bit shuffle active (flag bit2; applied per block when bsize >= typesize)
  CH_MEMCPYED = 4u,    // payload is the raw input after the 16-byte header (flag bit1)
  CH_SKIP = 8u,        // chunk needs no device work (error found on host, or empty)
  CH_FUSED_UNSHUF = 16u,  // decompress: the decode kernel itself unshuffles each block when its last stream is done
  CH_FUSED_SHUF = 32u,    // compress: the encode kernel itself shuffles each block (queue task) before its streams are encoded
  CH_FUSED_BITUNSH = 64u, // decompress, bitshuffle chunks: the wave that completes a block's last stream bit-unshuffles the block (k_decode.hip)
};

struct ChunkDesc {
  const uint8_t* src;   // decompress: compressed chunk.  compress: uncompressed input
  uint8_t* dst;         // decompress: output buffer.     compress: chunk being written
  uint8_t* filt;        // plane-major scratch for this chunk's filtered bytes (nullptr: no filter)
  uint8_t* stage;       // compress only: staging area, one slot of `neblock` bytes per stream
  int32_t nbytes;       // uncompressed size
  int32_t cbytes;       // decompress: header cbytes.  compress: maxbytes (destsize clamped)
  int32_t blocksize;
  int32_t typesize;
  int32_t nblocks;
  int32_t leftover;     // nbytes % blocksize
  int32_t nsplits;      // streams per full block (1 or typesize); the leftover block always has 1
  int32_t fmt;          // FMT_*
  uint32_t mode;        // CH_* bits
  int32_t first_block;  // index of this chunk's block 0 in BlockDesc[]
  int32_t first_stream; // index of its first stream in StreamDesc[]
  int32_t clevel;       // compress only
  int32_t hdr_flags;    // compress only: header flag byte to write
};

// Scratch layout of a filtered chunk: plane-major per block, planes bsize / typesize bytes apart.  (Round 3 padded the planes of fused chunks
// apart to keep them off one HBM channel: no effect, profiles/r03/r03p_dec_ab_plane_padding_no_effect.txt - removed in round 4.)
#if defined(__HIPCC__) || defined(BAMD_WAVE_EMU)
#define BAMD_HD __host__ __device__
#else
#define BAMD_HD
#endif
BAMD_HD inline size_t filt_block_stride(const ChunkDesc& c) {
  return (size_t)c.blocksize;
}
// plane stride inside one block: split blocks of fused chunks are padded, everything else is the plain plane-major image
BAMD_HD inline uint32_t filt_plane_stride(const ChunkDesc& c, uint32_t bsize, int nstreams) {
  (void)nstreams;
  return bsize / (uint32_t)(c.typesize > 0 ? c.typesize : 1);      // bytes per plane (an unsplit block is ONE stream, but still typesize planes)
}

struct BlockDesc {
  int32_t chunk;        // owning chunk
  int32_t blk;          // block index inside the chunk
  int32_t first_stream; // global stream index of split 0
  int32_t nstreams;     // 1 or typesize
  int32_t bsize;        // bytes in this block: blocksize, or `leftover` for a short last block.  Computed
                        // on the host: selecting between two ChunkDesc fields on the device tripped an
                        // AMDGPU backend miscompile (ROCm 7.2, the `leftover > 0` test was dropped).
  int32_t flags;        // BLK_* bits
};
enum : int32_t {
  BLK_Z = 2,            // decompress: a block of a Zstd / zlib chunk: every stream of it belongs to k_zstd_* / k_zlib_streams, k_decode_streams' queues leave it out
  BLK_ZLIB = 4,         // ... of a zlib chunk (set together with BLK_Z): k_zlib_streams has per-XCD queues of its own (queue_order.h)
};

struct StreamDesc {
  const uint8_t* in;    // decode: compressed bytes.  encode: (filtered) plain bytes
  uint8_t* out;         // decode: where the plain bytes go.  encode: staging slot
  int32_t in_size;      // decode: csize.  encode: neblock
  int32_t out_size;     // decode: neblock (must be produced exactly).  encode: slot capacity
  int32_t chunk;
  int32_t fmt;          // FMT_*
  int32_t aux;          // encode: clevel | (global block index << 4).  decode: global index of the owning block
  int32_t result;       // encode: compressed size (0 = store raw).  decode: bytes produced or <0
};

// One entry of k_getitem_gather's range table (k_decode.hip; include/blosc_gpu_getitem.h): nbytes bytes from src - a slot of decoded blocks in
// the workspace, or the payload of a MEMCPYED chunk - to the caller's dst, provided that none of the nstatus status words from status0 on
// (one per block the range touches; none for a MEMCPYED chunk) is negative.
struct GatherRange {
  const uint8_t* src;
  uint8_t* dst;
  uint32_t nbytes;
  int32_t status0;
  int32_t nstatus;
  int32_t pad_;
};

// The tables of k_take_mark / k_take_gather (k_take.hip; include/blosc_gpu_take.h).  TakeChunk[nchunks + 1]: the call's chunks as ONE array of
// rows - chunk c holds rows [row_first, next row_first) and the entries [block_first, next block_first) of the block table, one per block of
// `blocksize` bytes; a MEMCPYED chunk has blocksize 0 and one entry.  The last entry closes both prefixes (row_first: the call's rows).
struct TakeChunk {
  int64_t row_first;
  int32_t block_first;
  int32_t blocksize;
};
// TakeBlock, one per block and pass: where the block's first byte lies - in a slot of decoded blocks, its verdict the status word `status`;
// for a MEMCPYED chunk the payload, status -1: nothing to ask - or nullptr: not in this pass (another pass's chunk, or a block no row touches).
struct TakeBlock {
  const uint8_t* base;
  int32_t status;
  int32_t pad_;
};

// The tables of k_put_claim / k_put_scatter / k_put_assemble (k_put.hip; include/blosc_gpu_put.h), next to the call's TakeChunk table.
// PutChunk, one per chunk of a pass: the slot its plaintext was decoded into - nullptr: no index names the chunk -, the first of the owner
// words of its rows, and the decoder's verdict (negative: the chunk is carried over, its indices answer -1).
struct PutChunk {
  uint8_t* slot;
  uint64_t owner_first;
  int32_t status;
  int32_t pad_;
};
// PutCopy, one per chunk of a pass: nbytes from src to dst, then `pad` zero bytes (both 0: the chunk ends behind the caller's buffer).
struct PutCopy {
  const uint8_t* src;
  uint8_t* dst;
  uint32_t nbytes;
  uint32_t pad;
};

// The tables of k_where_mark / k_where_scan / k_where_write (k_where.hip; include/blosc_gpu_where.h).
// WhereChunk, one per chunk of a pass: the slot its plaintext was decoded into, the call's number of its first row, its rows and the
// decoder's verdict (negative: its tiles count nothing).  Next to it lies the prefix of the chunks' tiles, as k_put_assemble has it.
struct WhereChunk {
  const uint8_t* slot;
  int64_t row_first;
  uint32_t rows;
  int32_t status;
};
// WherePred: the caller's predicate as the kernels evaluate it.  Every kind compares ONE signed 64-bit key (where_key below), so a row costs
// one load and integer instructions whatever its type, and the floating-point mode of the device plays no part:
//   UINT   the value with bit 63 flipped;   INT   the value sign-extended;
//   FLOAT, BFLOAT16   the magnitude bits, negated under the sign bit - the order of IEEE 754 with -0 = +0 = key 0, the same for binary16,
//          bfloat16, binary32 and binary64 (widening is exact and monotone: the order of the narrow patterns IS the order of the widened values);
//          a pattern above `inf` is a NaN, and a NaN on either side makes every comparison false but NE.
struct WherePred {
  uint32_t offset, bytes;
  int32_t kind, op;      // kind: 0 UINT, 1 INT, 2 the floating-point formats;  op: 0 ... 5 = EQ NE LT LE GT GE
  int64_t key;           // the constant's key
  uint64_t inf;          // floating point: the pattern of +infinity
  int32_t nan;           // the constant is a NaN
  int32_t pad_;
};
// WhereTerms: a term list (include/blosc_gpu_clauses.h) as k_where_mark_terms and k_aggregate_tiles_terms evaluate it.  A table in device
// memory that every lane reads at the same index: it is the same for all rows, so it travels in scalar registers.
//   fields   the distinct (offset, bytes) pairs the terms read, each loaded once per row.  In aggregate field 0 is ALWAYS the aggregated
//            one, whether a term tests it or not, so that the kernel takes its value at a constant index;
//   test     the terms as WherePred, SORTED by the field they read: those of field f are test[first[f]] ... test[first[f + 1] - 1], so the
//            kernel walks the fields at constant indices and the terms of each under a uniform bound - no register array is indexed at run time;
//   bit      1 << clause of test[t];  clauses: the OR of all of them.  A row passes when the bits of its true terms make up `clauses`.
constexpr int WH_MAX_TERMS = 16;
constexpr int WH_MAX_FIELDS = WH_MAX_TERMS + 1;
struct WhereTerms {
  uint32_t nterms, nfields;
  uint32_t clauses;
  uint32_t pad_;
  uint32_t offset[WH_MAX_FIELDS], bytes[WH_MAX_FIELDS];
  uint32_t first[WH_MAX_FIELDS + 1];
  uint32_t bit[WH_MAX_TERMS];
  WherePred test[WH_MAX_TERMS];
};
// v: the field's `bytes` bytes, little endian, zero-extended.  *nan (floating point): the pattern is a NaN
#if defined(__HIPCC__) || defined(__HIP__)
__host__ __device__
#endif
inline int64_t where_key(uint64_t v, int32_t kind, uint32_t bytes, uint64_t inf, bool* nan) {
  const uint32_t up = 64u - 8u * bytes;
  *nan = false;
  if (kind == 0) return (int64_t)(v ^ 0x8000000000000000ull);
  if (kind == 1) return (int64_t)(v << up) >> up;
  const uint64_t sign = 1ull << (8u * bytes - 1u), mag = v & (sign - 1ull);
  *nan = mag > inf;
  return (v & sign) ? -(int64_t)mag : (int64_t)mag;
}

// The binary64 pattern of a floating-point field: v as where_key takes it, `mant` the mantissa bits of its format (binary16 10, bfloat16 7,
// binary32 23, binary64 52).  Every value of the narrow formats is a binary64, so widening is exact; the pattern is put together from
// integers - a subnormal is normalised by its leading bit - so that the floating-point mode of the wave (denormals flushed or kept) plays
// no part.  Infinities stay infinities, a NaN stays a NaN.
#if defined(__HIPCC__) || defined(__HIP__)
__host__ __device__
#endif
inline uint64_t widen_to_f64(uint64_t v, uint32_t bytes, uint32_t mant) {
  if (bytes == 8u) return v;
  const uint32_t bits = 8u * bytes, ebits = bits - 1u - mant;
  const uint64_t sign = (v >> (bits - 1u)) << 63, m = v & ((1ull << mant) - 1ull);
  const uint32_t e = (uint32_t)(v >> mant) & ((1u << ebits) - 1u), bias = (1u << (ebits - 1u)) - 1u;
  if (e == (1u << ebits) - 1u) return sign | (0x7ffull << 52) | (m << (52u - mant));
  if (e) return sign | ((uint64_t)(e + 1023u - bias) << 52) | (m << (52u - mant));
  if (!m) return sign;
  const uint32_t p = 63u - (uint32_t)__builtin_clzll(m);      // m * 2^(1 - bias - mant) = 1.xxx * 2^(p + 1 - bias - mant)
  return sign | ((uint64_t)(p + 1u + 1023u - bias - mant) << 52) | ((m ^ (1ull << p)) << (52u - p));
}

// The tables of k_aggregate_tiles / k_aggregate_chunks (k_aggregate.hip; include/blosc_gpu_aggregate.h), next to where's WhereChunk and tile prefix.
// AggField: the aggregated field.  kind as in WherePred; inf and mant: its floating-point format (0 for the integers).
struct AggField {
  uint32_t offset, bytes;
  int32_t kind;          // 0 UINT, 1 INT, 2 the floating-point formats
  uint32_t mant;
  uint64_t inf;
};
// AggPartial, one per tile: what its rows that pass the filter add up to.  The extremes are (key, row in chunk) pairs, the lower row winning
// among equal keys; row AGG_NO_ROW: no value.  sum: a 64-bit integer, or the pattern of a binary64.
constexpr uint32_t AGG_NO_ROW = 0xffffffffu;
struct AggPartial {
  int64_t min_key, max_key;
  uint64_t sum;
  uint32_t min_row, max_row;
  uint32_t count, nans;
};
// AggResult, one per chunk: blosc_gpu_aggregate as the device writes it (min and max: the field's bytes, little endian, zero-extended)
struct AggResult {
  uint64_t rows, count, nans;
  int64_t min_row, max_row;
  uint64_t min, max, sum;
};

// Negative per-chunk status codes written by kernels (host maps them to the reference's
// return values, blosc/blosc.c:762-782): -1 bad csize chain / bounds, -2 codec produced wrong size.
enum : int32_t { ST_OK = 0, ST_BADCHAIN = -1, ST_BADCODEC = -2 };

}  // namespace bamd
