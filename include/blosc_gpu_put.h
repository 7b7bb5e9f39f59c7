/* include/blosc_gpu_put.h — rows written INTO device-resident compressed chunks by an index table that lies on the device.
 *
 * table.index_copy_(0, idx, rows) for a table that is kept compressed - the writing half of include/blosc_gpu_take.h: an embedding row
 * that was trained, a line of a compressed cache that was replaced, a value of a key-value store.  Without these calls a caller decodes
 * the whole container (blosc_gpu_decompress_packed), updates the plaintext and encodes all of it again (blosc_gpu_compress_packed) - the
 * full decode, the full encode and the full plaintext footprint for an update that may touch one chunk in a hundred.  Here only the
 * chunks some row lands in are decoded and encoded again, every other chunk is carried over byte for byte, and the result is a NEW
 * packed container: the old one is not written and stays valid until the caller drops it.
 *
 * Conventions, rows and the census are those of include/blosc_gpu_take.h: src, offsets, params and every *_out table are HOST memory,
 * src[i], container, index, rows, dest and status DEVICE (or managed) memory on the current device.  The chunks of a call are ONE array
 * of rows of row_bytes bytes (1 ... 65536), chunk i holding nbytes_i / row_bytes of them; every chunk passes the header checks of
 * blosc_getitem in its order (blosc/blosc.c:1603-1632) and, in the packed form, the slot checks, and its nbytes is a multiple of row_bytes.
 * `index` is int64, in any order, repeats allowed; row index[k] is written from rows + k * row_bytes, at any alignment.
 *
 * The census has more to check than take's:
 *   params[i] passes the checks of blosc_gpu_compress_batch_params (include/blosc_gpu_params.h) for EVERY chunk, touched or not;
 *       its code (-10, -5) goes into chunk_rows_out[i]
 *   nidx <= UINT32_MAX - 1
 *   `align` follows include/blosc_gpu_packed.h (0 means 1; a power of two up to 4096); dest may be NULL only with destsize 0
 *   [dest, dest + destsize) overlaps neither the source container nor any src[i] chunk
 * With any check failing the call answers a negative value and writes nothing: not dest, not offsets_out, cbytes_out, rewritten_out,
 * status or *failed_out.  (chunk_rows_out holds every chunk's rows or its negative code, as in take.)
 *
 * After a passed census:
 *
 * Touched chunks.  A chunk is touched if some valid index names one of its rows.  A touched chunk that decodes is REWRITTEN: its
 * plaintext with the rows put in is compressed with params[i] exactly as blosc_gpu_compress_batch_params compresses it with
 * destsize = nbytes + 16 (what blosc_compress_ctx returns for that destsize, blosc.c:1254-1257: it never answers 0 for lack of room).  For
 * the deterministic settings ("blosclz", "lz4", "zstd" up to clevel 5) the bytes are that call's bytes; for every setting stock c-blosc
 * reads back the updated plaintext.  A touched MEMCPYED chunk is rewritten like any other and may come out compressed.
 *
 * Repeated indices.  If an index occurs several times, the LAST occurrence (the largest k) wins - whole rows, never a mix; that is
 * index_copy_ applied in the order of k.  status[k] = row_bytes for every valid index whose chunk was rewritten, winner or not.
 *
 * Indices that are not written.  An index outside [0, nrows) - every int64_t is a legal input - gets status[k] = -1.  A touched chunk
 * that does not decode (blosc_decompress would answer -1, blosc.c:1511-1514) is carried over unchanged, its indices get status[k] = -1
 * and rewritten_out[i] = -1.  *failed_out is the number of k with a negative status.
 *
 * Untouched chunks, and the carried-over ones above, are copied byte for byte (the `cbytes` of their header).  rewritten_out[i] is 1 for
 * a rewritten chunk, 0 for an untouched one, -1 for a touched chunk that did not decode.
 *
 * Layout of dest: blosc_gpu_compress_packed's rule over all chunks in the caller's order - offsets_out[0] = 0,
 * offsets_out[i + 1] = align_up(offsets_out[i] + cbytes_i, align) whether or not chunk i was written, so offsets_out[nchunks] is
 * always the size needed.  Chunk i is written iff offsets_out[i] + cbytes_i <= destsize; otherwise cbytes_out[i] = 0 and nothing is
 * written for it.  The bytes between a written chunk and offsets_out[i + 1] (below destsize) are zero.  Nothing at or behind
 * dest + destsize is written.  A dest of blosc_gpu_packed_bound(nchunks, nbytes, align) bytes always fits.
 *
 * nidx == 0: the census runs, then every chunk is copied as it is - the container laid out anew under `align`.
 *
 * Synchronous, ordered on `stream` (a hipStream_t as void*, NULL = default stream).  The chunks are dealt, in their order, to passes of
 * at most 256 MiB of plaintext of touched chunks (a larger chunk is a pass of its own).  A call synchronises with the host once for the
 * headers, once for the flags of the touched chunks, three times per pass that has a touched chunk and once at its end.  While a pass
 * runs the library holds, besides the decoder's and the encoder's workspaces, the plaintext of the pass's touched chunks, one 32-bit
 * owner word per row of them and nbytes + 16 bytes per touched chunk for the encoder's output.
 */
#ifndef BLOSC_AMD_BLOSC_GPU_PUT_H
#define BLOSC_AMD_BLOSC_GPU_PUT_H
#include <stddef.h>
#include <stdint.h>
#include "blosc_gpu_params.h"
#ifdef __cplusplus
extern "C" {
#endif
#ifndef BLOSC_EXPORT
#define BLOSC_EXPORT __attribute__((visibility("default")))
#endif

/* chunk i at src[i] */
BLOSC_EXPORT int blosc_gpu_put_batch(int nchunks, const void* const* src, size_t row_bytes,
                                     size_t nidx, const int64_t* index /* DEVICE [nidx] */,
                                     const void* rows /* DEVICE, nidx * row_bytes */,
                                     const blosc_gpu_cparams* params /* HOST [nchunks] */,
                                     void* dest, size_t destsize, size_t align,
                                     size_t* offsets_out /* HOST [nchunks + 1] */, int* cbytes_out /* HOST [nchunks] */,
                                     int* rewritten_out /* HOST [nchunks], may be NULL */,
                                     int* status /* DEVICE [nidx], may be NULL */,
                                     int* chunk_rows_out /* HOST [nchunks], may be NULL */,
                                     size_t* failed_out /* HOST, may be NULL */, void* stream);

/* The same out of a packed container (include/blosc_gpu_packed.h): chunk i is the offsets[i + 1] - offsets[i] bytes at
 * container + offsets[i].  `offsets` not non-decreasing or offsets[nchunks] > containersize answers a negative value. */
BLOSC_EXPORT int blosc_gpu_put_packed(int nchunks, const void* container, size_t containersize,
                                      const size_t* offsets /* HOST [nchunks + 1] */, size_t row_bytes,
                                      size_t nidx, const int64_t* index, const void* rows, const blosc_gpu_cparams* params,
                                      void* dest, size_t destsize, size_t align, size_t* offsets_out, int* cbytes_out,
                                      int* rewritten_out, int* status, int* chunk_rows_out, size_t* failed_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
