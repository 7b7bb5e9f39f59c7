/* include/blosc_gpu_take.h — rows of device-resident compressed chunks by an index table that lies on the device.
 *
 * table.index_select(0, idx) for a table that is kept compressed: embedding rows, a sampler over a compressed cache, a key-value lookup.
 * The calls of include/blosc_gpu_getitem.h serve this only through the host - every index one (chunk, start, nitems) range in three host
 * arrays, a destination pointer and a whole wave of the gather kernel per row.  These calls read the indices where they are: they fetch
 * the headers once, mark the blocks some row lies in, decode every marked block once in one launch of the pipeline, and write all rows
 * with one gather kernel that gives a row a lane or a few lanes.
 *
 * Conventions are those of include/blosc_gpu_getitem.h - src, offsets, chunk_rows_out and failed_out are HOST memory, src[i], container
 * and dest DEVICE (or managed) memory on the current device - with one difference: `index` and `status` are DEVICE arrays.  There may be
 * millions of them, and they come from device code.
 *
 * Rows.  The chunks of a call are ONE array of rows of row_bytes bytes each: chunk i holds rows [first(i), first(i + 1)),
 * first(0) = 0, first(i + 1) = first(i) + nbytes_i / row_bytes, and a row is bytes [r * row_bytes, (r + 1) * row_bytes) of its chunk's
 * plaintext, whatever typesize, filter and codec wrote the chunk.  row_bytes is 1 ... 65536; anything else answers a negative value.
 *
 * Census, before anything is decoded.  Every chunk's header passes the checks of blosc_getitem in its order (blosc/blosc.c:1603-1632:
 * -9 for the format version, -1 for the sizes, -5 / -9 for the codec, -1 for the block table), blosc_gpu_take_packed adds the slot
 * checks of blosc_gpu_getitem_packed (a slot that cannot hold a header, a header that claims more than its slot: -1), and a usable chunk's
 * nbytes is a multiple of row_bytes (-1 otherwise).  chunk_rows_out[i] is the chunk's row count, or that negative code.  A chunk of
 * nbytes 0 holds no rows (blosc.c:1606 leaves it no range to ask for; here it is a usable chunk without rows).  With any chunk unusable
 * the rows cannot be numbered: the call answers -1, decodes nothing and writes neither dest nor status (nor *failed_out).  nidx == 0 is
 * the census alone and answers 0.  MEMCPYED chunks are served from src + 16 (blosc.c:1678-1682) and decode nothing.
 *
 * Answers.  For 0 <= index[k] < nrows whose blocks all decode, the row's bytes are written at dest + k * row_bytes and
 * status[k] = row_bytes.  Any other index - every int64_t: -1, nrows, INT64_MIN, INT64_MAX - gets status[k] = -1 and nothing is written
 * for it.  A row that touches a block which does not decode gets the code of the first such block in block order (blosc.c:1689-1692: what
 * blosc_getitem answers for a range inside that block alone) and nothing is written for it; rows that touch only other blocks are
 * unaffected - the rule of blosc_gpu_getitem_batch.  *failed_out is the number of k with a negative status.  The call answers 0 whenever
 * the census passed and the device worked, whatever the rows' verdicts.
 *
 * Indices may repeat and come in any order; dest may have any alignment.  Nothing outside dest[0, nidx * row_bytes) and
 * status[0, nidx) is written.  status, chunk_rows_out and failed_out may be NULL.
 *
 * Synchronous, ordered on `stream` (a hipStream_t as void*, NULL = default stream).  A call synchronises with the host once for the
 * headers, once for the flags of the touched blocks and once per pass of 256 MiB of decoded blocks: 3 times where the touched blocks
 * hold up to 256 MiB, independent of nidx.
 */
#ifndef BLOSC_AMD_BLOSC_GPU_TAKE_H
#define BLOSC_AMD_BLOSC_GPU_TAKE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#ifndef BLOSC_EXPORT
#define BLOSC_EXPORT __attribute__((visibility("default")))
#endif

/* chunk i at src[i]; row index[k] -> dest + k * row_bytes */
BLOSC_EXPORT int blosc_gpu_take_batch(int nchunks, const void* const* src, size_t row_bytes,
                                      size_t nidx, const int64_t* index /* DEVICE [nidx] */,
                                      void* dest /* DEVICE, nidx * row_bytes */,
                                      int* status /* DEVICE [nidx], may be NULL */,
                                      int* chunk_rows_out /* HOST [nchunks], may be NULL */,
                                      size_t* failed_out /* HOST, may be NULL */, void* stream);

/* The same out of a packed container (include/blosc_gpu_packed.h): chunk i is the offsets[i + 1] - offsets[i] bytes at
 * container + offsets[i].  `offsets` not non-decreasing or offsets[nchunks] > containersize answers a negative value. */
BLOSC_EXPORT int blosc_gpu_take_packed(int nchunks, const void* container, size_t containersize,
                                       const size_t* offsets /* HOST [nchunks + 1] */, size_t row_bytes,
                                       size_t nidx, const int64_t* index, void* dest, int* status,
                                       int* chunk_rows_out, size_t* failed_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
