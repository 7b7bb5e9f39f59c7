/* include/blosc_gpu_where.h — the rows of device-resident compressed chunks whose field satisfies a predicate, as an index table on the device.
 *
 * torch.nonzero(op(table[:, column], value)) for a table that is kept compressed: the rows whose key equals k, the entries older than t,
 * the weights above a threshold.  The calls of include/blosc_gpu_take.h and include/blosc_gpu_put.h read such a table of row numbers from
 * device memory; these calls write it.  Without them a lookup by value decodes the whole container (blosc_gpu_decompress_packed), holds
 * all of its plaintext and compares it there.  Here the chunks are decoded pass by pass, each row's field is compared with a constant
 * where it was decoded, and only the numbers of the matching rows are kept: select-by-value, gather and update stay on the device.
 *
 * Conventions, rows and the census are those of include/blosc_gpu_take.h: src, offsets, pred and every *_out argument are HOST memory,
 * src[i], container and index_out DEVICE (or managed) memory on the current device.  The chunks of a call are ONE array of rows of
 * row_bytes bytes (1 ... 65536), chunk i holding nbytes_i / row_bytes of them, numbered as take numbers them; every chunk passes the header
 * checks of blosc_getitem in its order (blosc/blosc.c:1603-1632) and, in the packed form, the slot checks, and its nbytes is a multiple of
 * row_bytes.  A chunk of nbytes 0 has no rows.  chunk_rows_out[i] is the chunk's rows or its negative code.  With any chunk unusable the
 * call answers -1, decodes nothing and writes none of index_out, *total_out, chunk_matches_out and *unread_out.
 *
 * Arguments.  Answered from the arguments alone, with a negative value and NOTHING written (chunk_rows_out neither): pred NULL; op outside
 * 0 ... 5; a kind / bytes pair that is not in the table below; offset + bytes > row_bytes; row_bytes outside 1 ... 65536; capacity > 0
 * with index_out NULL; and take's: a negative count, NULL tables, an offset table that decreases or ends behind the container.  Once the
 * headers are known: [index_out, index_out + capacity) overlaps the container or any src[i] chunk - a negative value, nothing written.
 *
 * The predicate.  The field of row r is bytes [offset, offset + bytes) of the row, at whatever address that is: nothing is assumed about
 * alignment.  It is read as `kind` and the test is  field op value:
 *   BLOSC_GPU_FIELD_UINT / _INT   bytes 1, 2, 4, 8   integers of their signedness
 *   BLOSC_GPU_FIELD_FLOAT         bytes 2 (binary16), 4, 8
 *   BLOSC_GPU_FIELD_BFLOAT16      bytes 2
 * The floating-point kinds compare as IEEE 754: every comparison with a NaN on either side is false, except NE, which is true; -0 equals
 * +0; subnormals are numbers; binary16 and bfloat16 are widened exactly to binary32 before they are compared (widening keeps the order,
 * so no value is rounded anywhere).  The typesize, filter and codec that wrote a chunk play no part.
 *
 * Output.  The numbers of the matching rows, ascending, go to index_out[0], index_out[1], ...  *total_out is the number of matches whatever
 * the capacity; beyond `capacity` the first `capacity` of them are written, and nothing at or behind index_out + min(total, capacity) is
 * written.  chunk_matches_out[i] is the number of matches in chunk i.  The same call gives the same table: no order depends on timing.
 *
 * Chunks that do not decode.  A chunk for which blosc_decompress would answer a negative value (blosc.c:1511-1514) contributes no matches,
 * chunk_matches_out[i] is that negative value and its rows are counted in *unread_out.  The other chunks are unaffected and the call still
 * answers 0 - the rule of blosc_gpu_put_batch for a touched chunk.  MEMCPYED chunks go through the decoder like any other.
 *
 * nchunks == 0: *total_out = 0, *unread_out = 0, the answer is 0.  capacity == 0 (index_out may then be NULL): the count alone.
 *
 * Synchronous, ordered on `stream` (a hipStream_t as void*, NULL = default stream).  The chunks that hold rows are dealt, in their order,
 * to passes of at most 256 MiB of plaintext (a larger chunk is a pass of its own).  A call synchronises with the host once for the headers,
 * twice per pass (the decoder's headers and verdicts) and once at its end: 2 + 2 x passes, whatever the number of rows and of matches -
 * the running total is carried from pass to pass on the device.  While a pass runs the library holds, besides the decoder's workspace,
 * the plaintext of the pass's chunks and 140 bytes per 1024 rows of it (one mask bit per row, a count and a base per 1024 rows).
 */
#ifndef BLOSC_AMD_BLOSC_GPU_WHERE_H
#define BLOSC_AMD_BLOSC_GPU_WHERE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#ifndef BLOSC_EXPORT
#define BLOSC_EXPORT __attribute__((visibility("default")))
#endif

enum { BLOSC_GPU_WHERE_EQ = 0, BLOSC_GPU_WHERE_NE, BLOSC_GPU_WHERE_LT, BLOSC_GPU_WHERE_LE, BLOSC_GPU_WHERE_GT, BLOSC_GPU_WHERE_GE };
enum { BLOSC_GPU_FIELD_UINT = 0, BLOSC_GPU_FIELD_INT, BLOSC_GPU_FIELD_FLOAT, BLOSC_GPU_FIELD_BFLOAT16 };
typedef struct {
  uint32_t offset;    /* of the field inside a row, bytes */
  uint32_t bytes;     /* UINT / INT: 1, 2, 4, 8;  FLOAT: 2 (binary16), 4, 8;  BFLOAT16: 2 */
  int32_t  kind, op;
  uint8_t  value[8];  /* the constant, in the field's own little-endian representation, `bytes` bytes of it */
} blosc_gpu_predicate;

/* chunk i at src[i] */
BLOSC_EXPORT int blosc_gpu_where_batch(int nchunks, const void* const* src, size_t row_bytes,
                                       const blosc_gpu_predicate* pred /* HOST */,
                                       int64_t* index_out /* DEVICE [capacity]; may be NULL only with capacity 0 */, size_t capacity,
                                       size_t* total_out /* HOST, may be NULL */,
                                       int* chunk_matches_out /* HOST [nchunks], may be NULL */,
                                       int* chunk_rows_out /* HOST [nchunks], may be NULL */,
                                       size_t* unread_out /* HOST, may be NULL */, void* stream);

/* The same out of a packed container (include/blosc_gpu_packed.h): chunk i is the offsets[i + 1] - offsets[i] bytes at
 * container + offsets[i].  `offsets` not non-decreasing or offsets[nchunks] > containersize answers a negative value. */
BLOSC_EXPORT int blosc_gpu_where_packed(int nchunks, const void* container, size_t containersize,
                                        const size_t* offsets /* HOST [nchunks + 1] */, size_t row_bytes,
                                        const blosc_gpu_predicate* pred, int64_t* index_out, size_t capacity,
                                        size_t* total_out, int* chunk_matches_out, int* chunk_rows_out, size_t* unread_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
