/* include/blosc_gpu_aggregate.h — count, sum, min and max of a row field of device-resident compressed chunks, per chunk and for the call.
 *
 * table[mask, column].sum() / .min() / .max() / mask.sum() for a table that is kept compressed: how many rows match, the sum of a column over
 * the matching rows, the extreme of a column and the row that holds it.  Without these calls that is blosc_gpu_where_* into an index table
 * of 8 bytes per match, blosc_gpu_take_* of those rows and a reduction over the copy.  Here the chunks are decoded pass by pass, every row's
 * field is reduced where it was decoded, and 64 bytes per chunk come back: no plaintext is kept and no index table is written.  The
 * per-chunk minimum and maximum of a field are a zone map of the container.
 *
 * Everything shared is that of include/blosc_gpu_where.h and cited from there: src, offsets, field, filter and every *_out argument are HOST
 * memory, src[i] and container DEVICE (or managed) memory on the current device; the chunks of a call are ONE array of rows of row_bytes
 * bytes (1 ... 65536), numbered as take numbers them; the census with its chunk header checks and, in the packed form, slot checks;
 * chunk_rows_out[i], the chunk's rows or its negative code; the kind / bytes table of a field; the passes and the synchronisations.
 * Every output is host memory, so there is no overlap rule.
 *
 * Arguments.  Answered from the arguments alone, with a negative value and NOTHING written (chunk_rows_out neither): field NULL; field->pad_
 * not 0; a kind / bytes pair that is not in where's table; field->offset + field->bytes > row_bytes; a non-NULL filter that
 * blosc_gpu_where_* would refuse (an op outside 0 ... 5, a pair outside the table, a field that ends behind the row); and where's whole-call
 * checks that do not concern index_out: row_bytes outside 1 ... 65536, a negative count, NULL tables, an offset table that decreases or
 * ends behind the container.  With any chunk unusable (the census) the call answers -1, fills chunk_rows_out as where does and writes
 * nothing else.
 *
 * Filter.  With a filter only the rows whose filter field passes are aggregated.  The filter's field is any field of the row, of any kind; it
 * need not be the aggregated one.  Its semantics are exactly those of blosc_gpu_where_*: every comparison with a NaN on either side is false,
 * except NE; -0 equals +0; subnormals are numbers.  filter NULL: every row.
 *
 * count and nans.  rows: the rows that were read (their chunk decoded).  count: of them, the rows that pass the filter.  nans: of those, the
 * floating-point fields that hold a NaN; they are left out of min, max and sum.  For the integer kinds nans is 0.
 *
 * min and max range over the values that pass the filter and are no NaN, in the order of one key per type: integers by their signedness,
 * floating point in the IEEE 754 order with -0 = +0; subnormals and infinities are numbers.  min_row and max_row are the LOWEST row number
 * (take's numbering over the call) that attains the extreme, min[] and max[] that row's `bytes` bytes as they lie in the row, the rest 0: a
 * table with -0 in row 3 and +0 in row 9 reports -0 for both.  With no such value min_row = max_row = -1 and min[], max[] are all 0.
 *
 * sum.  UINT: the sum modulo 2^64 in sum.u.  INT: the two's-complement sum modulo 2^64 in sum.i.  The floating-point kinds widen every value
 * that is no NaN exactly to binary64 - binary16 and bfloat16 subnormals included, whatever the floating-point mode of the device - and add
 * in binary64 into sum.f.  That is IEEE arithmetic: +inf and -inf together give a NaN, overflow gives an infinity.  The sum of no values
 * is 0; the sign of a floating-point sum that is zero is unspecified.
 *
 * Determinism of the floating-point sum.  chunk_out[i] is a function of chunk i's plaintext, row_bytes, field and filter alone (its two row
 * numbers offset by the chunk's first row): it does not depend on the other chunks of the call, on the pass bound, on the entry point, on the
 * stream or on the grid.  The order of the additions inside a chunk is fixed by the chunk's number of rows: tiles of 1024 rows, inside a tile
 * lane l of 256 adds rows l, l + 256, l + 512, l + 768 in this order, the lanes of a wave are folded by a butterfly (l with l ^ 32, ^ 16,
 * ... ^ 1, the lower lane's operand in front), the four waves in their order; over the tiles of a chunk lane l adds tiles l, l + 256, ...
 * and the same tree follows.  There are no floating-point atomics.  total_out is the left fold of chunk_out[0], chunk_out[1], ... in chunk
 * order, done on the host: rows, counts and sums are added, the smaller min wins and on a tie the earlier chunk, max the same with the larger
 * value.  The same call gives the same 64 bytes, bit for bit.
 *
 * Chunks that do not decode.  A chunk for which blosc_decompress would answer a negative value: chunk_status_out[i] is that value (0 for
 * every other chunk), chunk_out[i] is all zero with both rows -1, and its rows are counted in *unread_out and not in total_out->rows.  The
 * other chunks are unaffected and the call still answers 0 - where's rule.  A chunk of nbytes 0 has all zero, rows -1 and status 0.
 *
 * nchunks == 0: *total_out all zero with both rows -1, *unread_out = 0, the answer is 0.
 *
 * Synchronous, ordered on `stream` (a hipStream_t as void*, NULL = default stream).  Passes are where's; a call synchronises with the host
 * 2 + 2 x passes times (passes that hold a row).  While a pass runs the library holds, besides the decoder's workspace, the plaintext of the
 * pass's chunks, 40 bytes per 1024 rows of it (one partial per tile of 1024 rows of a chunk) and 64 bytes per chunk of the call.
 */
#ifndef BLOSC_AMD_BLOSC_GPU_AGGREGATE_H
#define BLOSC_AMD_BLOSC_GPU_AGGREGATE_H
#include <stddef.h>
#include <stdint.h>
#include "blosc_gpu_where.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint32_t offset;    /* of the field inside a row, bytes */
  uint32_t bytes;     /* the kind / bytes table of blosc_gpu_where.h */
  int32_t  kind;      /* BLOSC_GPU_FIELD_* */
  int32_t  pad_;      /* 0 */
} blosc_gpu_field;

typedef struct {                       /* 64 bytes */
  uint64_t rows;                       /* rows that were read (their chunk decoded) */
  uint64_t count;                      /* of them, rows that pass the filter */
  uint64_t nans;                       /* of those, floating-point fields holding a NaN: left out of min, max and sum */
  int64_t  min_row, max_row;           /* the call's row number (take's numbering) of the LOWEST row holding the extreme; -1: none */
  uint8_t  min[8], max[8];             /* that row's field, its own little-endian representation, `bytes` bytes, rest 0 */
  union { int64_t i; uint64_t u; double f; } sum;
} blosc_gpu_aggregate;

/* chunk i at src[i] */
BLOSC_EXPORT int blosc_gpu_aggregate_batch(int nchunks, const void* const* src, size_t row_bytes,
                                           const blosc_gpu_field* field /* HOST */,
                                           const blosc_gpu_predicate* filter /* HOST, NULL: every row */,
                                           blosc_gpu_aggregate* total_out /* HOST, may be NULL */,
                                           blosc_gpu_aggregate* chunk_out /* HOST [nchunks], may be NULL */,
                                           int* chunk_status_out /* HOST [nchunks], may be NULL */,
                                           int* chunk_rows_out /* HOST [nchunks], may be NULL */,
                                           size_t* unread_out /* HOST, may be NULL */, void* stream);

/* The same out of a packed container (include/blosc_gpu_packed.h): chunk i is the offsets[i + 1] - offsets[i] bytes at
 * container + offsets[i].  `offsets` not non-decreasing or offsets[nchunks] > containersize answers a negative value. */
BLOSC_EXPORT int blosc_gpu_aggregate_packed(int nchunks, const void* container, size_t containersize,
                                            const size_t* offsets /* HOST [nchunks + 1] */, size_t row_bytes,
                                            const blosc_gpu_field* field, const blosc_gpu_predicate* filter,
                                            blosc_gpu_aggregate* total_out, blosc_gpu_aggregate* chunk_out, int* chunk_status_out,
                                            int* chunk_rows_out, size_t* unread_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
