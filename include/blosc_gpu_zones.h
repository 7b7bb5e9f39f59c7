/* include/blosc_gpu_zones.h — zone maps: several fields aggregated in one decode, and where / aggregate that skip the chunks a zone map excludes.
 *
 * The per-chunk minimum and maximum of a field (include/blosc_gpu_aggregate.h: chunk_out) are a zone map of the container.  A range over a
 * column that grows with the row number - a time stamp, an id, anything appended in order - can match in one or two chunks only, and the
 * calls of include/blosc_gpu_clauses.h still decode all of them: decoding is the cost of such a call.  Three things here:
 *   blosc_gpu_aggregate_fields_*   the aggregates of up to 16 fields in ONE decode - a zone map over every column for the price of one;
 *   blosc_gpu_zone_excludes        the rule that says whether a chunk described by such entries can hold a row that passes a term list;
 *   blosc_gpu_where_zoned_*, blosc_gpu_aggregate_zoned_*   the clause calls, which do not decode the chunks the rule excludes.
 *
 * Everything that is not named here is that of include/blosc_gpu_where.h, include/blosc_gpu_aggregate.h and include/blosc_gpu_clauses.h and is
 * cited from there, not restated: HOST and DEVICE arguments; rows, their numbering and the census with its codes; chunk_rows_out; chunks that
 * do not decode; index_out, `capacity`, *total_out and the overlap rule; nchunks == 0; the passes and the synchronisations (2 + 2 x passes that
 * hold a live row; the tables go up with the call's and add none); blosc_gpu_field, blosc_gpu_aggregate and the order of the additions of the
 * floating-point sum; blosc_gpu_term and the meaning of a term list.
 *
 * Several fields.  chunk_out[i * nfields + f] and total_out[f] are, byte for byte, what blosc_gpu_aggregate_clauses_* answers for fields[f]
 * with the same terms on the same chunks - for every pass bound, every stream and both entry points; the binary64 sum is the tree of additions
 * blosc_gpu_aggregate.h documents.  The term list is evaluated once per row, whatever nfields.  Fields may overlap, repeat, or be tested by a
 * term.  chunk_status_out, chunk_rows_out and *unread_out are per chunk and per call, as there.  While a pass runs the library holds
 * 40 x nfields bytes per 1024 rows of it and 64 x nfields bytes per chunk of the call.
 * Answered from the arguments alone, with a negative value and NOTHING written: nfields outside 1 ... BLOSC_GPU_MAX_ZONE_FIELDS; fields NULL;
 * any field and any term list blosc_gpu_aggregate_clauses_* would refuse, and its whole-call checks.
 * nchunks == 0: every total_out[f] all zero with both rows -1, *unread_out = 0, the answer is 0.
 *
 * The rule (blosc_gpu_zone_excludes; the ONE statement of it - the zoned calls call this function per chunk).  `entry` holds one
 * blosc_gpu_aggregate per zone field, for one chunk of chunk_rows rows.
 *   Entry f INFORMS about zfields[f] only if all of these hold: rows == chunk_rows > 0; count == rows (it came from an unfiltered aggregate);
 *   and either both min_row, max_row >= 0 or nans == rows.  Anything else is no information and never excludes.
 *   A term uses the first informing entry whose field's (offset, bytes, kind) equal its own.  A term without one may be true.
 *   With lo and hi the keys of the entry's min and max in the order of blosc_gpu_where.h (integers by their signedness, IEEE 754 with
 *   -0 = +0) and k the constant's key, a term CAN BE TRUE iff
 *       the constant is a NaN, or every value is one (nans == rows):   the op is NE;
 *       LT  lo < k;    LE  lo <= k;    GT  hi > k;    GE  hi >= k;    EQ  lo <= k <= hi;
 *       NE  not (lo == hi == k and nans == 0).
 *   The chunk is excluded iff some clause that occurs in the list has no term that can be true.
 * The answer is 1 (no row of such a chunk can pass), 0 (one may) or negative: nterms outside 0 ... 16, nzfields outside 0 ... 16, a NULL
 * table with a count above 0, a term blosc_gpu_where_* would refuse for a reason other than the row's length, a zone field with a pad_ that is
 * not 0 or a kind / bytes pair outside the table.  Host only: the function touches no device and may be called from any thread.
 *
 * The zoned calls.  zones[i * nzfields + f] describes zfields[f] in chunk i - what blosc_gpu_aggregate_fields_* with no terms wrote for it.
 * After the census a chunk that holds rows and that the rule excludes is NOT DECODED: it takes no slot and joins no pass; the passes are dealt
 * over the other chunks.  It reports exactly what a decoded chunk without a match reports: chunk_matches_out[i] = 0; in aggregate the entry
 * {rows, 0, 0, -1, -1, 0, 0, 0} with status 0, and its rows count in total_out->rows.  chunk_pruned_out[i] (may be NULL) is 1 for such a chunk
 * and 0 for every other.  With no chunk left the call launches no kernel and answers 0.
 * With a TRUTHFUL map every output equals that of blosc_gpu_where_clauses_* / blosc_gpu_aggregate_clauses_* byte for byte - the index table,
 * the totals, the per-chunk tables, *unread_out - with one exception: an excluded chunk that would not have decoded reports 0 where the clause
 * call reports its negative code and counts its rows in *unread_out.
 * A STALE MAP IS THE CALLER'S RESPONSIBILITY.  The library cannot know that a chunk was rewritten after its entry was computed: an entry that
 * no longer describes its chunk makes the call skip rows that would pass.  Recompute the entries of every chunk a blosc_gpu_put_* call reports
 * in rewritten_out.  The one guard is cheap: an entry whose rows is not 0 and differs from the census' rows of its chunk makes the call answer
 * a negative value before anything is decoded, with nothing but chunk_rows_out written.
 * nzfields == 0 (zones may be NULL): the clause call, chunk_pruned_out all 0.
 * Answered from the arguments alone, with a negative value and NOTHING written: nzfields outside 0 ... BLOSC_GPU_MAX_ZONE_FIELDS; zfields or
 * zones NULL with nzfields > 0; a zone field blosc_gpu_aggregate_* would refuse; everything the clause call refuses.
 * The zoned aggregate aggregates one field, as the clause call does.  A chunk that certainly passes is decoded like any other.
 */
#ifndef BLOSC_AMD_BLOSC_GPU_ZONES_H
#define BLOSC_AMD_BLOSC_GPU_ZONES_H
#include <stddef.h>
#include <stdint.h>
#include "blosc_gpu_clauses.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { BLOSC_GPU_MAX_ZONE_FIELDS = 16 };

/* blosc_gpu_aggregate_clauses_batch for nfields fields: chunk i at src[i] */
BLOSC_EXPORT int blosc_gpu_aggregate_fields_batch(int nchunks, const void* const* src, size_t row_bytes,
                                                  const blosc_gpu_field* fields /* HOST [nfields] */, int nfields /* 1 ... 16 */,
                                                  const blosc_gpu_term* terms /* HOST [nterms]; NULL with nterms 0: every row */, int nterms,
                                                  blosc_gpu_aggregate* total_out /* HOST [nfields], may be NULL */,
                                                  blosc_gpu_aggregate* chunk_out /* HOST [nchunks * nfields], chunk-major, may be NULL */,
                                                  int* chunk_status_out, int* chunk_rows_out, size_t* unread_out, void* stream);

/* the same out of a packed container */
BLOSC_EXPORT int blosc_gpu_aggregate_fields_packed(int nchunks, const void* container, size_t containersize,
                                                   const size_t* offsets /* HOST [nchunks + 1] */, size_t row_bytes,
                                                   const blosc_gpu_field* fields, int nfields, const blosc_gpu_term* terms, int nterms,
                                                   blosc_gpu_aggregate* total_out, blosc_gpu_aggregate* chunk_out, int* chunk_status_out,
                                                   int* chunk_rows_out, size_t* unread_out, void* stream);

/* 1: no row of a chunk described by `entry` can pass the list; 0: it may; negative: bad arguments.  Host only, touches no device. */
BLOSC_EXPORT int blosc_gpu_zone_excludes(const blosc_gpu_term* terms, int nterms, const blosc_gpu_field* zfields, int nzfields,
                                         const blosc_gpu_aggregate* entry /* [nzfields], one chunk's */, uint64_t chunk_rows);

/* blosc_gpu_where_clauses_batch, skipping the chunks the map excludes */
BLOSC_EXPORT int blosc_gpu_where_zoned_batch(int nchunks, const void* const* src, size_t row_bytes,
                                             const blosc_gpu_term* terms /* HOST [nterms] */, int nterms /* 1 ... 16 */,
                                             const blosc_gpu_field* zfields /* HOST [nzfields] */, int nzfields /* 0 ... 16 */,
                                             const blosc_gpu_aggregate* zones /* HOST [nchunks * nzfields], chunk-major; NULL only with nzfields 0 */,
                                             int64_t* index_out, size_t capacity, size_t* total_out, int* chunk_matches_out, int* chunk_rows_out,
                                             size_t* unread_out, uint8_t* chunk_pruned_out /* HOST [nchunks], may be NULL */, void* stream);

BLOSC_EXPORT int blosc_gpu_where_zoned_packed(int nchunks, const void* container, size_t containersize,
                                              const size_t* offsets /* HOST [nchunks + 1] */, size_t row_bytes,
                                              const blosc_gpu_term* terms, int nterms, const blosc_gpu_field* zfields, int nzfields,
                                              const blosc_gpu_aggregate* zones, int64_t* index_out, size_t capacity, size_t* total_out,
                                              int* chunk_matches_out, int* chunk_rows_out, size_t* unread_out, uint8_t* chunk_pruned_out,
                                              void* stream);

/* blosc_gpu_aggregate_clauses_batch, skipping the chunks the map excludes */
BLOSC_EXPORT int blosc_gpu_aggregate_zoned_batch(int nchunks, const void* const* src, size_t row_bytes,
                                                 const blosc_gpu_field* field /* HOST */,
                                                 const blosc_gpu_term* terms /* HOST [nterms]; NULL with nterms 0: every row */, int nterms,
                                                 const blosc_gpu_field* zfields, int nzfields, const blosc_gpu_aggregate* zones,
                                                 blosc_gpu_aggregate* total_out, blosc_gpu_aggregate* chunk_out, int* chunk_status_out,
                                                 int* chunk_rows_out, size_t* unread_out, uint8_t* chunk_pruned_out, void* stream);

BLOSC_EXPORT int blosc_gpu_aggregate_zoned_packed(int nchunks, const void* container, size_t containersize,
                                                  const size_t* offsets /* HOST [nchunks + 1] */, size_t row_bytes,
                                                  const blosc_gpu_field* field, const blosc_gpu_term* terms, int nterms,
                                                  const blosc_gpu_field* zfields, int nzfields, const blosc_gpu_aggregate* zones,
                                                  blosc_gpu_aggregate* total_out, blosc_gpu_aggregate* chunk_out, int* chunk_status_out,
                                                  int* chunk_rows_out, size_t* unread_out, uint8_t* chunk_pruned_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
