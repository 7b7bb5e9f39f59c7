/* include/blosc_gpu_clauses.h — where and aggregate with SEVERAL field tests per row: an AND of OR clauses, evaluated in one decode.
 *
 * torch.nonzero((t0 <= stamp) & (stamp < t1)), (stamp >= t0) & (kind == 3), (key == a) | (key == b) | (key == c) for a table that is kept
 * compressed.  blosc_gpu_where_* and the filter of blosc_gpu_aggregate_* test ONE field against ONE constant; a range, two fields or a small
 * key set took one call per comparison - each of which decodes the whole container again, and decoding is the cost of such a call - and an
 * intersection of index tables outside the library.  These calls decode once and test every term on the row where it was decoded.
 *
 * Everything that is not the term list is that of include/blosc_gpu_where.h and include/blosc_gpu_aggregate.h and is cited from there, not
 * restated: which arguments are HOST and which DEVICE memory; rows, their numbering and the census with its codes; chunk_rows_out; chunks that
 * do not decode (chunk_matches_out / chunk_status_out, *unread_out, the answer 0); index_out, `capacity`, *total_out and the overlap rule
 * for index_out; nchunks == 0; the passes, the workspace per 1024 rows and the synchronisations - 2 + 2 x passes that hold a row: the term
 * list goes up with the call's tables and adds none; blosc_gpu_aggregate, its count / nans / min / max / sum and the determinism of the
 * floating-point sum: chunk_out[i] is a function of chunk i's plaintext, row_bytes, field and the SET OF ROWS the list lets through, and
 * the order of the additions is the tree documented there.
 *
 * The term list.  terms[0 ... nterms - 1], HOST memory.  A term is one test of blosc_gpu_where.h - field `op` constant, of any kind, at any
 * offset, each term its own - and the number of the clause it belongs to, 0 ... 15.  A row passes when EVERY clause number that occurs in
 * the list has AT LEAST ONE term of that number whose test is true:
 *   a conjunction   n terms with n different clause numbers;
 *   a disjunction   n terms with one clause number;
 *   a range         two terms on one field in two clauses: {f GE t0, clause 0}, {f LT t1, clause 1};
 *   a range with a key set   {f GE t0, 0}, {f LT t1, 1}, {k EQ a, 2}, {k EQ b, 2}, {k EQ c, 2}.
 * Clause numbers need not be contiguous and the terms of a clause need not be adjacent.  The order of the terms, which numbers name the
 * clauses and a term given twice never change an answer.
 * Each test has where's semantics unchanged: a comparison with a NaN on either side is false, except NE; -0 equals +0; binary16 and bfloat16
 * are compared as their widened values; the alignment of a field plays no part.  So {f LT c, 0}, {f GE c, 0} selects exactly the rows whose
 * f is no NaN.
 * A field that several terms test - and in aggregate the aggregated field, when a term tests it - is read once per row.
 *
 * Arguments.  Answered from the arguments alone, with a negative value and NOTHING written (chunk_rows_out neither):
 *   blosc_gpu_where_clauses_*       terms NULL; nterms outside 1 ... BLOSC_GPU_MAX_TERMS;
 *   blosc_gpu_aggregate_clauses_*   nterms outside 0 ... BLOSC_GPU_MAX_TERMS; terms NULL with nterms > 0; terms not NULL with nterms 0;
 *   both   a clause above 15; a pad_ that is not 0; any term that blosc_gpu_where_* would refuse (an op outside 0 ... 5, a kind / bytes pair
 *          outside where's table, a field that ends behind the row); and the whole-call checks of blosc_gpu_where_* and of
 *          blosc_gpu_aggregate_* respectively.
 * blosc_gpu_aggregate_clauses_* with nterms 0 (terms NULL) aggregates every row, as blosc_gpu_aggregate_* does with filter NULL.
 */
#ifndef BLOSC_AMD_BLOSC_GPU_CLAUSES_H
#define BLOSC_AMD_BLOSC_GPU_CLAUSES_H
#include <stddef.h>
#include <stdint.h>
#include "blosc_gpu_where.h"
#include "blosc_gpu_aggregate.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { BLOSC_GPU_MAX_TERMS = 16 };
typedef struct {                 /* 32 bytes */
  blosc_gpu_predicate test;      /* field `op` constant, exactly as blosc_gpu_where.h defines it */
  uint32_t clause;               /* 0 ... 15: the clause this term belongs to */
  uint32_t pad_;                 /* 0 */
} blosc_gpu_term;

/* blosc_gpu_where_batch with a term list in the predicate's place: chunk i at src[i] */
BLOSC_EXPORT int blosc_gpu_where_clauses_batch(int nchunks, const void* const* src, size_t row_bytes,
                                               const blosc_gpu_term* terms /* HOST [nterms] */, int nterms /* 1 ... 16 */,
                                               int64_t* index_out /* DEVICE [capacity]; may be NULL only with capacity 0 */, size_t capacity,
                                               size_t* total_out, int* chunk_matches_out, int* chunk_rows_out, size_t* unread_out, void* stream);

/* blosc_gpu_where_packed with a term list in the predicate's place */
BLOSC_EXPORT int blosc_gpu_where_clauses_packed(int nchunks, const void* container, size_t containersize,
                                                const size_t* offsets /* HOST [nchunks + 1] */, size_t row_bytes,
                                                const blosc_gpu_term* terms, int nterms, int64_t* index_out, size_t capacity,
                                                size_t* total_out, int* chunk_matches_out, int* chunk_rows_out, size_t* unread_out, void* stream);

/* blosc_gpu_aggregate_batch with a term list in the filter's place: chunk i at src[i] */
BLOSC_EXPORT int blosc_gpu_aggregate_clauses_batch(int nchunks, const void* const* src, size_t row_bytes,
                                                   const blosc_gpu_field* field /* HOST */,
                                                   const blosc_gpu_term* terms /* HOST [nterms]; NULL with nterms 0: every row */, int nterms,
                                                   blosc_gpu_aggregate* total_out, blosc_gpu_aggregate* chunk_out, int* chunk_status_out,
                                                   int* chunk_rows_out, size_t* unread_out, void* stream);

/* blosc_gpu_aggregate_packed with a term list in the filter's place */
BLOSC_EXPORT int blosc_gpu_aggregate_clauses_packed(int nchunks, const void* container, size_t containersize,
                                                    const size_t* offsets /* HOST [nchunks + 1] */, size_t row_bytes,
                                                    const blosc_gpu_field* field, const blosc_gpu_term* terms, int nterms,
                                                    blosc_gpu_aggregate* total_out, blosc_gpu_aggregate* chunk_out, int* chunk_status_out,
                                                    int* chunk_rows_out, size_t* unread_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
