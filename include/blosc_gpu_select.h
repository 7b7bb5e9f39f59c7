/* include/blosc_gpu_select.h — trial compression: several parameter sets per chunk, the smallest result is kept.
 *
 * blosc_gpu_compress_batch_params and blosc_gpu_compress_packed_params (include/blosc_gpu_params.h) write what the caller names, one
 * parameter set per chunk.  Which filter or codec is best for an array is not predictable from its dtype - byte shuffle wins on
 * floats, bitshuffle on small integers, no filter on text-like bytes, Zstd on some columns only - so a caller who does not know the
 * data compresses the batch once per setting and compares size tables on the host.  Here chunk i comes with a LIST of candidate
 * parameter sets, cands[cand_first[i] .. cand_first[i + 1]): every candidate is encoded, the sizes are compared on the device, and
 * only the winner is written, once, in the caller's order - one call, one host synchronisation.
 *
 * Conventions are those of include/blosc_gpu_params.h: `cand_first`, `cands`, pointer and size arrays are HOST arrays; src[i], dest[i]
 * and the packed dest are DEVICE (or managed) memory on the current device; the calls are synchronous and ordered on `stream` (a
 * hipStream_t as void*, NULL = default stream).  nchunks == 0 returns 0.
 *
 * Answer.  The answer of candidate c of chunk i is what blosc_gpu_compress_batch_params reports for that chunk with cands[c] and
 * destsize[i] - in the packed form what blosc_gpu_compress_packed_params reports, that is destsize = nbytes[i] + 16 - with the
 * MEMCPYED fallback, the -10 / -5 errors of an unusable row, and 0 for "does not fit".
 *
 * Winner.  The candidate with the smallest positive answer; on a tie the lowest index.  choice_out[i] is its index relative to
 * cand_first[i], cbytes_out[i] its answer, and the bytes at dest[i] (or in the container) are the bytes that call writes: byte for
 * byte for the deterministic settings ("blosclz", "lz4", "zstd" up to clevel 5), a valid chunk of that setting of cbytes_out[i] bytes
 * for the others.  Nothing of a loser is ever written to caller memory.
 *
 * No positive answer.  choice_out[i] = -1 and cbytes_out[i] is the first candidate's answer (its error code, or 0); a chunk with no
 * candidates answers -10.  The destination stays untouched; in the packed form the chunk takes 0 bytes.
 *
 * cand_cbytes_out (optional, [cand_first[nchunks]]) receives every candidate's answer as found in this call, losers included; for
 * the settings that are not deterministic these are this call's sizes.  The winner is always the minimum of this table under the tie
 * rule.
 *
 * Packed form.  blosc_gpu_compress_packed's layout rule over the winners, in the caller's order; dest == NULL is the sizing call.  A
 * winner that would end behind destsize gets cbytes_out[i] = 0 and still counts in the offsets, while choice_out and cand_cbytes_out
 * keep what was found.  The bytes between a written chunk and the next offset are zeroed as before.
 *
 * The calls return 0, or a negative value - every output untouched - if the device could not be used or an argument is unusable as a
 * whole: a NULL table (cand_cbytes_out apart), cand_first[0] != 0, a cand_first entry that decreases, an unusable `align`.
 *
 * With exactly one candidate per chunk, results and bytes are those of the calls of include/blosc_gpu_params.h.
 *
 * Cost.  A chunk is encoded once per candidate.  The workspace holds a staging slot of nbytes[i] per candidate, and a filtered image
 * of nbytes[i] for every candidate with a filter; a call whose workspace cannot be allocated returns -1.
 */
#ifndef BLOSC_AMD_BLOSC_GPU_SELECT_H
#define BLOSC_AMD_BLOSC_GPU_SELECT_H
#include <stddef.h>
#include "blosc_gpu_params.h"
#ifdef __cplusplus
extern "C" {
#endif

/* blosc_gpu_compress_batch_params with the candidates cands[cand_first[i] .. cand_first[i + 1]) for chunk i; cand_first: [nchunks + 1],
 * cand_first[0] == 0, non-decreasing */
BLOSC_EXPORT int blosc_gpu_compress_batch_select(int nchunks, const int* cand_first, const blosc_gpu_cparams* cands,
                                                 const void* const* src, const size_t* nbytes, void* const* dest, const size_t* destsize,
                                                 int* cbytes_out /* [nchunks] */, int* choice_out /* [nchunks] */,
                                                 int* cand_cbytes_out /* [cand_first[nchunks]] or NULL */, void* stream);

/* blosc_gpu_compress_packed_params with the same candidate tables */
BLOSC_EXPORT int blosc_gpu_compress_packed_select(int nchunks, const int* cand_first, const blosc_gpu_cparams* cands,
                                                  const void* const* src, const size_t* nbytes,
                                                  void* dest /* may be NULL */, size_t destsize, size_t align,
                                                  size_t* offsets_out /* [nchunks + 1] */, int* cbytes_out /* [nchunks] */,
                                                  int* choice_out /* [nchunks] */, int* cand_cbytes_out /* or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
