/* include/blosc_gpu_params.h — the batched device compress calls with parameters PER CHUNK.
 *
 * blosc_gpu_compress_batch and blosc_gpu_compress_packed take one clevel, filter, typesize, compressor and blocksize for the whole
 * batch, while the read side (blosc_gpu_decompress_batch / _packed, the getitem calls) takes chunks of any format, typesize and filter
 * in one call.  What callers write is mixed by nature - the columns of a table, the tensors of a state dict: float32, bfloat16 and int8
 * side by side, often with a codec or filter per array - and with one parameter set per call that is one call, one synchronisation and
 * one container per distinct setting.  Here chunk i is compressed with params[i], the whole batch in ONE call with ONE host
 * synchronisation, however many settings it holds; the packed form writes one container in the caller's order.
 *
 * Conventions are those of include/blosc_gpu.h and include/blosc_gpu_packed.h: `params`, pointer and size arrays are HOST arrays;
 * src[i], dest[i] and the packed dest are DEVICE (or managed) memory on the current device; the calls are synchronous and ordered on
 * `stream` (a hipStream_t as void*, NULL = default stream).  They return 0, or a negative value if the device could not be used or an
 * argument is unusable as a whole: a NULL `params` table, and what the call's single-parameter form rejects (nchunks < 0, another NULL
 * table, an unusable `align`).  nchunks == 0 returns 0.
 *
 * Chunk i gets exactly what the existing call gives a chunk compressed with params[i]: the same return value in cbytes_out[i], the
 * same header, the same rules for destsize and for the bytes that stay untouched.  For the deterministic settings - "blosclz", "lz4",
 * and "zstd" up to clevel 5 - the bytes are, byte for byte, the ones blosc_gpu_compress_batch / blosc_gpu_compress_packed writes for
 * that chunk with those parameters.  The packed form keeps blosc_gpu_compress_packed's layout rule, over all chunks in the caller's
 * order, whatever their settings.
 *
 * An error belongs to its chunk alone; its neighbours are written as if it were not there:
 *   a clevel, doshuffle or typesize that blosc_compress_ctx rejects, or a splitmode outside 0 ... 4   cbytes_out[i] = -10
 *   a compcode that is not built (BLOSC_SNAPPY, any unknown code)                                     cbytes_out[i] = -5
 * and in the packed call both take 0 bytes.  (In the single-parameter calls an unusable compressor fails every chunk, because it is
 * every chunk's compressor; here it is one chunk's.)
 * Several candidate rows per chunk, of which the smallest result is written: include/blosc_gpu_select.h.
 */
#ifndef BLOSC_AMD_BLOSC_GPU_PARAMS_H
#define BLOSC_AMD_BLOSC_GPU_PARAMS_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#ifndef BLOSC_EXPORT
#define BLOSC_EXPORT __attribute__((visibility("default")))
#endif

typedef struct blosc_gpu_cparams {
  int clevel;        /* 0 ... 9 */
  int doshuffle;     /* BLOSC_NOSHUFFLE / BLOSC_SHUFFLE / BLOSC_BITSHUFFLE */
  int compcode;      /* BLOSC_BLOSCLZ ... BLOSC_ZSTD (include/blosc.h); -1 = the global compressor (blosc_set_compressor) */
  int splitmode;     /* BLOSC_ALWAYS_SPLIT ... BLOSC_FORWARD_COMPAT_SPLIT; 0 = the global one (blosc_set_splitmode).  The reference has
                        no per-call split mode - blosc_compress_ctx reads the global - so this field has no counterpart there. */
  size_t typesize;
  size_t blocksize;  /* 0 = automatic (then the global forced blocksize, blosc_set_blocksize, as in the existing calls) */
} blosc_gpu_cparams;

/* blosc_gpu_compress_batch (include/blosc_gpu.h) with params[i] for chunk i */
BLOSC_EXPORT int blosc_gpu_compress_batch_params(int nchunks, const blosc_gpu_cparams* params, const void* const* src, const size_t* nbytes,
                                                 void* const* dest, const size_t* destsize, int* cbytes_out, void* stream);

/* blosc_gpu_compress_packed (include/blosc_gpu_packed.h) with params[i] for chunk i */
BLOSC_EXPORT int blosc_gpu_compress_packed_params(int nchunks, const blosc_gpu_cparams* params, const void* const* src, const size_t* nbytes,
                                                  void* dest, size_t destsize, size_t align,
                                                  size_t* offsets_out /* [nchunks + 1] */, int* cbytes_out /* [nchunks] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
