/* include/blosc_gpu_packed.h — the batched device calls of include/blosc_gpu.h with the whole batch in ONE device buffer.
 *
 * blosc_gpu_compress_batch wants a destination per chunk, and a compress that must not fail wants nbytes[i] + 16 bytes for each: as
 * much destination memory as input, for a payload a small fraction of it.  What a writer, an exchange or a cache wants instead is the
 * chunks back to back with an offset table.  The engine chooses a chunk's final place after its size is known (the encoders write into a
 * scratch, one compaction pass writes the destination), so that layout costs no extra pass over the data: a prefix sum over the chunks'
 * sizes on the device sets every chunk's place inside one caller buffer.  blosc_gpu_decompress_packed is the reverse: it reads the
 * decoded sizes from the headers in device memory itself and decodes the chunks back to back.
 *
 * Conventions are those of include/blosc_gpu.h: pointer and size arrays are HOST arrays; src[i], dest and container are DEVICE (or
 * managed) memory on the current device; the calls are synchronous and ordered on `stream` (a hipStream_t as void*, NULL = default
 * stream).  They return 0, or a negative value if the device could not be used or an argument is unusable as a whole: `align` not a
 * power of two in 1 ... 4096 (0 means 1), a NULL table, `offsets` not non-decreasing, offsets[nchunks] > containersize.
 */
#ifndef BLOSC_AMD_BLOSC_GPU_PACKED_H
#define BLOSC_AMD_BLOSC_GPU_PACKED_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#ifndef BLOSC_EXPORT
#define BLOSC_EXPORT __attribute__((visibility("default")))
#endif

/* sum over i of align_up(nbytes[i] + 16, align): a dest of this size takes every chunk (0 for an unusable `align`) */
BLOSC_EXPORT size_t blosc_gpu_packed_bound(int nchunks, const size_t* nbytes, size_t align);

/* Batched blosc_compress_ctx into one buffer.  Chunk i is what blosc_compress_ctx returns for destsize = nbytes[i] + 16 - it never
 * answers 0 for lack of room of its own, incompressible input becomes a MEMCPYED chunk, a parameter error keeps its negative code and
 * takes 0 bytes - and, for "blosclz", "lz4" and "zstd" up to clevel 5, byte for byte what blosc_gpu_compress_batch writes with that destsize.
 *   offsets_out[0] = 0, offsets_out[i + 1] = align_up(offsets_out[i] + max(cbytes_i, 0), align)   whether or not chunk i was written:
 *   offsets_out[nchunks] is always the size the container needs, so a call with a too small dest (dest NULL, destsize 0 included)
 *   tells what to allocate.
 * Chunk i is written at dest + offsets_out[i] if and only if offsets_out[i] + cbytes_i <= destsize; otherwise cbytes_out[i] = 0 and
 * no byte at or behind offsets_out[i] is written for it.  The bytes between the end of a written chunk and offsets_out[i + 1] (below
 * destsize) are set to zero.  Nothing at or behind dest + destsize is ever written. */
BLOSC_EXPORT int blosc_gpu_compress_packed(int clevel, int doshuffle, size_t typesize, const char* compressor, size_t blocksize,
                                           int nchunks, const void* const* src, const size_t* nbytes,
                                           void* dest, size_t destsize, size_t align,
                                           size_t* offsets_out /* [nchunks + 1] */, int* cbytes_out /* [nchunks] */, void* stream);

/* Batched blosc_decompress out of one buffer.  Chunk i is the offsets[i + 1] - offsets[i] bytes at container + offsets[i]; that
 * difference is its srcsize (padding behind the chunk is fine, a header that claims more is rejected with -1).  The chunks decode back
 * to back: dest_offsets_out[i + 1] = dest_offsets_out[i] + the header's nbytes (0 for a chunk whose header does not pass validation);
 * nbytes_out[i] is blosc_decompress's return value; a valid chunk whose slot ends behind destsize answers -1 and writes nothing.
 * dest == NULL: the size query - dest_offsets_out and nbytes_out get the header sizes (or the validation errors), nothing is decoded. */
BLOSC_EXPORT int blosc_gpu_decompress_packed(int nchunks, const void* container, size_t containersize,
                                             const size_t* offsets /* [nchunks + 1] */,
                                             void* dest /* may be NULL */, size_t destsize,
                                             size_t* dest_offsets_out /* [nchunks + 1] */, int* nbytes_out /* [nchunks] */, void* stream);

/* blosc_cbuffer_sizes (include/blosc.h) for nchunks device-resident chunks; any out array may be NULL */
BLOSC_EXPORT int blosc_gpu_cbuffer_sizes_batch(int nchunks, const void* const* src,
                                               size_t* nbytes, size_t* cbytes, size_t* blocksize, void* stream);

#ifdef __cplusplus
}
#endif
#endif
