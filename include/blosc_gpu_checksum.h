/* include/blosc_gpu_checksum.h — zlib's adler32 / crc32 of many byte runs in device memory, in one call.
 *
 * A container format that stores compressed chunks (Bloscpack's, c-blosc_amd/blpk.py) keeps a checksum of every chunk's compressed bytes.
 * The chunks of include/blosc_gpu_packed.h lie in device memory; digesting them on the host means bringing every compressed byte down
 * first and running it through one host thread.  These calls digest the runs where they are: blosc_gpu_checksum_batch takes a pointer per
 * run, blosc_gpu_checksum_packed the runs of one buffer by offset table - the container blosc_gpu_compress_packed writes, or a file
 * image on its way into blosc_gpu_decompress_packed.
 *
 * Conventions are those of include/blosc_gpu_packed.h: the tables (src, nbytes, offsets, length, digest_out) are HOST arrays; src[i]
 * and container are DEVICE (or managed) memory on the current device; the calls are synchronous and ordered on `stream` (a hipStream_t
 * as void*, NULL = default stream).  They return 0, or a negative value if the device could not be used or an argument is unusable as a
 * whole: an unknown `kind`, a NULL table, `offsets` not non-decreasing, offsets[nruns] > containersize, a length[i] greater than its
 * span offsets[i + 1] - offsets[i], a run longer than INT32_MAX + 16 bytes (no chunk is longer).  digest_out is written only by a call
 * that answers 0.  nruns <= 0 answers 0.
 *
 * digest_out[i] is what zlib's adler32() / crc32() give for the run, started from adler32(0, NULL, 0) = 1 / crc32(0, NULL, 0) = 0; an
 * empty run therefore answers 1 / 0, and its pointer is never read.
 *
 *  - Any source alignment and any length.
 *  - No byte outside a run is read: every load lies between the run's first and last byte.  In particular nothing is touched beyond the
 *    aligned 16-byte words that hold bytes of the run, so no page the run does not lie on.
 *  - Offsets, lengths and totals are 64-bit throughout: a container larger than 4 GiB is fine.
 *  - One table upload, two kernel launches, one download of 4 bytes per run and one host synchronisation per call, whatever nruns and
 *    the sizes: one run of 2 GiB and 100 000 runs of 20 bytes both spread over the device.
 *  - Deterministic: both digests combine exactly, in any order.
 */
#ifndef BLOSC_AMD_BLOSC_GPU_CHECKSUM_H
#define BLOSC_AMD_BLOSC_GPU_CHECKSUM_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#ifndef BLOSC_EXPORT
#define BLOSC_EXPORT __attribute__((visibility("default")))
#endif

#define BLOSC_GPU_CHECKSUM_ADLER32 1      /* blpk.py's checksum kinds */
#define BLOSC_GPU_CHECKSUM_CRC32   2

/* digest_out[i] = the digest of the nbytes[i] bytes at src[i] */
BLOSC_EXPORT int blosc_gpu_checksum_batch(int kind, int nruns, const void* const* src, const size_t* nbytes,
                                          unsigned int* digest_out /* [nruns] */, void* stream);

/* run i = the first length[i] bytes at container + offsets[i]; length == NULL: the whole span offsets[i + 1] - offsets[i] */
BLOSC_EXPORT int blosc_gpu_checksum_packed(int kind, int nruns, const void* container, size_t containersize,
                                           const size_t* offsets /* [nruns + 1] */, const size_t* length /* [nruns] or NULL */,
                                           unsigned int* digest_out /* [nruns] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
