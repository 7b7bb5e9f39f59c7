/* include/blosc_gpu_getitem.h — blosc_getitem for many item ranges of many device-resident chunks in one call.
 *
 * blosc_gpu_getitem (include/blosc_gpu.h) serves one range of one chunk and pays a header fetch, a launch of the decode pipeline for
 * a handful of blocks and two synchronisations for it.  A sampler over a compressed cache, an index lookup or a reader of a packed
 * container (include/blosc_gpu_packed.h) wants thousands of small ranges at once: these calls fetch the headers of the chunks the
 * ranges name once, decode every block some range touches once - whatever the number of ranges that touch it - in one launch of the
 * pipeline, and write all slices with one gather kernel.  The number of host synchronisations of a call does not depend on the number
 * of ranges or chunks (it grows with the BYTES decoded: one more per 256 MiB of touched blocks).
 *
 * Conventions are those of include/blosc_gpu.h: the tables (src, chunk, start, nitems, dest, offsets and the two outputs) are HOST
 * arrays; src[i], dest[r], container and dest are DEVICE (or managed) memory on the current device; the calls are synchronous and
 * ordered on `stream` (a hipStream_t as void*, NULL = default stream).  They return 0, or a negative value if the device could not be
 * used or a table is NULL (blosc_gpu_getitem_packed: also for `offsets` not non-decreasing or offsets[nchunks] > containersize).
 *
 * Range r is items [start[r], start[r] + nitems[r]) of chunk chunk[r].  result_out[r] and the bytes written are exactly those of
 * blosc_getitem(src[chunk[r]], start[r], nitems[r], dest[r]): the byte count, 0 for an empty range, -1 for a range out of bounds, the
 * header codes -9 / -5 / -1 in blosc_getitem's order, and the code of the first block that does not decode.  A chunk[r] outside
 * 0 ... nchunks - 1 answers -1.  A range that fails writes nothing.  A range's outcome depends on the blocks it touches alone: a damaged
 * block fails the ranges that touch it and no others.  Ranges may overlap, repeat, come in any order and name chunks of any format,
 * typesize and filter, MEMCPYED chunks and chunks of nbytes 0 included; destinations may have any alignment and must not overlap
 * each other.
 */
#ifndef BLOSC_AMD_BLOSC_GPU_GETITEM_H
#define BLOSC_AMD_BLOSC_GPU_GETITEM_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#ifndef BLOSC_EXPORT
#define BLOSC_EXPORT __attribute__((visibility("default")))
#endif

/* range r -> dest[r] (room for nitems[r] * typesize bytes each) */
BLOSC_EXPORT int blosc_gpu_getitem_batch(int nchunks, const void* const* src,
                                         int nranges, const int* chunk, const int* start, const int* nitems,
                                         void* const* dest, int* result_out /* [nranges] */, void* stream);

/* The same out of a packed container, the slices back to back in ONE dest.  Chunk i is the offsets[i + 1] - offsets[i] bytes at
 * container + offsets[i], as blosc_gpu_decompress_packed takes them: that difference is its srcsize, and a header that claims more
 * answers -1 for every range of the chunk.
 *   dest_offsets_out[0] = 0, dest_offsets_out[r + 1] = dest_offsets_out[r] + max(result_out[r], 0)
 * Range r is written at dest + dest_offsets_out[r].  A valid range whose slot ends behind destsize answers -1, writes nothing and
 * takes no room.  dest == NULL is the size query: result_out and dest_offsets_out are what a call with a large enough dest gives,
 * from the headers alone - nothing is decoded.  (One case keeps its slot without filling it: a range whose header and bounds are
 * fine but whose block turns out not to decode answers blosc_getitem's negative code, and the next slice still begins behind the room
 * the size query counted for it.  The slots never depend on what the decoders find.) */
BLOSC_EXPORT int blosc_gpu_getitem_packed(int nchunks, const void* container, size_t containersize,
                                          const size_t* offsets /* [nchunks + 1] */,
                                          int nranges, const int* chunk, const int* start, const int* nitems,
                                          void* dest /* may be NULL */, size_t destsize,
                                          size_t* dest_offsets_out /* [nranges + 1] */, int* result_out /* [nranges] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
