// engine.h — host engine: turns a batch of chunks into descriptor tables + kernel launches.
//
// This is the GPU analogue of the reference's scheduler (do_job / serial_blosc / t_blosc,
// blosc/blosc.c:803-918, :1706-1887): where the reference hands blocks to a pthread pool, the
// engine flattens every block and split of every chunk of a batch into tables (dev_types.h) and
// launches one grid per pipeline stage over all of them.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace bamd {

struct CompressParams {
  int clevel;
  int doshuffle;          // 0 / 1 / 2  (blosc/blosc.h:54-56)
  size_t typesize;
  int codec;              // blosc/blosc.h:64-69
  int32_t forced_blocksize;
  int splitmode;          // blosc/blosc.h:114-117
};

struct Job {
  const void* src;
  void* dst;
  size_t srcsize;         // compress: nbytes.  decompress: bytes available at src (0 = trust the header)
  size_t dstsize;
};

// The packed calls (include/blosc_gpu_packed.h): the whole batch lives in ONE device buffer, chunk i at base + offsets[i].
// compress: the engine chooses the offsets from the chunks' sizes (multiples of `align`, a power of two) and writes what fits into `size`
// bytes.  decompress: the chunks decode back to back, their slots sized by their headers; base == nullptr only sizes.
// offsets: host array of n + 1 entries, written by the call.
struct PackedBuffer {
  void* base;
  size_t size;
  size_t align;           // compress only
  size_t* offsets;
};

// All three return 0 when the batch was processed (per-chunk outcomes in results[], with exactly the
// reference's return-value conventions) or a negative number when the device could not be
// used at all (no GPU, out of memory, launch failure) — never a silent CPU fallback.
// packed != nullptr (device pointers only): jobs[i].dst is ignored, jobs[i].dstsize is the chunk's own limit
// compress: per_chunk - chunk i is compressed with params[i] (include/blosc_gpu_params.h); otherwise every chunk with params[0].  A
// parameter error (-10) or a codec that is not built (-5) is the outcome of its chunk alone.
// compress: select (include/blosc_gpu_select.h; device pointers only, per_chunk) - chunk i has the candidates params[cand_first[i] ..
// cand_first[i + 1]).  Every candidate is encoded, the one with the smallest positive outcome (the lowest index on a tie) is the one
// written, and results[i] is its outcome; where no candidate has one, results[i] is the first candidate's outcome (-10 without
// candidates), nothing is written and the chunk takes 0 bytes of a packed buffer.
struct CandidateSelect {
  const int* cand_first;   // host [n + 1]: starts at 0 and never decreases (the caller has checked it)
  int* choice;             // host [n], written: the winner's index relative to cand_first[i], or -1
  int* cand_results;       // host [cand_first[n]], written, or nullptr: every candidate's outcome
};
int engine_compress_batch(const CompressParams* params, bool per_chunk, int n, const Job* jobs, int* results, bool device_ptrs,
                          hipStream_t stream, const PackedBuffer* packed = nullptr, const CandidateSelect* select = nullptr);
int engine_decompress_batch(int n, const Job* jobs, int* results, bool device_ptrs, hipStream_t stream,
                            const PackedBuffer* packed = nullptr);
// the parsed 16-byte headers of n device-resident chunks (one gather kernel, one synchronisation)
struct Header;
int engine_chunk_headers(int n, const void* const* src, Header* out, hipStream_t stream);
// blosc_getitem: engine_getitem_batch's pipeline for one range of one chunk, either pointer host or device memory (a host source is staged,
// a host dest is written only when the result is positive), with the reference's messages on stderr for a range out of bounds
int engine_getitem(const void* src, int start, int nitems, void* dest, bool src_on_device, bool dst_on_device,
                   hipStream_t stream);
// Many item ranges of many device-resident chunks in one call (include/blosc_gpu_getitem.h).  chunks[i]: src and srcsize (0 = trust the
// header) of chunk i.  Range r = items [start, start + nitems) of chunk `chunk`; results[r] is what blosc_getitem answers for it.
// packed == nullptr: the slice goes to ranges[r].dst.  packed: the slices back to back in packed->base (size: its capacity; offsets:
// nranges + 1 entries, written), ranges[r].dst is ignored; base == nullptr only sizes.
struct ItemRange { int chunk, start, nitems; void* dst; };
int engine_getitem_batch(int nchunks, const Job* chunks, int nranges, const ItemRange* ranges, int* results, hipStream_t stream,
                         const PackedBuffer* packed = nullptr);
void engine_getitem_pass_bytes(size_t bytes);   // test hook: decoded bytes per pass of engine_getitem_batch (0: the default, 256 MiB)
// Rows of row_bytes bytes by a DEVICE index table (include/blosc_gpu_take.h): the chunks are one array of rows, row index[k] goes to
// dest + k * row_bytes and status[k] (device, may be nullptr) is row_bytes or the row's negative code.  chunk_rows_out (host, may be nullptr):
// every chunk's rows or its negative census code - with one of those the call answers -1 and decodes nothing.  failed_out (host, may be
// nullptr): the rows with a negative status.  The passes are engine_getitem_batch's, under the same bound.
int engine_take(int nchunks, const Job* chunks, size_t row_bytes, size_t nidx, const int64_t* index, void* dest, int* status,
                int* chunk_rows_out, size_t* failed_out, hipStream_t stream);
// Rows written INTO the chunks (include/blosc_gpu_put.h): index_copy_ on the array of rows engine_take reads, `index` [nidx] and `rows`
// (nidx * row_bytes) device memory, the last occurrence of a row winning.  The chunks some valid index names are decoded, updated and
// compressed again with params[i] (one per chunk, all of them checked); the others are copied.  out: the new container as the packed compress
// call lays it out (base, size, align; offsets [nchunks + 1] written).  cbytes_out / rewritten_out (may be nullptr) [nchunks], status (device,
// may be nullptr) [nidx], chunk_rows_out and failed_out as in engine_take.  With a census failure the call answers -1 and writes nothing
// but chunk_rows_out.
int engine_put(int nchunks, const Job* chunks, size_t row_bytes, size_t nidx, const int64_t* index, const void* rows, const CompressParams* params,
               const PackedBuffer* out, int* cbytes_out, int* rewritten_out, int* status, int* chunk_rows_out, size_t* failed_out, hipStream_t stream);
// The rows whose field satisfies a predicate (include/blosc_gpu_where.h), over the array of rows engine_take reads: their numbers, ascending,
// go to index_out (device, `capacity` entries; nullptr with capacity 0: the count alone).  pred: the caller's predicate as the kernels
// evaluate it (dev_types.h: WherePred).  total_out: the matches, whatever the capacity; chunk_matches_out [nchunks]: per chunk, or the negative
// answer of the decoder for a chunk that does not decode, whose rows are counted in unread_out; chunk_rows_out as in engine_take (all host, may
// be nullptr).  With a census failure the call answers -1 and writes nothing but chunk_rows_out; with index_out inside a source, nothing at all.
struct WherePred;
int engine_where(int nchunks, const Job* chunks, size_t row_bytes, const WherePred& pred, int64_t* index_out, size_t capacity, size_t* total_out,
                 int* chunk_matches_out, int* chunk_rows_out, size_t* unread_out, hipStream_t stream);
// Count, sum, min and max of a row field (include/blosc_gpu_aggregate.h), over the array of rows engine_take reads, of the rows whose filter
// field passes (filter nullptr: of every row).  field, filter: the caller's as the kernels evaluate them (dev_types.h: AggField, WherePred).
// chunk_out [nchunks]: every chunk's result in blosc_gpu_aggregate's layout (dev_types.h: AggResult), the row numbers the call's; total_out: their
// left fold in chunk order; chunk_status_out [nchunks]: 0, or the negative answer of the decoder for a chunk that does not decode, whose rows are
// counted in unread_out; chunk_rows_out as in engine_take (all host, may be nullptr).  With a census failure the call answers -1 and writes
// nothing but chunk_rows_out.
struct AggField;
struct AggResult;
int engine_aggregate(int nchunks, const Job* chunks, size_t row_bytes, const AggField& field, const WherePred* filter, AggResult* total_out,
                     AggResult* chunk_out, int* chunk_status_out, int* chunk_rows_out, size_t* unread_out, hipStream_t stream);
// The two calls above for a term list (include/blosc_gpu_clauses.h): the rows for which every clause of the list has a true term.  terms: the
// caller's list as the kernels evaluate it (dev_types.h: WhereTerms; in aggregate its field 0 is `field`, and no terms let every row through).
// Everything else as above: the same body runs behind another mark / tile kernel.
// prune (include/blosc_gpu_zones.h; nullptr: none): behind the census excludes(ctx, chunk, its rows) is asked for every chunk - 1: the chunk
// is not decoded and answers what a decoded chunk without a match answers, 0: it is, negative: the call answers -1 with nothing but
// chunk_rows_out written.  pruned_out (host [nchunks], may be nullptr): 1 for every chunk that holds rows and was not decoded.
struct WhereTerms;
struct RowPrune {
  int (*excludes)(const void* ctx, size_t chunk, uint64_t rows);
  const void* ctx;
  uint8_t* pruned_out;
};
int engine_where_terms(int nchunks, const Job* chunks, size_t row_bytes, const WhereTerms& terms, int64_t* index_out, size_t capacity, size_t* total_out,
                       int* chunk_matches_out, int* chunk_rows_out, size_t* unread_out, hipStream_t stream, const RowPrune* prune = nullptr);
int engine_aggregate_terms(int nchunks, const Job* chunks, size_t row_bytes, const AggField& field, const WhereTerms& terms, AggResult* total_out,
                           AggResult* chunk_out, int* chunk_status_out, int* chunk_rows_out, size_t* unread_out, hipStream_t stream,
                           const RowPrune* prune = nullptr);
// engine_aggregate_terms for nfields fields in one decode (include/blosc_gpu_zones.h): terms holds the tested fields only (no field 0 of the
// aggregate), total_out [nfields], chunk_out [nchunks * nfields] chunk-major; every entry is what engine_aggregate_terms answers for its field.
int engine_aggregate_fields(int nchunks, const Job* chunks, size_t row_bytes, const AggField* fields, int nfields, const WhereTerms& terms, AggResult* total_out,
                            AggResult* chunk_out, int* chunk_status_out, int* chunk_rows_out, size_t* unread_out, hipStream_t stream);

// zlib's adler32 (kind 1) / crc32 (kind 2) of n runs in device memory (include/blosc_gpu_checksum.h): runs[i].src and runs[i].srcsize;
// an empty run's pointer is never read.  digests[] is written only when the call answers 0.
int engine_checksum_batch(int kind, int n, const Job* runs, uint32_t* digests, hipStream_t stream);
void engine_checksum_tile_bytes(size_t bytes);  // test hook: bytes per tile (a multiple of 16 up to 1 MiB; 0: the default, 256 KiB)

// one block through one filter kernel, host buffers (test hook; kind 0..3 = shuffle, unshuffle, bitshuffle, bitunshuffle)
int engine_filter(int kind, size_t typesize, size_t blocksize, const void* src, void* dst);

// test hooks of the persistent grids (engine.hip: query_persistent_grids; none of them launches a kernel): per persistent kernel its name, the workgroups per
// CU its launches ask for and the runtime's occupancy figure - returns how many kernels there are, fills the first `cap`; the occupancy of the LZ4 encode
// kernel with dynamic LDS on top; tasks taken / streams / shuffle tasks of the last compress call that ran streams
int engine_persistent_grids(int cap, const char** names, int* launched, int* occupancy);
int engine_enc_lz_occupancy(int dynamic_lds);
void engine_last_compress_tasks(uint32_t out[3]);

int engine_set_device(int dev);      // selects the HIP device for this process (default: current)
int engine_thread_device(int dev);   // >= 0: the calling THREAD's calls run on this device (multi-GPU entry points); -1: back to the process-wide one
int engine_device_count();
void engine_release();               // frees workspace memory (blosc_free_resources / blosc_destroy)
bool engine_is_device_pointer(const void* p);

// per-kernel timing (hipEvents on the launch stream), used by bench.py for the roofline numbers
void engine_prof_enable(int on);
void engine_prof_reset();
int engine_prof_get(const char* kernel, double* total_ms, int* launches);

}  // namespace bamd
