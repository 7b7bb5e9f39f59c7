// blosc_api.hip — the exported C ABI (include/blosc.h, include/blosc_gpu.h, include/blosc_gpu_packed.h, include/blosc_gpu_params.h,
// include/blosc_gpu_getitem.h, include/blosc_gpu_take.h, include/blosc_gpu_put.h, include/blosc_gpu_where.h, include/blosc_gpu_aggregate.h, include/blosc_gpu_checksum.h).
//
// Host-side mirror of the reference's public layer (blosc/blosc.c:1282-1703, :1951-2317):
// process globals, the per-call environment overrides, name/code tables and cbuffer introspection
// behave like the reference; the work itself is handed to the engine (engine.hip), never to a CPU
// implementation.
#include <errno.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <new>

#include "../../include/blosc.h"
#include "../../include/blosc_gpu.h"
#include "../../include/blosc_gpu_packed.h"
#include "../../include/blosc_gpu_params.h"
#include "../../include/blosc_gpu_select.h"
#include "../../include/blosc_gpu_getitem.h"
#include "../../include/blosc_gpu_take.h"
#include "../../include/blosc_gpu_put.h"
#include "../../include/blosc_gpu_where.h"
#include "../../include/blosc_gpu_aggregate.h"
#include "../../include/blosc_gpu_clauses.h"
#include "../../include/blosc_gpu_zones.h"
#include "../../include/blosc_gpu_checksum.h"
#include "blosc_format.h"
#include "dev_types.h"
#include "engine.h"

using namespace bamd;

// ---- process globals (blosc/blosc.c:143-150) ---------------------------------------------------
static pthread_mutex_t g_mutex = PTHREAD_MUTEX_INITIALIZER;   // the reference's global_comp_mutex
static int g_compressor = BLOSC_BLOSCLZ;
static int g_threads = 1;
static int g_force_blocksize = 0;
static int g_initlib = 0;
static int g_splitmode = BLOSC_FORWARD_COMPAT_SPLIT;

static const char* const kNames[6] = {BLOSC_BLOSCLZ_COMPNAME, BLOSC_LZ4_COMPNAME, BLOSC_LZ4HC_COMPNAME,
                                      BLOSC_SNAPPY_COMPNAME, BLOSC_ZLIB_COMPNAME, BLOSC_ZSTD_COMPNAME};
static bool codec_built(int code) { return code == BLOSC_BLOSCLZ || code == BLOSC_LZ4 || code == BLOSC_LZ4HC || code == BLOSC_ZLIB || code == BLOSC_ZSTD; }

// ---- marshalling of the batched extension: from the caller's arrays to the engine's tables --------------
// Whole-call checks by family.  A call that fails one answers -1 and writes nothing; tests/test_abi_arguments.py pins every line.
//   *_batch, *_batch_host, *_batch_multi   n <= 0 answers 0.  The arrays are the caller's word (include/blosc_gpu.h), only `srcsize` may be NULL.
//   compress_batch_params                   n <= 0 answers 0, then every array must be there.
//   compress_batch_select, _packed_select   their _params form's checks, then select_tables(): the candidate tables must be there (only
//                                           `cand_cbytes_out` may be NULL), cand_first must start at 0 and never decrease.
//   the packed calls                        packed_opening(): n < 0 or no table to write is unusable, n == 0 writes an empty table and answers 0;
//                                           then every array must be there.  `dest` may be NULL: the compress calls size (destsize must be 0
//                                           then), the reading calls size whatever destsize says.
//   getitem_batch                           a negative count is unusable, nranges == 0 answers 0, then every array (`src` when there are chunks).
//   take_*                                  take_opening(): a negative nchunks, row_bytes outside 1 ... 65536, no `index` or `dest` for nidx > 0 are
//                                           unusable; then `src` / the container and its offsets where there are chunks; no chunks and no indices answer 0.
//   put_*                                   put_opening(): take_opening() with `rows` for dest, then nidx above UINT32_MAX - 1, an unusable `align`, no `offsets_out`, a NULL
//                                           dest that claims bytes, no `params` or `cbytes_out` where there are chunks; then as take_*, and dest against the container.
//   where_*                                 where_opening(): a negative nchunks, row_bytes outside 1 ... 65536, no predicate or one outside the header's table, a field
//                                           that ends behind the row, a capacity without `index_out` are unusable; then as take_*, and index_out against the
//                                           container; no chunks answer 0 with a total of 0.
//   aggregate_*                             aggregate_opening(): a negative nchunks, row_bytes outside 1 ... 65536, no field, a field with pad_ set, outside the
//                                           header's table (field_of_table(), which where_opening() reads too) or ending behind the row; then a filter that
//                                           where_opening() refuses; then as take_*; no chunks answer 0 with the total of nothing.
//   checksum_*                              checksum_opening(): `kind` first, then nruns <= 0 answers 0; then the arrays (`length` may be NULL,
//                                           the container where every run is empty).
//   cbuffer_sizes_batch                     n < 0 is unusable, n == 0 answers 0, then `src`; every output may be NULL.
static const int kGo = 1;      // what a checks function answers for "go on"; anything else is the call's answer

// a call's temporary table, freed on every path; null: the allocation failed, the call answers -1
template <class T> using Table = std::unique_ptr<T[]>;
template <class T> static Table<T> table(int n) { return Table<T>(new (std::nothrow) T[(size_t)(n > 0 ? n : 1)]); }

// chunks given as parallel arrays; dest / insize / outsize NULL: no destination / 0
static Table<Job> jobs_from_arrays(int n, const void* const* src, void* const* dest, const size_t* insize, const size_t* outsize) {
  Table<Job> jobs = table<Job>(n);
  for (int i = 0; jobs && i < n; i++) jobs[i] = Job{src[i], dest ? dest[i] : nullptr, insize ? insize[i] : 0, outsize ? outsize[i] : 0};
  return jobs;
}

// Chunks (or runs) given as spans of one container: item i is what lies between offsets[i] and offsets[i + 1], all it may claim.  The table must
// rise and end inside the container, else the whole call is unusable (null is returned, as for a failed allocation: both answer -1).
//   length     (checksum) item i is the first length[i] bytes of its span; one that is longer than its span makes the call unusable.  NULL: the span
//   min_span   (chunks: BLOSC_MIN_HEADER_LENGTH) the engine reads srcsize 0 as "trust the header", so a span that cannot hold a header (an empty one
//              too) is passed as 1 byte, which it rejects without reading it.  0 (checksum): an empty run is a run
static Table<Job> jobs_from_spans(int n, const void* container, size_t containersize, const size_t* offsets, const size_t* length, size_t min_span) {
  for (int i = 0; i < n; i++)
    if (offsets[i + 1] < offsets[i] || (length && length[i] > offsets[i + 1] - offsets[i])) return nullptr;
  if (n > 0 && offsets[n] > containersize) return nullptr;
  Table<Job> jobs = table<Job>(n);
  for (int i = 0; jobs && i < n; i++) {
    const size_t size = length ? length[i] : offsets[i + 1] - offsets[i];
    jobs[i] = Job{(const void*)((uintptr_t)container + offsets[i]), nullptr, size < min_span ? 1 : size, 0};
  }
  return jobs;
}

// (clevel, doshuffle, typesize, compressor, blocksize) of a call with one parameter set, and the globals behind their defaults, as the engine's
// parameter set; false: the codec is not built (a name nobody knows too).  chunk_params() is the per-chunk counterpart
static bool call_params(int clevel, int doshuffle, size_t typesize, const char* compressor, size_t blocksize, CompressParams* p) {
  const int code = compressor ? blosc_compname_to_compcode(compressor) : g_compressor;
  if (code < 0 || !codec_built(code)) return false;
  *p = CompressParams{clevel, doshuffle, typesize, code, (int32_t)(blocksize ? blocksize : (size_t)g_force_blocksize), g_splitmode};
  return true;
}
// ... and what a call answers whose one parameter set names such a codec: every chunk -5, and none of them takes room
static int answer_not_built(int n, int* results, size_t* offsets_out) {
  for (int i = 0; i < n; i++) results[i] = -5;
  for (int i = 0; offsets_out && i <= n; i++) offsets_out[i] = 0;
  return 0;
}
// The engine checks every chunk's parameters by itself, in the reference's order (sizes, then parameters: -10, then the codec: -5), so an
// unusable row of include/blosc_gpu_params.h is the outcome of its chunk alone.
static Table<CompressParams> chunk_params(int nchunks, const blosc_gpu_cparams* params) {
  Table<CompressParams> p = table<CompressParams>(nchunks);
  for (int i = 0; p && i < nchunks; i++) {
    const blosc_gpu_cparams& c = params[i];
    p[i] = CompressParams{c.clevel, c.doshuffle, c.typesize, c.compcode == -1 ? g_compressor : c.compcode,
                          (int32_t)(c.blocksize ? c.blocksize : (size_t)g_force_blocksize), c.splitmode ? c.splitmode : g_splitmode};
    // a code outside 0 ... 5 is "not built" like Snappy (the engine's tables are indexed by the codes it knows)
    if (p[i].codec < 0 || p[i].codec > 5) p[i].codec = BLOSC_SNAPPY;
    // a split mode that does not exist is a parameter error of its chunk: handed on as a filter the engine's parameter check rejects
    // (the global mode of the single-parameter calls is never checked - as in the reference - so the check cannot live there)
    if (c.splitmode < 0 || c.splitmode > BLOSC_FORWARD_COMPAT_SPLIT) p[i].doshuffle = -1;
  }
  return p;
}

// The one road of the six compress entry points, of the four decompress and of the two getitem ones: a table that could not be made answers -1.
// (The callers make their tables in the argument list: such a temporary lives until the call has returned.)
// packed: every chunk's own limit is the size at which blosc_compress_ctx cannot answer 0; where it goes is the engine's layout step
static int compress_call(const CompressParams* params, bool per_chunk, int n, const Table<Job>& jobs, int* results, bool device_ptrs, void* stream,
                         const PackedBuffer* packed, const CandidateSelect* select = nullptr) {
  if (!params || !jobs) return -1;
  for (int i = 0; packed && i < n; i++) jobs[i].dstsize = jobs[i].srcsize + BLOSC_MAX_OVERHEAD;
  return engine_compress_batch(params, per_chunk, n, jobs.get(), results, device_ptrs, (hipStream_t)stream, packed, select);
}
static int decompress_call(int n, const Table<Job>& jobs, int* results, bool device_ptrs, void* stream, const PackedBuffer* packed) {
  return jobs ? engine_decompress_batch(n, jobs.get(), results, device_ptrs, (hipStream_t)stream, packed) : -1;
}
static int getitem_call(int nchunks, const Table<Job>& jobs, int nranges, const int* chunk, const int* start, const int* nitems, void* const* dest,
                        int* results, void* stream, const PackedBuffer* packed) {
  Table<ItemRange> ranges = table<ItemRange>(nranges);
  if (!jobs || !ranges) return -1;
  for (int i = 0; i < nranges; i++) ranges[i] = ItemRange{chunk[i], start[i], nitems[i], dest ? dest[i] : nullptr};
  return engine_getitem_batch(nchunks, jobs.get(), nranges, ranges.get(), results, (hipStream_t)stream, packed);
}

// how every packed call opens
static int packed_opening(int n, size_t* offsets_out) {
  if (n < 0 || !offsets_out) return -1;
  if (n == 0) { offsets_out[0] = 0; return 0; }
  return kGo;
}
static bool packed_align(size_t* align) {      // 0 means 1; a power of two up to 4096
  if (*align == 0) *align = 1;
  return *align <= 4096 && (*align & (*align - 1)) == 0;
}
// ... and the rest of what the two packed compress calls check (the alignment before the count: an empty batch with a bad one is unusable)
static int packed_compress_opening(int n, const void* const* src, const size_t* nbytes, void* dest, size_t destsize, size_t* align, size_t* offsets_out,
                                   int* cbytes_out) {
  if (!packed_align(align)) return -1;
  const int c = packed_opening(n, offsets_out);
  if (c != kGo) return c;
  return (!src || !nbytes || !cbytes_out || (!dest && destsize)) ? -1 : kGo;
}

// how both checksum calls open (`kind` before the count), and how they end
static int checksum_opening(int kind, int nruns) {
  if (kind != BLOSC_GPU_CHECKSUM_ADLER32 && kind != BLOSC_GPU_CHECKSUM_CRC32) return -1;
  return nruns <= 0 ? 0 : kGo;
}
static const size_t kChecksumMaxRun = (size_t)INT32_MAX + 16;      // beyond the largest chunk
static int checksum_call(int kind, int nruns, const Table<Job>& jobs, unsigned int* digest_out, void* stream) {
  if (!jobs) return -1;
  for (int i = 0; i < nruns; i++)
    if (jobs[i].srcsize > kChecksumMaxRun || (jobs[i].srcsize != 0 && !jobs[i].src)) return -1;
  return engine_checksum_batch(kind, nruns, jobs.get(), digest_out, (hipStream_t)stream);
}

extern "C" {

void blosc_init(void) { g_initlib = 1; }

void blosc_destroy(void) {
  if (!g_initlib) return;
  g_initlib = 0;
  engine_release();
}

int blosc_free_resources(void) {            // blosc/blosc.c:2311-2317
  if (!g_initlib) return -1;
  engine_release();
  return 0;
}

int blosc_get_nthreads(void) { return g_threads; }

int blosc_set_nthreads(int nthreads_new) {  // blosc/blosc.c:1958-1973
  int ret = g_threads;
  if (!g_initlib) blosc_init();
  if (nthreads_new != ret) g_threads = nthreads_new;
  return ret;
}

int blosc_compcode_to_compname(int compcode, const char** compname) {  // blosc/blosc.c:330-374
  const char* name = NULL;
  if (compcode >= 0 && compcode <= 5) name = kNames[compcode];
  *compname = name;
  return codec_built(compcode) ? compcode : -1;
}

int blosc_compname_to_compcode(const char* compname) {                 // blosc/blosc.c:377-409
  for (int c = 0; c <= 5; c++)
    if (codec_built(c) && strcmp(compname, kNames[c]) == 0) return c;
  return -1;
}

const char* blosc_get_compressor(void) {
  const char* n;
  blosc_compcode_to_compname(g_compressor, &n);
  return n;
}

int blosc_set_compressor(const char* compname) {                        // blosc/blosc.c:2010-2020
  int code = blosc_compname_to_compcode(compname);
  g_compressor = code;
  if (!g_initlib) blosc_init();
  return code;
}

const char* blosc_list_compressors(void) { return "blosclz,lz4,lz4hc,zlib,zstd"; }

const char* blosc_get_version_string(void) { return BLOSC_VERSION_STRING; }

int blosc_get_complib_info(const char* compname, char** complib, char** version) {  // blosc/blosc.c:2052-2109
  int clib = -1;
  const char* libname = NULL;
  const char* ver = "unknown";
  if (strcmp(compname, BLOSC_BLOSCLZ_COMPNAME) == 0) { clib = BLOSC_BLOSCLZ_LIB; libname = BLOSC_BLOSCLZ_LIBNAME; ver = "2.5.1"; }
  else if (strcmp(compname, BLOSC_LZ4_COMPNAME) == 0 || strcmp(compname, BLOSC_LZ4HC_COMPNAME) == 0) {
    clib = BLOSC_LZ4_LIB; libname = BLOSC_LZ4_LIBNAME; ver = "1.10.0";   // block format implemented, lz4.h:LZ4_VERSION_*
  }
  else if (strcmp(compname, BLOSC_ZSTD_COMPNAME) == 0) { clib = BLOSC_ZSTD_LIB; libname = BLOSC_ZSTD_LIBNAME; ver = "1.5.6"; }   // frame format written / read, zstd.h:ZSTD_VERSION_*
  else if (strcmp(compname, BLOSC_ZLIB_COMPNAME) == 0) { clib = BLOSC_ZLIB_LIB; libname = BLOSC_ZLIB_LIBNAME; ver = "1.3.1"; }   // stream format written / read, zlib.h:ZLIB_VERSION
  if (clib < 0) {   // Snappy is not built in: same answer as a stock build without it
    if (complib) *complib = NULL;
    if (version) *version = NULL;
    return -1;
  }
  if (complib) *complib = strdup(libname);
  if (version) *version = strdup(ver);
  return clib;
}

// ---- cbuffer introspection (blosc/blosc.c:2112-2180) --------------------------------------------
void blosc_cbuffer_sizes(const void* cbuffer, size_t* nbytes, size_t* cbytes, size_t* blocksize) {
  const uint8_t* s = (const uint8_t*)cbuffer;
  if (s[0] != BLOSC_VERSION_FORMAT) { *nbytes = *blocksize = *cbytes = 0; return; }
  *nbytes = (size_t)rd_i32(s + 4);
  *blocksize = (size_t)rd_i32(s + 8);
  *cbytes = (size_t)rd_i32(s + 12);
}

int blosc_cbuffer_validate(const void* cbuffer, size_t cbytes, size_t* nbytes) {
  size_t hc, hb;
  if (cbytes < BLOSC_MIN_HEADER_LENGTH) return -1;
  blosc_cbuffer_sizes(cbuffer, nbytes, &hc, &hb);
  if (hc != cbytes) return -1;
  if (*nbytes > BLOSC_MAX_BUFFERSIZE) return -1;
  return 0;
}

void blosc_cbuffer_metainfo(const void* cbuffer, size_t* typesize, int* flags) {
  const uint8_t* s = (const uint8_t*)cbuffer;
  if (s[0] != BLOSC_VERSION_FORMAT) { *flags = 0; *typesize = 0; return; }
  *flags = (int)s[2] & 7;
  *typesize = (size_t)s[3];
}

void blosc_cbuffer_versions(const void* cbuffer, int* version, int* versionlz) {
  const uint8_t* s = (const uint8_t*)cbuffer;
  *version = (int)s[0];
  *versionlz = (int)s[1];
}

const char* blosc_cbuffer_complib(const void* cbuffer) {
  static const char* const libs[5] = {BLOSC_BLOSCLZ_LIBNAME, BLOSC_LZ4_LIBNAME, BLOSC_SNAPPY_LIBNAME,
                                      BLOSC_ZLIB_LIBNAME, BLOSC_ZSTD_LIBNAME};
  int clib = (((const uint8_t*)cbuffer)[2] & 0xe0) >> 5;
  return clib < 5 ? libs[clib] : NULL;
}

int blosc_get_blocksize(void) { return g_force_blocksize; }
void blosc_set_blocksize(size_t size) { g_force_blocksize = (int32_t)size; }
void blosc_set_splitmode(int mode) { g_splitmode = mode; }

// ---- compression ---------------------------------------------------------------------------------
static int compress_one(int clevel, int doshuffle, size_t typesize, size_t nbytes, const void* src, void* dest,
                        size_t destsize, int compcode, size_t blocksize) {
  CompressParams p{clevel, doshuffle, typesize, compcode, (int32_t)blocksize, g_splitmode};
  // initialize_context_compression's checks that precede anything codec related (blosc.c:1076-1120)
  if (compcode < 0 || compcode > 5 || !codec_built(compcode)) {
    // order of the reference: size checks and parameter checks come first, the codec error (-5) last
    if (nbytes > (size_t)BLOSC_MAX_BUFFERSIZE || destsize < BLOSC_MAX_OVERHEAD) return 0;
    if (clevel < 0 || clevel > 9 || doshuffle < 0 || doshuffle > 2 || typesize == 0) return -10;
    fprintf(stderr, "Blosc has not been compiled with '%s' compression support.  Please use one having it.",
            (compcode >= 0 && compcode <= 5) ? kNames[compcode] : "(null)");
    return -5;
  }
  const bool sd = engine_is_device_pointer(src), dd = engine_is_device_pointer(dest);
  if (sd != dd && nbytes > 0) {
    fprintf(stderr, "blosc_amd: src and dest must both be host or both be device pointers\n");
    return -1;
  }
  Job job{src, dest, nbytes, destsize};
  int result = -1;
  if (engine_compress_batch(&p, false, 1, &job, &result, sd && dd, (hipStream_t)0) != 0) return -1;
  return result;
}

int blosc_compress_ctx(int clevel, int doshuffle, size_t typesize, size_t nbytes, const void* src, void* dest,
                       size_t destsize, const char* compressor, size_t blocksize, int numinternalthreads) {
  (void)numinternalthreads;
  return compress_one(clevel, doshuffle, typesize, nbytes, src, dest, destsize,
                      blosc_compname_to_compcode(compressor), blocksize);
}

int blosc_compress(int clevel, int doshuffle, size_t typesize, size_t nbytes, const void* src, void* dest,
                   size_t destsize) {
  if (!g_initlib) blosc_init();
  const char* ev;
  // environment overrides, re-read on every call (blosc/blosc.c:1320-1395)
  if ((ev = getenv("BLOSC_CLEVEL")) != NULL) { long v = strtol(ev, NULL, 10); if (v != EINVAL && v >= 0) clevel = (int)v; }
  if ((ev = getenv("BLOSC_SHUFFLE")) != NULL) {
    if (strcmp(ev, "NOSHUFFLE") == 0) doshuffle = BLOSC_NOSHUFFLE;
    if (strcmp(ev, "SHUFFLE") == 0) doshuffle = BLOSC_SHUFFLE;
    if (strcmp(ev, "BITSHUFFLE") == 0) doshuffle = BLOSC_BITSHUFFLE;
  }
  if ((ev = getenv("BLOSC_TYPESIZE")) != NULL) { long v = strtol(ev, NULL, 10); if (v != EINVAL && v > 0) typesize = (size_t)(int)v; }
  if ((ev = getenv("BLOSC_COMPRESSOR")) != NULL) { int r = blosc_set_compressor(ev); if (r < 0) return r; }
  if ((ev = getenv("BLOSC_BLOCKSIZE")) != NULL) { long v = strtol(ev, NULL, 10); if (v != EINVAL && v > 0) blosc_set_blocksize((size_t)v); }
  if ((ev = getenv("BLOSC_NTHREADS")) != NULL) { long v = strtol(ev, NULL, 10); if (v != EINVAL && v > 0) { int r = blosc_set_nthreads((int)v); if (r < 0) return r; } }
  if ((ev = getenv("BLOSC_SPLITMODE")) != NULL) {
    if (strcmp(ev, "FORWARD_COMPAT") == 0) blosc_set_splitmode(BLOSC_FORWARD_COMPAT_SPLIT);
    else if (strcmp(ev, "AUTO") == 0) blosc_set_splitmode(BLOSC_AUTO_SPLIT);
    else if (strcmp(ev, "ALWAYS") == 0) blosc_set_splitmode(BLOSC_ALWAYS_SPLIT);
    else if (strcmp(ev, "NEVER") == 0) blosc_set_splitmode(BLOSC_NEVER_SPLIT);
    else { fprintf(stderr, "BLOSC_SPLITMODE environment variable '%s' not recognized\n", ev); return -1; }
  }
  // BLOSC_NOLOCK (blosc.c:1400-1408) only changes locking in the reference; the engine serialises
  // device work itself, so both paths are the same call here.
  const bool nolock = getenv("BLOSC_NOLOCK") != NULL;
  if (!nolock) pthread_mutex_lock(&g_mutex);
  int r = compress_one(clevel, doshuffle, typesize, nbytes, src, dest, destsize, g_compressor, (size_t)g_force_blocksize);
  if (!nolock) pthread_mutex_unlock(&g_mutex);
  return r;
}

// ---- decompression -------------------------------------------------------------------------------
static int decompress_one(const void* src, void* dest, size_t destsize) {
  const bool sd = engine_is_device_pointer(src), dd = engine_is_device_pointer(dest);
  if (sd != dd) {
    // an empty chunk never touches dest (blosc.c:1463-1466); otherwise mixed residency is an error
    fprintf(stderr, "blosc_amd: src and dest must both be host or both be device pointers\n");
    return -1;
  }
  Job job{src, dest, 0, destsize};
  int result = -1;
  if (engine_decompress_batch(1, &job, &result, sd && dd, (hipStream_t)0) != 0) return -1;
  return result;
}

int blosc_decompress_ctx(const void* src, void* dest, size_t destsize, int numinternalthreads) {
  (void)numinternalthreads;
  return decompress_one(src, dest, destsize);
}

int blosc_decompress(const void* src, void* dest, size_t destsize) {
  if (!g_initlib) blosc_init();
  const char* ev;
  if ((ev = getenv("BLOSC_NTHREADS")) != NULL) {   // blosc.c:1546-1553
    long v = strtol(ev, NULL, 10);
    if (v != EINVAL && v > 0) { int r = blosc_set_nthreads((int)v); if (r < 0) return r; }
  }
  const bool nolock = getenv("BLOSC_NOLOCK") != NULL;
  if (!nolock) pthread_mutex_lock(&g_mutex);
  int r = decompress_one(src, dest, destsize);
  if (!nolock) pthread_mutex_unlock(&g_mutex);
  return r;
}

int blosc_getitem(const void* src, int start, int nitems, void* dest) {
  return engine_getitem(src, start, nitems, dest, engine_is_device_pointer(src), engine_is_device_pointer(dest), (hipStream_t)0);
}

// ---- device-resident batched extension (include/blosc_gpu.h) ---------------------------------------
int blosc_gpu_set_device(int device) { return engine_set_device(device); }

static int compress_batch(int clevel, int doshuffle, size_t typesize, const char* compressor, size_t blocksize,
                          int nchunks, const void* const* src, const size_t* nbytes, void* const* dest,
                          const size_t* destsize, int* cbytes_out, void* stream, bool device_ptrs) {
  if (nchunks <= 0) return 0;
  CompressParams p;
  if (!call_params(clevel, doshuffle, typesize, compressor, blocksize, &p)) return answer_not_built(nchunks, cbytes_out, nullptr);
  return compress_call(&p, false, nchunks, jobs_from_arrays(nchunks, src, dest, nbytes, destsize), cbytes_out, device_ptrs, stream, nullptr);
}
int blosc_gpu_compress_batch(int clevel, int doshuffle, size_t typesize, const char* compressor, size_t blocksize,
                             int nchunks, const void* const* src, const size_t* nbytes, void* const* dest,
                             const size_t* destsize, int* cbytes_out, void* stream) {
  return compress_batch(clevel, doshuffle, typesize, compressor, blocksize, nchunks, src, nbytes, dest, destsize, cbytes_out, stream, true);
}
// the same call on HOST buffers (staged over PCIe like the stock entry points): a file reader's chunks, c-blosc_amd/blpk.py
int blosc_gpu_compress_batch_host(int clevel, int doshuffle, size_t typesize, const char* compressor, size_t blocksize,
                                  int nchunks, const void* const* src, const size_t* nbytes, void* const* dest,
                                  const size_t* destsize, int* cbytes_out) {
  return compress_batch(clevel, doshuffle, typesize, compressor, blocksize, nchunks, src, nbytes, dest, destsize, cbytes_out, nullptr, false);
}

static int decompress_batch(int nchunks, const void* const* src, const size_t* srcsize, void* const* dest,
                            const size_t* destsize, int* nbytes_out, void* stream, bool device_ptrs) {
  if (nchunks <= 0) return 0;
  return decompress_call(nchunks, jobs_from_arrays(nchunks, src, dest, srcsize, destsize), nbytes_out, device_ptrs, stream, nullptr);
}
int blosc_gpu_decompress_batch(int nchunks, const void* const* src, const size_t* srcsize, void* const* dest,
                               const size_t* destsize, int* nbytes_out, void* stream) {
  return decompress_batch(nchunks, src, srcsize, dest, destsize, nbytes_out, stream, true);
}
int blosc_gpu_decompress_batch_host(int nchunks, const void* const* src, const size_t* srcsize, void* const* dest,
                                    const size_t* destsize, int* nbytes_out) {
  return decompress_batch(nchunks, src, srcsize, dest, destsize, nbytes_out, nullptr, false);
}

// ---- the batch in one device buffer (include/blosc_gpu_packed.h) ---------------------------------------
size_t blosc_gpu_packed_bound(int nchunks, const size_t* nbytes, size_t align) {
  if (nchunks <= 0 || !nbytes || !packed_align(&align)) return 0;
  size_t total = 0;
  for (int i = 0; i < nchunks; i++) total += (nbytes[i] + BLOSC_MAX_OVERHEAD + align - 1) / align * align;
  return total;
}

int blosc_gpu_compress_packed(int clevel, int doshuffle, size_t typesize, const char* compressor, size_t blocksize,
                              int nchunks, const void* const* src, const size_t* nbytes, void* dest, size_t destsize, size_t align,
                              size_t* offsets_out, int* cbytes_out, void* stream) {
  const int c = packed_compress_opening(nchunks, src, nbytes, dest, destsize, &align, offsets_out, cbytes_out);
  if (c != kGo) return c;
  CompressParams p;
  if (!call_params(clevel, doshuffle, typesize, compressor, blocksize, &p)) return answer_not_built(nchunks, cbytes_out, offsets_out);
  const PackedBuffer pk{dest, destsize, align, offsets_out};
  return compress_call(&p, false, nchunks, jobs_from_arrays(nchunks, src, nullptr, nbytes, nullptr), cbytes_out, true, stream, &pk);
}

// ---- parameters per chunk (include/blosc_gpu_params.h): the two calls above with chunk_params() ---------------------------------------
int blosc_gpu_compress_batch_params(int nchunks, const blosc_gpu_cparams* params, const void* const* src, const size_t* nbytes,
                                    void* const* dest, const size_t* destsize, int* cbytes_out, void* stream) {
  if (nchunks <= 0) return 0;
  if (!params || !src || !nbytes || !dest || !destsize || !cbytes_out) return -1;
  return compress_call(chunk_params(nchunks, params).get(), true, nchunks, jobs_from_arrays(nchunks, src, dest, nbytes, destsize), cbytes_out, true, stream,
                       nullptr);
}
int blosc_gpu_compress_packed_params(int nchunks, const blosc_gpu_cparams* params, const void* const* src, const size_t* nbytes,
                                     void* dest, size_t destsize, size_t align, size_t* offsets_out, int* cbytes_out, void* stream) {
  const int c = packed_compress_opening(nchunks, src, nbytes, dest, destsize, &align, offsets_out, cbytes_out);
  if (c != kGo) return c;
  if (!params) return -1;
  const PackedBuffer pk{dest, destsize, align, offsets_out};
  return compress_call(chunk_params(nchunks, params).get(), true, nchunks, jobs_from_arrays(nchunks, src, nullptr, nbytes, nullptr), cbytes_out, true, stream,
                       &pk);
}

// ---- candidates per chunk (include/blosc_gpu_select.h): the two calls above with a range of rows per chunk ---------------------------------------
static bool select_tables(int nchunks, const int* cand_first, const blosc_gpu_cparams* cands, const int* choice_out) {
  if (!cand_first || !cands || !choice_out || cand_first[0] != 0) return false;
  for (int i = 0; i < nchunks; i++) if (cand_first[i + 1] < cand_first[i]) return false;
  return true;
}
int blosc_gpu_compress_batch_select(int nchunks, const int* cand_first, const blosc_gpu_cparams* cands, const void* const* src, const size_t* nbytes,
                                    void* const* dest, const size_t* destsize, int* cbytes_out, int* choice_out, int* cand_cbytes_out, void* stream) {
  if (nchunks <= 0) return 0;
  if (!src || !nbytes || !dest || !destsize || !cbytes_out || !select_tables(nchunks, cand_first, cands, choice_out)) return -1;
  const CandidateSelect sel{cand_first, choice_out, cand_cbytes_out};
  return compress_call(chunk_params(cand_first[nchunks], cands).get(), true, nchunks, jobs_from_arrays(nchunks, src, dest, nbytes, destsize), cbytes_out, true,
                       stream, nullptr, &sel);
}
int blosc_gpu_compress_packed_select(int nchunks, const int* cand_first, const blosc_gpu_cparams* cands, const void* const* src, const size_t* nbytes,
                                     void* dest, size_t destsize, size_t align, size_t* offsets_out, int* cbytes_out, int* choice_out,
                                     int* cand_cbytes_out, void* stream) {
  const int c = packed_compress_opening(nchunks, src, nbytes, dest, destsize, &align, offsets_out, cbytes_out);
  if (c != kGo) return c;
  if (!select_tables(nchunks, cand_first, cands, choice_out)) return -1;
  const PackedBuffer pk{dest, destsize, align, offsets_out};
  const CandidateSelect sel{cand_first, choice_out, cand_cbytes_out};
  return compress_call(chunk_params(cand_first[nchunks], cands).get(), true, nchunks, jobs_from_arrays(nchunks, src, nullptr, nbytes, nullptr), cbytes_out, true,
                       stream, &pk, &sel);
}

int blosc_gpu_decompress_packed(int nchunks, const void* container, size_t containersize, const size_t* offsets,
                                void* dest, size_t destsize, size_t* dest_offsets_out, int* nbytes_out, void* stream) {
  const int c = packed_opening(nchunks, dest_offsets_out);
  if (c != kGo) return c;
  if (!container || !offsets || !nbytes_out) return -1;
  const PackedBuffer pk{dest, dest ? destsize : 0, 0, dest_offsets_out};
  return decompress_call(nchunks, jobs_from_spans(nchunks, container, containersize, offsets, nullptr, BLOSC_MIN_HEADER_LENGTH), nbytes_out, true, stream, &pk);
}

int blosc_gpu_cbuffer_sizes_batch(int nchunks, const void* const* src, size_t* nbytes, size_t* cbytes, size_t* blocksize, void* stream) {
  if (nchunks < 0 || (nchunks > 0 && !src)) return -1;
  if (nchunks == 0) return 0;
  Table<Header> h = table<Header>(nchunks);
  if (!h) return -1;
  const int r = engine_chunk_headers(nchunks, src, h.get(), (hipStream_t)stream);
  for (int i = 0; r == 0 && i < nchunks; i++) {
    const bool known = h[i].version == BLOSC_VERSION_FORMAT;      // blosc_cbuffer_sizes: zeros for another format version (blosc.c:2117-2123)
    if (nbytes) nbytes[i] = known ? (size_t)h[i].nbytes : 0;
    if (cbytes) cbytes[i] = known ? (size_t)h[i].cbytes : 0;
    if (blocksize) blocksize[i] = known ? (size_t)h[i].blocksize : 0;
  }
  return r;
}

// ---- one call, all GPUs of the node (include/blosc_gpu.h) --------------------------------------------
// The reference's one call fans its blocks out over a pool of worker threads (blosc/blosc.c:904-918 do_job, :871-899
// parallel_blosc, :1890-1949 init_threads).  Chunks of a batch are independent, so the same shape one level up: the chunk list is
// cut into contiguous ranges (blosc_gpu_partition = SURVEY 8e's floor(c G / n) rule, the one c-blosc_amd/multigpu.py and
// bench.py use across processes), one host thread per GPU runs the batched call on its range, bound to its device.
int blosc_gpu_device_count(void) { return engine_device_count(); }
int blosc_gpu_partition(size_t nchunks, int world, int rank, size_t* lo, size_t* hi) {
  if (world <= 0 || rank < 0 || rank >= world || !lo || !hi) return -1;
  const size_t w = (size_t)world, r = (size_t)rank;
  size_t l = (r * nchunks + w - 1) / w, h = ((r + 1) * nchunks + w - 1) / w;      // smallest c with floor(c w / nchunks) >= r
  if (h > nchunks) h = nchunks;
  *lo = l; *hi = h;
  return 0;
}
struct MultiArg {
  int dev, rc; bool compress; size_t lo, hi;
  int clevel, doshuffle; size_t typesize; const char* compressor; size_t blocksize;
  const void* const* src; const size_t* insize; void* const* dest; const size_t* destsize; int* out;
};
static void* multi_worker(void* p) {
  MultiArg& a = *(MultiArg*)p;
  a.rc = 0;
  if (a.hi == a.lo) return nullptr;
  if (engine_thread_device(a.dev) != 0) { a.rc = -1; return nullptr; }
  const int n = (int)(a.hi - a.lo);
  const bool devp = engine_is_device_pointer(a.src[a.lo]);      // a range is either host memory or memory of (or visible to) its GPU
  if (a.compress) a.rc = compress_batch(a.clevel, a.doshuffle, a.typesize, a.compressor, a.blocksize, n, a.src + a.lo, a.insize + a.lo, a.dest + a.lo,
                                        a.destsize + a.lo, a.out + a.lo, nullptr, devp);
  else a.rc = decompress_batch(n, a.src + a.lo, a.insize ? a.insize + a.lo : nullptr, a.dest + a.lo, a.destsize + a.lo, a.out + a.lo, nullptr, devp);
  (void)engine_thread_device(-1);
  return nullptr;
}
static int run_multi(MultiArg proto, int ndev, const int* devices, int nchunks) {
  if (nchunks <= 0) return 0;
  const int have = engine_device_count();
  if (ndev <= 0 || ndev > 64) return -1;
  MultiArg args[64];
  pthread_t th[64];
  for (int r = 0; r < ndev; r++) {
    args[r] = proto;
    args[r].dev = devices ? devices[r] : r;
    if (args[r].dev < 0 || args[r].dev >= have) { fprintf(stderr, "blosc_amd: multi-GPU call names device %d, this node shows %d\n", args[r].dev, have); return -1; }
    (void)blosc_gpu_partition((size_t)nchunks, ndev, r, &args[r].lo, &args[r].hi);
  }
  int started = 0, rc = 0;
  for (; started < ndev; started++) if (pthread_create(&th[started], nullptr, multi_worker, &args[started]) != 0) { rc = -1; break; }
  for (int r = 0; r < started; r++) { pthread_join(th[r], nullptr); if (args[r].rc < 0) rc = args[r].rc; }
  return rc;
}
int blosc_gpu_compress_batch_multi(int ndev, const int* devices, int clevel, int doshuffle, size_t typesize, const char* compressor, size_t blocksize,
                                   int nchunks, const void* const* src, const size_t* nbytes, void* const* dest, const size_t* destsize, int* cbytes_out) {
  MultiArg a{}; a.compress = true; a.clevel = clevel; a.doshuffle = doshuffle; a.typesize = typesize; a.compressor = compressor; a.blocksize = blocksize;
  a.src = src; a.insize = nbytes; a.dest = dest; a.destsize = destsize; a.out = cbytes_out;
  return run_multi(a, ndev, devices, nchunks);
}
int blosc_gpu_decompress_batch_multi(int ndev, const int* devices, int nchunks, const void* const* src, const size_t* srcsize, void* const* dest,
                                     const size_t* destsize, int* nbytes_out) {
  MultiArg a{}; a.compress = false; a.src = src; a.insize = srcsize; a.dest = dest; a.destsize = destsize; a.out = nbytes_out;
  return run_multi(a, ndev, devices, nchunks);
}

int blosc_gpu_getitem(const void* src, int start, int nitems, void* dest, void* stream) {
  return engine_getitem(src, start, nitems, dest, true, true, (hipStream_t)stream);
}

// ---- many item ranges in one call (include/blosc_gpu_getitem.h) ---------------------------------------
int blosc_gpu_getitem_batch(int nchunks, const void* const* src, int nranges, const int* chunk, const int* start, const int* nitems,
                            void* const* dest, int* result_out, void* stream) {
  if (nchunks < 0 || nranges < 0) return -1;
  if (nranges == 0) return 0;
  if ((nchunks > 0 && !src) || !chunk || !start || !nitems || !dest || !result_out) return -1;
  return getitem_call(nchunks, jobs_from_arrays(nchunks, src, nullptr, nullptr, nullptr), nranges, chunk, start, nitems, dest, result_out, stream, nullptr);
}
int blosc_gpu_getitem_packed(int nchunks, const void* container, size_t containersize, const size_t* offsets,
                             int nranges, const int* chunk, const int* start, const int* nitems,
                             void* dest, size_t destsize, size_t* dest_offsets_out, int* result_out, void* stream) {
  if (nchunks < 0) return -1;
  const int c = packed_opening(nranges, dest_offsets_out);
  if (c != kGo) return c;
  if ((nchunks > 0 && (!container || !offsets)) || !chunk || !start || !nitems || !result_out) return -1;
  const PackedBuffer pk{dest, dest ? destsize : 0, 0, dest_offsets_out};
  return getitem_call(nchunks, jobs_from_spans(nchunks, container, containersize, offsets, nullptr, BLOSC_MIN_HEADER_LENGTH), nranges, chunk, start, nitems,
                      nullptr, result_out, stream, &pk);
}

// ---- rows by a device index table (include/blosc_gpu_take.h) ---------------------------------------
static int take_opening(int nchunks, size_t row_bytes, size_t nidx, const void* index, const void* dest) {
  if (nchunks < 0 || row_bytes < 1 || row_bytes > 65536) return -1;
  if (nidx && (!index || !dest)) return -1;
  return kGo;
}
static int take_call(int nchunks, const Table<Job>& jobs, size_t row_bytes, size_t nidx, const int64_t* index, void* dest, int* status,
                     int* chunk_rows_out, size_t* failed_out, void* stream) {
  if (!jobs) return -1;
  if (nchunks == 0 && nidx == 0) return 0;      // no chunk to count, no row to answer
  return engine_take(nchunks, jobs.get(), row_bytes, nidx, index, dest, status, chunk_rows_out, failed_out, (hipStream_t)stream);
}
int blosc_gpu_take_batch(int nchunks, const void* const* src, size_t row_bytes, size_t nidx, const int64_t* index, void* dest, int* status,
                         int* chunk_rows_out, size_t* failed_out, void* stream) {
  const int c = take_opening(nchunks, row_bytes, nidx, index, dest);
  if (c != kGo) return c;
  if (nchunks > 0 && !src) return -1;
  return take_call(nchunks, jobs_from_arrays(nchunks, src, nullptr, nullptr, nullptr), row_bytes, nidx, index, dest, status, chunk_rows_out, failed_out, stream);
}
int blosc_gpu_take_packed(int nchunks, const void* container, size_t containersize, const size_t* offsets, size_t row_bytes, size_t nidx,
                          const int64_t* index, void* dest, int* status, int* chunk_rows_out, size_t* failed_out, void* stream) {
  const int c = take_opening(nchunks, row_bytes, nidx, index, dest);
  if (c != kGo) return c;
  if (nchunks > 0 && (!container || !offsets)) return -1;
  return take_call(nchunks, jobs_from_spans(nchunks, container, containersize, offsets, nullptr, BLOSC_MIN_HEADER_LENGTH), row_bytes, nidx, index, dest, status,
                   chunk_rows_out, failed_out, stream);
}

// ---- rows written by a device index table (include/blosc_gpu_put.h) --------------------------------
// put_opening(): take_opening()'s checks with `rows` in dest's place, then nidx, `align`, the tables the call writes and reads, a dest of no
// bytes that claims some; no chunks and no indices write an empty offset table and answer 0
static int put_opening(int nchunks, size_t row_bytes, size_t nidx, const void* index, const void* rows, const blosc_gpu_cparams* params, void* dest,
                       size_t destsize, size_t* align, size_t* offsets_out, int* cbytes_out) {
  const int c = take_opening(nchunks, row_bytes, nidx, index, rows);
  if (c != kGo) return c;
  if (nidx > (size_t)UINT32_MAX - 1 || !packed_align(align) || !offsets_out || (!dest && destsize)) return -1;
  if (nchunks > 0 && (!params || !cbytes_out)) return -1;
  return kGo;
}
static int put_call(int nchunks, const Table<Job>& jobs, size_t row_bytes, size_t nidx, const int64_t* index, const void* rows, const blosc_gpu_cparams* params,
                    void* dest, size_t destsize, size_t align, size_t* offsets_out, int* cbytes_out, int* rewritten_out, int* status, int* chunk_rows_out,
                    size_t* failed_out, void* stream) {
  if (!jobs) return -1;
  if (nchunks == 0 && nidx == 0) { offsets_out[0] = 0; if (failed_out) *failed_out = 0; return 0; }
  Table<CompressParams> p = chunk_params(nchunks, params);
  if (!p) return -1;
  const PackedBuffer pk{dest, destsize, align, offsets_out};
  return engine_put(nchunks, jobs.get(), row_bytes, nidx, index, rows, p.get(), &pk, cbytes_out, rewritten_out, status, chunk_rows_out, failed_out, (hipStream_t)stream);
}
int blosc_gpu_put_batch(int nchunks, const void* const* src, size_t row_bytes, size_t nidx, const int64_t* index, const void* rows,
                        const blosc_gpu_cparams* params, void* dest, size_t destsize, size_t align, size_t* offsets_out, int* cbytes_out,
                        int* rewritten_out, int* status, int* chunk_rows_out, size_t* failed_out, void* stream) {
  const int c = put_opening(nchunks, row_bytes, nidx, index, rows, params, dest, destsize, &align, offsets_out, cbytes_out);
  if (c != kGo) return c;
  if (nchunks > 0 && !src) return -1;
  return put_call(nchunks, jobs_from_arrays(nchunks, src, nullptr, nullptr, nullptr), row_bytes, nidx, index, rows, params, dest, destsize, align, offsets_out,
                  cbytes_out, rewritten_out, status, chunk_rows_out, failed_out, stream);
}
int blosc_gpu_put_packed(int nchunks, const void* container, size_t containersize, const size_t* offsets, size_t row_bytes, size_t nidx,
                         const int64_t* index, const void* rows, const blosc_gpu_cparams* params, void* dest, size_t destsize, size_t align,
                         size_t* offsets_out, int* cbytes_out, int* rewritten_out, int* status, int* chunk_rows_out, size_t* failed_out, void* stream) {
  const int c = put_opening(nchunks, row_bytes, nidx, index, rows, params, dest, destsize, &align, offsets_out, cbytes_out);
  if (c != kGo) return c;
  if (nchunks > 0 && (!container || !offsets)) return -1;
  // dest against the source container as a whole (the engine checks it against every chunk)
  const uintptr_t s0 = (uintptr_t)container, s1 = s0 + containersize, d0 = (uintptr_t)dest, d1 = d0 + destsize;
  if (nchunks > 0 && destsize && containersize && s0 < d1 && d0 < s1) return -1;
  return put_call(nchunks, jobs_from_spans(nchunks, container, containersize, offsets, nullptr, BLOSC_MIN_HEADER_LENGTH), row_bytes, nidx, index, rows, params,
                  dest, destsize, align, offsets_out, cbytes_out, rewritten_out, status, chunk_rows_out, failed_out, stream);
}

// ---- rows by a field predicate (include/blosc_gpu_where.h) -----------------------------------------
// where_opening(): the whole-call checks, and the predicate as the kernels evaluate it (dev_types.h: WherePred)
// The header's kind / bytes table, the one copy of it: false for a pair outside it, else the field as the kernels read it (dev_types.h:
// AggField - the kind of where_key, the pattern of +infinity and the mantissa bits of a floating-point format).  The field must end inside the row.
static bool field_of_table(int32_t kind, uint32_t b, uint32_t offset, size_t row_bytes, AggField* f) {
  uint64_t inf = 0;
  uint32_t mant = 0;
  switch (kind) {
    case BLOSC_GPU_FIELD_UINT: case BLOSC_GPU_FIELD_INT: if (b != 1 && b != 2 && b != 4 && b != 8) return false; break;
    case BLOSC_GPU_FIELD_FLOAT:
      if (b != 2 && b != 4 && b != 8) return false;
      inf = b == 2 ? 0x7c00ull : (b == 4 ? 0x7f800000ull : 0x7ff0000000000000ull); mant = b == 2 ? 10 : (b == 4 ? 23 : 52);
      break;
    case BLOSC_GPU_FIELD_BFLOAT16: if (b != 2) return false; inf = 0x7f80ull; mant = 7; break;
    default: return false;
  }
  if ((size_t)offset + b > row_bytes) return false;
  *f = AggField{offset, b, kind == BLOSC_GPU_FIELD_UINT ? 0 : (kind == BLOSC_GPU_FIELD_INT ? 1 : 2), mant, inf};
  return true;
}
static int where_opening(int nchunks, size_t row_bytes, const blosc_gpu_predicate* pred, const int64_t* index_out, size_t capacity, WherePred* q) {
  if (nchunks < 0 || row_bytes < 1 || row_bytes > 65536 || !pred) return -1;
  if (pred->op < BLOSC_GPU_WHERE_EQ || pred->op > BLOSC_GPU_WHERE_GE) return -1;
  AggField f;
  if (!field_of_table(pred->kind, pred->bytes, pred->offset, row_bytes, &f)) return -1;
  if (capacity && (!index_out || capacity > SIZE_MAX / sizeof(int64_t))) return -1;
  uint64_t v = 0;
  for (uint32_t i = 0; i < f.bytes; i++) v |= (uint64_t)pred->value[i] << (8 * i);
  bool nan = false;
  const int64_t key = where_key(v, f.kind, f.bytes, f.inf, &nan);
  *q = WherePred{pred->offset, f.bytes, f.kind, pred->op, key, f.inf, nan ? 1 : 0, 0};
  return kGo;
}
static int where_call(int nchunks, const Table<Job>& jobs, size_t row_bytes, const WherePred& q, int64_t* index_out, size_t capacity, size_t* total_out,
                      int* chunk_matches_out, int* chunk_rows_out, size_t* unread_out, void* stream) {
  if (!jobs) return -1;
  if (nchunks == 0) { if (total_out) *total_out = 0; if (unread_out) *unread_out = 0; return 0; }      // no chunk to count, no row to read
  return engine_where(nchunks, jobs.get(), row_bytes, q, index_out, capacity, total_out, chunk_matches_out, chunk_rows_out, unread_out, (hipStream_t)stream);
}
int blosc_gpu_where_batch(int nchunks, const void* const* src, size_t row_bytes, const blosc_gpu_predicate* pred, int64_t* index_out, size_t capacity,
                          size_t* total_out, int* chunk_matches_out, int* chunk_rows_out, size_t* unread_out, void* stream) {
  WherePred q;
  const int c = where_opening(nchunks, row_bytes, pred, index_out, capacity, &q);
  if (c != kGo) return c;
  if (nchunks > 0 && !src) return -1;
  return where_call(nchunks, jobs_from_arrays(nchunks, src, nullptr, nullptr, nullptr), row_bytes, q, index_out, capacity, total_out, chunk_matches_out,
                    chunk_rows_out, unread_out, stream);
}
int blosc_gpu_where_packed(int nchunks, const void* container, size_t containersize, const size_t* offsets, size_t row_bytes, const blosc_gpu_predicate* pred,
                           int64_t* index_out, size_t capacity, size_t* total_out, int* chunk_matches_out, int* chunk_rows_out, size_t* unread_out, void* stream) {
  WherePred q;
  const int c = where_opening(nchunks, row_bytes, pred, index_out, capacity, &q);
  if (c != kGo) return c;
  if (nchunks > 0 && (!container || !offsets)) return -1;
  // index_out against the source container as a whole (the engine checks it against every chunk)
  const uintptr_t s0 = (uintptr_t)container, s1 = s0 + containersize, d0 = (uintptr_t)index_out, d1 = d0 + capacity * sizeof(int64_t);
  if (nchunks > 0 && capacity && containersize && s0 < d1 && d0 < s1) return -1;
  return where_call(nchunks, jobs_from_spans(nchunks, container, containersize, offsets, nullptr, BLOSC_MIN_HEADER_LENGTH), row_bytes, q, index_out, capacity,
                    total_out, chunk_matches_out, chunk_rows_out, unread_out, stream);
}

// ---- count, sum, min, max of a row field (include/blosc_gpu_aggregate.h) ----------------------------
static_assert(sizeof(blosc_gpu_aggregate) == sizeof(AggResult) && sizeof(blosc_gpu_aggregate) == 64 && sizeof(blosc_gpu_field) == 16,
              "blosc_gpu_aggregate is the engine's AggResult");
// aggregate_opening(): the whole-call checks, and field and filter as the kernels evaluate them (dev_types.h: AggField, WherePred)
static int aggregate_opening(int nchunks, size_t row_bytes, const blosc_gpu_field* field, const blosc_gpu_predicate* filter, AggField* f, WherePred* q) {
  if (nchunks < 0 || row_bytes < 1 || row_bytes > 65536 || !field || field->pad_ != 0) return -1;
  if (!field_of_table(field->kind, field->bytes, field->offset, row_bytes, f)) return -1;
  return filter ? where_opening(nchunks, row_bytes, filter, nullptr, 0, q) : kGo;
}
static int aggregate_call(int nchunks, const Table<Job>& jobs, size_t row_bytes, const AggField& f, const WherePred* q, blosc_gpu_aggregate* total_out,
                          blosc_gpu_aggregate* chunk_out, int* chunk_status_out, int* chunk_rows_out, size_t* unread_out, void* stream) {
  if (!jobs) return -1;
  if (nchunks == 0) {      // no chunk to read: the total of nothing
    if (total_out) { memset(total_out, 0, sizeof *total_out); total_out->min_row = total_out->max_row = -1; }
    if (unread_out) *unread_out = 0;
    return 0;
  }
  return engine_aggregate(nchunks, jobs.get(), row_bytes, f, q, (AggResult*)total_out, (AggResult*)chunk_out, chunk_status_out, chunk_rows_out, unread_out,
                          (hipStream_t)stream);
}
int blosc_gpu_aggregate_batch(int nchunks, const void* const* src, size_t row_bytes, const blosc_gpu_field* field, const blosc_gpu_predicate* filter,
                              blosc_gpu_aggregate* total_out, blosc_gpu_aggregate* chunk_out, int* chunk_status_out, int* chunk_rows_out, size_t* unread_out,
                              void* stream) {
  AggField f; WherePred q;
  const int c = aggregate_opening(nchunks, row_bytes, field, filter, &f, &q);
  if (c != kGo) return c;
  if (nchunks > 0 && !src) return -1;
  return aggregate_call(nchunks, jobs_from_arrays(nchunks, src, nullptr, nullptr, nullptr), row_bytes, f, filter ? &q : nullptr, total_out, chunk_out,
                        chunk_status_out, chunk_rows_out, unread_out, stream);
}
int blosc_gpu_aggregate_packed(int nchunks, const void* container, size_t containersize, const size_t* offsets, size_t row_bytes, const blosc_gpu_field* field,
                               const blosc_gpu_predicate* filter, blosc_gpu_aggregate* total_out, blosc_gpu_aggregate* chunk_out, int* chunk_status_out,
                               int* chunk_rows_out, size_t* unread_out, void* stream) {
  AggField f; WherePred q;
  const int c = aggregate_opening(nchunks, row_bytes, field, filter, &f, &q);
  if (c != kGo) return c;
  if (nchunks > 0 && (!container || !offsets)) return -1;
  return aggregate_call(nchunks, jobs_from_spans(nchunks, container, containersize, offsets, nullptr, BLOSC_MIN_HEADER_LENGTH), row_bytes, f,
                        filter ? &q : nullptr, total_out, chunk_out, chunk_status_out, chunk_rows_out, unread_out, stream);
}

// ---- where and aggregate by a term list (include/blosc_gpu_clauses.h) -------------------------------
static_assert(sizeof(blosc_gpu_term) == 32 && BLOSC_GPU_MAX_TERMS == WH_MAX_TERMS, "blosc_gpu_term; the kernels' table holds every term");
// terms_opening(): the list's own checks, and the list as the kernels evaluate it (dev_types.h: WhereTerms) - every term through
// where_opening(), which refuses what blosc_gpu_where_* refuses and gives its key, `inf` and NaN flag; the distinct (offset, bytes) pairs, in
// front of them the aggregated field where there is one; the terms sorted by the pair they read.  min_terms: 1 (where) or 0 (aggregate)
static int terms_opening(int nchunks, size_t row_bytes, const blosc_gpu_term* terms, int nterms, int min_terms, const AggField* aggregated, WhereTerms* out) {
  if (nterms < min_terms || nterms > BLOSC_GPU_MAX_TERMS || (nterms > 0) != (terms != nullptr)) return -1;
  WhereTerms w{};
  WherePred q[WH_MAX_TERMS];
  uint32_t field_of[WH_MAX_TERMS];
  if (aggregated) { w.offset[0] = aggregated->offset; w.bytes[0] = aggregated->bytes; w.nfields = 1; }
  for (int t = 0; t < nterms; t++) {
    if (terms[t].clause >= 16 || terms[t].pad_ != 0) return -1;
    const int c = where_opening(nchunks, row_bytes, &terms[t].test, nullptr, 0, &q[t]);
    if (c != kGo) return c;
    uint32_t f = 0;
    while (f < w.nfields && (w.offset[f] != q[t].offset || w.bytes[f] != q[t].bytes)) f++;
    if (f == w.nfields) { w.offset[f] = q[t].offset; w.bytes[f] = q[t].bytes; w.nfields++; }
    field_of[t] = f;
    w.clauses |= 1u << terms[t].clause;
  }
  for (uint32_t f = 0; f < w.nfields; f++) {
    w.first[f] = w.nterms;
    for (int t = 0; t < nterms; t++)
      if (field_of[t] == f) { w.test[w.nterms] = q[t]; w.bit[w.nterms] = 1u << terms[t].clause; w.nterms++; }
  }
  for (uint32_t f = w.nfields; f <= (uint32_t)WH_MAX_FIELDS; f++) w.first[f] = w.nterms;
  *out = w;
  return kGo;
}
static int where_clauses_opening(int nchunks, size_t row_bytes, const blosc_gpu_term* terms, int nterms, const int64_t* index_out, size_t capacity, WhereTerms* w) {
  if (nchunks < 0 || row_bytes < 1 || row_bytes > 65536) return -1;
  if (capacity && (!index_out || capacity > SIZE_MAX / sizeof(int64_t))) return -1;
  return terms_opening(nchunks, row_bytes, terms, nterms, 1, nullptr, w);
}
static int where_clauses_call(int nchunks, const Table<Job>& jobs, size_t row_bytes, const WhereTerms& w, int64_t* index_out, size_t capacity, size_t* total_out,
                              int* chunk_matches_out, int* chunk_rows_out, size_t* unread_out, void* stream) {
  if (!jobs) return -1;
  if (nchunks == 0) { if (total_out) *total_out = 0; if (unread_out) *unread_out = 0; return 0; }      // no chunk to count, no row to read
  return engine_where_terms(nchunks, jobs.get(), row_bytes, w, index_out, capacity, total_out, chunk_matches_out, chunk_rows_out, unread_out, (hipStream_t)stream);
}
int blosc_gpu_where_clauses_batch(int nchunks, const void* const* src, size_t row_bytes, const blosc_gpu_term* terms, int nterms, int64_t* index_out,
                                  size_t capacity, size_t* total_out, int* chunk_matches_out, int* chunk_rows_out, size_t* unread_out, void* stream) {
  WhereTerms w;
  const int c = where_clauses_opening(nchunks, row_bytes, terms, nterms, index_out, capacity, &w);
  if (c != kGo) return c;
  if (nchunks > 0 && !src) return -1;
  return where_clauses_call(nchunks, jobs_from_arrays(nchunks, src, nullptr, nullptr, nullptr), row_bytes, w, index_out, capacity, total_out, chunk_matches_out,
                            chunk_rows_out, unread_out, stream);
}
int blosc_gpu_where_clauses_packed(int nchunks, const void* container, size_t containersize, const size_t* offsets, size_t row_bytes, const blosc_gpu_term* terms,
                                   int nterms, int64_t* index_out, size_t capacity, size_t* total_out, int* chunk_matches_out, int* chunk_rows_out,
                                   size_t* unread_out, void* stream) {
  WhereTerms w;
  const int c = where_clauses_opening(nchunks, row_bytes, terms, nterms, index_out, capacity, &w);
  if (c != kGo) return c;
  if (nchunks > 0 && (!container || !offsets)) return -1;
  // index_out against the source container as a whole (the engine checks it against every chunk)
  const uintptr_t s0 = (uintptr_t)container, s1 = s0 + containersize, d0 = (uintptr_t)index_out, d1 = d0 + capacity * sizeof(int64_t);
  if (nchunks > 0 && capacity && containersize && s0 < d1 && d0 < s1) return -1;
  return where_clauses_call(nchunks, jobs_from_spans(nchunks, container, containersize, offsets, nullptr, BLOSC_MIN_HEADER_LENGTH), row_bytes, w, index_out,
                            capacity, total_out, chunk_matches_out, chunk_rows_out, unread_out, stream);
}
static int aggregate_clauses_opening(int nchunks, size_t row_bytes, const blosc_gpu_field* field, const blosc_gpu_term* terms, int nterms, AggField* f, WhereTerms* w) {
  WherePred unused;
  const int c = aggregate_opening(nchunks, row_bytes, field, nullptr, f, &unused);
  return c != kGo ? c : terms_opening(nchunks, row_bytes, terms, nterms, 0, f, w);
}
static int aggregate_clauses_call(int nchunks, const Table<Job>& jobs, size_t row_bytes, const AggField& f, const WhereTerms& w, blosc_gpu_aggregate* total_out,
                                  blosc_gpu_aggregate* chunk_out, int* chunk_status_out, int* chunk_rows_out, size_t* unread_out, void* stream) {
  if (!jobs) return -1;
  if (nchunks == 0) return aggregate_call(0, jobs, row_bytes, f, nullptr, total_out, chunk_out, chunk_status_out, chunk_rows_out, unread_out, stream);      // the total of nothing
  return engine_aggregate_terms(nchunks, jobs.get(), row_bytes, f, w, (AggResult*)total_out, (AggResult*)chunk_out, chunk_status_out, chunk_rows_out, unread_out,
                                (hipStream_t)stream);
}
int blosc_gpu_aggregate_clauses_batch(int nchunks, const void* const* src, size_t row_bytes, const blosc_gpu_field* field, const blosc_gpu_term* terms, int nterms,
                                      blosc_gpu_aggregate* total_out, blosc_gpu_aggregate* chunk_out, int* chunk_status_out, int* chunk_rows_out,
                                      size_t* unread_out, void* stream) {
  AggField f; WhereTerms w;
  const int c = aggregate_clauses_opening(nchunks, row_bytes, field, terms, nterms, &f, &w);
  if (c != kGo) return c;
  if (nchunks > 0 && !src) return -1;
  return aggregate_clauses_call(nchunks, jobs_from_arrays(nchunks, src, nullptr, nullptr, nullptr), row_bytes, f, w, total_out, chunk_out, chunk_status_out,
                                chunk_rows_out, unread_out, stream);
}
int blosc_gpu_aggregate_clauses_packed(int nchunks, const void* container, size_t containersize, const size_t* offsets, size_t row_bytes,
                                       const blosc_gpu_field* field, const blosc_gpu_term* terms, int nterms, blosc_gpu_aggregate* total_out,
                                       blosc_gpu_aggregate* chunk_out, int* chunk_status_out, int* chunk_rows_out, size_t* unread_out, void* stream) {
  AggField f; WhereTerms w;
  const int c = aggregate_clauses_opening(nchunks, row_bytes, field, terms, nterms, &f, &w);
  if (c != kGo) return c;
  if (nchunks > 0 && (!container || !offsets)) return -1;
  return aggregate_clauses_call(nchunks, jobs_from_spans(nchunks, container, containersize, offsets, nullptr, BLOSC_MIN_HEADER_LENGTH), row_bytes, f, w,
                                total_out, chunk_out, chunk_status_out, chunk_rows_out, unread_out, stream);
}

// ---- zone maps (include/blosc_gpu_zones.h) ----------------------------------------------------------
static_assert(BLOSC_GPU_MAX_ZONE_FIELDS == 16, "blosc_gpu_zones.h");
static uint64_t little_endian(const uint8_t* p, uint32_t bytes) {
  uint64_t v = 0;
  for (uint32_t i = 0; i < bytes; i++) v |= (uint64_t)p[i] << (8 * i);
  return v;
}
// fields_opening(): nfields fields through aggregate_opening(), the list through terms_opening() without an aggregated field in front
static int fields_opening(int nchunks, size_t row_bytes, const blosc_gpu_field* fields, int nfields, const blosc_gpu_term* terms, int nterms, AggField* f, WhereTerms* w) {
  if (nfields < 1 || nfields > BLOSC_GPU_MAX_ZONE_FIELDS || !fields) return -1;
  WherePred unused;
  for (int k = 0; k < nfields; k++) {
    const int c = aggregate_opening(nchunks, row_bytes, &fields[k], nullptr, &f[k], &unused);
    if (c != kGo) return c;
  }
  return terms_opening(nchunks, row_bytes, terms, nterms, 0, nullptr, w);
}
static int fields_call(int nchunks, const Table<Job>& jobs, size_t row_bytes, const AggField* f, int nfields, const WhereTerms& w, blosc_gpu_aggregate* total_out,
                       blosc_gpu_aggregate* chunk_out, int* chunk_status_out, int* chunk_rows_out, size_t* unread_out, void* stream) {
  if (!jobs) return -1;
  if (nchunks == 0) {      // no chunk to read: the totals of nothing
    for (int k = 0; total_out && k < nfields; k++) { memset(&total_out[k], 0, sizeof *total_out); total_out[k].min_row = total_out[k].max_row = -1; }
    if (unread_out) *unread_out = 0;
    return 0;
  }
  return engine_aggregate_fields(nchunks, jobs.get(), row_bytes, f, nfields, w, (AggResult*)total_out, (AggResult*)chunk_out, chunk_status_out, chunk_rows_out,
                                 unread_out, (hipStream_t)stream);
}
int blosc_gpu_aggregate_fields_batch(int nchunks, const void* const* src, size_t row_bytes, const blosc_gpu_field* fields, int nfields, const blosc_gpu_term* terms,
                                     int nterms, blosc_gpu_aggregate* total_out, blosc_gpu_aggregate* chunk_out, int* chunk_status_out, int* chunk_rows_out,
                                     size_t* unread_out, void* stream) {
  AggField f[BLOSC_GPU_MAX_ZONE_FIELDS]; WhereTerms w;
  const int c = fields_opening(nchunks, row_bytes, fields, nfields, terms, nterms, f, &w);
  if (c != kGo) return c;
  if (nchunks > 0 && !src) return -1;
  return fields_call(nchunks, jobs_from_arrays(nchunks, src, nullptr, nullptr, nullptr), row_bytes, f, nfields, w, total_out, chunk_out, chunk_status_out,
                     chunk_rows_out, unread_out, stream);
}
int blosc_gpu_aggregate_fields_packed(int nchunks, const void* container, size_t containersize, const size_t* offsets, size_t row_bytes,
                                      const blosc_gpu_field* fields, int nfields, const blosc_gpu_term* terms, int nterms, blosc_gpu_aggregate* total_out,
                                      blosc_gpu_aggregate* chunk_out, int* chunk_status_out, int* chunk_rows_out, size_t* unread_out, void* stream) {
  AggField f[BLOSC_GPU_MAX_ZONE_FIELDS]; WhereTerms w;
  const int c = fields_opening(nchunks, row_bytes, fields, nfields, terms, nterms, f, &w);
  if (c != kGo) return c;
  if (nchunks > 0 && (!container || !offsets)) return -1;
  return fields_call(nchunks, jobs_from_spans(nchunks, container, containersize, offsets, nullptr, BLOSC_MIN_HEADER_LENGTH), row_bytes, f, nfields, w, total_out,
                     chunk_out, chunk_status_out, chunk_rows_out, unread_out, stream);
}

// The rule, as the header states it: whether a term can be true in a chunk whose field the INFORMING entry e describes
static bool zone_term_can_be_true(const blosc_gpu_predicate& q, const AggField& f, const blosc_gpu_aggregate& e) {
  bool nan = false, unused;
  const int64_t k = where_key(little_endian(q.value, f.bytes), f.kind, f.bytes, f.inf, &nan);
  if (nan || e.nans == e.rows) return q.op == BLOSC_GPU_WHERE_NE;
  const int64_t lo = where_key(little_endian(e.min, f.bytes), f.kind, f.bytes, f.inf, &unused);
  const int64_t hi = where_key(little_endian(e.max, f.bytes), f.kind, f.bytes, f.inf, &unused);
  switch (q.op) {
    case BLOSC_GPU_WHERE_LT: return lo < k;
    case BLOSC_GPU_WHERE_LE: return lo <= k;
    case BLOSC_GPU_WHERE_GT: return hi > k;
    case BLOSC_GPU_WHERE_GE: return hi >= k;
    case BLOSC_GPU_WHERE_EQ: return lo <= k && k <= hi;
    default: return !(lo == k && hi == k && e.nans == 0);
  }
}
int blosc_gpu_zone_excludes(const blosc_gpu_term* terms, int nterms, const blosc_gpu_field* zfields, int nzfields, const blosc_gpu_aggregate* entry,
                            uint64_t chunk_rows) {
  if (nterms < 0 || nterms > BLOSC_GPU_MAX_TERMS || nzfields < 0 || nzfields > BLOSC_GPU_MAX_ZONE_FIELDS) return -1;
  if ((nterms && !terms) || (nzfields && (!zfields || !entry))) return -1;
  AggField unused;
  for (int f = 0; f < nzfields; f++)
    if (zfields[f].pad_ != 0 || !field_of_table(zfields[f].kind, zfields[f].bytes, 0, 8, &unused)) return -1;
  uint32_t occurs = 0, open = 0;      // the clauses of the list; those with a term that can be true
  for (int t = 0; t < nterms; t++) {
    const blosc_gpu_predicate& q = terms[t].test;
    AggField tf;
    if (terms[t].clause >= 16 || terms[t].pad_ != 0 || q.op < BLOSC_GPU_WHERE_EQ || q.op > BLOSC_GPU_WHERE_GE) return -1;
    if (!field_of_table(q.kind, q.bytes, 0, 8, &tf)) return -1;
    bool can = true;
    for (int f = 0; f < nzfields; f++) {
      const blosc_gpu_aggregate& e = entry[f];
      if (zfields[f].offset != q.offset || zfields[f].bytes != q.bytes || zfields[f].kind != q.kind) continue;
      if (e.rows != chunk_rows || !chunk_rows || e.count != e.rows || !((e.min_row >= 0 && e.max_row >= 0) || e.nans == e.rows)) continue;      // no information
      can = zone_term_can_be_true(q, tf, e);
      break;
    }
    occurs |= 1u << terms[t].clause;
    if (can) open |= 1u << terms[t].clause;
  }
  return occurs != open ? 1 : 0;
}

// zones_opening(): the map's own checks;  zone_prune(): what the engine asks behind the census (engine.h: RowPrune) - the cheap guard, then the rule
namespace {
struct ZoneMap { const blosc_gpu_term* terms; int nterms; const blosc_gpu_field* zfields; int nzfields; const blosc_gpu_aggregate* zones; };
}  // namespace
static int zones_opening(size_t row_bytes, const blosc_gpu_field* zfields, int nzfields, const blosc_gpu_aggregate* zones) {
  if (nzfields < 0 || nzfields > BLOSC_GPU_MAX_ZONE_FIELDS || (nzfields && (!zfields || !zones))) return -1;
  AggField unused;
  for (int f = 0; f < nzfields; f++)
    if (zfields[f].pad_ != 0 || !field_of_table(zfields[f].kind, zfields[f].bytes, zfields[f].offset, row_bytes, &unused)) return -1;
  return kGo;
}
static int zone_prune(const void* ctx, size_t chunk, uint64_t rows) {
  const ZoneMap& z = *(const ZoneMap*)ctx;
  if (!z.nzfields) return 0;
  const blosc_gpu_aggregate* entry = z.zones + chunk * (size_t)z.nzfields;
  for (int f = 0; f < z.nzfields; f++)
    if (entry[f].rows != 0 && entry[f].rows != rows) return -1;      // a map of another container
  return blosc_gpu_zone_excludes(z.terms, z.nterms, z.zfields, z.nzfields, entry, rows);
}
static int where_zoned_call(int nchunks, const Table<Job>& jobs, size_t row_bytes, const WhereTerms& w, const ZoneMap& z, int64_t* index_out, size_t capacity,
                            size_t* total_out, int* chunk_matches_out, int* chunk_rows_out, size_t* unread_out, uint8_t* chunk_pruned_out, void* stream) {
  if (!jobs) return -1;
  if (nchunks == 0) { if (total_out) *total_out = 0; if (unread_out) *unread_out = 0; return 0; }
  const RowPrune prune{zone_prune, &z, chunk_pruned_out};
  return engine_where_terms(nchunks, jobs.get(), row_bytes, w, index_out, capacity, total_out, chunk_matches_out, chunk_rows_out, unread_out, (hipStream_t)stream,
                            &prune);
}
int blosc_gpu_where_zoned_batch(int nchunks, const void* const* src, size_t row_bytes, const blosc_gpu_term* terms, int nterms, const blosc_gpu_field* zfields,
                                int nzfields, const blosc_gpu_aggregate* zones, int64_t* index_out, size_t capacity, size_t* total_out, int* chunk_matches_out,
                                int* chunk_rows_out, size_t* unread_out, uint8_t* chunk_pruned_out, void* stream) {
  WhereTerms w;
  int c = where_clauses_opening(nchunks, row_bytes, terms, nterms, index_out, capacity, &w);
  if (c == kGo) c = zones_opening(row_bytes, zfields, nzfields, zones);
  if (c != kGo) return c;
  if (nchunks > 0 && !src) return -1;
  const ZoneMap z{terms, nterms, zfields, nzfields, zones};
  return where_zoned_call(nchunks, jobs_from_arrays(nchunks, src, nullptr, nullptr, nullptr), row_bytes, w, z, index_out, capacity, total_out, chunk_matches_out,
                          chunk_rows_out, unread_out, chunk_pruned_out, stream);
}
int blosc_gpu_where_zoned_packed(int nchunks, const void* container, size_t containersize, const size_t* offsets, size_t row_bytes, const blosc_gpu_term* terms,
                                 int nterms, const blosc_gpu_field* zfields, int nzfields, const blosc_gpu_aggregate* zones, int64_t* index_out, size_t capacity,
                                 size_t* total_out, int* chunk_matches_out, int* chunk_rows_out, size_t* unread_out, uint8_t* chunk_pruned_out, void* stream) {
  WhereTerms w;
  int c = where_clauses_opening(nchunks, row_bytes, terms, nterms, index_out, capacity, &w);
  if (c == kGo) c = zones_opening(row_bytes, zfields, nzfields, zones);
  if (c != kGo) return c;
  if (nchunks > 0 && (!container || !offsets)) return -1;
  // index_out against the source container as a whole (the engine checks it against every chunk)
  const uintptr_t s0 = (uintptr_t)container, s1 = s0 + containersize, d0 = (uintptr_t)index_out, d1 = d0 + capacity * sizeof(int64_t);
  if (nchunks > 0 && capacity && containersize && s0 < d1 && d0 < s1) return -1;
  const ZoneMap z{terms, nterms, zfields, nzfields, zones};
  return where_zoned_call(nchunks, jobs_from_spans(nchunks, container, containersize, offsets, nullptr, BLOSC_MIN_HEADER_LENGTH), row_bytes, w, z, index_out,
                          capacity, total_out, chunk_matches_out, chunk_rows_out, unread_out, chunk_pruned_out, stream);
}
static int aggregate_zoned_call(int nchunks, const Table<Job>& jobs, size_t row_bytes, const AggField& f, const WhereTerms& w, const ZoneMap& z,
                                blosc_gpu_aggregate* total_out, blosc_gpu_aggregate* chunk_out, int* chunk_status_out, int* chunk_rows_out, size_t* unread_out,
                                uint8_t* chunk_pruned_out, void* stream) {
  if (!jobs) return -1;
  if (nchunks == 0) return aggregate_call(0, jobs, row_bytes, f, nullptr, total_out, chunk_out, chunk_status_out, chunk_rows_out, unread_out, stream);
  const RowPrune prune{zone_prune, &z, chunk_pruned_out};
  return engine_aggregate_terms(nchunks, jobs.get(), row_bytes, f, w, (AggResult*)total_out, (AggResult*)chunk_out, chunk_status_out, chunk_rows_out, unread_out,
                                (hipStream_t)stream, &prune);
}
int blosc_gpu_aggregate_zoned_batch(int nchunks, const void* const* src, size_t row_bytes, const blosc_gpu_field* field, const blosc_gpu_term* terms, int nterms,
                                    const blosc_gpu_field* zfields, int nzfields, const blosc_gpu_aggregate* zones, blosc_gpu_aggregate* total_out,
                                    blosc_gpu_aggregate* chunk_out, int* chunk_status_out, int* chunk_rows_out, size_t* unread_out, uint8_t* chunk_pruned_out,
                                    void* stream) {
  AggField f; WhereTerms w;
  int c = aggregate_clauses_opening(nchunks, row_bytes, field, terms, nterms, &f, &w);
  if (c == kGo) c = zones_opening(row_bytes, zfields, nzfields, zones);
  if (c != kGo) return c;
  if (nchunks > 0 && !src) return -1;
  const ZoneMap z{terms, nterms, zfields, nzfields, zones};
  return aggregate_zoned_call(nchunks, jobs_from_arrays(nchunks, src, nullptr, nullptr, nullptr), row_bytes, f, w, z, total_out, chunk_out, chunk_status_out,
                              chunk_rows_out, unread_out, chunk_pruned_out, stream);
}
int blosc_gpu_aggregate_zoned_packed(int nchunks, const void* container, size_t containersize, const size_t* offsets, size_t row_bytes, const blosc_gpu_field* field,
                                     const blosc_gpu_term* terms, int nterms, const blosc_gpu_field* zfields, int nzfields, const blosc_gpu_aggregate* zones,
                                     blosc_gpu_aggregate* total_out, blosc_gpu_aggregate* chunk_out, int* chunk_status_out, int* chunk_rows_out, size_t* unread_out,
                                     uint8_t* chunk_pruned_out, void* stream) {
  AggField f; WhereTerms w;
  int c = aggregate_clauses_opening(nchunks, row_bytes, field, terms, nterms, &f, &w);
  if (c == kGo) c = zones_opening(row_bytes, zfields, nzfields, zones);
  if (c != kGo) return c;
  if (nchunks > 0 && (!container || !offsets)) return -1;
  const ZoneMap z{terms, nterms, zfields, nzfields, zones};
  return aggregate_zoned_call(nchunks, jobs_from_spans(nchunks, container, containersize, offsets, nullptr, BLOSC_MIN_HEADER_LENGTH), row_bytes, f, w, z, total_out,
                              chunk_out, chunk_status_out, chunk_rows_out, unread_out, chunk_pruned_out, stream);
}

// ---- adler32 / crc32 of many runs (include/blosc_gpu_checksum.h) ---------------------------------------
int blosc_gpu_checksum_batch(int kind, int nruns, const void* const* src, const size_t* nbytes, unsigned int* digest_out, void* stream) {
  const int c = checksum_opening(kind, nruns);
  if (c != kGo) return c;
  if (!src || !nbytes || !digest_out) return -1;
  return checksum_call(kind, nruns, jobs_from_arrays(nruns, src, nullptr, nbytes, nullptr), digest_out, stream);
}
int blosc_gpu_checksum_packed(int kind, int nruns, const void* container, size_t containersize, const size_t* offsets,
                              const size_t* length, unsigned int* digest_out, void* stream) {
  const int c = checksum_opening(kind, nruns);
  if (c != kGo) return c;
  if (!offsets || !digest_out) return -1;
  if (!container && offsets[nruns] > offsets[0]) return -1;      // no container: only for a table of empty spans (jobs_from_spans() checks that it rises)
  return checksum_call(kind, nruns, jobs_from_spans(nruns, container, containersize, offsets, length, 0), digest_out, stream);
}

// test hooks of the persistent grids (engine.h)
__attribute__((visibility("default"))) int blosc_internal_persistent_grids(int cap, const char** names, int* launched, int* occupancy) {
  return bamd::engine_persistent_grids(cap, names, launched, occupancy);
}
__attribute__((visibility("default"))) int blosc_internal_enc_lz_occupancy(int dynamic_lds) { return bamd::engine_enc_lz_occupancy(dynamic_lds); }
__attribute__((visibility("default"))) void blosc_internal_last_compress_tasks(unsigned out[3]) { bamd::engine_last_compress_tasks(out); }

// Filters as stand-alone calls on HOST buffers, same names and signatures as the symbols the
// reference exports for its own shuffle tests (blosc/shuffle.h:34-61 under BLOSC_TESTING).  The
// shuffle variants of the byte filter with a bitshuffle-only case (bsize < typesize: not applied,
// blosc/blosc.c:608-609) are handled by the kernels exactly like inside a chunk.
__attribute__((visibility("default"))) void blosc_internal_shuffle(const size_t typesize, const size_t blocksize,
                                                                   const uint8_t* src, const uint8_t* dest) {
  if (engine_filter(0, typesize, blocksize, src, (void*)dest) != 0) fprintf(stderr, "blosc_amd: shuffle failed (no GPU?)\n");
}
__attribute__((visibility("default"))) void blosc_internal_unshuffle(const size_t typesize, const size_t blocksize,
                                                                     const uint8_t* src, const uint8_t* dest) {
  if (engine_filter(1, typesize, blocksize, src, (void*)dest) != 0) fprintf(stderr, "blosc_amd: unshuffle failed (no GPU?)\n");
}
// the "generic" entry points the reference's tests/test_shuffle_roundtrip_generic.c links (blosc/shuffle-generic.h:86-93):
// same byte transposition, there is only one implementation here
__attribute__((visibility("default"))) void blosc_internal_shuffle_generic(const size_t typesize, const size_t blocksize,
                                                                           const uint8_t* const src, uint8_t* const dest) {
  blosc_internal_shuffle(typesize, blocksize, src, dest);
}
__attribute__((visibility("default"))) void blosc_internal_unshuffle_generic(const size_t typesize, const size_t blocksize,
                                                                             const uint8_t* const src, uint8_t* const dest) {
  blosc_internal_unshuffle(typesize, blocksize, src, dest);
}
// ... and the names its SSE2 / AVX2 translation units export for tests/test_shuffle_roundtrip_{sse2,avx2}.c (blosc/shuffle-sse2.h:25-32,
// blosc/shuffle-avx2.h:25-32): there is one implementation here - the HIP kernels
#define BAMD_SHUFFLE_ALIAS(isa)                                                                                                                  \
  __attribute__((visibility("default"))) void blosc_internal_shuffle_##isa(const size_t typesize, const size_t blocksize, const uint8_t* const src, \
                                                                           uint8_t* const dest) { blosc_internal_shuffle(typesize, blocksize, src, dest); } \
  __attribute__((visibility("default"))) void blosc_internal_unshuffle_##isa(const size_t typesize, const size_t blocksize, const uint8_t* const src, \
                                                                             uint8_t* const dest) { blosc_internal_unshuffle(typesize, blocksize, src, dest); }
BAMD_SHUFFLE_ALIAS(sse2)
BAMD_SHUFFLE_ALIAS(avx2)
#undef BAMD_SHUFFLE_ALIAS
__attribute__((visibility("default"))) int blosc_internal_bitshuffle(const size_t typesize, const size_t blocksize,
                                                                     const uint8_t* src, const uint8_t* dest,
                                                                     const uint8_t* tmp) {
  (void)tmp;
  if (engine_filter(2, typesize, blocksize, src, (void*)dest) != 0) return -1;
  const size_t n = blocksize / typesize;                      // return value of shuffle.c:393-416
  return (int)((n % 8) ? n : n * typesize);
}
__attribute__((visibility("default"))) int blosc_internal_bitunshuffle(const size_t typesize, const size_t blocksize,
                                                                       const uint8_t* src, const uint8_t* dest,
                                                                       const uint8_t* tmp) {
  (void)tmp;
  if (engine_filter(3, typesize, blocksize, src, (void*)dest) != 0) return -1;
  const size_t n = blocksize / typesize;
  return (int)((n % 8) ? n : n * typesize);
}

// test hooks for the host policy (tests/test_host_abi.py::test_policy_equals_oracle compares them with the oracle)
__attribute__((visibility("default"))) int blosc_amd_policy_blocksize(int clevel, int typesize, int nbytes, int forced,
                                                                      int codec, int splitmode) {
  return compute_blocksize(clevel, typesize, nbytes, forced, codec, splitmode);
}
__attribute__((visibility("default"))) int blosc_amd_policy_split(int codec, int typesize, int blocksize, int splitmode) {
  return split_block(codec, typesize, blocksize, splitmode);
}
// test hook for the pass logic of the batched getitem (tests/test_gpu_getitem_ranges.py, tests/test_emu_getitem_ranges.py): 0 = the default bound
__attribute__((visibility("default"))) void blosc_amd_getitem_pass_bytes(size_t bytes) { engine_getitem_pass_bytes(bytes); }

// test hook for the tile logic of the checksum calls (tests/test_emu_checksum.py): 0 = the default tile
__attribute__((visibility("default"))) void blosc_amd_checksum_tile_bytes(size_t bytes) { engine_checksum_tile_bytes(bytes); }

void blosc_gpu_profile(int enable) { engine_prof_enable(enable); }
void blosc_gpu_profile_reset(void) { engine_prof_reset(); }
int blosc_gpu_profile_get(const char* kernel, double* total_ms, int* launches) { return engine_prof_get(kernel, total_ms, launches); }

}  // extern "C"
