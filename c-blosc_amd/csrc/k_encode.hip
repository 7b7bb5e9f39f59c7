// k_encode.hip — per-stream LZ4 / BloscLZ encoders and the chunk assembly kernels
// (rows K4, K6, C1, S1, T1 of SURVEY §8a).
//
// Replaces blosc_c's split loop (blosc/blosc.c:635-719) with its codec calls
//   LZ4_compress_fast   (lz4.c:1453 -> LZ4_compress_generic_validated :930-1338)
//   blosclz_compress    (blosc/blosclz.c:421-613)
// and serial_blosc/t_blosc's output placement (blosc/blosc.c:814-860, :1843-1860).
//
// The compressed BYTES are not the reference's (no reference test pins them, and the
// reference's own multi-threaded output order is nondeterministic); the contract is the
// FORMAT: every stream written here decodes with stock LZ4_decompress_safe /
// blosclz_decompress, every chunk with stock blosc_decompress (tests/ check exactly that).
//
// One kernel per batch (k_encode_streams): persistent wavefronts draw tasks from per-XCD queues - "shuffle
// block b" (typesize 4 / 8; the transposes run underneath the match finding of other waves) or "encode
// stream s".  Match finder, one wavefront per stream: the 64 lanes look at 64 consecutive positions at once
// (own bytes out of a 768-byte register window), probe a 2048-entry tagged hash table in LDS (LZ4's 4-byte
// multiplicative hash) plus distance 1, rank the candidates by exact match length (up to 20 bytes), extend
// the winner backwards and forwards with ballots, emit the sequence with the whole wave, and pick again
// among the lanes behind the match while it ends inside the step.  DESIGN.md 3.3 has the measurements.
//
// Layout: this file holds the per-stream dispatch (encode_one_stream), the persistent kernel in its modes and the chunk
// assembly kernels; the wave-level code it dispatches to sits in enc_lz.h (match finders: plain and LZ4HC-grade),
// enc_zstd.h (Zstd frames, per-block tables), enc_zlib.h (zlib streams) and enc_shuffle.h (the fused byte shuffle and the
// periodic-plane shortcut) - textual parts of this translation unit, included below inside namespace bamd.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_types.h"
#include "wave_prims.h"
#include "zstd_enc.h"
#include "deflate_enc.h"

namespace bamd {

// Optional phase profiling of the encoder (prof build, scripts/enc_phase.py); same slot layout as k_decode.hip's.
// slots: 0 steps, 1 steps without a match, 2 forward extensions, 3 literal runs copied from memory, 6 sequences,
//        5 backward extensions tried, 7 of those > 0 bytes, 4 of those > 4 bytes
//        (Zstd: 4 cycles tail literals + offset values, 5 cycles sequences section)
//        13 cycles: waiting for the block's shuffle task
//        8 cycles: window+probe, 9 candidates+select, 10 extension, 11 emit, 12 tail; 15: the device's real-time clock (100 MHz, one for all CUs) at the stream's end
// and per persistent wave (the kernel's last parameter, scripts/enc_wave_time.py), 16 words: 0-1 real-time clock at entry, 2-3 at exit (s_memtime, the
// shader clock the cycle counts are in, starts differently on every shader engine: it orders nothing between two waves), 4 cycles inside
// encode_one_stream (slot 13 of its streams - the second wait for the block's shuffle - included), 5 inside shuffle_block_task, 6 in the queue loop's
// wait for a block that is not shuffled yet (without the shuffle tasks taken meanwhile), 7 tasks taken, 8 of them streams, 9 shuffle tasks run
// (queue entries and help), 10 XCC id, 12 cycles from entry to exit, 13 the part of 6 in front of the wave's first stream (the launch's ramp).
// What is left of exit - entry is tickets, descriptors and the calls.
#ifdef BAMD_PROFILE_DECODE
#define EPROF_ARG , DecProf& prof_
#define EPROF_PASS , prof_
#else
#define EPROF_ARG
#define EPROF_PASS
#endif

#include "enc_lz.h"
#include "enc_lz4p.h"
#include "enc_zstd.h"
#include "enc_zlib.h"
#include "enc_shuffle.h"

// The modes of k_encode_streams_t, one row each - a launch serves ONE variant, so every kernel carries only its own code path.  A row says which
// writer the mode ends in (LZ: LZ4 / BloscLZ by the stream's format) and what stands in front of or inside it: `search` the LZ4HC-grade search
// (enc_lz.h) instead of the plain match finder, `tables` Zstd sequence tables made per block instead of the predefined ones, `huffman`
// Huffman-coded Zstd literals, `dynamic` zlib with dynamic Huffman codes (two passes).  Everything else that has to know a mode - the
// dispatch, LDS, register budget and scratch below, the host's grid table, its choice of a variant and its launch (engine.hip) - reads the row.
// The rows' order is the modes' numbering (kernel symbols, profiles/ and scripts/make_traffic_json.py count on it): new rows go to the end.
enum { FAM_LZ, FAM_ZSTD, FAM_ZLIB };
struct EncMode { const char* name; int family; bool search, tables, huffman, dynamic; };
//    mode             family    search tables huffman dynamic
#define BAMD_ENC_MODES(ROW) \
  ROW(ENC_LZ,          FAM_LZ,   false, false, false, false) \
  ROW(ENC_ZSTD,        FAM_ZSTD, false, false, false, false) \
  ROW(ENC_ZLIB,        FAM_ZLIB, false, false, false, false) \
  ROW(ENC_HC,          FAM_LZ,   true,  false, false, false) \
  ROW(ENC_ZSTD_T,      FAM_ZSTD, false, true,  false, false) \
  ROW(ENC_ZSTD_HC,     FAM_ZSTD, true,  true,  false, false) \
  ROW(ENC_ZLIB_HC,     FAM_ZLIB, true,  false, false, false) \
  ROW(ENC_ZSTD_TH,     FAM_ZSTD, false, true,  true,  false) \
  ROW(ENC_ZSTD_HCH,    FAM_ZSTD, true,  true,  true,  false) \
  ROW(ENC_ZLIB_DYN,    FAM_ZLIB, false, false, false, true)  \
  ROW(ENC_ZLIB_DYN_HC, FAM_ZLIB, true,  false, false, true)
#define BAMD_ENC_ENUMERATOR(NAME, ...) NAME,
#define BAMD_ENC_ROW(NAME, ...) {"k_encode_streams_t<" #NAME ">", __VA_ARGS__},
enum { BAMD_ENC_MODES(BAMD_ENC_ENUMERATOR) kEncModes };
constexpr EncMode kEncMode[kEncModes] = {BAMD_ENC_MODES(BAMD_ENC_ROW)};      // (name: the kernel instance with the enumerator spelled out)
#undef BAMD_ENC_ENUMERATOR
#undef BAMD_ENC_ROW
// sequence scratch of one persistent wave in 64-bit words: the Zstd writers' sequences, the tokens of dynamic zlib's first pass.  The kernel
// strides by it, the host allocates by it.
constexpr uint32_t enc_seq_words(int mode) { return kEncMode[mode].family == FAM_ZSTD ? ZS_SEQCAP : (kEncMode[mode].dynamic ? ZD_SCRATCH_U64 : 0u); }
#ifndef BAMD_ENC_HELP
#define BAMD_ENC_HELP 256     // a wave whose stream's block is not shuffled yet takes shuffle tasks instead of sleeping, up to this many blocks ahead (0: never)
#endif
// one stream, not inlined into the queue loop (see decode_one_stream in k_decode.hip for why)
template <int MODE>
__device__ __attribute__((noinline)) void encode_one_stream(StreamDesc* sd_, enc_entry_t* tab_, const ChunkDesc* chunks_, uint32_t* blk_ready_, int lane,
                                                            const BlockDesc* blocks_, uint32_t sid_, uint32_t* plane_cost_, uint64_t* seqbuf_
#ifdef BAMD_PROFILE_DECODE
                                                            , uint32_t* profslot_
#endif
                                                            ) {
  StreamDesc* sd; enc_entry_t* tab; const ChunkDesc* chunks; uint32_t* blk_ready; const BlockDesc* blocks; uint32_t sid; uint32_t* plane_cost; uint64_t* seqbuf;
#ifdef BAMD_PROFILE_DECODE
  uint32_t* profslot;
#endif
  PROF_DECL
#ifdef BAMD_PROFILE_DECODE
  prof_.c[4] = 0; prof_.c[5] = 0;
#endif
  // The arguments of a real call arrive in vector registers; every one of them is wave-uniform and most are needed again behind the encoder's loop.
  // Left where they are they cost the loop 16 of its 80 registers - or are spilled and RELOADED inside it, and a scratch reload waits for vmcnt(0),
  // i.e. for the step's stores (round 6: the parallel LZ4 step at 9.2 ms instead of 8.2 until these moved to scalar registers).
  sd = uni_gp(sd_); tab = uni_gp(tab_); chunks = uni_gp(chunks_); blk_ready = uni_gp(blk_ready_); blocks = uni_gp(blocks_);
  plane_cost = uni_gp(plane_cost_); seqbuf = uni_gp(seqbuf_); sid = uni(sid_);
#ifdef BAMD_PROFILE_DECODE
  profslot = uni_gp(profslot_);
#endif
  const uint32_t n = uni((uint32_t)sd->in_size), cap = uni((uint32_t)sd->out_size);
  const uint32_t aux = uni((uint32_t)sd->aux);
  const int clevel = (int)(aux & 15u);
  if (uni(chunks[uni((uint32_t)sd->chunk)].mode) & CH_FUSED_SHUF) {
    // the block's shuffle task sits earlier in this XCD's queue, so a running wave already owns it
    const uint32_t gb = aux >> 4;
    while (__hip_atomic_load(&blk_ready[gb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) __builtin_amdgcn_s_sleep(16);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  PROF_LAP(13);
  const uint64_t cost_t0 = __builtin_amdgcn_s_memtime();
  uint32_t r;
  const int32_t hint = (int32_t)uni((uint32_t)sd->result);      // < 0: the shuffle task found this plane periodic (period -hint)
  constexpr EncMode M = kEncMode[MODE];
  if (M.family == FAM_ZSTD) r = seqbuf ? zstd_encode_wave<M.tables, M.search, M.huffman>(uni_ptr(as_global(sd->in)), n, uni_ptr(as_global(sd->out)), cap, clevel, tab, (BAMD_GAS uint64_t*)seqbuf, lane EPROF_PASS) : 0u;
  else if (M.dynamic) r = seqbuf ? zlib_dyn_encode_wave<M.search>(uni_ptr(as_global(sd->in)), n, uni_ptr(as_global(sd->out)), cap, clevel, tab, (BAMD_GAS uint64_t*)seqbuf, lane EPROF_PASS) : 0u;
  else if (M.family == FAM_ZLIB) r = zlib_encode_wave<M.search>(uni_ptr(as_global(sd->in)), n, uni_ptr(as_global(sd->out)), cap, clevel, tab, lane EPROF_PASS);
  else if (hint < 0) r = emit_periodic_stream(uni_ptr(as_global(sd->in)), n, uni_ptr(as_global(sd->out)), cap, (uint32_t)-hint, uni((uint32_t)sd->fmt) == (uint32_t)FMT_LZ4, lane);
  else if (M.search) r = lz4hc_encode_wave(uni_ptr(as_global(sd->in)), n, uni_ptr(as_global(sd->out)), cap, tab, lane);
  else if (sd->fmt == FMT_LZ4) r = BAMD_ENC_PAR ? lz4_encode_wave_auto(uni_ptr(as_global(sd->in)), n, uni_ptr(as_global(sd->out)), cap, clevel, tab, lane EPROF_PASS)
                                                : lz_encode_wave<EF_LZ4>(uni_ptr(as_global(sd->in)), n, uni_ptr(as_global(sd->out)), cap, clevel, tab, lane EPROF_PASS);
  else r = lz_encode_wave<EF_BLOSCLZ>(uni_ptr(as_global(sd->in)), n, uni_ptr(as_global(sd->out)), cap, clevel, tab, lane EPROF_PASS);
  if (lane == 0) sd->result = (int32_t)r;
  // cost feedback for the host's queue order (queue_order.h: build_encode_queues): cycles per plane index
  if (plane_cost && lane == 0) {
    const uint32_t j = sid - (uint32_t)blocks[aux >> 4].first_stream;
    atomicAdd(plane_cost + (j & 255u), (uint32_t)((__builtin_amdgcn_s_memtime() - cost_t0) >> 10));
  }
#ifdef BAMD_PROFILE_DECODE
  prof_.c[15] = (uint32_t)__builtin_amdgcn_s_memrealtime();
  if (lane == 0 && profslot) for (int i_ = 0; i_ < 16; i_++) profslot[i_] = prof_.c[i_];
#endif
}

// Persistent waves + per-XCD ticket queues, like k_decode_streams (stream costs differ by orders of
// magnitude).  A queue entry >= 0 is a stream to encode; an entry < 0 is "shuffle block -(entry+1)".  The
// host puts every block's shuffle task a few dozen entries ahead of its streams (queue_order.h:
// build_encode_queues), so the bandwidth-bound transposes run underneath the latency/issue-bound match
// finding of other waves instead of in a kernel of their own.
// LDS of one workgroup: the match finder's table, the writers' LDS behind it (ENC_LZ: the 64 scratch dwords of the parallel LZ4 emitter, enc_lz4p.h)
constexpr int enc_tab_bytes(int mode) { return kEncMode[mode].search ? HC_TAB_BYTES : ENC_TAB_BYTES; }
constexpr int enc_writer_lds_bytes(int mode) { return kEncMode[mode].family == FAM_ZSTD ? ZS_LDS_BYTES : (kEncMode[mode].family == FAM_ZLIB ? DFL_LDS_BYTES : (mode == ENC_LZ ? ENC_SCR_BYTES : 0)); }
constexpr int enc_lds_bytes(int mode) { return enc_tab_bytes(mode) + enc_writer_lds_bytes(mode); }
// waves per SIMD the register allocator plans for: the 24 KiB table of the search leaves room for 1.5, the LDS of Zstd with per-block tables for 5
constexpr int enc_min_waves(int mode) { return kEncMode[mode].search ? 2 : (kEncMode[mode].tables ? 5 : (mode == ENC_LZ ? BAMD_ENC_LZ_MINWAVES : BAMD_ENC_MINWAVES)); }
// upper bound of the persistent grid per CU: whole LDS granules (enc_lz.h), and no more waves than the CU has slots for.  The launch takes the
// runtime's occupancy figure (engine.hip: query_persistent_grids), which also knows the registers the compiler really used.
constexpr int enc_grid_bound(int mode) { return lds_workgroups_per_cu(enc_lds_bytes(mode)) < 32 ? lds_workgroups_per_cu(enc_lds_bytes(mode)) : 32; }
template <int MODE>
__global__ __launch_bounds__(64 * ENC_WAVES, enc_min_waves(MODE)) void k_encode_streams_t(
    StreamDesc* __restrict__ streams, uint32_t* __restrict__ tickets /*[8]*/, const int32_t* __restrict__ qlist,
    const int32_t* __restrict__ qoff /*[9]*/, const int32_t* __restrict__ shoff /*[9] | shuffle list*/, const ChunkDesc* __restrict__ chunks, const BlockDesc* __restrict__ blocks,
    uint32_t* __restrict__ blk_ready, uint32_t* __restrict__ plane_cost, int single_queue,
    uint64_t* __restrict__ seqbufs, const zenc::CTabs* __restrict__ ctabs, int detect_periodic
#ifdef BAMD_PROFILE_DECODE
    , uint32_t* __restrict__ profbuf, uint32_t* __restrict__ profwave
#endif
    ) {
#ifdef BAMD_PROFILE_DECODE
  const uint64_t wt_entry = __builtin_amdgcn_s_memtime(), wr_entry = __builtin_amdgcn_s_memrealtime();
  uint64_t wt_stream = 0, wt_shuffle = 0, wt_wait = 0, wt_wait_first = 0;
  uint32_t wn_stream = 0, wn_shuffle = 0;
#define WPROF_BEGIN(t) const uint64_t t = __builtin_amdgcn_s_memtime()
#define WPROF_END(acc, t) acc += __builtin_amdgcn_s_memtime() - t
#else
#define WPROF_BEGIN(t)
#define WPROF_END(acc, t)
#endif
  constexpr bool ZSTD = kEncMode[MODE].family == FAM_ZSTD;
  constexpr uint32_t SEQWORDS = enc_seq_words(MODE);
  constexpr int TABBYTES = enc_tab_bytes(MODE);      // the match finder's table; the writers' LDS sits behind it
  // declared in whole granules, which is what the workgroup occupies anyway: the runtime's occupancy figure divides the CU's LDS by the declared size
  // (profiles/r07b_lds_granule.txt) and is the resident count only then
  __shared__ __attribute__((aligned(16))) enc_entry_t tabs[ENC_WAVES][lds_occupied(enc_lds_bytes(MODE)) / 4];
  static_assert(ENC_WAVES == 1, "one stream per wave, one wave per workgroup");
  const int lane = threadIdx.x & 63;
  if (ZSTD) {       // the predefined FSE tables of the sequence coder, once per persistent wave
    const uint32_t* g = (const uint32_t*)ctabs;
    for (uint32_t k = (uint32_t)lane; k < sizeof(zenc::CTabs) / 4u; k += 64u) tabs[0][TABBYTES / 4 + k] = g[k];
  }
  uint64_t* seqbuf = SEQWORDS ? seqbufs + (size_t)blockIdx.x * SEQWORDS : nullptr;      // this wave's sequence scratch
  // HW_REG_XCC_ID[3:0]; queue 0 for everybody in the single-queue fallback (no in-kernel hand-offs there)
  const uint32_t xcc = single_queue ? 0u : (__builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u);
  const uint32_t qbase = (uint32_t)qoff[xcc], qlen = (uint32_t)qoff[xcc + 1] - qbase;
  // Shuffle tasks are claimed in list order through a counter of their own (queue_order.h): a negative queue entry means "one
  // shuffle task", and a wave whose stream's block is not ready yet claims shuffle tasks too instead of sleeping.  No deadlock: a
  // shuffle task never waits, and a stream waits only for a block whose task either is claimed by a running wave or is still on
  // the list - where the waiting wave itself reaches it (claims are in list order, the list is finite).
  const uint32_t shbase = (uint32_t)shoff[xcc], shlen = (uint32_t)shoff[xcc + 1] - shbase;
  const int32_t* shlist = shoff + 9;
  auto shuffle_one = [&]() -> bool {
    const uint32_t s = take_ticket(tickets + 8 + xcc, lane);
    if (s >= shlen) return false;
    WPROF_BEGIN(ts_);
    shuffle_block_task(chunks, blocks, uni((uint32_t)shlist[shbase + s]), blk_ready, streams, detect_periodic, lane, (volatile uint32_t*)tabs[0]);
    WPROF_END(wt_shuffle, ts_);
#ifdef BAMD_PROFILE_DECODE
    wn_shuffle++;
#endif
    return true;
  };
  uint32_t t = take_ticket(tickets + xcc, lane);
  uint32_t ndone = 0;      // tasks this wave took: summed into plane_cost[256], the host checks the total
  while (t < qlen) {
    const int32_t task = (int32_t)uni((uint32_t)qlist[qbase + t]);
    if (task < 0) {
      shuffle_one();
    } else {
      const StreamDesc* sd = streams + task;
      if (uni(chunks[uni((uint32_t)sd->chunk)].mode) & CH_FUSED_SHUF) {
        const uint32_t gb = uni((uint32_t)sd->aux) >> 4;
        // only for the LDS-tile shuffle of the "other" typesizes (a task of theirs takes a wave several times as long as the register forms
        // of 2 / 4 / 8 / 16, so the few waves that drew the negative entries cannot keep incompressible data coming: random bytes, typesize 6:
        // 13.3 -> 9.6 ms).  With the fast forms helping costs 4 % on compressible data and gains nothing on random bytes
        // (profiles/r04/r04z2_enc_ab_help_bound_variants.txt).
        const ChunkDesc* cd = chunks + uni((uint32_t)sd->chunk);
        bool more = !(uni(cd->mode) & CH_BITSHUFFLE) && shuffle_generic_T(uni((uint32_t)cd->typesize));
#ifdef BAMD_PROFILE_DECODE
        const uint64_t tw_ = __builtin_amdgcn_s_memtime(), sh0_ = wt_shuffle;
#endif
        while (__hip_atomic_load(&blk_ready[gb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
          // ... but not further ahead of its own block than BAMD_ENC_HELP blocks of the list: planes shuffled much earlier than they are
          // encoded have left the L2 / MALL by then (unbounded: config 2 + 7 %, profiles/r04/r04z_enc_ab_help_unbounded_vs_off.txt)
          if (BAMD_ENC_HELP && more && __hip_atomic_load(tickets + 8 + xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (single_queue ? gb : gb / 8u) + (uint32_t)BAMD_ENC_HELP) more = shuffle_one();
          else __builtin_amdgcn_s_sleep(16);
        }
#ifdef BAMD_PROFILE_DECODE
        wt_wait += (__builtin_amdgcn_s_memtime() - tw_) - (wt_shuffle - sh0_);
        if (wn_stream == 0) wt_wait_first = wt_wait;
#endif
      }
#ifdef BAMD_PROFILE_DECODE
      const uint64_t te_ = __builtin_amdgcn_s_memtime();
      encode_one_stream<MODE>(streams + task, tabs[0], chunks, blk_ready, lane, blocks, (uint32_t)task, plane_cost, seqbuf, profbuf ? profbuf + (size_t)task * 16 : nullptr);
      wt_stream += __builtin_amdgcn_s_memtime() - te_; wn_stream++;
#else
      encode_one_stream<MODE>(streams + task, tabs[0], chunks, blk_ready, lane, blocks, (uint32_t)task, plane_cost, seqbuf);
#endif
    }
    ndone++;
    t = take_ticket(tickets + xcc, lane);
  }
  if (lane == 0 && ndone) atomicAdd(plane_cost + 256, ndone);
#ifdef BAMD_PROFILE_DECODE
  if (lane == 0 && profwave) {
    uint32_t* w = profwave + (size_t)blockIdx.x * 16;
    const uint64_t wt_exit = __builtin_amdgcn_s_memtime(), wr_exit = __builtin_amdgcn_s_memrealtime();
    w[0] = (uint32_t)wr_entry; w[1] = (uint32_t)(wr_entry >> 32); w[2] = (uint32_t)wr_exit; w[3] = (uint32_t)(wr_exit >> 32);
    w[4] = (uint32_t)wt_stream; w[5] = (uint32_t)wt_shuffle; w[6] = (uint32_t)wt_wait; w[7] = ndone; w[8] = wn_stream; w[9] = wn_shuffle; w[10] = xcc;
    w[11] = 1u;      // the record is written
    w[12] = (uint32_t)(wt_exit - wt_entry); w[13] = (uint32_t)wt_wait_first;
  }
#endif
#undef WPROF_BEGIN
#undef WPROF_END
}

// The stream table of a compress call, one thread per block: stream s of block j reads the block's split s out of the filtered image
// (or the source when the chunk has no filter) and writes into its staging slot of the same size (blosc/blosc.c:608-672: the per-split loop
// of blosc_c).  Made here instead of on the host: for 8 GiB that table is 2.6 MB - built, copied to pinned memory and uploaded per call
// it cost 0.2 ms of host time in front of every launch (round 4, BLOSC_AMD_HOSTTIME).
__global__ __launch_bounds__(256) void k_encode_plan(const ChunkDesc* __restrict__ chunks, const BlockDesc* __restrict__ blocks,
                                                     StreamDesc* __restrict__ streams, int nblocks_total) {
  const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (g >= nblocks_total) return;
  const BlockDesc b = blocks[g];
  if (b.nstreams <= 0) return;
  const ChunkDesc& c = chunks[b.chunk];
  const uint8_t* inbase = (c.mode & (CH_SHUFFLE | CH_BITSHUFFLE)) ? c.filt : c.src;
  const int32_t neblock = b.bsize / b.nstreams;
  const size_t at = (size_t)b.blk * (size_t)c.blocksize;
  for (int32_t k = 0; k < b.nstreams; k++) {
    StreamDesc sd;
    sd.in = inbase + at + (size_t)k * (size_t)neblock;
    sd.out = c.stage + at + (size_t)k * (size_t)neblock;
    sd.in_size = neblock; sd.out_size = neblock; sd.chunk = b.chunk; sd.fmt = c.fmt; sd.aux = c.clevel | (int32_t)((uint32_t)g << 4); sd.result = 0;
    streams[(size_t)b.first_stream + k] = sd;
  }
}

// ---------------------------------------------------------------------------------------------
// chunk assembly
// ---------------------------------------------------------------------------------------------
// k_chunk_scan: one workgroup per chunk.  Sums 4 + csize over each block's streams, prefix-sums
// the blocks IN BLOCK ORDER (deterministic layout; the reference's threaded path is completion
// order, blosc.c:1845-1860), writes the 16-byte header (blosc.c:1154-1244, :1275) and bstarts
// (absolute offsets, blosc.c:816), and decides the whole-chunk fallbacks (blosc.c:1264-1272):
//   total <= maxbytes            -> regular chunk,          result = total
//   else nbytes + 16 <= maxbytes -> MEMCPYED chunk,         result = nbytes + 16
//   else                         -> does not fit,           result = 0
constexpr int SCAN_THREADS = 256;

__device__ __forceinline__ void st_i32(gu8* p, int32_t v) { g_st_i32le(p, v); }

// PACKED (blosc_gpu_compress_packed): the chunk's place is chosen from its size, by k_packed_layout behind this kernel - sizes, block
// offsets and fallbacks as below, but nothing is written to c.dst (header and bstarts: k_packed_headers)
template <bool PACKED>
__device__ __forceinline__ void chunk_scan(ChunkDesc* __restrict__ chunks,
                                           const BlockDesc* __restrict__ blocks,
                                           const StreamDesc* __restrict__ streams,
                                           int32_t* __restrict__ blk_off,   // [nblocks_total] out
                                           int32_t* __restrict__ results) { // [nchunks] out
  __shared__ int32_t part[SCAN_THREADS];
  __shared__ int32_t carry_s;
  const int cid = blockIdx.x, tid = threadIdx.x;
  ChunkDesc& c = chunks[cid];
  if (c.mode & CH_SKIP) return;
  gu8* d = as_global(c.dst);
  if (c.mode & CH_MEMCPYED) {  // decided on the host (clevel 0 / nbytes < 128, blosc.c:1219-1229)
    if (tid == 0) {
      if (!PACKED) {
        d[0] = 2; d[1] = 1; d[2] = (uint8_t)c.hdr_flags; d[3] = (uint8_t)c.typesize;  // versionlz byte: see below
        st_i32(d + 4, c.nbytes); st_i32(d + 8, c.blocksize); st_i32(d + 12, c.nbytes + 16);
      }
      results[cid] = c.nbytes + 16;
    }
    return;
  }
  if (tid == 0) carry_s = 16 + 4 * c.nblocks;
  __syncthreads();
  for (int base = 0; base < c.nblocks; base += SCAN_THREADS) {
    const int j = base + tid;
    int32_t mine = 0;
    if (j < c.nblocks) {
      const BlockDesc b = blocks[c.first_block + j];
      for (int s = 0; s < b.nstreams; s++) {
        const StreamDesc& sd = streams[b.first_stream + s];
        mine += 4 + (sd.result > 0 ? sd.result : sd.in_size);
      }
    }
    part[tid] = mine;
    __syncthreads();
    // inclusive Hillis-Steele scan over the 256 partials
    for (int o = 1; o < SCAN_THREADS; o <<= 1) {
      int32_t v = (tid >= o) ? part[tid - o] : 0;
      __syncthreads();
      part[tid] += v;
      __syncthreads();
    }
    const int32_t carry = carry_s;
    // saturate instead of wrapping: a chunk cannot exceed INT_MAX anyway
    if (j < c.nblocks) {
      int64_t start = (int64_t)carry + part[tid] - mine;
      blk_off[c.first_block + j] = start > 0x7fffffff ? 0x7fffffff : (int32_t)start;
    }
    __syncthreads();
    if (tid == SCAN_THREADS - 1) {
      int64_t nc = (int64_t)carry + part[tid];
      carry_s = nc > 0x7fffffff ? 0x7fffffff : (int32_t)nc;
    }
    __syncthreads();
  }
  const int32_t total = carry_s;
  const int32_t maxbytes = c.cbytes;
  int32_t res;
  uint32_t flags = (uint32_t)c.hdr_flags;
  if (total <= maxbytes) {
    res = total;
    if (!PACKED) for (int j = tid; j < c.nblocks; j += SCAN_THREADS) st_i32(d + 16 + 4 * (size_t)j, blk_off[c.first_block + j]);
  } else if ((int64_t)c.nbytes + 16 <= (int64_t)maxbytes) {
    res = c.nbytes + 16;
    flags |= 0x2u;
    if (tid == 0) c.mode |= CH_MEMCPYED;   // compact kernel copies the raw input instead
  } else {
    res = 0;
    if (tid == 0) c.mode |= CH_SKIP;
  }
  if (tid == 0) {
    if (!PACKED) {
      d[0] = 2;                      // BLOSC_VERSION_FORMAT (blosc.h:29)
      d[1] = 1;                      // codec format version, 1 for every codec (blosc.h:104-109)
      d[2] = (uint8_t)flags; d[3] = (uint8_t)c.typesize;
      st_i32(d + 4, c.nbytes); st_i32(d + 8, c.blocksize); st_i32(d + 12, res);
    }
    results[cid] = res;
  }
}
__global__ __launch_bounds__(SCAN_THREADS) void k_chunk_scan(ChunkDesc* __restrict__ chunks, const BlockDesc* __restrict__ blocks,
                                                            const StreamDesc* __restrict__ streams, int32_t* __restrict__ blk_off,
                                                            int32_t* __restrict__ results) {
  chunk_scan<false>(chunks, blocks, streams, blk_off, results);
}
__global__ __launch_bounds__(SCAN_THREADS) void k_chunk_scan_packed(ChunkDesc* __restrict__ chunks, const BlockDesc* __restrict__ blocks,
                                                                   const StreamDesc* __restrict__ streams, int32_t* __restrict__ blk_off,
                                                                   int32_t* __restrict__ results) {
  chunk_scan<true>(chunks, blocks, streams, blk_off, results);
}

// k_candidate_select (include/blosc_gpu_select.h): ONE wave per chunk of the caller, behind k_chunk_scan_packed and in front of whatever writes
// caller memory.  The entries [first[i], first[i + 1]) of the call's chunk table are the candidate encodings of chunk i, results[] their sizes
// (or the row errors the host found, which it marked CH_SKIP: never winners).  The lanes stride over the range, each keeping the smallest
// key (size, entry) of its entries - the smallest positive size wins, the lowest entry on a tie -, the wave takes the smallest of the 64.
// answers[] gets every entry's result as found; then every entry but the winner becomes a chunk nothing behind this kernel touches:
// CH_SKIP and result 0, as k_packed_layout leaves a chunk that has no place.  choice[i]: the winner relative to first[i], or -1.
// A size never has all 32 bits set, so that is "no size" (INT32_MAX is the size of a MEMCPYED chunk of the largest buffer).
constexpr int SELECT_THREADS = 64;
__global__ __launch_bounds__(SELECT_THREADS) void k_candidate_select(ChunkDesc* __restrict__ chunks, int32_t* __restrict__ results,
                                                                    const int32_t* __restrict__ first,   // [nchunks + 1]
                                                                    int32_t* __restrict__ answers,       // [first[nchunks]] out
                                                                    int32_t* __restrict__ choice) {      // [nchunks] out
  const int i = blockIdx.x, lane = threadIdx.x;
  const int32_t e0 = first[i], e1 = first[i + 1];
  uint64_t best = ~0ull;
  for (int32_t e = e0 + lane; e < e1; e += SELECT_THREADS) {
    const int32_t r = results[e];
    answers[e] = r;
    if (r > 0 && !(chunks[e].mode & CH_SKIP)) {
      const uint64_t key = ((uint64_t)(uint32_t)r << 32) | (uint32_t)e;
      best = key < best ? key : best;
    }
  }
  best = wave_min_u64(best);
  const int32_t winner = (uint32_t)(best >> 32) != 0xffffffffu ? (int32_t)(uint32_t)best : -1;
  for (int32_t e = e0 + lane; e < e1; e += SELECT_THREADS)
    if (e != winner) { chunks[e].mode |= CH_SKIP; results[e] = 0; }
  if (lane == 0) choice[i] = winner >= 0 ? winner - e0 : -1;
}

// k_packed_layout: ONE workgroup walks the batch in tiles of its width, the running offset carried from tile to tile in 64 bits (a container
// passes 4 GiB long before a batch passes a few thousand chunks).  Chunk i of size r_i = max(results[i], 0) starts at
//   off_0 = 0,  off_(i+1) = align_up(off_i + r_i, align)      (every off_i is a multiple of align: a prefix sum of align_up(r_i, align))
// and is written there if it ends inside the caller's buffer: c.dst = dest + off_i.  A chunk that does not gets CH_SKIP and result 0 - nothing of
// it is written by the kernels behind this one - and still counts with its size, so offsets[nchunks] is what the whole batch needs.
__global__ __launch_bounds__(SCAN_THREADS) void k_packed_layout(ChunkDesc* __restrict__ chunks, int32_t* __restrict__ results, int nchunks,
                                                               uint8_t* dest, uint64_t destsize, uint64_t align /* power of two */,
                                                               uint64_t* __restrict__ offsets) {   // [nchunks + 1] out
  __shared__ uint64_t part[SCAN_THREADS];
  __shared__ uint64_t carry_s;
  const int tid = threadIdx.x;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < nchunks; base += SCAN_THREADS) {
    const int i = base + tid;
    uint64_t size = 0, mine = 0;
    if (i < nchunks) {
      const int32_t r = results[i];
      size = r > 0 ? (uint64_t)r : 0;
      mine = (size + align - 1) & ~(align - 1);
    }
    part[tid] = mine;
    __syncthreads();
    for (int o = 1; o < SCAN_THREADS; o <<= 1) {
      uint64_t v = (tid >= o) ? part[tid - o] : 0;
      __syncthreads();
      part[tid] += v;
      __syncthreads();
    }
    const uint64_t carry = carry_s;
    if (i < nchunks) {
      const uint64_t off = carry + part[tid] - mine;
      offsets[i] = off;
      ChunkDesc& c = chunks[i];
      if (!(c.mode & CH_SKIP)) {
        if (off + size <= destsize) c.dst = dest + off;
        else { c.mode |= CH_SKIP; results[i] = 0; }
      }
    }
    __syncthreads();
    if (tid == SCAN_THREADS - 1) carry_s = carry + part[tid];
    __syncthreads();
  }
  if (tid == 0) offsets[nchunks] = carry_s;
}

// k_packed_headers: one workgroup per chunk, behind the layout: header and bstarts of every chunk that has a place, and zeros from its end to
// the next chunk's start (or to the end of the caller's buffer, where that comes first) - a container is a function of its input alone
__global__ __launch_bounds__(SCAN_THREADS) void k_packed_headers(const ChunkDesc* __restrict__ chunks, const int32_t* __restrict__ blk_off,
                                                                const int32_t* __restrict__ results, const uint64_t* __restrict__ offsets,
                                                                uint64_t destsize) {
  const int cid = blockIdx.x, tid = threadIdx.x;
  const ChunkDesc& c = chunks[cid];
  if (c.mode & CH_SKIP) return;
  gu8* d = as_global(c.dst);
  const int32_t res = results[cid];
  const bool memcpyed = (c.mode & CH_MEMCPYED) != 0;      // decided on the host or by the scan
  if (!memcpyed) for (int j = tid; j < c.nblocks; j += SCAN_THREADS) st_i32(d + 16 + 4 * (size_t)j, blk_off[c.first_block + j]);
  if (tid == 0) {      // the 16 header bytes, as k_chunk_scan writes them
    d[0] = 2; d[1] = 1; d[2] = (uint8_t)((uint32_t)c.hdr_flags | (memcpyed ? 0x2u : 0u)); d[3] = (uint8_t)c.typesize;
    st_i32(d + 4, c.nbytes); st_i32(d + 8, c.blocksize); st_i32(d + 12, res);
  }
  const uint64_t next = offsets[cid + 1] < destsize ? offsets[cid + 1] : destsize;
  for (uint64_t k = offsets[cid] + (uint64_t)res + (uint64_t)tid; k < next; k += SCAN_THREADS) d[k - offsets[cid]] = 0;
}

// k_chunk_compact: one workgroup per block; moves the block's streams to their final place.
constexpr int COMPACT_THREADS = 256;

__device__ __forceinline__ void wg_copy(gu8* dst, const gu8* src, uint32_t n) {
  const uint32_t tid = threadIdx.x;
  uint32_t full = n & ~15u;
  for (uint32_t k = tid * 16u; k < full; k += COMPACT_THREADS * 16u) st16u(dst + k, ld16u(src + k));
  for (uint32_t k = full + tid; k < n; k += COMPACT_THREADS) dst[k] = src[k];
}

__global__ __launch_bounds__(COMPACT_THREADS) void k_chunk_compact(const ChunkDesc* __restrict__ chunks,
                                                                  const BlockDesc* __restrict__ blocks,
                                                                  const StreamDesc* __restrict__ streams,
                                                                  const int32_t* __restrict__ blk_off) {
  const BlockDesc b = blocks[blockIdx.x];
  const ChunkDesc& c = chunks[b.chunk];
  if (c.mode & CH_SKIP) return;
  const uint32_t bsize = (uint32_t)b.bsize;
  if (c.mode & CH_MEMCPYED) {   // payload = raw input right after the header (blosc.c:825-830)
    wg_copy(as_global(c.dst) + 16 + (size_t)b.blk * c.blocksize, as_global(c.src) + (size_t)b.blk * c.blocksize, bsize);
    return;
  }
  uint32_t pos = (uint32_t)blk_off[blockIdx.x];
  for (int s = 0; s < b.nstreams; s++) {
    const StreamDesc& sd = streams[b.first_stream + s];
    const bool raw = sd.result <= 0;
    const uint32_t sz = raw ? (uint32_t)sd.in_size : (uint32_t)sd.result;
    if (threadIdx.x == 0) st_i32(as_global(c.dst) + pos, (int32_t)sz);
    wg_copy(as_global(c.dst) + pos + 4, as_global(raw ? sd.in : (const uint8_t*)sd.out), sz);
    pos += 4u + sz;
  }
}

// plain byte copy of whole chunks (MEMCPYED chunks on the decompress side, blosc.c:843-848)
__global__ __launch_bounds__(COMPACT_THREADS) void k_copy_chunks(const ChunkDesc* __restrict__ chunks, int src_skip) {
  const ChunkDesc& c = chunks[blockIdx.y];
  if (!(c.mode & CH_MEMCPYED) || (c.mode & CH_SKIP)) return;
  const uint64_t per = (uint64_t)COMPACT_THREADS * 16u * 8u;  // 32 KiB per workgroup step
  for (uint64_t lo = (uint64_t)blockIdx.x * per; lo < (uint64_t)c.nbytes; lo += (uint64_t)gridDim.x * per) {
    uint64_t hi = lo + per < (uint64_t)c.nbytes ? lo + per : (uint64_t)c.nbytes;
    wg_copy(as_global(c.dst) + lo, as_global(c.src) + src_skip + lo, (uint32_t)(hi - lo));
  }
}

}  // namespace bamd
