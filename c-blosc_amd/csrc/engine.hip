// engine.hip — host engine implementation (see engine.h).  Compiled together with the kernels.
#include "engine.h"

#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>
#include <algorithm>

#include <chrono>
#include "blosc_format.h"
#include "dev_types.h"
#include "queue_order.h"

#include "k_filters.hip"
#include "k_decode.hip"
#include "k_encode.hip"
#include "k_zstd.hip"
#include "k_zstd2.hip"
#include "k_zlib.hip"
#include "k_checksum.hip"
#include "k_take.hip"
#include "k_put.hip"
#include "k_where.hip"
#include "k_aggregate.hip"
#include "k_zones.hip"

namespace bamd {

// ---------------------------------------------------------------------------------------------
// small utilities
// ---------------------------------------------------------------------------------------------
static std::atomic<bool> g_warned{false};
#define HIP_TRY(expr)                                                                             \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) {                                                                       \
      fprintf(stderr, "blosc_amd: HIP error '%s' at %s:%d (%s)\n", hipGetErrorString(_e), __FILE__, __LINE__, #expr); \
      return -1;                                                                                  \
    }                                                                                             \
  } while (0)

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
struct Carver {   // layout helper: sub-allocations inside one arena
  size_t off = 0; size_t take(size_t bytes, size_t align = 256) { off = align_up(off, align); size_t r = off; off += bytes; return r; }
};

// ---------------------------------------------------------------------------------------------
// switches: every BLOSC_AMD_* name the engine reads (INTEGRATION.md has the users' table; BLOSC_AMD_SCHED is queue_order.h's)
// ---------------------------------------------------------------------------------------------
// Two readers.  switch_every_call: for what a test flips between two calls of one process.  SWITCH_ONCE: read at first use and kept -
// a getenv on a production path races with a concurrent setenv of the caller.  SWITCH_SET: "set at all", whatever the value.
constexpr long SWITCH_SET = -0x7fffffffL;
static long switch_every_call(const char* name, long dflt) {
  const char* e = getenv(name);
  return dflt == SWITCH_SET ? (e != nullptr) : (e ? atol(e) : dflt);
}
#define SWITCH_ONCE(name, dflt) ([] { static const long v = switch_every_call(name, dflt); return v; }())
#ifdef BAMD_ENV_EVERY_CALL      // (the placement scripts move the skew between re-allocations inside ONE process: make tune NAME=env DEFS=-DBAMD_ENV_EVERY_CALL)
#define SWITCH_PLACEMENT switch_every_call
#else
#define SWITCH_PLACEMENT SWITCH_ONCE
#endif
#ifndef BAMD_LZ4HC_DEFAULT
#define BAMD_LZ4HC_DEFAULT 1   // "lz4hc" without BLOSC_AMD_LZ4HC in the environment: 1 = LZ4HC-grade search, 0 = plain LZ4 match finder
#endif
#ifndef BAMD_ZSTD_TABLES_DEFAULT
#define BAMD_ZSTD_TABLES_DEFAULT 1   // measured on MI355X (profiles/r03/r03a_encopts_bench_cfg4t.json): bench19 ratio 18.3 -> 23.8 for +5.6 % encode time
#endif
static bool is_on(long v) { return (int)v != 0; }      // every flag parses as atoi(...) != 0
// -- once per process --
static bool debug_cost_enabled()  { return is_on(SWITCH_ONCE("BLOSC_AMD_DEBUG_COST", SWITCH_SET)); }   // table-cache hits and decode plane costs on stderr
static bool hosttime_on()         { return is_on(SWITCH_ONCE("BLOSC_AMD_HOSTTIME", 0)); }      // host time per phase of the batched calls, printed at release
static bool table_cache_enabled() { return is_on(SWITCH_ONCE("BLOSC_AMD_TABLE_CACHE", 1)); }   // 0: every call builds and uploads its block table and queues
static bool fuse_enabled()        { return is_on(SWITCH_ONCE("BLOSC_AMD_FUSE", 1)); }          // 0: (un)shuffle in kernels of their own (k_shuffle / k_unshuffle ...)
static bool span_enabled()        { return is_on(SWITCH_ONCE("BLOSC_AMD_SPANS", 1)); }         // 0: decoded periodic planes go through the scratch like every other plane
static bool periodic_enabled()    { return is_on(SWITCH_ONCE("BLOSC_AMD_PERIODIC", 1)); }      // 0: every plane goes through the match finder (no periodic-plane shortcut)
// Zstd decode: 2 = two-phase path, 16 frames per wave, tables in a global scratch (k_zstd2.hip); 1 = the same with the tables in LDS (one wave
// per CU); 0 = one wave per frame for everything (k_zstd_streams).  8 GiB of reference-written frames, mode 0 / 2: bench19 107 / 50 ms,
// linspace 17.8 / 15.9, random walk 23.7 / 16.5 (profiles/r02/r02f_zstd_decode_modes.txt)
static int zstd2_mode()           { return (int)SWITCH_ONCE("BLOSC_AMD_ZSTD2", 2); }
static int contexts_wanted()      { return (int)SWITCH_ONCE("BLOSC_AMD_CONTEXTS", 8); }     // workspaces for concurrent callers, clamped to 1 .. kMaxCtx
// placement experiment (scripts/placement_probe.py): the arenas' base this many KiB behind what hipMalloc returned, clamped to 0 .. 64 MiB
static size_t arena_skew_bytes()  { const long k = SWITCH_PLACEMENT("BLOSC_AMD_ARENA_SKEW_KIB", 0); return (size_t)(k < 0 ? 0 : (k > 65536 ? 65536 : k)) << 10; }
// -- every call --
static bool debug_enabled()        { return is_on(switch_every_call("BLOSC_AMD_DEBUG", SWITCH_SET)); }      // arena allocations and the topology probe on stderr
static bool single_queue_forced()  { return is_on(switch_every_call("BLOSC_AMD_SINGLE_QUEUE", 0)); }        // read by probe_topology, once per device set-up
static bool lz4hc_search_enabled() { return is_on(switch_every_call("BLOSC_AMD_LZ4HC", BAMD_LZ4HC_DEFAULT)); }         // 0: "lz4hc" served by the plain LZ4 match finder
static bool zstd_tables_enabled()  { return is_on(switch_every_call("BLOSC_AMD_ZSTD_TABLES", BAMD_ZSTD_TABLES_DEFAULT)); }   // 0: predefined sequence tables only
static bool zstd_search_enabled(int clevel) { return is_on(switch_every_call("BLOSC_AMD_ZSTD_SEARCH", clevel >= 6)); } // LZ4HC-grade search in front of the Zstd writer
static bool zlib_search_enabled()  { return is_on(switch_every_call("BLOSC_AMD_ZLIB_SEARCH", 1)); }         // ... in front of the zlib writer
static bool zstd_huffman_enabled() { return is_on(switch_every_call("BLOSC_AMD_ZSTD_HUFFMAN", 0)); }        // Huffman-coded literals in Zstd frames
static bool zlib_dynamic_enabled() { return is_on(switch_every_call("BLOSC_AMD_ZLIB_DYNAMIC", 1)); }        // 0: fixed Huffman codes
// (the instrumented build's BLOSC_AMD_ENC_PROFILE / BLOSC_AMD_DEC_PROFILE / BLOSC_AMD_ZSTD_PROFILE name files, not values: StreamProfile below)

struct DeviceArena {   // one grow-only device allocation carved up per call
  uint8_t* base = nullptr;
  uint8_t* raw = nullptr;   // what hipMalloc returned (base = raw + skew; BLOSC_AMD_ARENA_SKEW_KIB, a placement experiment: scripts/placement_probe.py)
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes <= cap) return 0;
    if (raw) { (void)hipFree(raw); raw = base = nullptr; cap = 0; }
    size_t want = align_up(bytes + bytes / 8, 1 << 20);
    const size_t skew = arena_skew_bytes();
    HIP_TRY(hipMalloc((void**)&raw, want + skew));
    base = raw + skew;
    cap = want;
    if (debug_enabled()) fprintf(stderr, "[blosc_amd] device arena %p, %zu MiB\n", (void*)base, want >> 20);
    return 0;
  }
  void release() { if (raw) (void)hipFree(raw); raw = base = nullptr; cap = 0; }
};
struct PinnedArena {
  uint8_t* base = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes <= cap) return 0;
    if (base) { (void)hipHostFree(base); base = nullptr; cap = 0; }
    size_t want = align_up(bytes + bytes / 4, 1 << 16);
    HIP_TRY(hipHostMalloc((void**)&base, want, hipHostMallocDefault));
    cap = want;
    return 0;
  }
  void release() { if (base) (void)hipHostFree(base); base = nullptr; cap = 0; }
};

struct ProfEntry { double ms = 0; int launches = 0; };

// per-launch feedback words of the persistent kernels: [0,256) cycles per plane index, [256] tasks taken by the
// stream kernel, [257] streams taken by the Zstd kernel, [259] streams taken by the Zlib kernel - the host compares them with
// what it queued
constexpr size_t kCostWords = 264;
static int check_done(const uint32_t* fb, size_t expect, size_t expect_zstd, const char* what, size_t expect_zlib = 0) {
  if (fb[256] == expect && fb[257] == expect_zstd && fb[259] == expect_zlib) return 0;
  fprintf(stderr, "blosc_amd: %s: the device took %u of %zu queued tasks (Zstd: %u of %zu, Zlib: %u of %zu) - results discarded\n",
          what, fb[256], expect, fb[257], expect_zstd, fb[259], expect_zlib);
  return -1;
}

// The persistent kernels: one-wave workgroups that draw tasks from queues, launched as many as stay resident - a workgroup beyond that starts when
// the first ones leave, finds the queues empty and goes, and a grid below it leaves wave slots empty for the whole launch.  How many stay resident is
// the runtime's to say (registers the compiler really used, LDS in the device's granules): hipOccupancyMaxActiveBlocksPerMultiprocessor, asked once per
// kernel when a context meets its device; the constexpr bound next to each kernel caps it.  Entries 0 .. kEncModes - 1 are k_encode_streams_t's modes, row by row of its table (k_encode.hip).
// Every row states the LDS of one workgroup, and that as many workgroups as its bound says fit the CU's LDS in the device's granules.
// (k_getitem_gather's grid is a choice, not a residency: 16 waves per CU saturate the copy it is)
enum { GRID_DECODE = kEncModes, GRID_ZSTD_EXEC, GRID_ZSTD_STREAMS, GRID_ZLIB_STREAMS, kGridKernels };
struct GridKernel { const char* name; const void* fn; int threads; int bound; int lds; };      // lds: bytes of one workgroup
template <int LDS, int BOUND>
static GridKernel grid_row(const char* name, const void* fn, int threads) {
  static_assert(lds_occupied(LDS) * BOUND <= LDS_BYTES_PER_CU, "the workgroups of one CU fit its LDS, granule by granule");
  return {name, fn, threads, BOUND, LDS};
}
template <int... MODE>
static const GridKernel* grid_kernels(std::integer_sequence<int, MODE...>) {
  static const GridKernel k[kGridKernels] = {
    grid_row<enc_lds_bytes(MODE), enc_grid_bound(MODE)>(kEncMode[MODE].name, (const void*)k_encode_streams_t<MODE>, 64 * ENC_WAVES)...,
    grid_row<DEC_WAVES * (int)DR_LDS_BYTES, DEC_WAVES_PER_CU>("k_decode_streams", (const void*)k_decode_streams, 64 * DEC_WAVES),
    grid_row<(int)sizeof(uint32_t) * (int)ZXB_WORDS, ZEXEC_WAVES_PER_CU>("k_zstd_exec", (const void*)k_zstd_exec, 64),
    grid_row<(int)sizeof(ZstdLds), ZSTD_WAVES_PER_CU>("k_zstd_streams", (const void*)k_zstd_streams, 64),
    grid_row<(int)sizeof(zi::Tabs), ZLIB_WAVES_PER_CU>("k_zlib_streams", (const void*)k_zlib_streams, 64)};
  return k;
}
static const GridKernel* grid_kernels() { return grid_kernels(std::make_integer_sequence<int, kEncModes>{}); }
// the kernel of an encoder mode as its launch wants it: the table's entry in its own type (the modes share one parameter list)
using EncKernel = decltype(&k_encode_streams_t<0>);
static EncKernel enc_kernel(int mode) { return reinterpret_cast<EncKernel>(const_cast<void*>(grid_kernels()[mode].fn)); }
// launches nothing; occupancy[i] = 0 where the runtime gave no answer (the bound alone sizes that grid)
static void query_persistent_grids(int* wpc, int* occupancy) {
  const GridKernel* k = grid_kernels();
  for (int i = 0; i < kGridKernels; i++) {
    int occ = 0;
#ifndef BAMD_WAVE_EMU      // (the emulator runs a grid's workgroups one after the other: any size is a right one)
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k[i].fn, k[i].threads, 0) != hipSuccess || occ < 0) { (void)hipGetLastError(); occ = 0; }
#endif
    occupancy[i] = occ;
    wpc[i] = (occ > 0 && occ < k[i].bound) ? occ : k[i].bound;
  }
}

struct EngineState {
  std::mutex mu;
  bool device_ok = false;
  int device = -1;
  std::atomic<int> device_hint{-1};   // = device once the context is set up; read without the lock by callers choosing where to queue
  DeviceArena dev;      // descriptors + scratch
  DeviceArena io;       // staging for host-pointer calls
  PinnedArena pin;
  PinnedArena put_pin; // engine_put's own tables: they outlive the decode and encode calls inside it, which carve `pin` anew
  // profiling (switched on for all contexts at once: g_prof)
  std::map<std::string, ProfEntry> prof_acc;
  struct Pending { std::string name; hipEvent_t a, b; };
  std::vector<Pending> prof_pending;
  std::vector<hipEvent_t> ev_pool;
  // Scheduling feedback: cycles the previous batch spent per plane index (stream index inside its block),
  // summed by the kernels.  Streams of one batch differ by 100x in cost and the expensive ones are, call
  // after call, the same byte planes; the queue builders use this to keep them out of the kernels' tails.
  uint32_t enc_cost[256] = {0}, dec_cost[256] = {0};
  bool enc_cost_valid = false, dec_cost_valid = false;
  // false: the device deals workgroups round-robin to 8 XCDs whose ids the kernels can read (SPX-mode MI355X),
  // so per-XCD queues and in-kernel hand-offs through one XCD's L2 are valid.  true: anything else (probe below,
  // or BLOSC_AMD_SINGLE_QUEUE=1) - one queue, shuffle / unshuffle in kernels of their own.
  bool single_queue = false;
  int cus = 0;          // compute units of the selected device (persistent grids)
  // workgroups per CU of every persistent kernel on this device: the runtime's occupancy figure, never above the kernel's own bound (query_persistent_grids above)
  int grid_wpc[kGridKernels] = {0}, grid_occupancy[kGridKernels] = {0};
  // Tables that are a function of a batch's GEOMETRY alone - the block table and the task queues (0.5 MB for 128 chunks of 64 MiB) - stay on the
  // device from one call to the next (round 6).  A call that finds its own block table, fusion flags and SET of expensive planes (order_signature) equal to the ones the tables
  // were made from neither builds the queues nor uploads anything but its chunk descriptors: callers send equal-shaped chunks call after call
  // (bench/bench.c:383 does), and the host side of a call is time the device stands idle.  Buffers of their own: the call arena is overwritten by whatever call comes next.
  //
  // The protocol of a call, all of it here: begin() compares the call's key with the one the tables on the device were made from.  A miss
  // marks the cache invalid, has the caller's builder fill `queues` (and `zqueues`), and reserves device and pinned room; upload() enqueues
  // the copies; commit() - AFTER the call's synchronisation, when the uploads are known to have arrived - adopts the key.  A call that
  // fails in between therefore leaves valid == false, and the next one builds again.
  // modes[i], compress: chunk i's fusion flag and, above it, the encoder variant its streams go to (0: it has none) - batches that group
  // differently have different queues
  struct TableKey { std::vector<BlockDesc> blocks; std::vector<uint32_t> modes; std::vector<int> order; int nq = 0; };
  // compress: the task queues of one encoder variant inside `queues` (queue_order.h: build_encode_queues) - off[9] at q_at, shoff[9] at sh_at
  struct EncGroup { int mode; size_t q_at, sh_at; int32_t ntasks; };
  struct TableCache {
    TableKey key; bool valid = false;
    DeviceArena tabs; size_t o_queues = 0, o_zqueues = 0; std::vector<EncGroup> groups;      // the block table lies at tabs.base
    bool hit = false;                                                                          // this call's begin()
    std::vector<int32_t> queues, zqueues; size_t p_blocks = 0, p_queues = 0, p_zqueues = 0;    // a miss's tables on their way to the device
    bool same(const TableKey& k) const {
      return valid && key.nq == k.nq && key.blocks.size() == k.blocks.size() && key.modes == k.modes && key.order == k.order &&
             (k.blocks.empty() || memcmp(key.blocks.data(), k.blocks.data(), k.blocks.size() * sizeof(BlockDesc)) == 0);
    }
    // queue_words / zqueue_words: device room of the two queue tables (0: as long as what `build` made)
    template <class Build>
    int begin(const char* what, const TableKey& k, size_t queue_words, size_t zqueue_words, Carver& pin, Build&& build) {
      hit = table_cache_enabled() && same(k);
      if (debug_cost_enabled()) fprintf(stderr, "[blosc_amd] %s: block table and queues %s\n", what, hit ? "still on the device" : "built and uploaded");
      if (hit) return 0;
      valid = false;
      queues.clear(); zqueues.clear();
      build(*this);
      const size_t nblk = k.blocks.size();
      Carver tcv;
      tcv.take(sizeof(BlockDesc) * (nblk ? nblk : 1));
      o_queues = tcv.take(sizeof(int32_t) * (queue_words ? queue_words : queues.size()));
      if (zqueue_words) o_zqueues = tcv.take(sizeof(int32_t) * zqueue_words);
      if (tabs.ensure(tcv.off)) return -1;
      p_blocks = pin.take(sizeof(BlockDesc) * (nblk ? nblk : 1));
      p_queues = pin.take(sizeof(int32_t) * queues.size());
      p_zqueues = pin.take(sizeof(int32_t) * (zqueues.size() + 1));
      return 0;
    }
    int upload(const TableKey& k, uint8_t* P, hipStream_t stream) {      // P: the pinned arena `pin` of begin() was carved for
      if (hit) return 0;
      const struct { size_t dev, pin; const void* from; size_t bytes; } up[3] = {
        {0, p_blocks, k.blocks.data(), sizeof(BlockDesc) * k.blocks.size()},
        {o_queues, p_queues, queues.data(), sizeof(int32_t) * queues.size()},
        {o_zqueues, p_zqueues, zqueues.data(), sizeof(int32_t) * zqueues.size()}};
      for (const auto& u : up) {
        if (!u.bytes) continue;
        memcpy(P + u.pin, u.from, u.bytes);
        HIP_TRY(hipMemcpyAsync(tabs.base + u.dev, P + u.pin, u.bytes, hipMemcpyHostToDevice, stream));
      }
      return 0;
    }
    void commit(TableKey& k) { if (!hit) { std::swap(key, k); valid = true; } }
    BlockDesc* d_blocks() const { return (BlockDesc*)tabs.base; }
    const int32_t* d_qoff() const { return (const int32_t*)(tabs.base + o_queues); }        // qoff[9], then the queue lists
    const int32_t* d_zqoff() const { return (const int32_t*)(tabs.base + o_zqueues); }
    void drop() { valid = false; tabs.release(); }
  } enc_tabs, dec_tabs;
  hipStream_t own = nullptr;   // host-buffer calls that name no stream run here (non-blocking: see the contexts below)
};

// Contexts (round 3).  blosc_compress_ctx / blosc_decompress_ctx / blosc_getitem are re-entrant in the reference: every call builds
// a context of its own and callers on different threads run side by side (blosc/blosc.c:1288-1305, :1560-1572, :1618-1690).
// A call here needs a workspace - arenas, pinned tables, an event pool, the cost feedback of its last batch - and there are
// ctx_count() of them (BLOSC_AMD_CONTEXTS, default and at most 8 - one per GPU of a node for the multi-GPU calls).  A caller takes the first one that is free, so a single-threaded
// program only ever touches context 0 and never pays for the others; with every context busy a caller queues on one of them in
// turn.  A host-buffer call that names no stream runs on its context's own non-blocking stream: the staging copies of one caller
// overlap the kernels of another instead of lining up on the null stream (the PCIe-bound stock ABI is where that pays).
// Device-pointer calls keep the caller's stream and its ordering.  The selected device is process-wide (g_device); a context
// notices a change the next time it is used.
constexpr int kMaxCtx = 8;
static EngineState g_ctx[kMaxCtx];
static std::atomic<int> g_device{-1};      // -1: whatever device is current when the library is first used
// The device of the CALLING THREAD's calls when >= 0 (engine_thread_device): the multi-GPU entry points run one host thread per
// GPU inside one process, each bound to its device, without touching the process-wide choice other threads rely on.
static thread_local int tl_device = -1;
static bool g_forked = false;
// The device a call of THIS thread runs on: the thread's own binding (multi-GPU entry points), else the process-wide one.  While
// nobody has chosen one, "the current HIP device of the first caller" is resolved HERE and pinned - never "whatever device the context
// that happens to be free lives on": after a _multi call the contexts live on devices 0 .. N-1, and a plain call with device-0
// pointers must not be handed to (and must not silently re-select) another GPU.  -1 only when HIP has no device at all.
static int wanted_device() {
  if (tl_device >= 0) return tl_device;
  int d = g_device.load();
  if (d >= 0 || g_forked) return d;
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur < 0) { (void)hipGetLastError(); return -1; }
  int none = -1;
  (void)g_device.compare_exchange_strong(none, cur);
  return g_device.load();
}
static std::atomic<bool> g_prof{false};
static std::atomic<unsigned> g_ctx_turn{0};
static int ctx_count() {
#ifdef BAMD_WAVE_EMU
  return 1;                                // the wavefront emulator (tests/tools) runs one launch at a time
#else
  return std::min(std::max(contexts_wanted(), 1), kMaxCtx);
#endif
}
static std::mutex g_pick_mu;                // context selection is serialised: a probing thread never makes another one miss "its" context
struct CtxGuard {                          // owns one context for the duration of a call
  EngineState* st = nullptr;
  CtxGuard() {
    const int n = ctx_count();
    // a free context that already lives on the device this thread wants (its arenas stay), else a free one that has no device
    // yet, else any free one (it moves: ensure_device), else wait - for one that lives on the wanted device when there is one
    const int want = wanted_device();
    int wait_on = -1;
    {
      std::lock_guard<std::mutex> pick(g_pick_mu);
      for (int pass = 0; pass < 3 && !st; pass++)
        for (int i = 0; i < n && !st; i++) {
          if (!g_ctx[i].mu.try_lock()) continue;
          const bool ok = pass == 2 || (pass == 0 ? (g_ctx[i].device_ok && g_ctx[i].device == want) : !g_ctx[i].device_ok);
          if (ok) st = &g_ctx[i]; else g_ctx[i].mu.unlock();
        }
      if (!st) {
        // every context is busy.  `device` of a busy context is only read as a hint here (its owner may be moving it): a wrong
        // guess costs a migration in ensure_device, never correctness
        const unsigned turn = g_ctx_turn.fetch_add(1u);
        for (int k = 0; k < n && wait_on < 0; k++) { const int i = (int)((turn + (unsigned)k) % (unsigned)n); if (g_ctx[i].device_hint.load(std::memory_order_relaxed) == want) wait_on = i; }
        if (wait_on < 0) wait_on = (int)(turn % (unsigned)n);
      }
    }
    if (!st) { st = &g_ctx[wait_on]; st->mu.lock(); }
  }
  ~CtxGuard() { st->mu.unlock(); }
  CtxGuard(const CtxGuard&) = delete;
  CtxGuard& operator=(const CtxGuard&) = delete;
};

// Where do 64 consecutive workgroups land?  Expected on an SPX-mode MI355X: XCC ids 0..7, eight workgroups each.
__global__ void k_probe_xcc(uint32_t* hist) {
  if (threadIdx.x == 0) atomicAdd(&hist[__builtin_amdgcn_s_getreg((3 << 11) | 20) & 15u], 1u);
}
static void probe_topology(EngineState& st) {
  st.single_queue = single_queue_forced();
  if (st.single_queue) return;
  uint32_t* d = nullptr; uint32_t h[16] = {0};
  bool ok = hipMalloc((void**)&d, sizeof h) == hipSuccess && hipMemset(d, 0, sizeof h) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(k_probe_xcc, dim3(64), dim3(64), 0, 0, d);
    ok = hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost) == hipSuccess;
  }
  if (d) (void)hipFree(d);
  for (int x = 0; ok && x < 16; x++) ok = h[x] == (x < 8 ? 8u : 0u);
  if (!ok) {
    st.single_queue = true;
    if (debug_enabled()) fprintf(stderr, "blosc_amd: workgroups are not dealt round-robin to 8 XCDs here; using one task queue and unfused filters\n");
  }
}

// fork(): the reference re-creates its thread pool in the child (blosc/blosc.c:2210-2221 blosc_atfork_child).  A HIP
// context does not survive fork(), so there is nothing to re-create here: the child is marked and every compute call
// in it fails loudly (-1) instead of touching the parent's device state.  prepare/parent keep the context mutexes
// consistent across the fork (a forking thread never inherits one locked by somebody else).
// (g_pick_mu first, as CtxGuard takes it: a child forked while another thread was choosing a context would inherit it locked and hang in its first
//  call instead of failing with the message below)
static void atfork_prepare() { g_pick_mu.lock(); for (int i = 0; i < kMaxCtx; i++) g_ctx[i].mu.lock(); }
static void atfork_parent() { for (int i = kMaxCtx - 1; i >= 0; i--) g_ctx[i].mu.unlock(); g_pick_mu.unlock(); }
static void atfork_child() { for (int i = kMaxCtx - 1; i >= 0; i--) g_ctx[i].mu.unlock(); g_pick_mu.unlock(); g_forked = true; }

static int ensure_device(EngineState& st) {
  if (g_forked) {
    fprintf(stderr, "blosc_amd: this process was forked after the library had initialised its HIP device; a device context does not survive fork() - call exec() or use the library only in the parent\n");
    return -1;
  }
  static std::once_flag atfork_once;
  std::call_once(atfork_once, [] { (void)pthread_atfork(atfork_prepare, atfork_parent, atfork_child); });
  // the HIP current device is per host thread: every entry point (they all come through here, holding a
  // context) re-selects the engine's device for the calling thread
  const int want_dev = wanted_device();
  if (st.device_ok && want_dev == st.device) { HIP_TRY(hipSetDevice(st.device)); return 0; }
  if (st.device_ok) {                      // the process moved to another device (engine_set_device through another context)
    (void)hipSetDevice(st.device);
    st.dev.release(); st.io.release(); st.enc_tabs.drop(); st.dec_tabs.drop();     // arenas, stream and events belong to the device they were created on
    if (st.own) { (void)hipStreamDestroy(st.own); st.own = nullptr; }
    for (auto& p : st.prof_pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    st.prof_pending.clear();
    for (hipEvent_t e : st.ev_pool) (void)hipEventDestroy(e);
    st.ev_pool.clear();
    st.device_ok = false;
  }
  st.device = want_dev;
  int cnt = 0;
  hipError_t e = hipGetDeviceCount(&cnt);
  if (e != hipSuccess || cnt <= 0) {
    if (!g_warned.exchange(true))
      fprintf(stderr, "blosc_amd: no usable HIP device (%s); this library has no CPU path\n",
              e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    return -1;
  }
  if (st.device >= 0) HIP_TRY(hipSetDevice(st.device));
  else { HIP_TRY(hipGetDevice(&st.device)); int none = -1; (void)g_device.compare_exchange_strong(none, st.device); }
  probe_topology(st);
  hipDeviceProp_t pr;
  const bool have_props = hipGetDeviceProperties(&pr, st.device) == hipSuccess;
  st.cus = (have_props && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256;
  // The in-kernel hand-offs (k_decode.hip: decode_one_stream, k_encode.hip) are "drain stores, relaxed atomic at the XCD's L2" - an argument
  // about gfx942 / gfx950's write-through L1 and one L2 per XCC, outside the HIP memory model.  Any other part gets the single-queue path,
  // which has no in-kernel hand-off at all, whatever the probe above saw.
  if (!st.single_queue && !(have_props && (strncmp(pr.gcnArchName, "gfx950", 6) == 0 || strncmp(pr.gcnArchName, "gfx942", 6) == 0))) {
    st.single_queue = true;
    if (debug_enabled()) fprintf(stderr, "blosc_amd: %s is not on the allow-list of the relaxed in-kernel hand-off; using one task queue and unfused filters\n", have_props ? pr.gcnArchName : "(unknown device)");
  }
  query_persistent_grids(st.grid_wpc, st.grid_occupancy);
  st.enc_cost_valid = st.dec_cost_valid = false;
  st.device_ok = true;
  st.device_hint.store(st.device, std::memory_order_relaxed);
  return 0;
}

// ---- profiling helpers ------------------------------------------------------------------------
static hipEvent_t prof_event(EngineState& st) {
  if (!st.ev_pool.empty()) { hipEvent_t e = st.ev_pool.back(); st.ev_pool.pop_back(); return e; }
  hipEvent_t e; (void)hipEventCreate(&e); return e;
}
// BLOSC_AMD_HOSTTIME=1: wall time of the host side of the batched calls per phase, printed when the library is released
// (where do the ~0.4 ms per call outside the kernels go?)
struct HostTime { double t[2][6] = {}; long calls[2] = {}; };
static HostTime g_ht;
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static std::mutex g_ht_mu;     // several contexts run at once: the accumulators are shared
struct HostPhases {            // one batched call's clock: mark(i) books the time since the last mark (or the constructor) on phase i
  const int dir; double last = 0.0;
  explicit HostPhases(int dir_) : dir(dir_) { if (hosttime_on()) { last = now_ms(); std::lock_guard<std::mutex> l(g_ht_mu); g_ht.calls[dir]++; } }
  void mark(int i) {
    if (!hosttime_on()) return;
    const double t = now_ms();
    std::lock_guard<std::mutex> l(g_ht_mu);
    g_ht.t[dir][i] += t - last; last = t;
  }
};
struct ProfScope {
  EngineState& st; hipStream_t s; const char* name; hipEvent_t a{}, b{}; bool on;
  ProfScope(EngineState& st_, hipStream_t s_, const char* n) : st(st_), s(s_), name(n), on(g_prof.load(std::memory_order_relaxed)) {
    if (on) { a = prof_event(st); b = prof_event(st); (void)hipEventRecord(a, s); }
  }
  ~ProfScope() { if (on) { (void)hipEventRecord(b, s); st.prof_pending.push_back({name, a, b}); } }
};
static void prof_collect(EngineState& st) {   // call after the stream has been synchronised
  for (auto& p : st.prof_pending) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { auto& e = st.prof_acc[p.name]; e.ms += ms; e.launches++; }
    st.ev_pool.push_back(p.a); st.ev_pool.push_back(p.b);
  }
  st.prof_pending.clear();
}

// ---- gather of the 16-byte headers of device-resident chunks ------------------------------------
__global__ void k_gather_headers(const uint8_t* const* __restrict__ srcs, uint8_t* __restrict__ out, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * 16) return;
  out[i] = srcs[i >> 4][i & 15];
}

// grid of a persistent one-wave-per-workgroup kernel: as many waves as the device keeps resident
static unsigned persistent_grid(const EngineState& st, size_t nitems, int waves_per_cu) {
  const int cus = st.cus > 0 ? st.cus : 256;
  size_t g = (size_t)cus * (size_t)waves_per_cu;
  if (nitems < g) g = nitems;
  // workgroups are dealt round-robin to the 8 XCDs and every XCD serves only its own queue: never fewer than 8
  return (unsigned)(g < 8 ? 8 : g);
}

static dim3 grid1(size_t n, int per) { return dim3((unsigned)((n + per - 1) / per)); }

// ---------------------------------------------------------------------------------------------
// compress
// ---------------------------------------------------------------------------------------------
// typesizes whose byte (un)shuffle runs inside the codec kernels (enc_shuffle.h, k_decode.hip: unshuffle_block_wave); the others, and everything
// under BLOSC_AMD_FUSE=0 / BLOSC_AMD_SINGLE_QUEUE=1, go through the stand-alone filter kernels
static bool fused_typesize(int T) { return T >= 2 && T <= 32; }          // 2 / 4 / 8 / 16: register transposes; the others up to 32 (round 4): an LDS tile of the wave
static bool fused_fast_typesize(int T) { return T == 8 || T == 4 || T == 2 || T == 16; }     // what the Zstd / zlib kernels' own-block unshuffle handles
// bitshuffle chunks of these typesizes are (un)shuffled inside the codec kernels as well (round 4: bitshuffle_block_wave_T / bitunshuffle_block_wave)
static bool bitunshuffle_fused_host(int T) { return T == 1 || T == 2 || T == 4 || T == 8; }      // 8: round 5 (float64 + bitshuffle is a mainstream caller setting)

// the stream a call runs on: the caller's, or - host buffers and no stream named - the context's own
// What the queue builders make of the cost feedback for the stream counts of this batch's blocks: the part of a queue's identity that is not in the block table
static void order_signature(const std::vector<BlockDesc>& blocks, const uint32_t* cost, bool valid, std::vector<int>& sig) {
  bool seen[257] = {false};
  for (const BlockDesc& b : blocks) seen[b.nstreams < 0 ? 0 : (b.nstreams > 256 ? 256 : b.nstreams)] = true;
  sig.clear();
  std::vector<int> order; int nheavy = 0;
  for (int T = 2; T <= 256; T++) {
    if (!seen[T]) continue;
    plane_order(cost, valid && sched_enabled(), T, order, &nheavy);
    // WHICH planes are the expensive ones, not their order: the cheap planes of the benchmark data cost within a few percent of each other and
    // change places from call to call (with the exact order as signature no second call ever found its tables: profiles/r06zo_*); any order of
    // a queue is a correct one, and the one thing the order is there for - the expensive planes first - is what the set says
    std::sort(order.begin(), order.begin() + (nheavy < T ? nheavy : T));
    sig.push_back(T); sig.push_back(nheavy); sig.insert(sig.end(), order.begin(), order.begin() + (nheavy < T ? nheavy : 0));
  }
}

static int call_stream(EngineState& st, bool host_buffers, hipStream_t* stream) {
  if (!host_buffers || *stream != (hipStream_t)0 || ctx_count() == 1) return 0;
  if (!st.own) HIP_TRY(hipStreamCreateWithFlags(&st.own, hipStreamNonBlocking));
  *stream = st.own;
  return 0;
}

static int filter_tile_count(int32_t elems, int per_tile) { const int t = (elems + per_tile - 1) / per_tile; return t < 1 ? 1 : t; }

// Sub-offsets of the area that holds a call's per-chunk result (encode) / status (decode) words: the ticket words of the per-XCD queues
// begin kTicketGap bytes behind the last of them; what follows the tickets is the direction's own (decode: one arrival counter per block)
constexpr size_t kTicketGap = 32;
constexpr size_t kEncTicketWords = 16;     // 8 of the task queues + 8 of the shuffle lists
constexpr size_t kDecTicketWords = 8;
static size_t ticket_offset(size_t nchunks) { return sizeof(int32_t) * nchunks + kTicketGap; }

// Host-pointer calls: every live chunk's input and output get a 256-byte aligned slot in st.io, the inputs in front of the outputs.
// add() per live chunk -> reserve() -> stage() per live chunk, in the same order -> (kernels) -> collect().  Device-pointer calls: all no-ops.
struct HostStaging {
  const bool host;
  size_t in_bytes = 0, out_bytes = 0, in_at = 0, out_at = 0;
  uint8_t *in_base = nullptr, *out_base = nullptr;
  void add(size_t in, size_t out) { if (host) { in_bytes = align_up(in_bytes, 256) + in; out_bytes = align_up(out_bytes, 256) + out; } }
  int reserve(DeviceArena& io) {
    if (!host) return 0;
    const size_t out_off = align_up(in_bytes + 256, 256);
    if (io.ensure(out_off + out_bytes + 512)) return -1;
    in_base = io.base; out_base = io.base + out_off; return 0;
  }
  // enqueues the copy of the chunk's input and points c.src / c.dst at its two slots
  int stage(ChunkDesc& c, const void* src, size_t in, size_t out, hipStream_t stream) {
    if (!host) return 0;
    in_at = align_up(in_at, 256); out_at = align_up(out_at, 256);
    HIP_TRY(hipMemcpyAsync(in_base + in_at, src, in, hipMemcpyHostToDevice, stream));
    c.src = in_base + in_at; c.dst = out_base + out_at;
    in_at += in; out_at += out; return 0;
  }
  // results[i] bytes of every live chunk with a positive result back to the caller's buffer, then waits for them
  int collect(int n, const Job* jobs, const std::vector<ChunkDesc>& chunks, const std::vector<uint8_t>& live, const int* results, hipStream_t stream) {
    if (!host) return 0;
    for (int i = 0; i < n; i++)
      if (live[(size_t)i] && results[i] > 0) HIP_TRY(hipMemcpyAsync(jobs[i].dst, chunks[(size_t)i].dst, (size_t)results[i], hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
  }
};

// Instrumented build only (make prof; scripts/enc_phase.py, dec_phase.py, zstd_phase.py): a kernel writes 64 bytes per stream through one more,
// last parameter.  BAMD_STREAM_PROFILE in front of the launch allocates and clears them where the switch names a file; at the end of the scope
// it waits for the kernel, writes the file and frees them.  BAMD_PROF_ARG is that last argument.  The product build has neither.
#ifdef BAMD_PROFILE_DECODE
struct StreamProfile {
  uint32_t* d = nullptr; std::string path; size_t bytes; hipStream_t stream;
  // suffix: a second file next to the one the switch names (the encode kernel's per-wave records: <file>.waves, one record per workgroup of the grid)
  StreamProfile(const char* switch_name, size_t nrec, hipStream_t s, const char* suffix = "") : path(getenv(switch_name) ? getenv(switch_name) : ""), bytes(nrec * 64), stream(s) {
    if (!path.empty()) path += suffix;
    if (!path.empty() && bytes && hipMalloc((void**)&d, bytes) == hipSuccess) (void)hipMemsetAsync(d, 0, bytes, stream);
  }
  ~StreamProfile() {
    if (!d) return;
    std::vector<uint32_t> h(bytes / 4);
    (void)hipStreamSynchronize(stream); (void)hipMemcpy(h.data(), d, bytes, hipMemcpyDeviceToHost); (void)hipFree(d);
    FILE* f = fopen(path.c_str(), "wb");
    if (f) { fwrite(h.data(), 4, h.size(), f); fclose(f); }
  }
};
#define BAMD_STREAM_PROFILE(var, switch_name, nstr) StreamProfile var(switch_name, nstr, stream)
#define BAMD_WAVE_PROFILE(var, switch_name, nwaves) StreamProfile var(switch_name, nwaves, stream, ".waves")
#define BAMD_PROF_ARG(var) , var.d
#else
#define BAMD_STREAM_PROFILE(var, switch_name, nstr)
#define BAMD_WAVE_PROFILE(var, switch_name, nwaves)
#define BAMD_PROF_ARG(var)
#endif

// The variant of k_encode_streams_t that serves a (codec, clevel), and what its launch needs.  The switches are read per call, as ever.
// What a launch needs beyond the two comes from the mode's row (k_encode.hip): Zstd - the predefined FSE tables; Zstd and zlib with dynamic codes - one
// sequence scratch per persistent wave (enc_seq_words); the LZ family - the periodic-plane shortcut of the shuffle tasks; the name its time is booked under.
struct EncVariant { int mode = kEncModes; int waves_per_cu = 0; };      // waves_per_cu: what stays resident on a CU (EngineState::grid_wpc)
static const char* enc_profile_name(int mode) {
  return kEncMode[mode].family == FAM_ZSTD ? "k_zstd_encode" : (kEncMode[mode].family == FAM_ZLIB ? "k_zlib_encode" : (kEncMode[mode].search ? "k_lz4hc_encode" : "k_encode_streams"));
}
// The mode of the row the switches ask for (kEncModes: there is none); a family takes its own switches.  Zstd: the search comes with per-block
// tables, and Huffman-coded literals count on top of either only.
constexpr int enc_mode_wanted(int family, bool search, bool tables, bool huffman, bool dynamic) {
  const bool zstd = family == FAM_ZSTD;
  const EncMode want = {nullptr, family, search, zstd && (tables || search), zstd && huffman && (tables || search), family == FAM_ZLIB && dynamic};
  int m = 0;
  while (m < kEncModes && !(kEncMode[m].family == want.family && kEncMode[m].search == want.search && kEncMode[m].tables == want.tables &&
                            kEncMode[m].huffman == want.huffman && kEncMode[m].dynamic == want.dynamic)) m++;
  return m;
}
// how many rows the settings of the switches compose: 2 of the LZ family, 5 of Zstd, 4 of zlib; -1: a setting without its row
constexpr int enc_modes_composed() {
  unsigned seen = 0;
  for (int s = 0; s < (FAM_ZLIB + 1) * 16; s++) {     // family s / 16, the four switches the bits of s % 16
    const int m = enc_mode_wanted(s >> 4, s & 1, s & 2, s & 4, s & 8);
    if (m == kEncModes) return -1;
    seen |= 1u << m;
  }
  return __builtin_popcount(seen);
}
static_assert(enc_modes_composed() == kEncModes, "every setting of the encoder switches has its row, and every row a setting");
static EncVariant encoder_variant(const EngineState& st, int codec, int clevel) {
  EncVariant v;
  const int family = codec == kZstd ? FAM_ZSTD : (codec == kZlib ? FAM_ZLIB : FAM_LZ);
  // "lz4hc": the LZ4HC-grade search of k_encode.hip (lz4hc_encode_wave), or the plain LZ4 match finder at its highest effort.
  // The LZ4HC-grade search in front of the Zstd writer (with per-block tables) / the zlib writer:
  // defaults after the device timings of round 3 (profiles/r03/r03a_encopts_bench_*.json, 8 GiB bench19): Zstd - the search costs 2.6 x the
  // encode time (35.8 -> 94.9 ms) for ratio 23.8 -> 35.1, so it serves the upper clevels (the reference maps clevel >= 6 to its
  // lazy / optimal strategies, blosc.c:502-504 + clevels.h) and stays off at the default clevel; zlib - whoever names zlib wants its
  // ratio: search + dynamic codes give 73.4 (reference 47.4, fixed codes without search 40.5) at 57 ms per 8 GiB, still 150 GB/s.
  // Zstd tables: sequence tables made per block (k_encode.hip: zt_make_tables) instead of the predefined ones.
  const bool search = family == FAM_ZSTD ? zstd_search_enabled(clevel) : (family == FAM_ZLIB ? zlib_search_enabled() : codec == kLZ4HC && lz4hc_search_enabled());
  v.mode = enc_mode_wanted(family, search, zstd_tables_enabled(), zstd_huffman_enabled(), zlib_dynamic_enabled());
  v.waves_per_cu = st.grid_wpc[v.mode];
  return v;
}

// What the per-chunk loop of a compress call adds up: the tables and the sizes of the scratch areas
struct EncodeBatch {
  std::vector<ChunkDesc> chunks; std::vector<uint8_t> live;
  std::vector<uint8_t> variant;                      // per chunk: the encoder variant its streams go to; kEncModes: it has no streams
  EncVariant variants[kEncModes]; bool present[kEncModes] = {false}; int ngroups = 0;
  EngineState::TableKey key;                         // key.blocks: the block table
  size_t nstr = 0, filt_bytes = 0, stage_bytes = 0;  // (the stream table itself is made on the device: k_encode_plan)
  int tiles_shuf = 0, tiles_bit = 0; bool any_shuf = false, any_bit = false;
  explicit EncodeBatch(int n) : chunks((size_t)n), live((size_t)n, 0), variant((size_t)n, (uint8_t)kEncModes) {}
};

// The parameter checks of a chunk of nbytes into destsize, in the compress call's order (blosc.c:1062-1145, :1197-1207; Snappy: not built).
// false: it cannot be written, *result is what the compress call answers for it: 0 (too large, or no room for a header), -10, -5.
static bool check_cparams(const CompressParams& p, size_t nbytes, size_t destsize, int* result) {
  *result = 0;
  if (nbytes > (size_t)kMaxBufferSize || destsize < (size_t)kMaxOverhead) return false;
  if (p.clevel < 0 || p.clevel > 9 || (p.doshuffle != 0 && p.doshuffle != 1 && p.doshuffle != 2) || p.typesize == 0) *result = -10;
  else if (p.codec != kBloscLZ && p.codec != kLZ4 && p.codec != kLZ4HC && p.codec != kZlib && p.codec != kZstd) *result = -5;
  return *result == 0;
}

// Parameter checks and geometry of chunk i of n (blosc.c:1062-1145, :1148-1247).  false: nothing runs for it, *result is its outcome.
static bool add_encode_chunk(const CompressParams& p, const Job& job, int i, int n, bool may_fuse, EncodeBatch& B, int* result) {
  ChunkDesc& c = B.chunks[(size_t)i];
  std::vector<BlockDesc>& blocks = B.key.blocks;
  memset(&c, 0, sizeof c);
  c.mode = CH_SKIP;
  size_t nbytes = job.srcsize, destsize = job.dstsize, typesize = p.typesize;
  const int codec = p.codec;
  if (!check_cparams(p, nbytes, destsize, result)) return false;
  if (destsize - kMaxOverhead > nbytes) destsize = nbytes + kMaxOverhead;
  if (typesize > (size_t)kMaxTypeSize) typesize = 1;
  const int32_t T = (int32_t)typesize, nb = (int32_t)nbytes;
  const int32_t bs = compute_blocksize(p.clevel, T, nb, p.forced_blocksize, codec, p.splitmode);
  const int32_t leftover = nb % bs, nblocks = nb / bs + (leftover > 0 ? 1 : 0);
  const bool memcpyed = (p.clevel == 0) || (nb < kMinBufferSize);
  const int split = split_block(codec, T, bs, p.splitmode);
  int flags = ((!split) << 4) | (codec_to_format(codec) << 5);
  if (memcpyed) flags |= kFlagMemcpyed;
  if (p.doshuffle == 1) flags |= kFlagShuffle;
  if (p.doshuffle == 2) flags |= kFlagBitShuffle;
  if (memcpyed && (size_t)nb + kMaxOverhead > destsize) return false;  // blosc.c:1254-1257

  c.src = (const uint8_t*)job.src; c.dst = (uint8_t*)job.dst;
  c.nbytes = nb; c.cbytes = (int32_t)destsize; c.blocksize = bs; c.typesize = T;
  c.nblocks = nblocks; c.leftover = leftover; c.nsplits = split ? T : 1;
  c.fmt = codec_to_format(codec); c.clevel = (codec == kLZ4HC) ? 9 : p.clevel; c.hdr_flags = flags;
  c.mode = 0;
  c.first_block = (int32_t)blocks.size(); c.first_stream = (int32_t)B.nstr;
  if (memcpyed) c.mode |= CH_MEMCPYED;
  else if (p.doshuffle == 1 && T > 1) { c.mode |= CH_SHUFFLE; if (fused_typesize(T) && fuse_enabled() && may_fuse) c.mode |= CH_FUSED_SHUF; }
  else if (p.doshuffle == 2) { c.mode |= CH_BITSHUFFLE; if (bitunshuffle_fused_host(T) && fuse_enabled() && may_fuse) c.mode |= CH_FUSED_SHUF; }
  const bool filtered = (c.mode & (CH_SHUFFLE | CH_BITSHUFFLE)) != 0;
  if (filtered && !(c.mode & CH_FUSED_SHUF)) {       // (fused: shuffled by tasks of the encode kernel)
    if (c.mode & CH_SHUFFLE) { B.any_shuf = true; B.tiles_shuf = std::max(B.tiles_shuf, filter_tile_count(bs / T, shuffle_tile_elems(T))); }
    else { B.any_bit = true; B.tiles_bit = std::max(B.tiles_bit, filter_tile_count(bs / T, bitshuffle_tile_elems(T))); }
  }
  // blocks; their streams (in = the block's bytes in the filtered image or the source, out = its staging slot) are k_encode_plan's
  if (blocks.capacity() < blocks.size() + (size_t)nblocks) blocks.reserve(std::max(blocks.size() + (size_t)nblocks, (size_t)(n - i) * (size_t)nblocks + blocks.size()));   // (equal chunks: one allocation)
  for (int32_t j = 0; j < nblocks; j++) {
    BlockDesc b;
    b.chunk = i; b.blk = j; b.first_stream = (int32_t)B.nstr;
    const bool last = (j == nblocks - 1) && leftover > 0;
    b.nstreams = memcpyed ? 0 : ((split && !last) ? T : 1);
    b.bsize = last ? leftover : bs; b.flags = 0;
    B.nstr += (size_t)b.nstreams;
    blocks.push_back(b);
  }
  if (!memcpyed) {
    if (filtered) B.filt_bytes = align_up(B.filt_bytes, 256) + (size_t)nb;
    B.stage_bytes = align_up(B.stage_bytes, 256) + (size_t)nb;
  }
  return true;
}

// test hooks (tests/test_gpu_persistent_grid.py).  Neither launches a kernel: a context that has met its device answers from what it asked then,
// otherwise the runtime is asked now, for the device the calling thread would use.
int engine_persistent_grids(int cap, const char** names, int* launched, int* occupancy) {
  CtxGuard ctx; EngineState& st = *ctx.st;
  int wpc[kGridKernels], occ[kGridKernels];
  if (st.device_ok && wanted_device() == st.device) { memcpy(wpc, st.grid_wpc, sizeof wpc); memcpy(occ, st.grid_occupancy, sizeof occ); }
  else {
    const int dev = wanted_device();
    if (dev < 0 || hipSetDevice(dev) != hipSuccess) return -1;
    query_persistent_grids(wpc, occ);
  }
  for (int i = 0; i < kGridKernels && i < cap; i++) { names[i] = grid_kernels()[i].name; launched[i] = wpc[i]; occupancy[i] = occ[i]; }
  return kGridKernels;
}
// resident workgroups per CU of the LZ4 / BloscLZ encode kernel with `dynamic_lds` bytes on top of its own LDS (scripts/lds_granule.py: where the
// figure steps says how the device hands out LDS); < 0: no answer
int engine_enc_lz_occupancy(int dynamic_lds) {
#ifdef BAMD_WAVE_EMU
  return -1;
#else
  const int dev = wanted_device();
  int occ = -1;
  if (dev < 0 || hipSetDevice(dev) != hipSuccess) return -1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, grid_kernels()[ENC_LZ].fn, 64 * ENC_WAVES, (size_t)dynamic_lds) != hipSuccess) { (void)hipGetLastError(); return -1; }
  return occ;
#endif
}
// the last compress call of this process that ran streams: tasks its kernels took (the sum of every launch's plane_cost[256]), streams and shuffle tasks it queued
static std::atomic<uint32_t> g_last_enc_tasks[3];
void engine_last_compress_tasks(uint32_t out[3]) { for (int i = 0; i < 3; i++) out[i] = g_last_enc_tasks[i].load(); }

// A call with candidates (engine.h: CandidateSelect) as compress_entries sees it: its n chunks are the ENTRIES, one per candidate, those of
// one caller chunk adjacent - entries [first[i], first[i + 1]) are the candidates of caller chunk i of nchunks.  choice: [nchunks],
// answers: [n], host arrays it writes.
struct SelectRun { int nchunks; const int* first; int* choice; int* answers; };

// The compress call over a table of n chunks.  sel == nullptr: engine_compress_batch as it is without candidates - not a launch, not a byte more.
// compress_entries_in is the call in a context its caller holds (engine_put runs its decode and its encode in ONE context); compress_entries takes one.
static int compress_entries_in(EngineState& st, const CompressParams* params, bool per_chunk, int n, const Job* jobs, int* results, bool device_ptrs,
                               hipStream_t stream, const PackedBuffer* packed, const SelectRun* sel) {
  if (n <= 0) return 0;
  if ((packed || sel) && !device_ptrs) return -1;
  if (ensure_device(st) || call_stream(st, !device_ptrs, &stream)) return -1;
  HostPhases ht(0);
  // ---- check and lay out the chunks ----
  EncodeBatch B(n);
  HostStaging io{!device_ptrs};
  std::vector<ChunkDesc>& chunks = B.chunks;
  // the encoder variant of every chunk that has streams: the chunks of one variant are one group, with one launch of its kernel.
  // (codec, clevel) -> variant is looked up once per call, not per chunk: the switches behind it are environment reads
  int8_t variant_of[6][10]; memset(variant_of, -1, sizeof variant_of);
  for (int i = 0; i < n; i++) {
    const CompressParams& p = params[per_chunk ? i : 0];
    B.live[(size_t)i] = add_encode_chunk(p, jobs[i], i, n, !st.single_queue, B, &results[i]);
    if (!B.live[(size_t)i]) continue;
    io.add((size_t)chunks[(size_t)i].nbytes, (size_t)chunks[(size_t)i].cbytes);
    if (chunks[(size_t)i].mode & CH_MEMCPYED) continue;
    int8_t& m = variant_of[p.codec][p.clevel];      // (both in range: the chunk passed add_encode_chunk's checks)
    if (m < 0) { const EncVariant v = encoder_variant(st, p.codec, p.clevel); m = (int8_t)v.mode; B.variants[v.mode] = v; }
    B.variant[(size_t)i] = (uint8_t)m;
    if (!B.present[m]) { B.present[m] = true; B.ngroups++; }
  }
  const size_t nblk = B.key.blocks.size(), nstr = B.nstr;
  // One set of plane-cost words cannot describe two kernels: a call with more than one group runs in plain block order and leaves the
  // feedback of the one-group calls around it alone
  const bool feedback = B.ngroups <= 1;
  const bool cost_valid = feedback && st.enc_cost_valid;
  const size_t ngrp = (size_t)(B.ngroups > 0 ? B.ngroups : 1);
  ht.mark(0);     // per-chunk geometry + block / stream tables
  // ---- tables: the block table and the queues, still on the device from the last call of this geometry or built and uploaded now ----
  EngineState::TableCache& tc = st.enc_tabs;
  B.key.nq = st.single_queue ? 1 : 8;
  B.key.modes.resize((size_t)n);
  for (int i = 0; i < n; i++) B.key.modes[(size_t)i] = (chunks[(size_t)i].mode & CH_FUSED_SHUF) | (B.variant[(size_t)i] < kEncModes ? (uint32_t)(B.variant[(size_t)i] + 1) << 8 : 0u);
  order_signature(B.key.blocks, st.enc_cost, cost_valid, B.key.order);
  Carver pc;
  if (tc.begin("compress", B.key, 0, 0, pc, [&](EngineState::TableCache& t) {
        // every group's queues behind one another in the one queue table; a one-group batch: the whole batch, as it always was
        t.groups.clear();
        std::vector<int32_t> q;
        for (int m = 0; m < kEncModes; m++) {
          if (!B.present[m]) continue;
          size_t sh_at = 0;
          build_encode_queues(B.key.blocks, chunks, st.enc_cost, cost_valid, q, B.key.nq, &sh_at, B.ngroups > 1 ? B.variant.data() : nullptr, m);
          t.groups.push_back({m, t.queues.size(), t.queues.size() + sh_at, q[8]});
          t.queues.insert(t.queues.end(), q.begin(), q.end());
        }
      })) return -1;
  // ---- workspace ----
  Carver cv;
  const size_t o_chunks = cv.take(sizeof(ChunkDesc) * (size_t)n);
  const size_t o_streams = cv.take(sizeof(StreamDesc) * (nstr ? nstr : 1));
  const size_t o_blkoff = cv.take(sizeof(int32_t) * (nblk ? nblk : 1));
  // results + tickets | block-ready flags | cost words: taken back to back, ONE fill clears the three of them
  // (every group has ticket words and cost words of its own: group k's are the k-th set)
  // (candidates: the choices and the candidate answers lie directly in front of the results - ONE download brings the three back)
  const size_t sel_bytes = sel ? sizeof(int32_t) * ((size_t)sel->nchunks + (size_t)n) : 0;
  const size_t o_sel = cv.take(sel_bytes + ticket_offset((size_t)n) + sizeof(uint32_t) * kEncTicketWords * ngrp);
  const size_t o_results = o_sel + sel_bytes;
  const size_t o_ready = cv.take(sizeof(uint32_t) * (nblk ? nblk : 1));
  const size_t o_cost = cv.take(sizeof(uint32_t) * kCostWords * ngrp);
  const size_t clear_bytes = cv.off - o_results;
  const size_t o_filt = cv.take(B.filt_bytes + 256);
  const size_t o_stage = cv.take(B.stage_bytes + 256);
  // pinned memory, behind the tables of tc.begin(): what goes up with the call and what comes back from it
  const size_t p_chunks = pc.take(sizeof(ChunkDesc) * (size_t)n);
  const size_t p_results = pc.take(sel_bytes + sizeof(int32_t) * (size_t)n);
  const size_t p_first = sel ? pc.take(sizeof(int32_t) * ((size_t)sel->nchunks + 1 + (size_t)n)) : 0;      // the range table and the entries' outcomes so far
  const size_t p_cost = pc.take(sizeof(uint32_t) * kCostWords * ngrp);
  const size_t p_offsets = packed ? pc.take(sizeof(uint64_t) * ((size_t)n + 1)) : 0;
  // The groups of the call, for everything behind this layout.  Zstd: the predefined FSE tables; Zstd and zlib with dynamic codes: one sequence
  // scratch per persistent wave
  // (offsets: o_ctabs, o_seqbufs - 0: the variant wants none -, the group's ticket words and cost words in the device arena; the cost words in pinned memory)
  struct GroupRun { const EngineState::EncGroup* g; EncVariant v; size_t o_ctabs, o_seqbufs, o_ticket, o_cost, p_cost; };
  std::vector<GroupRun> runs;
  for (size_t k = 0; k < tc.groups.size(); k++) {
    GroupRun r{&tc.groups[k], B.variants[tc.groups[k].mode], 0, 0, o_results + ticket_offset((size_t)n) + sizeof(uint32_t) * kEncTicketWords * k,
               o_cost + sizeof(uint32_t) * kCostWords * k, p_cost + sizeof(uint32_t) * kCostWords * k};
    const size_t zwaves = (size_t)(st.cus > 0 ? st.cus : 256) * (size_t)r.v.waves_per_cu;
    if (kEncMode[r.v.mode].family == FAM_ZSTD) r.o_ctabs = cv.take(sizeof(zenc::CTabs) + 64);
    if (enc_seq_words(r.v.mode)) r.o_seqbufs = cv.take(zwaves * enc_seq_words(r.v.mode) * sizeof(uint64_t) + 64);
    runs.push_back(r);
  }
  const size_t o_offsets = (packed || sel) ? cv.take(sizeof(uint64_t) * ((size_t)n + 1)) : 0;      // packed: the offset table k_packed_layout writes
  const size_t o_first = sel ? cv.take(sizeof(int32_t) * ((size_t)sel->nchunks + 1)) : 0;         // candidates: where every caller chunk's entries begin
  if (st.dev.ensure(cv.off)) return -1;
  uint8_t* D = st.dev.base;
  for (const GroupRun& r : runs) {
    if (!r.o_ctabs) continue;
    static const zenc::CTabs host_tabs = [] { zenc::CTabs t; zenc::build_predefined(t); return t; }();
    HIP_TRY(hipMemcpyAsync(D + r.o_ctabs, &host_tabs, sizeof host_tabs, hipMemcpyHostToDevice, stream));
  }
  // ---- stage the inputs of a host-pointer call, point every chunk at its scratch ----
  if (io.reserve(st.io)) return -1;
  {
    size_t fo = 0, so = 0;
    for (int i = 0; i < n; i++) {
      if (!B.live[(size_t)i]) continue;
      ChunkDesc& c = chunks[(size_t)i];
      if (io.stage(c, jobs[i].src, (size_t)c.nbytes, (size_t)c.cbytes, stream)) return -1;
      if (c.mode & CH_MEMCPYED) continue;
      const bool filtered = (c.mode & (CH_SHUFFLE | CH_BITSHUFFLE)) != 0;
      if (filtered) { fo = align_up(fo, 256); c.filt = D + o_filt + fo; fo += (size_t)c.nbytes; }
      so = align_up(so, 256); c.stage = D + o_stage + so; so += (size_t)c.nbytes;
    }
  }
  ht.mark(1);     // queues, workspace, pointer patching
  // ---- upload the tables ----
  if (st.pin.ensure(pc.off)) return -1;
  uint8_t* P = st.pin.base;
  memcpy(P + p_chunks, chunks.data(), sizeof(ChunkDesc) * (size_t)n);
  if (tc.upload(B.key, P, stream)) return -1;
  HIP_TRY(hipMemsetAsync(D + o_results, 0, clear_bytes, stream));
  HIP_TRY(hipMemcpyAsync(D + o_chunks, P + p_chunks, sizeof(ChunkDesc) * (size_t)n, hipMemcpyHostToDevice, stream));
  if (sel) {      // the range table, and what the host has answered already (row errors: k_candidate_select hands them on with the sizes)
    const size_t first_bytes = sizeof(int32_t) * ((size_t)sel->nchunks + 1);
    memcpy(P + p_first, sel->first, first_bytes);
    memcpy(P + p_first + first_bytes, results, sizeof(int32_t) * (size_t)n);
    HIP_TRY(hipMemcpyAsync(D + o_first, P + p_first, first_bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(D + o_results, P + p_first + first_bytes, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, stream));
  }

  ChunkDesc* d_chunks = (ChunkDesc*)(D + o_chunks); BlockDesc* d_blocks = tc.d_blocks(); StreamDesc* d_streams = (StreamDesc*)(D + o_streams);
  int32_t* d_blkoff = (int32_t*)(D + o_blkoff); int32_t* d_results = (int32_t*)(D + o_results);
  ht.mark(2);     // table copies to pinned memory + upload enqueues
  // ---- launch ----
  if (nstr) hipLaunchKernelGGL(k_encode_plan, grid1(nblk, 256), dim3(256), 0, stream, d_chunks, d_blocks, d_streams, (int)nblk);
  if (B.any_shuf && nblk) {
    ProfScope ps(st, stream, "k_shuffle");
    hipLaunchKernelGGL(k_shuffle, dim3((unsigned)nblk, (unsigned)B.tiles_shuf), dim3(FT_THREADS), 0, stream, d_chunks, d_blocks);
  }
  if (B.any_bit && nblk) {      // full tiles of typesize 1 / 2 / 4 / 8 through k_bitfilter_fast, the rest through the generic kernel
    ProfScope ps(st, stream, "k_bitshuffle");
    hipLaunchKernelGGL(k_bitfilter_fast<0>, dim3((unsigned)nblk, (unsigned)B.tiles_bit), dim3(FT_THREADS), 0, stream, d_chunks, d_blocks);
    hipLaunchKernelGGL(k_bitshuffle, dim3((unsigned)nblk, (unsigned)B.tiles_bit), dim3(FT_THREADS), 0, stream, d_chunks, d_blocks, 1);
  }
  // one launch per group: its own queues, ticket words, cost words and scratch; the tables of chunks, blocks and streams and the
  // block-ready flags are the batch's (a group's queues name the blocks of its own chunks only)
  for (const GroupRun& r : runs) {
    const EngineState::EncGroup& g = *r.g;
    if (!nstr || g.ntasks <= 0) continue;
    ProfScope ps(st, stream, enc_profile_name(r.v.mode));
    const int32_t* d_qoff = tc.d_qoff() + g.q_at; const int32_t* d_qlist = d_qoff + 9; const int32_t* d_shoff = tc.d_qoff() + g.sh_at;
    uint32_t* d_ticket = (uint32_t*)(D + r.o_ticket);
    uint32_t* d_cost = (uint32_t*)(D + r.o_cost);
    uint32_t* d_ready = (uint32_t*)(D + o_ready);
    uint64_t* d_seqbufs = r.o_seqbufs ? (uint64_t*)(D + r.o_seqbufs) : nullptr;
    const zenc::CTabs* d_ctabs = r.o_ctabs ? (const zenc::CTabs*)(D + r.o_ctabs) : nullptr;
    const int detect = (kEncMode[r.v.mode].family == FAM_LZ && periodic_enabled()) ? 1 : 0;     // the periodic-plane shortcut of the shuffle tasks
    const dim3 grid(persistent_grid(st, (size_t)g.ntasks, r.v.waves_per_cu)), block(64 * ENC_WAVES);
    BAMD_STREAM_PROFILE(prof, "BLOSC_AMD_ENC_PROFILE", nstr);
    BAMD_WAVE_PROFILE(wprof, "BLOSC_AMD_ENC_PROFILE", grid.x);
    hipLaunchKernelGGL(enc_kernel(r.v.mode), grid, block, 0, stream, d_streams, d_ticket, d_qlist, d_qoff, d_shoff, d_chunks, d_blocks, d_ready, d_cost, st.single_queue ? 1 : 0, d_seqbufs, d_ctabs, detect BAMD_PROF_ARG(prof) BAMD_PROF_ARG(wprof));
  }
  if (!packed && !sel) {
    ProfScope ps(st, stream, "k_chunk_scan");
    hipLaunchKernelGGL(k_chunk_scan, dim3((unsigned)n), dim3(SCAN_THREADS), 0, stream, d_chunks, d_blocks, d_streams, d_blkoff, d_results);
  } else {
    // sizes first, then every chunk's place inside the caller's buffer (c.dst, or CH_SKIP where it ends), then what the scan writes itself
    // when the place is known beforehand: header, bstarts - and the zeros between the chunks.  k_chunk_compact reads c.dst from the device table.
    uint64_t* d_offsets = (uint64_t*)(D + o_offsets);
    {
      ProfScope ps(st, stream, "k_chunk_scan");
      hipLaunchKernelGGL(k_chunk_scan_packed, dim3((unsigned)n), dim3(SCAN_THREADS), 0, stream, d_chunks, d_blocks, d_streams, d_blkoff, d_results);
    }
    // candidates: the sizes are known and nothing is written yet - every entry but its chunk's winner leaves the call here (CH_SKIP, result 0:
    // no room in the layout, no header, no compaction)
    if (sel) {
      ProfScope ps(st, stream, "k_candidate_select");
      hipLaunchKernelGGL(k_candidate_select, dim3((unsigned)sel->nchunks), dim3(SELECT_THREADS), 0, stream, d_chunks, d_results, (const int32_t*)(D + o_first),
                         (int32_t*)(D + o_sel) + sel->nchunks, (int32_t*)(D + o_sel));
    }
    if (packed) {
      ProfScope ps(st, stream, "k_packed_layout");
      hipLaunchKernelGGL(k_packed_layout, dim3(1), dim3(SCAN_THREADS), 0, stream, d_chunks, d_results, n, (uint8_t*)packed->base, (uint64_t)packed->size,
                         (uint64_t)packed->align, d_offsets);
      hipLaunchKernelGGL(k_packed_headers, dim3((unsigned)n), dim3(SCAN_THREADS), 0, stream, d_chunks, d_blkoff, d_results, d_offsets, (uint64_t)packed->size);
    } else {
      // candidates, a destination per chunk: c.dst is the caller's.  The winner's header and bstarts come from k_packed_headers over a table of
      // zeros and a buffer of no bytes, so it pads nothing
      HIP_TRY(hipMemsetAsync(d_offsets, 0, sizeof(uint64_t) * ((size_t)n + 1), stream));
      hipLaunchKernelGGL(k_packed_headers, dim3((unsigned)n), dim3(SCAN_THREADS), 0, stream, d_chunks, d_blkoff, d_results, d_offsets, (uint64_t)0);
    }
  }
  if (nblk) {
    ProfScope ps(st, stream, "k_chunk_compact");
    hipLaunchKernelGGL(k_chunk_compact, dim3((unsigned)nblk), dim3(COMPACT_THREADS), 0, stream, d_chunks, d_blocks, d_streams, d_blkoff);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(P + p_results, D + o_sel, sel_bytes + sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(P + p_cost, D + o_cost, sizeof(uint32_t) * kCostWords * ngrp, hipMemcpyDeviceToHost, stream));
  if (packed) HIP_TRY(hipMemcpyAsync(P + p_offsets, D + o_offsets, sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, stream));
  ht.mark(3);     // kernel launches
  // ---- collect ----
  HIP_TRY(hipStreamSynchronize(stream));
  ht.mark(4);     // waiting for the device
  prof_collect(st);
  uint32_t taken = 0, nshuf = 0;
  for (const GroupRun& r : runs) {
    if (!nstr) break;
    const uint32_t* cost = (const uint32_t*)(P + r.p_cost);
    if (check_done(cost, (size_t)r.g->ntasks, 0, "compress")) return -1;      // every group's launch took what was queued for it
    taken += cost[256];
    nshuf += (uint32_t)tc.queues[r.g->sh_at + 8];      // shoff[8]: the entries of the group's eight shuffle lists
  }
  if (packed) for (int i = 0; i <= n; i++) packed->offsets[i] = (size_t)((const uint64_t*)(P + p_offsets))[i];
  if (nstr) { g_last_enc_tasks[0] = taken; g_last_enc_tasks[1] = (uint32_t)nstr; g_last_enc_tasks[2] = nshuf; }
  tc.commit(B.key);
  if (feedback && nstr >= 4096) { memcpy(st.enc_cost, P + p_cost, sizeof st.enc_cost); st.enc_cost_valid = true; }   // small calls say little
  const int32_t* r = (const int32_t*)(P + p_results + sel_bytes);
  for (int i = 0; i < n; i++) if (B.live[(size_t)i]) results[i] = r[i];
  if (sel) {
    memcpy(sel->choice, P + p_results, sizeof(int32_t) * (size_t)sel->nchunks);
    memcpy(sel->answers, P + p_results + sizeof(int32_t) * (size_t)sel->nchunks, sizeof(int32_t) * (size_t)n);
  }
  return io.collect(n, jobs, chunks, B.live, results, stream);
}

static int compress_entries(const CompressParams* params, bool per_chunk, int n, const Job* jobs, int* results, bool device_ptrs,
                            hipStream_t stream, const PackedBuffer* packed, const SelectRun* sel) {
  if (n <= 0) return 0;
  if ((packed || sel) && !device_ptrs) return -1;
  CtxGuard ctx;
  return compress_entries_in(*ctx.st, params, per_chunk, n, jobs, results, device_ptrs, stream, packed, sel);
}

int engine_compress_batch(const CompressParams* params, bool per_chunk, int n, const Job* jobs, int* results, bool device_ptrs,
                          hipStream_t stream, const PackedBuffer* packed, const CandidateSelect* select) {
  if (!select) return compress_entries(params, per_chunk, n, jobs, results, device_ptrs, stream, packed, nullptr);
  if (n <= 0) return 0;
  if (!device_ptrs || !per_chunk) return -1;
  // one entry per candidate: the candidates of a chunk share its source, its destination and its limit.  Everything the entries' call
  // writes goes to tables of this function, so a call that fails leaves the caller's untouched
  const int* first = select->cand_first;
  const int E = first[n];
  std::vector<Job> entries((size_t)E);
  for (int i = 0; i < n; i++) for (int e = first[i]; e < first[i + 1]; e++) entries[(size_t)e] = jobs[i];
  std::vector<int> sizes((size_t)E, 0), answers((size_t)E, 0), choice((size_t)n, -1);
  std::vector<size_t> offsets((size_t)E + 1, 0);
  PackedBuffer pk{};
  if (packed) { pk = *packed; pk.offsets = offsets.data(); }
  const SelectRun run{n, first, choice.data(), answers.data()};
  if (compress_entries(params, true, E, entries.data(), sizes.data(), true, stream, packed ? &pk : nullptr, &run)) return -1;
  // fold the entries' tables into the caller's: a chunk is its winner (in a packed buffer the losers took no room: the chunk begins
  // where its first entry does)
  for (int i = 0; i < n; i++) {
    const int f = first[i], c = choice[(size_t)i];
    results[i] = f == first[i + 1] ? -10 : (c >= 0 ? sizes[(size_t)(f + c)] : answers[(size_t)f]);
    select->choice[i] = c;
    if (packed) packed->offsets[i] = offsets[(size_t)f];
  }
  if (packed) packed->offsets[n] = offsets[(size_t)E];
  if (select->cand_results && E > 0) memcpy(select->cand_results, answers.data(), sizeof(int) * (size_t)E);
  return 0;
}

// ---------------------------------------------------------------------------------------------
// decompress
// ---------------------------------------------------------------------------------------------
// header validation shared by decompress and getitem; returns 1 = go on, else *res holds the result
static int classify_for_decompress(const Header& h, size_t srcsize, size_t destsize, int* res, int* fmt) {
  if (h.nbytes == 0) { *res = 0; return 0; }                                   // blosc.c:1463-1466
  if (h.blocksize <= 0 || (size_t)h.blocksize > destsize || h.blocksize > kMaxBlockSize || h.typesize <= 0) { *res = -1; return 0; }
  if (h.version != kVersionFormat) { *res = -1; return 0; }                    // blosc.c:1474-1477
  if (h.flags & kFlagReserved) { *res = -1; return 0; }                        // blosc.c:1478-1481
  // A NEGATIVE nbytes (bit 31 set: damaged input only) is not "> destsize" for the reference's signed comparison (blosc.c:1490); it then counts
  // nbytes / blocksize <= 0 blocks (C's truncating division, the leftover is <= 0: blosc.c:1485-1487), passes or fails the remaining header
  // checks with that count, runs no block and returns 0 with nothing written (serial_blosc's loop, blosc.c:814).  Same here (round 6; rounds 1 - 5
  // answered -1).
  const bool neg = h.nbytes < 0;
  if (!neg && (size_t)h.nbytes > destsize) { *res = -1; return 0; }            // blosc.c:1490-1492
  if (srcsize && (h.cbytes < 0 || (size_t)h.cbytes > srcsize)) { *res = -1; return 0; }  // extension: caller told us the buffer size
  if (h.flags & kFlagMemcpyed) {
    if ((int32_t)((uint32_t)h.nbytes + (uint32_t)kMaxOverhead) != h.cbytes) { *res = -1; return 0; }   // blosc.c:1494-1499
    *fmt = 0;
    if (neg) { *res = 0; return 0; }
    return 1;
  }
  const int f = (h.flags & 0xe0) >> 5;                                         // blosc.c:525-574
  if (f != FMT_BLOSCLZ && f != FMT_LZ4 && f != FMT_ZLIB && f != FMT_ZSTD) { *res = -5; return 0; }   // Snappy: not built, like a stock build without it
  if (h.versionlz != 1) { *res = -9; return 0; }
  *fmt = f;
  int32_t nblocks = h.nbytes / h.blocksize + ((h.nbytes % h.blocksize) > 0 ? 1 : 0);
  if (nblocks > (h.cbytes - 16) / 4) { *res = -1; return 0; }                  // blosc.c:1504-1507
  if (neg) { *res = 0; return 0; }                                             // nblocks <= 0: nothing runs
  return 1;
}

static int fetch_headers(EngineState& st, int n, const Job* jobs, bool device_ptrs, hipStream_t stream,
                         std::vector<Header>& hdrs) {
  hdrs.resize((size_t)n);
  if (!device_ptrs) {
    for (int i = 0; i < n; i++) hdrs[(size_t)i] = parse_header((const uint8_t*)jobs[i].src);
    return 0;
  }
  // device room: the first 16 bytes of the arena alone (carved first: a fixed offset), zeroed for the entries below.  The pointer table and the
  // headers live in the pinned arena only
  if (st.dev.ensure(16)) return -1;
  Carver cv;
  const size_t o_ptrs = cv.take(sizeof(void*) * (size_t)n);
  const size_t o_hdr = cv.take(16 * (size_t)n);
  if (st.pin.ensure(cv.off)) return -1;
  const void** pp = (const void**)(st.pin.base + o_ptrs);
  // an entry whose caller-stated size cannot hold a header is never dereferenced: it reads those 16 zeroed bytes
  // instead and is rejected by classify_for_decompress (cbytes 0 > ... version 0)
  bool any_short = false;
  for (int i = 0; i < n; i++) { const bool sh = jobs[i].srcsize && jobs[i].srcsize < (size_t)kMaxOverhead; any_short |= sh; pp[i] = sh ? (const void*)st.dev.base : jobs[i].src; }
  if (any_short) HIP_TRY(hipMemsetAsync(st.dev.base, 0, 16, stream));
  // the kernel reads the pointer table from, and writes the headers to, the pinned arena directly, through its host address: one device operation
  // in front of the synchronisation instead of three (late in round 6; the call's host side is time the device stands idle).  This relies on
  // hipHostMalloc memory being mapped on every device, at the address the host uses
  hipLaunchKernelGGL(k_gather_headers, grid1((size_t)n * 16, 256), dim3(256), 0, stream,
                     (const uint8_t* const*)(st.pin.base + o_ptrs), st.pin.base + o_hdr, n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(stream));
  for (int i = 0; i < n; i++) hdrs[(size_t)i] = parse_header(st.pin.base + o_hdr + 16 * (size_t)i);
  for (int i = 0; i < n; i++) if (jobs[i].srcsize && jobs[i].srcsize < (size_t)kMaxOverhead) { hdrs[(size_t)i] = Header{}; hdrs[(size_t)i].nbytes = -1; hdrs[(size_t)i].version = -1; }
  return 0;
}

// Builds the tables for decoding blocks [j0, j1) of one validated chunk.
static void add_decode_chunk(const Header& h, int fmt, int chunk_index, int32_t j0, int32_t j1,
                             ChunkDesc& c, std::vector<BlockDesc>& blocks, size_t& nstreams) {
  memset(&c, 0, sizeof c);
  const int32_t T = h.typesize, bs = h.blocksize;
  c.nbytes = h.nbytes; c.cbytes = h.cbytes; c.blocksize = bs; c.typesize = T;
  c.nblocks = h.nbytes / bs + ((h.nbytes % bs) ? 1 : 0);
  c.leftover = h.nbytes % bs;
  c.fmt = fmt;
  const bool dont_split = (h.flags & kFlagDontSplit) != 0;
  const bool split = !dont_split && T <= kMaxSplits && bs / T >= kMinBufferSize;   // blosc.c:749-757
  c.nsplits = split ? T : 1;
  c.mode = 0;
  if (h.flags & kFlagMemcpyed) c.mode |= CH_MEMCPYED;
  else if ((h.flags & kFlagShuffle) && T > 1) c.mode |= CH_SHUFFLE;            // blosc.c:739-741
  else if (h.flags & kFlagBitShuffle) c.mode |= CH_BITSHUFFLE;
  c.first_block = (int32_t)blocks.size();
  c.first_stream = (int32_t)nstreams;
  if (c.mode & CH_MEMCPYED) return;
  for (int32_t j = j0; j < j1; j++) {
    BlockDesc b;
    b.chunk = chunk_index; b.blk = j; b.first_stream = (int32_t)nstreams;
    const bool last = (j == c.nblocks - 1) && c.leftover > 0;
    b.nstreams = (split && !last) ? T : 1;
    b.bsize = last ? c.leftover : bs; b.flags = fmt == FMT_ZSTD ? BLK_Z : (fmt == FMT_ZLIB ? (BLK_Z | BLK_ZLIB) : 0);   // BLK_Z: not in k_decode_streams' queues
    nstreams += (size_t)b.nstreams;
    blocks.push_back(b);
  }
}

// Everything launch_decode hands to the kernels.  The device pointers into the call's workspace are set by decode_workspace(); the block
// table and the queues (d_blocks, d_q*, d_zq*: the table cache's, or getitem's in its table area) and the any_* / tiles_* of filter_tiles() by the caller.
struct DecodeLaunch {
  ChunkDesc* d_chunks; BlockDesc* d_blocks; StreamDesc* d_streams; int32_t* d_status; uint32_t* d_ticket; uint32_t* d_blkdone;
  size_t clear_bytes;                            // d_status .. the end of d_cost: cleared by clear_decode_counters() before every launch
  uint32_t* d_spans; uint8_t* d_pat;             // periodic spans of the fused unshuffle (k_decode.hip: SpanCtx)
  uint32_t* d_cost;                              // [256] cycles per plane index (scheduling feedback)
  uint32_t* d_zticket; bool any_zstd;            // Zstd frames: k_zstd_entropy + k_zstd_exec (two-phase), the rest through k_zstd_streams
  bool any_zlib;                                 // zlib streams: k_zlib_streams with per-XCD queues of its own (ticket words d_zticket[8..15])
  const int32_t* d_zqlist; const int32_t* d_zqoff; size_t nstr_zlib;
  ZMeta* d_zmeta; ptrdiff_t zseq_delta;          // nullptr: everything through k_zstd_streams
  ZgLds* d_zgscr;                                // table scratch of the global two-phase variant (nullptr: not allocated)
  ZcTab* d_zctab;                                // its 16-bit sequence tables, one dense record per frame (k_zstd_seq; nullptr: the 32-bit ones inside d_zgscr)
  const int32_t* d_qlist; const int32_t* d_qoff;   // per-XCD stream queues: qoff[9] followed by qlist[nstr]
  size_t nblk, nstr; int nchunks;
  bool any_shuf, any_bit, any_copy; int tiles_shuf, tiles_bit;
  size_t nstr_queued;                              // streams left to k_decode_streams
};

// The decode workspace in st.dev, for decompress and for getitem.
struct DecodeShape {
  int nchunks; size_t nblk, nstr;
  size_t filt_bytes;        // filter scratch of the shuffled / bitshuffled chunks
  size_t zlit_bytes;        // literal scratch of the Zstd chunks (and as much again for the sequence triples of the two-phase path)
  bool any_zstd, two_phase; // two_phase:           // Zstd frames may go through k_zstd_entropy / k_zstd_exec (zstd2_mode()); false: all of them through k_zstd_streams
  size_t out_bytes = 0;     // getitem only: the decoded blocks land in the workspace,
  size_t extra_bytes = 0;   //               and so do all of its tables, in one more area (it uploads them as one piece, past the table cache)
};
struct DecodeAreas { uint8_t *filt, *zlit, *out, *extra; };
static int decode_workspace(EngineState& st, const DecodeShape& s, DecodeLaunch& L, DecodeAreas& A) {
  const size_t n = (size_t)s.nchunks, nblk1 = s.nblk ? s.nblk : 1, nstr1 = s.nstr ? s.nstr : 1;
  const int zstd2 = (s.any_zstd && s.two_phase) ? zstd2_mode() : 0;
  const bool use_zctab = zstd2 == 2 && BAMD_ZSTD_SEQ_KERNEL && !BAMD_ZSTD_LDS_FSE;
  Carver cv;
  const size_t o_chunks = cv.take(sizeof(ChunkDesc) * n);
  const size_t o_streams = cv.take(sizeof(StreamDesc) * nstr1);
  // status words + tickets + per-block arrival counters | cost words: taken back to back, ONE fill clears them (clear_decode_counters)
  const size_t o_blkdone = ticket_offset(n) + sizeof(uint32_t) * kDecTicketWords;
  const size_t o_status = cv.take(o_blkdone + sizeof(uint32_t) * nblk1);
  const size_t o_cost = cv.take(sizeof(uint32_t) * kCostWords);
  L.clear_bytes = cv.off - o_status;
  const size_t o_spans = cv.take(8 * nstr1);
  const size_t o_pat = cv.take(span_enabled() ? (size_t)2048 * nstr1 : 256);
  const size_t o_filt = cv.take(s.filt_bytes + 256);
  const size_t o_zlit = cv.take(s.zlit_bytes + 256);
  const size_t o_zseq = cv.take(s.zlit_bytes + 512);      // same layout as the literal scratch
  const size_t o_zmeta = cv.take(s.any_zstd && s.two_phase ? sizeof(ZMeta) * nstr1 : 64);
  const size_t o_zticket = cv.take(64);
  const size_t o_zgscr = cv.take(zstd2 == 2 ? sizeof(ZgLds) * nstr1 : 64);
  const size_t o_zctab = cv.take(use_zctab ? sizeof(ZcTab) * nstr1 : 64);
  const size_t o_out = cv.take(s.out_bytes ? s.out_bytes + 256 : 0);
  const size_t o_extra = cv.take(s.extra_bytes);
  if (st.dev.ensure(cv.off)) return -1;
  uint8_t* D = st.dev.base;
  A = DecodeAreas{D + o_filt, D + o_zlit, D + o_out, D + o_extra};
  L.d_chunks = (ChunkDesc*)(D + o_chunks); L.d_streams = (StreamDesc*)(D + o_streams);
  L.d_status = (int32_t*)(D + o_status);
  L.d_ticket = (uint32_t*)(D + o_status + ticket_offset(n));
  L.d_blkdone = (uint32_t*)(D + o_status + o_blkdone);
  L.d_cost = (uint32_t*)(D + o_cost);
  L.d_spans = span_enabled() ? (uint32_t*)(D + o_spans) : nullptr; L.d_pat = D + o_pat;
  L.d_zticket = (uint32_t*)(D + o_zticket);
  L.d_zmeta = (s.any_zstd && s.two_phase) ? (ZMeta*)(D + o_zmeta) : nullptr; L.zseq_delta = (ptrdiff_t)o_zseq - (ptrdiff_t)o_zlit + 8;
  L.d_zgscr = zstd2 == 2 ? (ZgLds*)(D + o_zgscr) : nullptr;
  L.d_zctab = use_zctab ? (ZcTab*)(D + o_zctab) : nullptr;
  L.nblk = s.nblk; L.nstr = s.nstr; L.nchunks = s.nchunks;
  return 0;
}
static int clear_decode_counters(const DecodeLaunch& L, hipStream_t stream) {
  HIP_TRY(hipMemsetAsync(L.d_status, 0, L.clear_bytes, stream));
  if (L.any_zstd || L.any_zlib) HIP_TRY(hipMemsetAsync(L.d_zticket, 0, 64, stream));
  return 0;
}

// The other end of a launch: the chunks' status words and the feedback words into pinned memory (read_back_decode, behind launch_decode) and,
// once the stream has been synchronised, decode_feedback: every queued task was taken, and a launch of 4096 streams or more - fewer say
// little - leaves its plane costs for the queue order of the calls that follow.
static int read_back_decode(const DecodeLaunch& L, void* status, void* cost, hipStream_t stream) {
  HIP_TRY(hipMemcpyAsync(status, L.d_status, sizeof(int32_t) * (size_t)L.nchunks, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(cost, L.d_cost, sizeof(uint32_t) * kCostWords, hipMemcpyDeviceToHost, stream));
  return 0;
}
static int decode_feedback(EngineState& st, const DecodeLaunch& L, const void* cost, const char* what) {
  if (check_done((const uint32_t*)cost, L.nstr_queued, L.any_zstd ? L.nstr : 0, what, L.nstr_zlib)) return -1;
  if (L.nstr >= 4096) { memcpy(st.dec_cost, cost, sizeof st.dec_cost); st.dec_cost_valid = true; }
  return 0;
}

static int launch_decode(EngineState& st, const DecodeLaunch& L, hipStream_t stream) {
  if (L.nblk) {
    {
      ProfScope ps(st, stream, "k_decode_plan");
      hipLaunchKernelGGL(k_decode_plan, grid1(L.nblk, 256), dim3(256), 0, stream, L.d_chunks, L.d_blocks, L.d_streams, L.d_status, (int)L.nblk);
    }
    if (L.nstr_queued) {
      ProfScope ps(st, stream, "k_decode_streams");
      const dim3 dgrid(persistent_grid(st, L.nstr_queued ? L.nstr_queued : 1, st.grid_wpc[GRID_DECODE]));
      BAMD_STREAM_PROFILE(prof, "BLOSC_AMD_DEC_PROFILE", L.nstr);
      hipLaunchKernelGGL(k_decode_streams, dgrid, dim3(64 * DEC_WAVES), 0, stream, L.d_streams, L.d_status, L.d_ticket, L.d_qlist, L.d_qoff, L.d_chunks, L.d_blocks, L.d_blkdone, L.d_spans, L.d_pat, L.d_cost, st.single_queue ? 1 : 0 BAMD_PROF_ARG(prof));
    }
    // single-block frames through k_zstd_entropy (16 frames per wave) + k_zstd_exec (zstd2_mode above); every other frame
    // shape is left to k_zstd_streams.
    // (Round 4 sent the batch through in 4 / 8 slices, every slice's entropy -> seq -> exec chain on a stream of its own with the entropy
    //  kernels in slice order, so that one slice's sequence chains run underneath the other slices' phases: 30.2 -> 28.5 ms on the reference
    //  frames of config 4, 11.0 -> 13.4 ms on linspace.  The timeline (profiles/r04/r04zp_*): the phases do overlap, but every kernel is slower
    //  in company - k_zstd_seq is bound by its scattered table reads, not by an idle chip - and 8 streams share 4 hardware queues.  Not kept.)
    const int zstd2 = zstd2_mode();
    const uint32_t* d_taken = nullptr;
    if (L.any_zstd && L.d_zmeta && zstd2) {
      {
        ProfScope ps(st, stream, "k_zstd_entropy");
        if (zstd2 == 2 && L.d_zgscr) hipLaunchKernelGGL(k_zstd_entropy_t<true>, grid1(L.nstr, ZG_FRAMES), dim3(64), 0, stream, L.d_streams, (int)L.nstr, L.d_chunks, L.d_blocks, L.d_zmeta, L.zseq_delta, L.d_zgscr, L.d_zctab);
        else hipLaunchKernelGGL(k_zstd_entropy_t<false>, grid1(L.nstr, ZG_FRAMES), dim3(64), 0, stream, L.d_streams, (int)L.nstr, L.d_chunks, L.d_blocks, L.d_zmeta, L.zseq_delta, (ZgLds*)nullptr, (ZcTab*)nullptr);
      }
      if (zstd2 == 2 && L.d_zgscr && BAMD_ZSTD_SEQ_KERNEL && !BAMD_ZSTD_LDS_FSE) {
        ProfScope ps(st, stream, "k_zstd_seq");      // the sequence streams of the frames phase A took, one lane per frame
        hipLaunchKernelGGL(k_zstd_seq, grid1(L.nstr, ZSEQ_FRAMES), dim3(64), 0, stream, L.d_streams, (int)L.nstr, L.d_chunks, L.d_blocks, L.d_zmeta, L.zseq_delta, L.d_zgscr, L.d_zctab);
      }
      {
        ProfScope ps(st, stream, "k_zstd_exec");
        hipLaunchKernelGGL(k_zstd_exec, dim3(persistent_grid(st, L.nstr, st.grid_wpc[GRID_ZSTD_EXEC])), dim3(64), 0, stream, L.d_streams, (int)L.nstr, L.d_status, L.d_zticket + 1,
                           L.d_chunks, L.d_blocks, L.d_zmeta, L.zseq_delta);
      }
      d_taken = (const uint32_t*)L.d_zmeta;
    }
    if (L.any_zstd) {
      ProfScope ps(st, stream, "k_zstd_streams");
      BAMD_STREAM_PROFILE(zprof, "BLOSC_AMD_ZSTD_PROFILE", L.nstr);
      hipLaunchKernelGGL(k_zstd_streams, dim3(persistent_grid(st, L.nstr, st.grid_wpc[GRID_ZSTD_STREAMS])), dim3(64), 0, stream, L.d_streams, (int)L.nstr, L.d_status,
                         L.d_zticket, L.d_chunks, L.d_blocks, L.d_cost + 257, d_taken BAMD_PROF_ARG(zprof));
    }
    if (L.any_zlib) {
      ProfScope ps(st, stream, "k_zlib_streams");
      hipLaunchKernelGGL(k_zlib_streams, dim3(persistent_grid(st, L.nstr_zlib ? L.nstr_zlib : 1, st.grid_wpc[GRID_ZLIB_STREAMS])), dim3(64), 0, stream, L.d_streams, L.d_status,
                         L.d_zticket + 8, L.d_zqlist, L.d_zqoff, L.d_cost + 259, L.d_chunks, L.d_blocks, L.d_blkdone, st.single_queue ? 1 : 0);
    }
    if (L.any_shuf) {
      ProfScope ps(st, stream, "k_unshuffle");
      hipLaunchKernelGGL(k_unshuffle, dim3((unsigned)L.nblk, (unsigned)L.tiles_shuf), dim3(FT_THREADS), 0, stream, L.d_chunks, L.d_blocks);
    }
    if (L.any_bit) {      // full tiles of typesize 1 / 2 / 4 / 8 through k_bitfilter_fast, the rest through the generic kernel
      ProfScope ps(st, stream, "k_bitunshuffle");
      hipLaunchKernelGGL(k_bitfilter_fast<1>, dim3((unsigned)L.nblk, (unsigned)L.tiles_bit), dim3(FT_THREADS), 0, stream, L.d_chunks, L.d_blocks);
      hipLaunchKernelGGL(k_bitunshuffle, dim3((unsigned)L.nblk, (unsigned)L.tiles_bit), dim3(FT_THREADS), 0, stream, L.d_chunks, L.d_blocks, 1);
    }
  }
  if (L.any_copy) {
    ProfScope ps(st, stream, "k_copy_chunks");
    hipLaunchKernelGGL(k_copy_chunks, dim3(64, (unsigned)L.nchunks), dim3(COMPACT_THREADS), 0, stream, L.d_chunks, kMaxOverhead);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// which filter work of chunk c runs inside the codec kernels (mode bits), and how many tiles the stand-alone filter kernels need for the rest
static void filter_tiles(ChunkDesc& c, DecodeLaunch& L, bool may_fuse) {
  const int32_t T = c.typesize, N = c.blocksize / T;
  // (Zstd chunks: only unsplit ones - the wave that decodes a block's one stream unshuffles it, k_decode.hip: fused_unshuffle_own_block;
  //  zlib chunks: split ones too, k_zlib_streams has per-XCD queues and the hand-off of the LZ4 kernel)
  const bool zfmt = c.fmt == FMT_ZSTD || c.fmt == FMT_ZLIB;
  if ((c.mode & CH_SHUFFLE) && fuse_enabled() && may_fuse && (zfmt ? (fused_fast_typesize(T) && (c.fmt == FMT_ZLIB || c.nsplits == 1)) : fused_typesize(T))) { c.mode |= CH_FUSED_UNSHUF; return; }
  if (c.mode & CH_SHUFFLE) {
    L.any_shuf = true;
    L.tiles_shuf = std::max(L.tiles_shuf, filter_tile_count(N, shuffle_tile_elems(T)));
  } else if ((c.mode & CH_BITSHUFFLE) && bitunshuffle_fused_host(T) && fuse_enabled() && may_fuse && !zfmt) {
    c.mode |= CH_FUSED_BITUNSH;      // round 4: the decode kernel bit-unshuffles every block when its last stream is done (k_decode.hip: bitunshuffle_block_wave)
  } else if (c.mode & CH_BITSHUFFLE) {
    L.any_bit = true;
    L.tiles_bit = std::max(L.tiles_bit, filter_tile_count(N, bitshuffle_tile_elems(T)));
  }
}

// The packed call's destinations: chunk i decodes into the h.nbytes bytes behind chunk i - 1's, a chunk whose header does not pass validation
// takes none.  A valid chunk whose slot ends behind the caller's buffer gets a destination of size 0, i.e. -1 like blosc_decompress with a short one.
// false: the caller only asked for the sizes (base == nullptr), results[] holds them.
static bool place_packed_chunks(int n, const std::vector<Header>& hdrs, const PackedBuffer& pk, std::vector<Job>& jobs, int* results) {
  constexpr size_t kAnySize = (size_t)INT32_MAX;      // validation alone: no header size exceeds it
  size_t off = 0;
  for (int i = 0; i < n; i++) {
    const Header& h = hdrs[(size_t)i];
    int res = -1, fmt = 0;
    const bool valid = classify_for_decompress(h, jobs[(size_t)i].srcsize, kAnySize, &res, &fmt) == 1;
    const size_t width = valid ? (size_t)h.nbytes : 0;
    pk.offsets[i] = off;
    jobs[(size_t)i].dst = pk.base ? (uint8_t*)pk.base + off : nullptr;
    jobs[(size_t)i].dstsize = valid ? (off + width <= pk.size ? width : 0) : kAnySize;
    if (!pk.base) results[i] = valid ? h.nbytes : res;
    off += width;
  }
  pk.offsets[n] = off;
  return pk.base != nullptr;
}

int engine_chunk_headers(int n, const void* const* src, Header* out, hipStream_t stream) {
  if (n <= 0) return 0;
  CtxGuard ctx; EngineState& st = *ctx.st;
  if (ensure_device(st)) return -1;
  std::vector<Job> jobs((size_t)n);
  for (int i = 0; i < n; i++) jobs[(size_t)i] = Job{src[i], nullptr, 0, 0};
  std::vector<Header> hdrs;
  if (fetch_headers(st, n, jobs.data(), true, stream, hdrs)) return -1;
  std::copy(hdrs.begin(), hdrs.end(), out);
  return 0;
}

// The call in a context its caller holds (engine_decompress_batch takes one; engine_put brings its own).
static int decompress_batch_in(EngineState& st, int n, const Job* jobs, int* results, bool device_ptrs, hipStream_t stream, const PackedBuffer* packed) {
  if (n <= 0) return 0;
  if (packed && !device_ptrs) return -1;
  if (ensure_device(st) || call_stream(st, !device_ptrs, &stream)) return -1;
  HostPhases ht(1);
  std::vector<Header> hdrs;
  if (fetch_headers(st, n, jobs, device_ptrs, stream, hdrs)) return -1;
  ht.mark(0);     // header gather (kernel + copy + sync)
  // ---- the destinations: the caller's, or - packed - what the headers say ----
  std::vector<Job> placed;
  if (packed) {
    placed.assign(jobs, jobs + n);
    if (!place_packed_chunks(n, hdrs, *packed, placed, results)) return 0;
    jobs = placed.data();
  }
  // ---- check and lay out the chunks ----
  std::vector<ChunkDesc> chunks((size_t)n);
  std::vector<uint8_t> live((size_t)n, 0);
  EngineState::TableKey key;                         // (modes stays empty: the decode queues are made of the block table and the plane order alone)
  std::vector<BlockDesc>& blocks = key.blocks;
  HostStaging io{!device_ptrs};
  size_t nstr = 0, nstr_z = 0, nstr_zlib = 0, filt_bytes = 0, zlit_bytes = 0;      // nstr_z: streams of Zstd / zlib chunks (their own kernels')
  DecodeLaunch L{};
  for (int i = 0; i < n; i++) {
    ChunkDesc& c = chunks[(size_t)i];
    const Header& h = hdrs[(size_t)i];
    memset(&c, 0, sizeof c);
    c.mode = CH_SKIP;
    int res = -1, fmt = 0;
    if (!classify_for_decompress(h, jobs[i].srcsize, jobs[i].dstsize, &res, &fmt)) { results[i] = res; continue; }
    add_decode_chunk(h, fmt, i, 0, h.nbytes / h.blocksize + ((h.nbytes % h.blocksize) ? 1 : 0), c, blocks, nstr);
    c.src = (const uint8_t*)jobs[i].src; c.dst = (uint8_t*)jobs[i].dst;
    live[(size_t)i] = 1;
    results[i] = c.nbytes;
    if (c.mode & CH_MEMCPYED) L.any_copy = true;
    filter_tiles(c, L, !st.single_queue);
    if (c.mode & (CH_SHUFFLE | CH_BITSHUFFLE)) filt_bytes = align_up(filt_bytes, 256) + (size_t)c.nblocks * filt_block_stride(c);
    if (c.fmt == FMT_ZSTD && !(c.mode & CH_MEMCPYED)) { L.any_zstd = true; zlit_bytes = align_up(zlit_bytes, 256) + (size_t)c.nbytes; }
    if (c.fmt == FMT_ZLIB && !(c.mode & CH_MEMCPYED)) L.any_zlib = true;
    if (c.fmt == FMT_ZSTD || c.fmt == FMT_ZLIB) nstr_z += nstr - (size_t)c.first_stream;     // (memcpyed chunks have no streams)
    if (c.fmt == FMT_ZLIB) nstr_zlib += nstr - (size_t)c.first_stream;
    io.add((size_t)c.cbytes, (size_t)c.nbytes);
  }
  const size_t nblk = blocks.size();
  // ---- workspace ----
  DecodeAreas A;
  if (decode_workspace(st, DecodeShape{n, nblk, nstr, filt_bytes, zlit_bytes, L.any_zstd, /*two_phase*/ true}, L, A)) return -1;
  // ---- stage the inputs of a host-pointer call, point every chunk at its scratch ----
  if (io.reserve(st.io)) return -1;
  {
    size_t fo = 0, zo = 0;
    for (int i = 0; i < n; i++) {
      if (!live[(size_t)i]) continue;
      ChunkDesc& c = chunks[(size_t)i];
      if (io.stage(c, jobs[i].src, (size_t)c.cbytes, (size_t)c.nbytes, stream)) return -1;
      if (c.mode & (CH_SHUFFLE | CH_BITSHUFFLE)) { fo = align_up(fo, 256); c.filt = A.filt + fo; fo += (size_t)c.nblocks * filt_block_stride(c); }
      if (c.fmt == FMT_ZSTD && !(c.mode & CH_MEMCPYED)) { zo = align_up(zo, 256); c.stage = A.zlit + zo; zo += (size_t)c.nbytes; }
    }
  }
  // ---- tables: the block table and the queues, still on the device from the last call of this geometry or built and uploaded now ----
  EngineState::TableCache& tc = st.dec_tabs;
  key.nq = st.single_queue ? 1 : 8;
  order_signature(blocks, st.dec_cost, st.dec_cost_valid, key.order);
  Carver pc;
  const size_t queue_words = 9 + (nstr ? nstr : 1);      // room for k_decode_streams' queues, and as much for k_zlib_streams'
  if (tc.begin("decompress", key, queue_words, queue_words, pc, [&](EngineState::TableCache& t) {
        build_xcd_queues(blocks, nstr, st.dec_cost, st.dec_cost_valid, t.queues, key.nq);
        if (L.any_zlib) build_xcd_queues(blocks, nstr, nullptr, false, t.zqueues, key.nq, BLK_ZLIB);
      })) return -1;
  const size_t p_chunks = pc.take(sizeof(ChunkDesc) * (size_t)n);
  const size_t p_status = pc.take(sizeof(int32_t) * (size_t)n);
  const size_t p_cost = pc.take(sizeof(uint32_t) * kCostWords);
  if (st.pin.ensure(pc.off)) return -1;
  uint8_t* P = st.pin.base;
  memcpy(P + p_chunks, chunks.data(), sizeof(ChunkDesc) * (size_t)n);
  HIP_TRY(hipMemcpyAsync(L.d_chunks, P + p_chunks, sizeof(ChunkDesc) * (size_t)n, hipMemcpyHostToDevice, stream));
  if (tc.upload(key, P, stream) || clear_decode_counters(L, stream)) return -1;
  L.d_blocks = tc.d_blocks();
  L.d_qoff = tc.d_qoff(); L.d_qlist = L.d_qoff + 9;
  L.d_zqoff = tc.d_zqoff(); L.d_zqlist = L.d_zqoff + 9; L.nstr_zlib = nstr_zlib;
  L.nstr_queued = nstr - nstr_z;
  ht.mark(2);     // tables, queues, uploads
  // ---- launch ----
  if (launch_decode(st, L, stream) || read_back_decode(L, P + p_status, P + p_cost, stream)) return -1;
  ht.mark(3);     // kernel launches
  // ---- collect ----
  HIP_TRY(hipStreamSynchronize(stream));
  ht.mark(4);     // waiting for the device
  prof_collect(st);
  if (nblk && decode_feedback(st, L, P + p_cost, "decompress")) return -1;
  tc.commit(key);
  if (debug_cost_enabled()) {
    fprintf(stderr, "[blosc_amd] decode plane costs:");
    for (int k = 0; k < 16; k++) fprintf(stderr, " %u", st.dec_cost[k]);
    fprintf(stderr, "\n");
  }
  const int32_t* stt = (const int32_t*)(P + p_status);
  for (int i = 0; i < n; i++) if (live[(size_t)i] && stt[i] < 0) results[i] = -1;       // blosc.c:1511-1514: every block-level error surfaces as -1
  return io.collect(n, jobs, chunks, live, results, stream);
}

int engine_decompress_batch(int n, const Job* jobs, int* results, bool device_ptrs, hipStream_t stream, const PackedBuffer* packed) {
  if (n <= 0) return 0;
  if (packed && !device_ptrs) return -1;
  CtxGuard ctx;
  return decompress_batch_in(*ctx.st, n, jobs, results, device_ptrs, stream, packed);
}

// ---------------------------------------------------------------------------------------------
// getitem (blosc/blosc.c:1574-1703): decode only the blocks overlapping [start, start+nitems)
// ---------------------------------------------------------------------------------------------
// the header checks of blosc_getitem in its order (blosc.c:1601-1632), for the single call and the batch: 1 = go on, else *res is the call's result
static int classify_for_getitem(const Header& h, int* res, int* fmt) {
  if (h.version != kVersionFormat) { *res = -9; return 0; }                      // blosc.c:1603-1604
  if (h.blocksize <= 0 || h.blocksize > h.nbytes || h.blocksize > kMaxBlockSize || h.typesize <= 0) { *res = -1; return 0; }
  *fmt = 0;
  if (h.flags & kFlagMemcpyed) {
    if (h.nbytes + kMaxOverhead != h.cbytes) { *res = -1; return 0; }
    return 1;
  }
  const int f = (h.flags & 0xe0) >> 5;
  if (f != FMT_BLOSCLZ && f != FMT_LZ4 && f != FMT_ZLIB && f != FMT_ZSTD) { *res = -5; return 0; }
  if (h.versionlz != 1) { *res = -9; return 0; }
  *fmt = f;
  const int32_t nblocks = h.nbytes / h.blocksize + ((h.nbytes % h.blocksize) ? 1 : 0);
  if (nblocks >= (h.cbytes - 16) / 4) { *res = -1; return 0; }                   // blosc.c:1630-1632 (sic: >=)
  return 1;
}

// One pipeline serves every entry point: many item ranges of many device-resident chunks (include/blosc_gpu_getitem.h: getitem_ranges below),
// and blosc_getitem / blosc_gpu_getitem as one range of one chunk (engine_getitem at the end).
//   1. one header fetch for the distinct chunks the ranges name, then every range is validated on the host (blosc.c:1645-1653);
//   2. per chunk the union of the blocks its valid ranges touch, cut into maximal runs of consecutive blocks.  A run decodes into one
//      slot of the workspace (the kernels address block j at base + j * blocksize, so the bases are biased to put the run's first block at
//      its slot: a range that crosses blocks reads one contiguous piece), and a block is decoded once however many ranges touch it.
//      Ranges of MEMCPYED chunks are served straight from src + 16;
//   3. one table upload and one launch_decode for all runs, formats mixed as in engine_decompress_batch;
//   4. k_getitem_gather (k_decode.hip) writes every slice, after reading the verdict of the blocks the slice depends on: a range that fails
//      writes nothing;
//   5. status and cost words come back, one synchronisation.
// Verdicts.  The decode kernels keep one status word per ChunkDesc, and blosc_getitem answers the code of the FIRST block (in block order) that
// does not decode, whatever happens to blocks the range does not touch.  So every block of a run enters the tables as a ChunkDesc of its own
// (add_decode_chunk with the interval [j, j + 1)): the status word the kernels already set is then per block, at 88 bytes of table per block
// decoded, and no kernel changes.  One word per run would blame a range for a neighbour's block.
// Passes.  The slots of one launch hold at most kGetitemPassBytes of decoded blocks (the filter scratch and the Zstd literal scratch take as
// much again each); a call that touches more runs as several passes - whole chunks are dealt to passes in the order the ranges name them, a
// single chunk beyond the bound is a pass of its own - each with its own launch and synchronisation.  The number of passes depends on the
// bytes decoded alone, never on the number of ranges.
constexpr size_t kGetitemPassBytes = (size_t)256 << 20;
static std::atomic<size_t> g_getitem_pass_bytes{kGetitemPassBytes};
void engine_getitem_pass_bytes(size_t bytes) { g_getitem_pass_bytes.store(bytes ? bytes : kGetitemPassBytes); }      // test hook: the pass logic on small inputs

namespace {
struct BlockRun { int32_t j0, j1; size_t off; int32_t entry0; };      // blocks [j0, j1): where block j0 lies in the pass's slots, and its table entry
struct RangeChunk {            // one distinct chunk the ranges name
  int fmt = 0, verdict = -1, pass = 0;
  bool usable = false, memcpyed = false;
  std::vector<BlockRun> runs;  // the block intervals of its ranges as they come, then (merge_runs) the maximal runs in block order
};
struct PlacedRange { int slot = -1; int64_t lo = 0; uint32_t want = 0; int32_t j0 = 0, j1 = 0; uint8_t* dst = nullptr; };
}  // namespace

static size_t merge_runs(std::vector<BlockRun>& runs, size_t bs) {      // returns the bytes of their slots
  std::sort(runs.begin(), runs.end(), [](const BlockRun& a, const BlockRun& b) { return a.j0 < b.j0; });
  size_t m = 0, bytes = 0;
  for (size_t i = 1; i < runs.size(); i++) {
    if (runs[i].j0 <= runs[m].j1) runs[m].j1 = std::max(runs[m].j1, runs[i].j1);
    else runs[++m] = runs[i];
  }
  if (!runs.empty()) runs.resize(m + 1);
  for (const BlockRun& r : runs) bytes += align_up((size_t)(r.j1 - r.j0) * bs, 256);
  return bytes;
}

// Chunks dealt to passes in their order, for getitem and every row call: a pass holds at most `bound` of their bytes, a single chunk beyond
// the bound is a pass of its own.  Returns the pass of each chunk.  A chunk without bytes stays in the pass of the chunk before it;
// empty_opens (getitem_ranges alone): behind a chunk beyond the bound it opens the next pass, as a chunk with bytes does.
static std::vector<int> deal_to_passes(const std::vector<size_t>& bytes, size_t bound, bool empty_opens = false) {
  std::vector<int> pass_of(bytes.size(), 0);
  size_t in_pass = 0; int pass = 0;
  for (size_t k = 0; k < bytes.size(); k++) {
    if (in_pass && (bytes[k] || empty_opens) && in_pass + bytes[k] > bound) { pass++; in_pass = 0; }
    pass_of[k] = pass; in_pass += bytes[k];
  }
  return pass_of;
}
// ... for the two calls that decode block runs (getitem_ranges, engine_take): the runs merged, their slots' bytes dealt.  Returns the passes.
static int deal_runs_to_passes(std::vector<RangeChunk>& uc, const std::vector<Header>& hdrs, bool empty_opens) {
  std::vector<size_t> bytes(uc.size());
  for (size_t k = 0; k < uc.size(); k++) bytes[k] = merge_runs(uc[k].runs, (size_t)(hdrs[k].blocksize > 0 ? hdrs[k].blocksize : 1));
  const std::vector<int> pass_of = deal_to_passes(bytes, g_getitem_pass_bytes.load(), empty_opens);
  for (size_t k = 0; k < uc.size(); k++) uc[k].pass = pass_of[k];
  return uc.empty() ? 1 : pass_of.back() + 1;
}

// "Decode the runs of one pass", shared by getitem_pass and take_pass (which differ in their gather tables and gather kernel alone):
// lay_out_runs, then decode_runs up to launch_decode, then - behind the caller's read_back_decode and gather launch - finish_pass.
struct PassRuns {
  std::vector<ChunkDesc> entries; std::vector<BlockDesc> blocks;      // one table entry per block decoded (+ the caller's extra status words)
  size_t nstr = 0, nstr_z = 0, nstr_zlib = 0, span = 0;
  bool any_filt = false;
  DecodeLaunch L{}; DecodeAreas A{};
  size_t t_gather = 0;                 // the caller's gather tables inside the pass's table area: A.extra + t_gather on the device
  size_t p_status = 0, p_cost = 0;     // what read_back_decode brings into the pinned arena
};

// the runs of the chunks dealt to `pass`: their slots, one table entry per block.  extra_status: status words behind the blocks' that the
// caller's gather kernel counts in (cleared and read back with them); they are entries without blocks
static void lay_out_runs(EngineState& st, int pass, std::vector<RangeChunk>& uc, const std::vector<Header>& hdrs, int extra_status, PassRuns& R) {
  std::vector<ChunkDesc>& entries = R.entries; std::vector<BlockDesc>& blocks = R.blocks;
  size_t &nstr = R.nstr, &nstr_z = R.nstr_z, &nstr_zlib = R.nstr_zlib, &span = R.span;
  bool& any_filt = R.any_filt;
  DecodeLaunch& L = R.L;
  for (size_t k = 0; k < uc.size(); k++) {
    RangeChunk& u = uc[k];
    if (u.pass != pass) continue;
    const Header& h = hdrs[k];
    for (BlockRun& r : u.runs) {
      r.off = span; r.entry0 = (int32_t)entries.size();
      span += align_up((size_t)(r.j1 - r.j0) * (size_t)h.blocksize, 256);
      for (int32_t j = r.j0; j < r.j1; j++) {
        ChunkDesc c;
        const size_t s0 = nstr;
        add_decode_chunk(h, u.fmt, (int)entries.size(), j, j + 1, c, blocks, nstr);
        filter_tiles(c, L, !st.single_queue);
        if (c.mode & (CH_SHUFFLE | CH_BITSHUFFLE)) any_filt = true;
        if (c.fmt == FMT_ZSTD) L.any_zstd = true;
        if (c.fmt == FMT_ZLIB) { L.any_zlib = true; nstr_zlib += nstr - s0; }
        if (c.fmt == FMT_ZSTD || c.fmt == FMT_ZLIB) nstr_z += nstr - s0;
        entries.push_back(c);
      }
    }
  }
  for (int k = 0; k < extra_status; k++) { ChunkDesc c; memset(&c, 0, sizeof c); entries.push_back(c); }
}

// Queues, workspace, every table of the pass - fill_gather(host image of the caller's gather_bytes of tables), called once the slots have
// their addresses (R.A) - in one upload, and the decode launches.  The status words are cleared whenever there is one.
template <class FillGather>
static int decode_runs(EngineState& st, int pass, const std::vector<RangeChunk>& uc, const std::vector<Header>& hdrs, const std::vector<Job>& jobs,
                       PassRuns& R, size_t gather_bytes, FillGather&& fill_gather, hipStream_t stream) {
  std::vector<ChunkDesc>& entries = R.entries; const std::vector<BlockDesc>& blocks = R.blocks;
  const size_t n = entries.size(), nblk = blocks.size(), nstr = R.nstr, span = R.span;
  DecodeLaunch& L = R.L; DecodeAreas& A = R.A;
  // ---- queues, as engine_decompress_batch builds them (a few blocks each time: the table cache stays the decompress path's alone) ----
  const int nq = st.single_queue ? 1 : 8;
  std::vector<int32_t> queues, zqueues;
  build_xcd_queues(blocks, nstr, st.dec_cost, st.dec_cost_valid, queues, nq);
  if (L.any_zlib) build_xcd_queues(blocks, nstr, nullptr, false, zqueues, nq, BLK_ZLIB);
  // ---- workspace; every table of the pass in one piece, laid out alike in pinned and in device memory ----
  Carver tv;
  const size_t t_chunks = tv.take(sizeof(ChunkDesc) * (n ? n : 1));
  const size_t t_blocks = tv.take(sizeof(BlockDesc) * (nblk ? nblk : 1));
  const size_t t_queues = tv.take(sizeof(int32_t) * queues.size());
  const size_t t_zqueues = tv.take(sizeof(int32_t) * (zqueues.size() + 1));
  R.t_gather = tv.take(gather_bytes);
  const size_t table_bytes = tv.off;
  R.p_status = tv.take(sizeof(int32_t) * (n ? n : 1));      // (pinned only: what comes back)
  R.p_cost = tv.take(sizeof(uint32_t) * kCostWords);
  if (decode_workspace(st, DecodeShape{(int)n, nblk, nstr, R.any_filt ? span : 0, L.any_zstd ? span : 0, L.any_zstd, /*two_phase*/ false, /*out_bytes*/ span, table_bytes}, L, A)) return -1;
  if (st.pin.ensure(tv.off)) return -1;
  uint8_t* P = st.pin.base;
  // kernels address block j at base + j * blocksize: bias the bases so that block r.j0 lands at the run's slot
  for (size_t k = 0; k < uc.size(); k++) {
    if (uc[k].pass != pass) continue;
    const size_t bs = (size_t)hdrs[k].blocksize;
    for (const BlockRun& r : uc[k].runs)
      for (int32_t j = r.j0; j < r.j1; j++) {
        ChunkDesc& c = entries[(size_t)(r.entry0 + (j - r.j0))];
        c.src = (const uint8_t*)jobs[k].src;
        c.dst = A.out + r.off - (size_t)r.j0 * bs;
        c.stage = c.fmt == FMT_ZSTD ? A.zlit + r.off - (size_t)r.j0 * bs : nullptr;
        c.filt = (c.mode & (CH_SHUFFLE | CH_BITSHUFFLE)) ? A.filt + r.off - (size_t)r.j0 * filt_block_stride(c) : nullptr;
      }
  }
  memcpy(P + t_chunks, entries.data(), sizeof(ChunkDesc) * n);
  memcpy(P + t_blocks, blocks.data(), sizeof(BlockDesc) * nblk);
  memcpy(P + t_queues, queues.data(), sizeof(int32_t) * queues.size());
  memcpy(P + t_zqueues, zqueues.data(), sizeof(int32_t) * zqueues.size());
  fill_gather(P + R.t_gather);
  HIP_TRY(hipMemcpyAsync(A.extra, P, table_bytes, hipMemcpyHostToDevice, stream));
  L.d_chunks = (ChunkDesc*)(A.extra + t_chunks); L.d_blocks = (BlockDesc*)(A.extra + t_blocks);
  L.d_qoff = (const int32_t*)(A.extra + t_queues); L.d_qlist = L.d_qoff + 9;
  L.d_zqoff = (const int32_t*)(A.extra + t_zqueues); L.d_zqlist = L.d_zqoff + 9; L.nstr_zlib = R.nstr_zlib;
  L.nstr_queued = nstr - R.nstr_z;
  if ((nblk || n) && clear_decode_counters(L, stream)) return -1;
  if (nblk && launch_decode(st, L, stream)) return -1;
  return 0;
}

// the pass's one synchronisation; the decode kernels took every task they were queued
static int finish_pass(EngineState& st, const PassRuns& R, const char* what, hipStream_t stream) {
  HIP_TRY(hipStreamSynchronize(stream));
  prof_collect(st);
  return R.blocks.empty() ? 0 : decode_feedback(st, R.L, st.pin.base + R.p_cost, what);
}

// one pass: decodes the runs of the chunks dealt to `pass` and gathers the ranges of those chunks
static int getitem_pass(EngineState& st, int pass, std::vector<RangeChunk>& uc, const std::vector<Header>& hdrs, const std::vector<Job>& jobs,
                        int nranges, const std::vector<PlacedRange>& pr, int* results, hipStream_t stream) {
  PassRuns R;
  lay_out_runs(st, pass, uc, hdrs, 0, R);
  const size_t nblk = R.blocks.size();
  // ---- the gather table: the ranges of this pass's chunks, in the caller's order ----
  std::vector<GatherRange> gr((size_t)nranges);
  std::vector<uint32_t> tile_first((size_t)nranges + 1, 0);
  for (int r = 0; r < nranges; r++) {
    GatherRange& g = gr[(size_t)r];
    memset(&g, 0, sizeof g);
    const PlacedRange& p = pr[(size_t)r];
    uint32_t tiles = 0;
    if (p.slot >= 0 && uc[(size_t)p.slot].pass == pass) { g.nbytes = p.want; g.dst = p.dst; tiles = (p.want + GI_TILE - 1) / GI_TILE; }
    tile_first[(size_t)r + 1] = tile_first[(size_t)r] + tiles;
  }
  const uint32_t ntiles = tile_first[(size_t)nranges];
  if (!nblk && !ntiles) return 0;
  // (the two tables 256 bytes apart, as every table of the pass)
  const size_t g_tiles = align_up(sizeof(GatherRange) * (size_t)nranges, 256), gather_bytes = g_tiles + sizeof(uint32_t) * ((size_t)nranges + 1);
  const auto fill_gather = [&](uint8_t* G) {
    for (int r = 0; r < nranges; r++) {
      GatherRange& g = gr[(size_t)r];
      if (!g.nbytes) continue;
      const PlacedRange& p = pr[(size_t)r];
      const RangeChunk& u = uc[(size_t)p.slot];
      if (u.memcpyed) { g.src = (const uint8_t*)jobs[(size_t)p.slot].src + kMaxOverhead + p.lo; continue; }
      // the run that holds block j0 (every block of the range lies in it: runs are unions of the ranges' intervals)
      auto it = std::upper_bound(u.runs.begin(), u.runs.end(), p.j0, [](int32_t j, const BlockRun& b) { return j < b.j0; });
      const BlockRun& run = *(it - 1);
      g.src = R.A.out + run.off + (size_t)(p.lo - (int64_t)run.j0 * hdrs[(size_t)p.slot].blocksize);
      g.status0 = run.entry0 + (p.j0 - run.j0); g.nstatus = p.j1 - p.j0;
    }
    memcpy(G, gr.data(), sizeof(GatherRange) * (size_t)nranges);
    memcpy(G + g_tiles, tile_first.data(), sizeof(uint32_t) * ((size_t)nranges + 1));
  };
  if (decode_runs(st, pass, uc, hdrs, jobs, R, gather_bytes, fill_gather, stream)) return -1;
  // ---- collect ----
  uint8_t* P = st.pin.base;
  if (nblk && read_back_decode(R.L, P + R.p_status, P + R.p_cost, stream)) return -1;
  if (ntiles) {
    ProfScope ps(st, stream, "k_getitem_gather");
    hipLaunchKernelGGL(k_getitem_gather, dim3(persistent_grid(st, ntiles, GI_WAVES_PER_CU)), dim3(GI_THREADS), 0, stream,
                       (const GatherRange*)(R.A.extra + R.t_gather), (const uint32_t*)(R.A.extra + R.t_gather + g_tiles), nranges, (const int32_t*)R.L.d_status);
    HIP_TRY(hipGetLastError());
  }
  if (finish_pass(st, R, "getitem", stream)) return -1;
  if (!nblk) return 0;
  const int32_t* stt = (const int32_t*)(P + R.p_status);
  for (int r = 0; r < nranges; r++) {
    const GatherRange& g = gr[(size_t)r];
    for (int32_t k = 0; k < g.nstatus; k++)
      if (stt[g.status0 + k] < 0) { results[r] = stt[g.status0 + k]; break; }      // blosc.c:1689-1692: blosc_d's code of the first block that fails
  }
  return 0;
}

// The call, in a context its caller holds.  chunks[].src is device memory; `given`: the headers of chunks[] where the caller has fetched them
// (nchunks entries), nullptr: fetched here.  `say`: the reference's two messages on stderr for ranges out of bounds (blosc_getitem's; the batched
// calls are silent).  results[r] is written for every range; -1: the call itself failed.
static int getitem_ranges(EngineState& st, int nchunks, const Job* chunks, const Header* given, int nranges, const ItemRange* ranges, int* results,
                          hipStream_t stream, const PackedBuffer* packed, bool say) {
  // ---- the headers of the distinct chunks the ranges name: one fetch ----
  std::vector<int> slot_of((size_t)(nchunks > 0 ? nchunks : 0), -1);
  std::vector<Job> jobs;
  std::vector<Header> hdrs;
  for (int r = 0; r < nranges; r++) {
    const int ci = ranges[r].chunk;
    if (ci < 0 || ci >= nchunks || slot_of[(size_t)ci] >= 0) continue;
    slot_of[(size_t)ci] = (int)jobs.size();
    jobs.push_back(chunks[ci]);
    if (given) hdrs.push_back(given[ci]);
  }
  if (!given && !jobs.empty() && fetch_headers(st, (int)jobs.size(), jobs.data(), true, stream, hdrs)) return -1;
  std::vector<RangeChunk> uc(jobs.size());
  for (size_t k = 0; k < uc.size(); k++) {
    RangeChunk& u = uc[k];
    const Header& h = hdrs[k];
    const size_t srcsize = jobs[k].srcsize;      // packed: what lies between two offsets is all a chunk may claim
    if (srcsize && srcsize < (size_t)kMaxOverhead) u.verdict = -1;
    else if (!classify_for_getitem(h, &u.verdict, &u.fmt)) continue;
    else if (srcsize && (h.cbytes < 0 || (size_t)h.cbytes > srcsize)) u.verdict = -1;
    else { u.usable = true; u.memcpyed = (h.flags & kFlagMemcpyed) != 0; }
  }
  // ---- the ranges: blosc_getitem's checks; packed: the slices back to back ----
  std::vector<PlacedRange> pr((size_t)nranges);
  size_t off = 0;
  for (int r = 0; r < nranges; r++) {
    if (packed) packed->offsets[r] = off;
    results[r] = -1;
    const int ci = ranges[r].chunk;
    if (ci < 0 || ci >= nchunks) continue;
    const int slot = slot_of[(size_t)ci];
    RangeChunk& u = uc[(size_t)slot];
    if (!u.usable) { results[r] = u.verdict; continue; }
    const Header& h = hdrs[(size_t)slot];
    const int32_t T = h.typesize, bs = h.blocksize;
    const int start = ranges[r].start, stop = (int)((unsigned)start + (unsigned)ranges[r].nitems);
    if (start < 0 || (int64_t)start * T > h.nbytes) { if (say) fprintf(stderr, "`start` out of bounds"); continue; }      // blosc.c:1645-1653
    if (stop < 0 || (int64_t)stop * T > h.nbytes) { if (say) fprintf(stderr, "`start`+`nitems` out of bounds"); continue; }
    const int64_t lo = (int64_t)start * T, hi = (int64_t)stop * T;
    if (hi <= lo) { results[r] = 0; continue; }
    PlacedRange& p = pr[(size_t)r];
    p.want = (uint32_t)(hi - lo); p.lo = lo; p.dst = (uint8_t*)ranges[r].dst;
    if (packed) {
      if (packed->base && off + p.want > packed->size) continue;      // a slot that ends behind the caller's buffer: -1, nothing written, no room taken
      p.dst = packed->base ? (uint8_t*)packed->base + off : nullptr;
      off += p.want;
    }
    results[r] = (int)p.want;
    p.slot = slot;
    p.j0 = (int32_t)(lo / bs); p.j1 = (int32_t)((hi + bs - 1) / bs);
    if (!u.memcpyed) u.runs.push_back(BlockRun{p.j0, p.j1, 0, 0});
  }
  if (packed) { packed->offsets[nranges] = off; if (!packed->base) return 0; }
  // ---- runs per chunk, chunks dealt to passes ----
  const int npass = deal_runs_to_passes(uc, hdrs, /*empty_opens*/ true);
  for (int p = 0; p < npass; p++)
    if (getitem_pass(st, p, uc, hdrs, jobs, nranges, pr, results, stream)) return -1;
  return 0;
}

int engine_getitem_batch(int nchunks, const Job* chunks, int nranges, const ItemRange* ranges, int* results, hipStream_t stream,
                         const PackedBuffer* packed) {
  if (packed) packed->offsets[0] = 0;
  if (nranges <= 0) return 0;
  CtxGuard ctx; EngineState& st = *ctx.st;
  if (ensure_device(st)) return -1;
  return getitem_ranges(st, nchunks, chunks, nullptr, nranges, ranges, results, stream, packed, /*say*/ false);
}

// ---------------------------------------------------------------------------------------------
// the row calls - take, put, where, aggregate: their shared front end
// ---------------------------------------------------------------------------------------------
// Every row call begins with one header fetch (first synchronisation) and rows_census on the host; a call with an unusable chunk ends there.
// Behind it: mark_touched and row_lanes_log2 (take, put), overlaps_a_source (put, where), deal_to_passes (above: getitem's too), and RowScan,
// the whole-chunk pipeline of put, where and aggregate.  The indices and the rows never come to the host.

// The census, before anything is decoded: which chunks are usable - classify_for_getitem's checks, the
// packed form's slot checks, nbytes a multiple of row_bytes -, and the rows and table entries in front of each (table: [n + 1]).
// chunk_rows_out[k] (may be nullptr): the chunk's rows or its negative code.  whole_chunks (put): every chunk is ONE block of nbytes, so
// k_take_mark's flags are per chunk - a MEMCPYED chunk too, which take gives blocksize 0 because it decodes nothing of it.
// false: a chunk is unusable, the rows cannot be numbered.
static bool rows_census(const std::vector<Job>& jobs, const std::vector<Header>& hdrs, size_t row_bytes, bool whole_chunks,
                        std::vector<RangeChunk>& uc, std::vector<TakeChunk>& table, int* chunk_rows_out) {
  const size_t n = jobs.size();
  table.resize(n + 1);
  int64_t rows = 0, blocks = 0;
  bool unusable = false;
  for (size_t k = 0; k < n; k++) {
    RangeChunk& u = uc[k];
    const Header& h = hdrs[k];
    const size_t srcsize = jobs[k].srcsize;      // packed: what lies between two offsets is all a chunk may claim
    const bool fits = !srcsize || (h.cbytes >= 0 && (size_t)h.cbytes <= srcsize);
    int32_t nblk = 0;
    u.verdict = -1;
    if (srcsize && srcsize < (size_t)kMaxOverhead) {}
    else if (h.version == kVersionFormat && h.nbytes == 0) u.usable = fits;      // no rows: no range blosc_getitem could be asked for
    else if (!classify_for_getitem(h, &u.verdict, &u.fmt)) {}
    else if (fits && (size_t)h.nbytes % row_bytes == 0) {
      u.usable = true; u.memcpyed = (h.flags & kFlagMemcpyed) != 0;
      nblk = u.memcpyed ? 1 : h.nbytes / h.blocksize + ((h.nbytes % h.blocksize) ? 1 : 0);
    } else u.verdict = -1;
    const int64_t mine = u.usable ? (int64_t)((size_t)h.nbytes / row_bytes) : 0;
    if (chunk_rows_out) chunk_rows_out[k] = u.usable ? (int)mine : u.verdict;
    unusable |= !u.usable;
    if (whole_chunks) { table[k] = TakeChunk{rows, (int32_t)k, mine ? h.nbytes : 0}; nblk = 1; }
    else table[k] = TakeChunk{rows, (int32_t)blocks, (u.usable && !u.memcpyed && h.nbytes) ? h.blocksize : 0};
    rows += mine; blocks += nblk;
  }
  table[n] = TakeChunk{rows, (int32_t)blocks, 0};
  return !unusable && blocks <= (int64_t)INT32_MAX;
}

static unsigned take_grid(const EngineState& st, size_t nidx, int lanes_log2) {
  const size_t per_group = (size_t)(TK_THREADS >> lanes_log2);
  return persistent_grid(st, (nidx + per_group - 1) / per_group, TK_WAVES_PER_CU / (TK_THREADS / 64));
}

// The blocks (take) or chunks (put: one block per chunk) some valid index names: k_take_mark over the census' table, in st.dev / st.pin.
// *flags: nflags bytes in st.pin, read behind the one synchronisation - theirs until the next decode or encode call of the context carves st.pin.
static int mark_touched(EngineState& st, const std::vector<TakeChunk>& table, size_t nflags, const int64_t* index, size_t nidx, size_t row_bytes,
                        hipStream_t stream, const uint8_t** flags) {
  const size_t table_bytes = sizeof(TakeChunk) * table.size();
  Carver cv;
  const size_t o_chunks = cv.take(table_bytes), o_touched = cv.take(nflags);
  if (st.dev.ensure(cv.off) || st.pin.ensure(cv.off)) return -1;
  uint8_t *D = st.dev.base, *P = st.pin.base;
  memcpy(P + o_chunks, table.data(), table_bytes);
  HIP_TRY(hipMemcpyAsync(D + o_chunks, P + o_chunks, table_bytes, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemsetAsync(D + o_touched, 0, nflags, stream));
  {
    ProfScope ps(st, stream, "k_take_mark");
    hipLaunchKernelGGL(k_take_mark, dim3(take_grid(st, nidx, 0)), dim3(TK_THREADS), 0, stream, (const TakeChunk*)(D + o_chunks), (int)table.size() - 1, index,
                       nidx, (uint32_t)row_bytes, D + o_touched);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(P + o_touched, D + o_touched, nflags, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  prof_collect(st);
  *flags = P + o_touched;
  return 0;
}

// Lanes per row, as a power of two: one up to 16 bytes; above, one per 16-byte piece (at most the wave), and at least 16 where rows have head
// and tail bytes - misaligned: row_bytes, or an address the rows are laid out from, is no multiple of 16.
static int row_lanes_log2(size_t row_bytes, bool misaligned) {
  int lanes_log2 = 0;
  if (row_bytes > 16) {
    while (((size_t)16 << lanes_log2) < row_bytes && lanes_log2 < 6) lanes_log2++;
    if (misaligned && lanes_log2 < 4) lanes_log2 = 4;
  }
  return lanes_log2;
}

// An output [lo, hi) of the call that lies over a chunk it reads
static bool overlaps_a_source(const std::vector<Job>& jobs, const std::vector<Header>& hdrs, uintptr_t lo, uintptr_t hi) {
  for (size_t k = 0; k < jobs.size(); k++) {
    const uintptr_t s0 = (uintptr_t)jobs[k].src, s1 = s0 + (jobs[k].srcsize ? jobs[k].srcsize : (size_t)hdrs[k].cbytes);
    if (s0 < hi && lo < s1) return true;
  }
  return false;
}

// RowScan.  census() fetches the headers and counts the rows; the caller then says which chunks are live - decoded, because they hold rows
// (where, aggregate) or an index names them (put); deal() deals the live chunks' plaintext to passes and sizes the workspace; decode_pass()
// decodes the next pass (the decompress call's two synchronisations, headers and verdicts - the verdicts are on the host, so what the caller
// launches behind it needs no status words of the device).  A chunk that does not decode (blosc.c:1511-1514) keeps its slot and has code[k] < 0.
// Memory.  st.io holds a table of entry_bytes per chunk for the caller (WhereChunk, PutChunk), a prefix of n + npass tile counts (pass p over
// chunks [c0, c1): entries [c0 + p, c1 + p]), back_bytes at o_back for whatever else the call uploads or brings down, and the workspace of
// the largest pass: the slots, and extra_of[k] more per live chunk, free from `at` on.  st.put_pin holds the host images of all but the
// workspace, at the same offsets.  The decode and encode calls inside carve st.dev / st.pin anew and leave these two alone.
struct RowScan {
  size_t n = 0, npass = 0, unread = 0;          // unread: the rows of the chunks that did not decode
  std::vector<Header> hdrs; std::vector<Job> jobs; std::vector<TakeChunk> table;
  std::vector<int> rows_of, pass_of, code;      // rows_of: the chunk's rows or its negative code; code, negative: what the decoder answered
  std::vector<uint8_t> live;                    // [n], the caller's, between census() and deal()
  std::vector<uint8_t> pruned;                  // [n] or empty, the caller's, in front of deal_tiles(): chunks that hold rows and are not to be decoded
  std::vector<uint8_t*> slot_of;                // the plaintext of a live chunk once its pass is decoded
  std::vector<uint32_t> tiles_of;
  size_t o_chunks = 0, o_tiles = 0, o_back = 0, o_ws = 0;
  uint8_t *D = nullptr, *P = nullptr;
  // the pass decode_pass() has just decoded: chunks [c0, c1), the workspace free from `at` on
  size_t pass = 0, c0 = 0, c1 = 0, at = 0;
  uint32_t ntiles = 0;
  std::vector<Job> djobs; std::vector<int> dres;

  // one header fetch and the census; *usable false: rows_of holds every chunk's rows or its negative code, and the call is to answer -1
  int census(EngineState& st, int nchunks, const Job* chunks, size_t row_bytes, hipStream_t stream, bool* usable) {
    n = (size_t)(nchunks > 0 ? nchunks : 0);
    if (n && fetch_headers(st, (int)n, chunks, true, stream, hdrs)) return -1;
    jobs.assign(chunks, chunks + n);
    std::vector<RangeChunk> uc(n);
    rows_of.assign(n ? n : 1, 0);
    *usable = rows_census(jobs, hdrs, row_bytes, /*whole_chunks*/ true, uc, table, rows_of.data());
    return 0;
  }
  void rows_to(int* chunk_rows_out) const {
    if (chunk_rows_out) std::copy(rows_of.begin(), rows_of.begin() + (ptrdiff_t)n, chunk_rows_out);
  }
  // live chunks dealt to passes in chunk order; the workspace of the largest pass
  int deal(EngineState& st, const std::vector<size_t>& extra_of, size_t bound, size_t entry_bytes, size_t back_bytes) {
    std::vector<size_t> bytes(n, 0);
    for (size_t k = 0; k < n; k++) if (live[k]) bytes[k] = align_up((size_t)hdrs[k].nbytes, 256);
    pass_of = deal_to_passes(bytes, bound);
    npass = n ? (size_t)pass_of[n - 1] + 1 : 1;
    std::vector<size_t> ws_of(npass, 0);
    for (size_t k = 0; k < n; k++) if (live[k]) ws_of[(size_t)pass_of[k]] += bytes[k] + extra_of[k];
    code.assign(n, 0); slot_of.assign(n, nullptr);
    Carver cv;
    o_chunks = cv.take(entry_bytes * (n ? n : 1));
    o_tiles = cv.take(sizeof(uint32_t) * (n + npass));
    o_back = cv.take(back_bytes);
    const size_t table_bytes = cv.take(0);
    o_ws = cv.take(*std::max_element(ws_of.begin(), ws_of.end()) + 4 * 256);
    if (st.io.ensure(cv.off) || st.put_pin.ensure(table_bytes)) return -1;
    D = st.io.base; P = st.put_pin.base;
    return 0;
  }
  // Pass p = 0, 1, ... npass - 1, in this order.  *any_live false: the pass has no live chunk, nothing was launched
  int decode_pass(EngineState& st, size_t p, hipStream_t stream, bool* any_live) {
    pass = p;
    c0 = p ? c1 : 0; c1 = c0;
    while (c1 < n && pass_of[c1] == (int)pass) c1++;
    at = o_ws;
    djobs.clear();
    for (size_t k = c0; k < c1; k++) {
      if (!live[k]) continue;
      slot_of[k] = D + at;
      djobs.push_back(Job{jobs[k].src, D + at, jobs[k].srcsize, (size_t)hdrs[k].nbytes});
      at += align_up((size_t)hdrs[k].nbytes, 256);
    }
    *any_live = !djobs.empty();
    if (djobs.empty()) return 0;
    dres.assign(djobs.size(), -1);
    if (decompress_batch_in(st, (int)djobs.size(), djobs.data(), dres.data(), true, stream, nullptr)) return -1;
    for (size_t k = c0, i = 0; k < c1; k++) {
      if (!live[k]) continue;
      const int r = dres[i++];
      if (r != hdrs[k].nbytes) { code[k] = r < 0 ? r : -1; unread += (size_t)rows_of[k]; }
    }
    return 0;
  }

  // ---- where and aggregate: the chunks that hold rows are live, tile_bytes of workspace per tile of WH_TILE rows, the tables k_where.hip reads ----
  // The bound is at most 1 GiB, so that the counts of a pass stay in 32 bits.
  int deal_tiles(EngineState& st, size_t tile_bytes, size_t back_bytes) {
    std::vector<size_t> extra_of(n);
    live.assign(n, 0); tiles_of.assign(n, 0);
    for (size_t k = 0; k < n; k++) {
      live[k] = rows_of[k] != 0 && !(pruned.size() && pruned[k]);
      tiles_of[k] = live[k] ? (uint32_t)(((size_t)rows_of[k] + WH_TILE - 1) / WH_TILE) : 0u;      // a pruned chunk has no tile: nothing looks at it
      extra_of[k] = tile_bytes * tiles_of[k];
    }
    return deal(st, extra_of, std::min(g_getitem_pass_bytes.load(), (size_t)1 << 30), sizeof(WhereChunk), back_bytes);
  }
  // The zoned calls (include/blosc_gpu_zones.h), behind the census: the caller's rule on every chunk that holds rows.  false: the rule
  // refused the call.  pruned_out (may be nullptr) is written once every chunk has been asked
  bool prune(const RowPrune* by) {
    if (!by) return true;
    pruned.assign(n, 0);
    for (size_t k = 0; k < n; k++) {
      const int x = by->excludes(by->ctx, k, (uint64_t)rows_of[k]);
      if (x < 0) return false;
      pruned[k] = rows_of[k] != 0 && x > 0;
    }
    if (by->pruned_out) std::copy(pruned.begin(), pruned.end(), by->pruned_out);
    return true;
  }
  const WhereChunk* d_chunks() const { return (const WhereChunk*)(D + o_chunks) + c0; }
  const uint32_t* d_tiles() const { return (const uint32_t*)(D + o_tiles) + c0 + pass; }
  // decode_pass(), then the pass's WhereChunk table - a chunk that did not decode has a negative status, its tiles count nothing - and tile
  // prefix go up.  What the caller launches behind it finds its ntiles tiles' words from D + at on.
  int decode_tiles(EngineState& st, size_t p, hipStream_t stream, bool* holds_rows) {
    if (decode_pass(st, p, stream, holds_rows)) return -1;
    if (!*holds_rows) return 0;
    WhereChunk* h_chunks = (WhereChunk*)(P + o_chunks);
    uint32_t* tiles = (uint32_t*)(P + o_tiles) + c0 + pass;
    tiles[0] = 0;
    for (size_t k = c0; k < c1; k++) {
      h_chunks[k] = WhereChunk{slot_of[k], table[k].row_first, (uint32_t)rows_of[k], live[k] && code[k] >= 0 ? 0 : -1};
      tiles[k - c0 + 1] = tiles[k - c0] + tiles_of[k];
    }
    ntiles = tiles[c1 - c0];
    HIP_TRY(hipMemcpyAsync(D + o_chunks + sizeof(WhereChunk) * c0, h_chunks + c0, sizeof(WhereChunk) * (c1 - c0), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(D + o_tiles + sizeof(uint32_t) * (c0 + pass), tiles, sizeof(uint32_t) * (c1 - c0 + 1), hipMemcpyHostToDevice, stream));
    return 0;
  }
};

// ---------------------------------------------------------------------------------------------
// take (include/blosc_gpu_take.h): rows of the chunks by an index table that lies on the device
// ---------------------------------------------------------------------------------------------
// The shared front end (census over the chunks' blocks, mark_touched, row_lanes_log2) in front of getitem's block-run pipeline:
//   1. the maximal intervals of touched blocks are the chunks' runs - merged and dealt to passes as getitem_ranges does, but a chunk that
//      decodes nothing never opens a pass: a pass is a gather over all indices;
//   2. per pass decode_runs, then k_take_gather over ALL indices, with a table over the blocks of the call (dev_types.h: TakeBlock) that says
//      where a block lies in this pass's slots; rows of other passes' chunks are skipped, indices outside the rows are answered by the first pass;
//   3. the rows that failed are counted in one more status word behind the blocks', which comes down with them: one synchronisation per pass.
// Synchronisations: 2 + the passes, whatever nidx.
namespace {
struct TakeCall {
  std::vector<TakeChunk> chunks;      // [nchunks + 1]
  uint32_t row_bytes; int lanes_log2;
  size_t nidx; const int64_t* index; uint8_t* dest; int32_t* status;
  size_t failed = 0;
};
}  // namespace

static int take_pass(EngineState& st, int pass, std::vector<RangeChunk>& uc, const std::vector<Header>& hdrs, const std::vector<Job>& jobs,
                     TakeCall& tc, hipStream_t stream) {
  PassRuns R;
  lay_out_runs(st, pass, uc, hdrs, /*extra_status: the rows that failed*/ 1, R);
  const size_t nchunks = uc.size(), nblocks = (size_t)tc.chunks[nchunks].block_first;
  const size_t g_blocks = align_up(sizeof(TakeChunk) * (nchunks + 1), 256), gather_bytes = g_blocks + sizeof(TakeBlock) * (nblocks ? nblocks : 1);
  const auto fill_gather = [&](uint8_t* G) {
    memcpy(G, tc.chunks.data(), sizeof(TakeChunk) * (nchunks + 1));
    TakeBlock* tb = (TakeBlock*)(G + g_blocks);
    memset(tb, 0, sizeof(TakeBlock) * (nblocks ? nblocks : 1));      // base nullptr: not in this pass
    for (size_t k = 0; k < nchunks; k++) {
      if (uc[k].pass != pass) continue;
      TakeBlock* cb = tb + tc.chunks[k].block_first;
      if (uc[k].memcpyed) { cb[0].base = (const uint8_t*)jobs[k].src + kMaxOverhead; cb[0].status = -1; continue; }
      const size_t bs = (size_t)hdrs[k].blocksize;
      for (const BlockRun& r : uc[k].runs)
        for (int32_t j = r.j0; j < r.j1; j++) { cb[j].base = R.A.out + r.off + (size_t)(j - r.j0) * bs; cb[j].status = r.entry0 + (j - r.j0); }
    }
  };
  if (decode_runs(st, pass, uc, hdrs, jobs, R, gather_bytes, fill_gather, stream)) return -1;
  const size_t n = R.entries.size();
  {
    ProfScope ps(st, stream, "k_take_gather");
    hipLaunchKernelGGL(k_take_gather, dim3(take_grid(st, tc.nidx, tc.lanes_log2)), dim3(TK_THREADS), 0, stream,
                       (const TakeChunk*)(R.A.extra + R.t_gather), (int)nchunks, (const TakeBlock*)(R.A.extra + R.t_gather + g_blocks),
                       (const int32_t*)R.L.d_status, tc.index, tc.nidx, tc.row_bytes, tc.lanes_log2, tc.dest, tc.status,
                       (uint32_t*)(R.L.d_status + (n - 1)), pass == 0 ? 1 : 0);
    HIP_TRY(hipGetLastError());
  }
  if (read_back_decode(R.L, st.pin.base + R.p_status, st.pin.base + R.p_cost, stream) || finish_pass(st, R, "take", stream)) return -1;
  tc.failed += (size_t)((const uint32_t*)(st.pin.base + R.p_status))[n - 1];
  return 0;
}

int engine_take(int nchunks, const Job* chunks, size_t row_bytes, size_t nidx, const int64_t* index, void* dest, int* status,
                int* chunk_rows_out, size_t* failed_out, hipStream_t stream) {
  CtxGuard ctx; EngineState& st = *ctx.st;
  if (ensure_device(st)) return -1;
  const size_t n = (size_t)(nchunks > 0 ? nchunks : 0);
  std::vector<Header> hdrs;
  if (n && fetch_headers(st, (int)n, chunks, true, stream, hdrs)) return -1;
  // ---- the census: which chunks are usable, and the rows and blocks in front of each ----
  std::vector<Job> jobs(chunks, chunks + n);
  std::vector<RangeChunk> uc(n);
  TakeCall tc;
  if (!rows_census(jobs, hdrs, row_bytes, /*whole_chunks*/ false, uc, tc.chunks, chunk_rows_out)) return -1;
  const int64_t blocks = tc.chunks[n].block_first;
  if (failed_out) *failed_out = 0;
  if (!nidx) return 0;
  tc.row_bytes = (uint32_t)row_bytes; tc.nidx = nidx; tc.index = index; tc.dest = (uint8_t*)dest; tc.status = status;
  tc.lanes_log2 = row_lanes_log2(row_bytes, (((uintptr_t)dest | row_bytes) & 15) != 0);      // dest: the rows lie back to back from it
  // ---- the blocks the rows touch ----
  if (blocks) {
    const uint8_t* touched;
    if (mark_touched(st, tc.chunks, (size_t)blocks, index, nidx, row_bytes, stream, &touched)) return -1;
    // ---- runs: the maximal intervals of touched blocks of every chunk (a row's blocks are all marked, so they lie in one run) ----
    for (size_t k = 0; k < n; k++) {
      if (uc[k].memcpyed || !tc.chunks[k].blocksize) continue;
      const uint8_t* t = touched + tc.chunks[k].block_first;
      const int32_t nblk = tc.chunks[k + 1].block_first - tc.chunks[k].block_first;
      for (int32_t j = 0; j < nblk; j++) {
        if (!t[j]) continue;
        int32_t e = j + 1;
        while (e < nblk && t[e]) e++;
        uc[k].runs.push_back(BlockRun{j, e, 0, 0});
        j = e;
      }
    }
  }
  const int npass = deal_runs_to_passes(uc, hdrs, /*empty_opens*/ false);
  for (int p = 0; p < npass; p++)
    if (take_pass(st, p, uc, hdrs, jobs, tc, stream)) return -1;
  if (failed_out) *failed_out = tc.failed;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// put (include/blosc_gpu_put.h): rows written into the chunks by an index table that lies on the device; the result is a new container
// ---------------------------------------------------------------------------------------------
// RowScan with the chunks an index names as the live ones, and the engine's whole-chunk encoder behind it, in ONE context:
//   1. the census, then every chunk's parameters (check_cparams) and dest against the sources; mark_touched over one block per chunk, before
//      anything else has carved st.dev / st.pin: second synchronisation;
//   2. the touched chunks dealt under engine_take's bound, unclipped - a pass is a range [c0, c1) of chunks, and every chunk's place in dest
//      is known once the sizes of its pass are.  A live chunk's extra workspace: one owner word per row and nbytes + 16 for the encoder's output;
//   3. per pass with a touched chunk: decode_pass, k_put_claim and k_put_scatter over all indices, the chunks that decoded are compressed
//      (compress_entries_in's synchronisation), the others carried over as they are; per pass, touched chunk or not: the host sets the
//      offsets, k_put_assemble writes the pass's piece of dest (RowScan's tile prefix counts the PA_TILE pieces of the copies here);
//   4. the count of failed rows comes down, last synchronisation; the caller's host tables are written.
// Synchronisations: 3 + 3 per pass that has a touched chunk, whatever nidx.
int engine_put(int nchunks, const Job* chunks, size_t row_bytes, size_t nidx, const int64_t* index, const void* rows, const CompressParams* params,
               const PackedBuffer* out, int* cbytes_out, int* rewritten_out, int* status, int* chunk_rows_out, size_t* failed_out, hipStream_t stream) {
  CtxGuard ctx; EngineState& st = *ctx.st;
  if (ensure_device(st)) return -1;
  // ---- the census; then every chunk's parameters, its cbytes as the room: -1 for no chunk the compress call would write, or none to copy ----
  RowScan rs;
  bool usable = false;
  if (rs.census(st, nchunks, chunks, row_bytes, stream, &usable)) return -1;
  const size_t n = rs.n;
  const std::vector<Header>& hdrs = rs.hdrs;
  for (size_t k = 0; k < n; k++) {
    if (rs.rows_of[k] < 0) continue;      // unusable
    int code;
    if (check_cparams(params[k], (size_t)hdrs[k].nbytes, (size_t)std::max(hdrs[k].cbytes, 0), &code)) continue;
    rs.rows_of[k] = code ? code : -1;
    usable = false;
  }
  rs.rows_to(chunk_rows_out);
  if (!usable) return -1;
  if (out->base && out->size && overlaps_a_source(rs.jobs, hdrs, (uintptr_t)out->base, (uintptr_t)out->base + out->size)) return -1;
  // ---- the chunks some valid index names: k_take_mark over one block per chunk ----
  rs.live.assign(n, 0);
  bool any_touched = false;
  if (nidx && n) {
    const uint8_t* touched;
    if (mark_touched(st, rs.table, n, index, nidx, row_bytes, stream, &touched)) return -1;
    rs.live.assign(touched, touched + n);
    any_touched = std::count(touched, touched + n, 0) != (ptrdiff_t)n;
  }
  // ---- the passes; behind RowScan's tables the call's TakeChunk table, the chunks' PutCopy and the count of failed rows ----
  std::vector<size_t> extra_of(n);
  for (size_t k = 0; k < n; k++) {
    const size_t nb = (size_t)hdrs[k].nbytes;
    extra_of[k] = align_up(sizeof(uint32_t) * (nb / row_bytes), 256) + align_up(nb + kMaxOverhead, 256);
  }
  Carver back;
  const size_t b_table = back.take(sizeof(TakeChunk) * (n + 1)), b_copy = back.take(sizeof(PutCopy) * (n ? n : 1)), b_failed = back.take(sizeof(uint32_t));
  if (rs.deal(st, extra_of, g_getitem_pass_bytes.load(), sizeof(PutChunk), back.off)) return -1;
  const size_t o_put = rs.o_chunks, o_tiles = rs.o_tiles, o_table = rs.o_back + b_table, o_copy = rs.o_back + b_copy, o_failed = rs.o_back + b_failed;
  uint8_t *D = rs.D, *P = rs.P;
  memcpy(P + o_table, rs.table.data(), sizeof(TakeChunk) * (n + 1));
  HIP_TRY(hipMemcpyAsync(D + o_table, P + o_table, sizeof(TakeChunk) * (n + 1), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemsetAsync(D + o_failed, 0, sizeof(uint32_t), stream));
  const int lanes_log2 = row_lanes_log2(row_bytes, (row_bytes & 15) != 0);      // (the slots are aligned)
  const TakeChunk* d_table = (const TakeChunk*)(D + o_table);
  uint32_t* d_failed = (uint32_t*)(D + o_failed);
  PutChunk* h_put = (PutChunk*)(P + o_put); PutCopy* h_copy = (PutCopy*)(P + o_copy); uint32_t* h_tiles = (uint32_t*)(P + o_tiles);
  const auto scatter = [&](size_t c0, size_t c1, const uint32_t* owner, bool first) {
    ProfScope ps(st, stream, "k_put_scatter");
    hipLaunchKernelGGL(k_put_scatter, dim3(take_grid(st, nidx, lanes_log2)), dim3(TK_THREADS), 0, stream, d_table, (int)n, (const PutChunk*)(D + o_put) + c0,
                       (int)c0, (int)c1, owner, index, nidx, (uint32_t)row_bytes, lanes_log2, (const uint8_t*)rows, status, d_failed, first ? 1 : 0);
  };
  std::vector<size_t> offsets(n + 1, 0);
  std::vector<int> cbytes(n, 0), rewritten(n, 0);
  std::vector<Job> cjobs; std::vector<int> cres; std::vector<CompressParams> cpar;
  bool answered = false;      // the indices outside the rows have their -1
  for (size_t p = 0; p < rs.npass; p++) {
    // ---- the touched chunks of the pass: decode, claim, scatter, encode ----
    bool touched = false;
    if (rs.decode_pass(st, p, stream, &touched)) return -1;
    const size_t c0 = rs.c0, c1 = rs.c1;
    if (touched) {
      size_t at = rs.at, nrows = 0;      // behind the slots: the encoder's slots, then the owner words
      cjobs.clear(); cpar.clear();
      for (size_t k = c0; k < c1; k++) {      // an untouched chunk: no slot, all zero
        h_put[k] = PutChunk{rs.slot_of[k], rs.live[k] ? nrows : 0, rs.code[k] < 0 ? -1 : 0, 0};
        if (!rs.live[k]) continue;
        const size_t nb = (size_t)hdrs[k].nbytes;
        nrows += nb / row_bytes;
        rewritten[k] = rs.code[k] < 0 ? -1 : 1;      // -1: carried over as it is
        if (rewritten[k] != 1) continue;
        cjobs.push_back(Job{rs.slot_of[k], D + at, nb, nb + kMaxOverhead});
        cpar.push_back(params[k]);
        at += align_up(nb + kMaxOverhead, 256);
      }
      uint32_t* owner = (uint32_t*)(D + at);
      HIP_TRY(hipMemcpyAsync(D + o_put + sizeof(PutChunk) * c0, h_put + c0, sizeof(PutChunk) * (c1 - c0), hipMemcpyHostToDevice, stream));
      HIP_TRY(hipMemsetAsync(owner, 0xff, sizeof(uint32_t) * nrows, stream));
      {
        ProfScope ps(st, stream, "k_put_claim");
        hipLaunchKernelGGL(k_put_claim, dim3(take_grid(st, nidx, 0)), dim3(TK_THREADS), 0, stream, d_table, (int)n, (const PutChunk*)(D + o_put) + c0, (int)c0, (int)c1,
                           index, nidx, owner);
      }
      scatter(c0, c1, owner, !answered);
      answered = true;
      HIP_TRY(hipGetLastError());
      cres.assign(cjobs.size(), 0);
      if (compress_entries_in(st, cpar.data(), true, (int)cjobs.size(), cjobs.data(), cres.data(), true, stream, nullptr, nullptr)) return -1;
      for (size_t k = c0, j = 0; k < c1; k++) {
        if (rewritten[k] != 1) continue;
        if (cres[j] <= 0) return -1;      // (with destsize nbytes + 16 and checked parameters the call has no such answer)
        cbytes[k] = cres[j]; h_copy[k].src = (const uint8_t*)cjobs[j].dst; j++;
      }
    } else if (nidx && !any_touched) {      // no index names a row: the one scatter launch answers them all
      scatter(0, 0, nullptr, true);
      HIP_TRY(hipGetLastError());
      answered = true;
    }
    // ---- the pass's piece of dest ----
    uint32_t* tiles = h_tiles + c0 + p;
    tiles[0] = 0;
    for (size_t k = c0; k < c1; k++) {
      if (rewritten[k] != 1) { cbytes[k] = hdrs[k].cbytes; h_copy[k].src = (const uint8_t*)rs.jobs[k].src; }
      const size_t end = offsets[k] + (size_t)cbytes[k];
      offsets[k + 1] = align_up(end, out->align);
      h_copy[k].dst = (uint8_t*)out->base + offsets[k]; h_copy[k].nbytes = 0; h_copy[k].pad = 0;
      if (end <= out->size) { h_copy[k].nbytes = (uint32_t)cbytes[k]; h_copy[k].pad = (uint32_t)(std::min(offsets[k + 1], out->size) - end); }
      else cbytes[k] = 0;
      tiles[k - c0 + 1] = tiles[k - c0] + (h_copy[k].nbytes + h_copy[k].pad + PA_TILE - 1) / PA_TILE;
    }
    const uint32_t ntiles = tiles[c1 - c0];
    if (ntiles) {
      HIP_TRY(hipMemcpyAsync(D + o_copy + sizeof(PutCopy) * c0, h_copy + c0, sizeof(PutCopy) * (c1 - c0), hipMemcpyHostToDevice, stream));
      HIP_TRY(hipMemcpyAsync(D + o_tiles + sizeof(uint32_t) * (c0 + p), tiles, sizeof(uint32_t) * (c1 - c0 + 1), hipMemcpyHostToDevice, stream));
      ProfScope ps(st, stream, "k_put_assemble");
      hipLaunchKernelGGL(k_put_assemble, dim3(persistent_grid(st, ntiles, PA_WAVES_PER_CU)), dim3(PA_THREADS), 0, stream, (const PutCopy*)(D + o_copy) + c0,
                         (const uint32_t*)(D + o_tiles) + c0 + p, (int)(c1 - c0));
      HIP_TRY(hipGetLastError());
    }
  }
  // ---- collect ----
  uint32_t* h_failed = (uint32_t*)(P + o_failed);
  HIP_TRY(hipMemcpyAsync(h_failed, d_failed, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  prof_collect(st);
  for (size_t k = 0; k < n; k++) { out->offsets[k] = offsets[k]; if (cbytes_out) cbytes_out[k] = cbytes[k]; if (rewritten_out) rewritten_out[k] = rewritten[k]; }
  out->offsets[n] = offsets[n];
  if (failed_out) *failed_out = (size_t)*h_failed;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// where (include/blosc_gpu_where.h): the rows whose field satisfies a predicate, as the index table take and put read
// ---------------------------------------------------------------------------------------------
// RowScan with the chunks that hold rows as the live ones (deal_tiles, decode_tiles), in ONE context, around the three kernels of k_where.hip:
//   1. the census, index_out against every source;
//   2. per pass that holds a row: decode_tiles, then k_where_mark, and - where the caller gave a table - k_where_scan and k_where_write.  The
//      running total stays on the device: no pass waits for a count;
//   3. the chunks' counters come down, last synchronisation; the caller's host tables are written.
// Synchronisations: 2 + 2 per pass that holds a row, whatever the rows and the matches.
// Workspace per tile of WH_TILE rows: WH_WORDS mask words, a count and a base (140 bytes per 1024 rows).
// The body is written once for the one predicate and for a term list (include/blosc_gpu_clauses.h): `mark` launches the pass's mark kernel
// under its own profile name; `terms` (nullptr: none) goes up once, behind the counters, and `mark` receives its device address.
namespace {
struct MarkPass {      // what a mark kernel is launched with
  dim3 grid; const WhereChunk* d_chunks; const uint32_t* d_tiles; int in_pass; uint32_t row_bytes;
  uint64_t* d_masks; uint32_t* d_tile_count; uint32_t* d_count;
};
}  // namespace
template <class Mark>
static int where_passes(int nchunks, const Job* chunks, size_t row_bytes, const WhereTerms* terms, Mark mark, int64_t* index_out, size_t capacity,
                        size_t* total_out, int* chunk_matches_out, int* chunk_rows_out, size_t* unread_out, hipStream_t stream, const RowPrune* prune = nullptr) {
  CtxGuard ctx; EngineState& st = *ctx.st;
  if (ensure_device(st)) return -1;
  // ---- the census; then index_out against every source - a call that fails the second writes nothing at all ----
  RowScan rs;
  bool usable = false;
  if (rs.census(st, nchunks, chunks, row_bytes, stream, &usable)) return -1;
  const size_t n = rs.n;
  if (!usable) { rs.rows_to(chunk_rows_out); return -1; }
  if (capacity && overlaps_a_source(rs.jobs, rs.hdrs, (uintptr_t)index_out, (uintptr_t)index_out + capacity * sizeof(int64_t))) return -1;
  rs.rows_to(chunk_rows_out);
  if (!rs.prune(prune)) return -1;
  // ---- the passes: per tile its mask words, a count and a base; the running total and the chunks' counters come down at the end ----
  const size_t back_bytes = sizeof(uint64_t) + sizeof(uint32_t) * (n ? n : 1), o_terms = align_up(back_bytes, 16);
  if (rs.deal_tiles(st, sizeof(uint64_t) * WH_WORDS + sizeof(uint32_t) + sizeof(uint64_t), o_terms + (terms ? sizeof(WhereTerms) : 0))) return -1;
  uint8_t *D = rs.D, *P = rs.P;
  const size_t o_back = rs.o_back;
  uint64_t* d_running = (uint64_t*)(D + o_back);
  uint32_t* d_count = (uint32_t*)(D + o_back + sizeof(uint64_t));
  HIP_TRY(hipMemsetAsync(D + o_back, 0, back_bytes, stream));
  if (terms) {
    memcpy(P + o_back + o_terms, terms, sizeof(WhereTerms));
    HIP_TRY(hipMemcpyAsync(D + o_back + o_terms, P + o_back + o_terms, sizeof(WhereTerms), hipMemcpyHostToDevice, stream));
  }
  for (size_t p = 0; p < rs.npass; p++) {
    bool holds_rows = false;
    if (rs.decode_tiles(st, p, stream, &holds_rows)) return -1;
    if (holds_rows) {
      const size_t c0 = rs.c0, c1 = rs.c1;
      const uint32_t ntiles = rs.ntiles;
      Carver wv; wv.off = rs.at;
      uint64_t* d_masks = (uint64_t*)(D + wv.take(sizeof(uint64_t) * WH_WORDS * ntiles));
      uint32_t* d_tile_count = (uint32_t*)(D + wv.take(sizeof(uint32_t) * ntiles));
      uint64_t* d_tile_base = (uint64_t*)(D + wv.take(sizeof(uint64_t) * ntiles));
      const WhereChunk* d_chunks = rs.d_chunks();
      const uint32_t* d_tiles = rs.d_tiles();
      const dim3 grid(persistent_grid(st, ntiles, WH_WAVES_PER_CU / WH_WAVES));
      if (mark(st, stream, MarkPass{grid, d_chunks, d_tiles, (int)(c1 - c0), (uint32_t)row_bytes, d_masks, d_tile_count, d_count + c0},
               (const WhereTerms*)(D + o_back + o_terms))) return -1;
      if (capacity) {
        {
          ProfScope ps(st, stream, "k_where_scan");
          hipLaunchKernelGGL(k_where_scan, dim3(1), dim3(WH_SCAN_THREADS), 0, stream, (const uint32_t*)d_tile_count, ntiles, d_tile_base, d_running);
          HIP_TRY(hipGetLastError());
        }
        ProfScope ps(st, stream, "k_where_write");
        hipLaunchKernelGGL(k_where_write, grid, dim3(WH_THREADS), 0, stream, d_chunks, d_tiles, (int)(c1 - c0), (const uint64_t*)d_masks,
                           (const uint32_t*)d_tile_count, (const uint64_t*)d_tile_base, index_out, (uint64_t)capacity);
        HIP_TRY(hipGetLastError());
      }
    }
  }
  // ---- collect ----
  const uint32_t* h_count = (const uint32_t*)(P + o_back + sizeof(uint64_t));
  if (n) HIP_TRY(hipMemcpyAsync(P + o_back + sizeof(uint64_t), d_count, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  prof_collect(st);
  size_t total = 0;
  for (size_t k = 0; k < n; k++) {
    if (rs.code[k] >= 0) total += (size_t)h_count[k];
    if (chunk_matches_out) chunk_matches_out[k] = rs.code[k] < 0 ? rs.code[k] : (int)h_count[k];
  }
  if (total_out) *total_out = total;
  if (unread_out) *unread_out = rs.unread;
  return 0;
}
int engine_where(int nchunks, const Job* chunks, size_t row_bytes, const WherePred& pred, int64_t* index_out, size_t capacity, size_t* total_out,
                 int* chunk_matches_out, int* chunk_rows_out, size_t* unread_out, hipStream_t stream) {
  auto mark = [&pred](EngineState& st, hipStream_t stream, const MarkPass& m, const WhereTerms*) {
    ProfScope ps(st, stream, "k_where_mark");
    hipLaunchKernelGGL(k_where_mark, m.grid, dim3(WH_THREADS), 0, stream, m.d_chunks, m.d_tiles, m.in_pass, m.row_bytes, pred, m.d_masks, m.d_tile_count, m.d_count);
    HIP_TRY(hipGetLastError());
    return 0;
  };
  return where_passes(nchunks, chunks, row_bytes, nullptr, mark, index_out, capacity, total_out, chunk_matches_out, chunk_rows_out, unread_out, stream);
}
int engine_where_terms(int nchunks, const Job* chunks, size_t row_bytes, const WhereTerms& terms, int64_t* index_out, size_t capacity, size_t* total_out,
                       int* chunk_matches_out, int* chunk_rows_out, size_t* unread_out, hipStream_t stream, const RowPrune* prune) {
  auto mark = [](EngineState& st, hipStream_t stream, const MarkPass& m, const WhereTerms* d_terms) {
    ProfScope ps(st, stream, "k_where_mark_terms");
    hipLaunchKernelGGL(k_where_mark_terms, m.grid, dim3(WH_THREADS), 0, stream, m.d_chunks, m.d_tiles, m.in_pass, m.row_bytes, d_terms, m.d_masks, m.d_tile_count,
                       m.d_count);
    HIP_TRY(hipGetLastError());
    return 0;
  };
  return where_passes(nchunks, chunks, row_bytes, &terms, mark, index_out, capacity, total_out, chunk_matches_out, chunk_rows_out, unread_out, stream, prune);
}

// ---------------------------------------------------------------------------------------------
// aggregate (include/blosc_gpu_aggregate.h): count, sum, min and max of a row field, per chunk and for the call
// ---------------------------------------------------------------------------------------------
// RowScan as engine_where runs it, around the two kernels of k_aggregate.hip: per pass k_aggregate_tiles writes one AggPartial per tile,
// k_aggregate_chunks folds them into the chunks' entries of a device table of nchunks AggResult, which comes down with the last
// synchronisation.  Synchronisations: 2 + 2 per pass that holds a row.  Workspace: 40 bytes per tile of WH_TILE rows, 64 bytes per chunk.
// The call's total is folded here, on the host, from the chunks' results in chunk order: what a chunk answers does not depend on its neighbours.
static void aggregate_none(AggResult* r) { *r = AggResult{0, 0, 0, -1, -1, 0, 0, 0}; }
static void aggregate_fold(AggResult* total, const AggResult& c, const AggField& f) {
  bool nan;
  total->rows += c.rows; total->count += c.count; total->nans += c.nans;
  if (f.kind == 2) {
    double a, b;
    memcpy(&a, &total->sum, 8); memcpy(&b, &c.sum, 8);
    a += b;
    memcpy(&total->sum, &a, 8);
  } else total->sum += c.sum;
  // the smaller min and the larger max win, the earlier chunk among equals
  if (c.min_row >= 0 && (total->min_row < 0 || where_key(c.min, f.kind, f.bytes, f.inf, &nan) < where_key(total->min, f.kind, f.bytes, f.inf, &nan))) {
    total->min_row = c.min_row; total->min = c.min;
  }
  if (c.max_row >= 0 && (total->max_row < 0 || where_key(c.max, f.kind, f.bytes, f.inf, &nan) > where_key(total->max, f.kind, f.bytes, f.inf, &nan))) {
    total->max_row = c.max_row; total->max = c.max;
  }
}
// The body is written once, as where's: `tiles` launches the pass's tile kernel under its own profile name; `terms` (nullptr: none) goes up
// once, behind the chunks' results, and `tiles` receives its device address.
namespace {
struct TilesPass {      // what a tile kernel is launched with
  dim3 grid; const WhereChunk* d_chunks; const uint32_t* d_tiles; int in_pass; uint32_t row_bytes; AggPartial* d_partials;
};
}  // namespace
// Several fields (include/blosc_gpu_zones.h): nf partials per tile and nf results per chunk, chunk-major; `tiles` receives the device address
// of the field table, which goes up behind the term list, and k_aggregate_chunks_fields folds in k_aggregate_chunks' place.  several false:
// one field, no table, and both launches take what they always took.  prune (nullptr: none): the zoned calls' rule, asked behind the census;
// a chunk it excludes is in no launch and answers its rows and nothing else.
template <class Tiles>
static int aggregate_passes(int nchunks, const Job* chunks, size_t row_bytes, const AggField* fields, size_t nf, bool several, const WhereTerms* terms, Tiles tiles,
                            AggResult* total_out, AggResult* chunk_out, int* chunk_status_out, int* chunk_rows_out, size_t* unread_out, hipStream_t stream,
                            const RowPrune* prune = nullptr) {
  CtxGuard ctx; EngineState& st = *ctx.st;
  if (ensure_device(st)) return -1;
  RowScan rs;
  bool usable = false;
  if (rs.census(st, nchunks, chunks, row_bytes, stream, &usable)) return -1;
  const size_t n = rs.n;
  rs.rows_to(chunk_rows_out);
  if (!usable || !rs.prune(prune)) return -1;
  const size_t back_bytes = sizeof(AggResult) * nf * (n ? n : 1), o_fields = back_bytes + (terms ? sizeof(WhereTerms) : 0);
  if (rs.deal_tiles(st, sizeof(AggPartial) * nf, o_fields + (several ? sizeof(AggField) * nf : 0))) return -1;
  uint8_t *D = rs.D, *P = rs.P;
  AggResult* d_results = (AggResult*)(D + rs.o_back);
  const AggField* d_fields = (const AggField*)(D + rs.o_back + o_fields);
  if (terms) {
    memcpy(P + rs.o_back + back_bytes, terms, sizeof(WhereTerms));
    HIP_TRY(hipMemcpyAsync(D + rs.o_back + back_bytes, P + rs.o_back + back_bytes, sizeof(WhereTerms), hipMemcpyHostToDevice, stream));
  }
  if (several) {
    memcpy(P + rs.o_back + o_fields, fields, sizeof(AggField) * nf);
    HIP_TRY(hipMemcpyAsync(D + rs.o_back + o_fields, P + rs.o_back + o_fields, sizeof(AggField) * nf, hipMemcpyHostToDevice, stream));
  }
  for (size_t p = 0; p < rs.npass; p++) {
    bool holds_rows = false;
    if (rs.decode_tiles(st, p, stream, &holds_rows)) return -1;
    if (!holds_rows) continue;
    const int in_pass = (int)(rs.c1 - rs.c0);
    Carver wv; wv.off = rs.at;
    AggPartial* d_partials = (AggPartial*)(D + wv.take(sizeof(AggPartial) * nf * rs.ntiles));
    if (tiles(st, stream, TilesPass{dim3(persistent_grid(st, rs.ntiles, WH_WAVES_PER_CU / WH_WAVES)), rs.d_chunks(), rs.d_tiles(), in_pass, (uint32_t)row_bytes, d_partials},
              (const WhereTerms*)(D + rs.o_back + back_bytes), d_fields)) return -1;
    if (several) {
      ProfScope ps(st, stream, "k_aggregate_chunks_fields");
      hipLaunchKernelGGL(k_aggregate_chunks_fields, dim3(persistent_grid(st, (size_t)in_pass * nf, WH_WAVES_PER_CU / WH_WAVES)), dim3(WH_THREADS), 0, stream,
                         rs.d_chunks(), rs.d_tiles(), in_pass, (uint32_t)row_bytes, d_fields, (int)nf, (const AggPartial*)d_partials, d_results + rs.c0 * nf);
      HIP_TRY(hipGetLastError());
      continue;
    }
    ProfScope ps(st, stream, "k_aggregate_chunks");
    hipLaunchKernelGGL(k_aggregate_chunks, dim3(persistent_grid(st, (size_t)in_pass, WH_WAVES_PER_CU / WH_WAVES)), dim3(WH_THREADS), 0, stream, rs.d_chunks(),
                       rs.d_tiles(), in_pass, (uint32_t)row_bytes, fields[0], (const AggPartial*)d_partials, d_results + rs.c0);
    HIP_TRY(hipGetLastError());
  }
  // ---- collect: the chunks' entries; a chunk without rows, a pruned one, or one that did not decode, was in no launch or counts nothing ----
  const AggResult* h_results = (const AggResult*)(P + rs.o_back);
  if (n) HIP_TRY(hipMemcpyAsync(P + rs.o_back, d_results, sizeof(AggResult) * nf * n, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  prof_collect(st);
  std::vector<AggResult> total(nf);
  for (size_t f = 0; f < nf; f++) aggregate_none(&total[f]);
  for (size_t k = 0; k < n; k++) {
    const bool skipped = rs.pruned.size() && rs.pruned[k];
    for (size_t f = 0; f < nf; f++) {
      AggResult r;
      aggregate_none(&r);
      if (skipped) r.rows = (uint64_t)rs.rows_of[k];      // what a decoded chunk without a match answers
      else if (rs.rows_of[k] && rs.code[k] >= 0) r = h_results[k * nf + f];
      aggregate_fold(&total[f], r, fields[f]);
      if (chunk_out) chunk_out[k * nf + f] = r;
    }
    if (chunk_status_out) chunk_status_out[k] = rs.code[k];
  }
  if (total_out) std::copy(total.begin(), total.end(), total_out);
  if (unread_out) *unread_out = rs.unread;
  return 0;
}
int engine_aggregate(int nchunks, const Job* chunks, size_t row_bytes, const AggField& field, const WherePred* filter, AggResult* total_out,
                     AggResult* chunk_out, int* chunk_status_out, int* chunk_rows_out, size_t* unread_out, hipStream_t stream) {
  const WherePred q = filter ? *filter : WherePred{};
  const int filtered = filter ? 1 : 0;
  auto tiles = [&field, &q, filtered](EngineState& st, hipStream_t stream, const TilesPass& m, const WhereTerms*, const AggField*) {
    ProfScope ps(st, stream, "k_aggregate_tiles");
    hipLaunchKernelGGL(k_aggregate_tiles, m.grid, dim3(WH_THREADS), 0, stream, m.d_chunks, m.d_tiles, m.in_pass, m.row_bytes, field, q, filtered, m.d_partials);
    HIP_TRY(hipGetLastError());
    return 0;
  };
  return aggregate_passes(nchunks, chunks, row_bytes, &field, 1, false, nullptr, tiles, total_out, chunk_out, chunk_status_out, chunk_rows_out, unread_out, stream);
}
int engine_aggregate_terms(int nchunks, const Job* chunks, size_t row_bytes, const AggField& field, const WhereTerms& terms, AggResult* total_out,
                           AggResult* chunk_out, int* chunk_status_out, int* chunk_rows_out, size_t* unread_out, hipStream_t stream, const RowPrune* prune) {
  auto tiles = [&field](EngineState& st, hipStream_t stream, const TilesPass& m, const WhereTerms* d_terms, const AggField*) {
    ProfScope ps(st, stream, "k_aggregate_tiles_terms");
    hipLaunchKernelGGL(k_aggregate_tiles_terms, m.grid, dim3(WH_THREADS), 0, stream, m.d_chunks, m.d_tiles, m.in_pass, m.row_bytes, field, d_terms, m.d_partials);
    HIP_TRY(hipGetLastError());
    return 0;
  };
  return aggregate_passes(nchunks, chunks, row_bytes, &field, 1, false, &terms, tiles, total_out, chunk_out, chunk_status_out, chunk_rows_out, unread_out, stream, prune);
}
int engine_aggregate_fields(int nchunks, const Job* chunks, size_t row_bytes, const AggField* fields, int nfields, const WhereTerms& terms, AggResult* total_out,
                            AggResult* chunk_out, int* chunk_status_out, int* chunk_rows_out, size_t* unread_out, hipStream_t stream) {
  auto tiles = [nfields](EngineState& st, hipStream_t stream, const TilesPass& m, const WhereTerms* d_terms, const AggField* d_fields) {
    ProfScope ps(st, stream, "k_aggregate_tiles_fields");
    hipLaunchKernelGGL(k_aggregate_tiles_fields, m.grid, dim3(WH_THREADS), 0, stream, m.d_chunks, m.d_tiles, m.in_pass, m.row_bytes, d_fields, nfields, d_terms,
                       m.d_partials);
    HIP_TRY(hipGetLastError());
    return 0;
  };
  return aggregate_passes(nchunks, chunks, row_bytes, fields, (size_t)nfields, true, &terms, tiles, total_out, chunk_out, chunk_status_out, chunk_rows_out, unread_out,
                          stream);
}

// blosc_getitem / blosc_gpu_getitem: one chunk, one range, one result, each pointer host or device memory.  What only this call has: a stream
// of the context's own for host buffers; a host source staged into st.io, its header parsed where it lies and its cbytes trusted as
// blosc_getitem trusts it; a host destination served from a slot behind the source and copied out once the result is known to be
// positive - a call that fails writes nothing to dest.
int engine_getitem(const void* src, int start, int nitems, void* dest, bool src_dev, bool dst_dev, hipStream_t stream) {
  CtxGuard ctx; EngineState& st = *ctx.st;
  if (ensure_device(st) || call_stream(st, !src_dev && !dst_dev, &stream)) return -1;
  Job chunk{src, nullptr, 0, 0};
  ItemRange range{0, start, nitems, dest};
  std::vector<Header> hdrs;
  if (fetch_headers(st, 1, &chunk, src_dev, stream, hdrs)) return -1;
  const Header& h = hdrs[0];
  const bool host = !src_dev || !dst_dev;
  int verdict = -1, fmt = 0;
  if (host && nitems > 0 && classify_for_getitem(h, &verdict, &fmt)) {      // (any other call decodes nothing and touches neither pointer)
    const size_t in = src_dev ? 0 : align_up((size_t)h.cbytes, 256);
    const size_t out = dst_dev ? 0 : (size_t)std::min<int64_t>((int64_t)nitems * h.typesize, h.nbytes);
    if (st.io.ensure(in + out + 256)) return -1;
    if (!src_dev) { HIP_TRY(hipMemcpyAsync(st.io.base, src, (size_t)h.cbytes, hipMemcpyHostToDevice, stream)); chunk.src = st.io.base; }
    if (!dst_dev) range.dst = st.io.base + in;
  }
  int result = -1;
  if (getitem_ranges(st, 1, &chunk, &h, 1, &range, &result, stream, nullptr, /*say*/ true)) return -1;
  if (!dst_dev && result > 0) HIP_TRY(hipMemcpyAsync(dest, range.dst, (size_t)result, hipMemcpyDeviceToHost, stream));
  if (host) HIP_TRY(hipStreamSynchronize(stream));      // the staged source has been read, dest is written
  return result;
}

// ---------------------------------------------------------------------------------------------
// adler32 / crc32 of many runs (include/blosc_gpu_checksum.h, k_checksum.hip)
// ---------------------------------------------------------------------------------------------
static std::atomic<uint32_t> g_checksum_tile{CK_TILE_DEFAULT};
void engine_checksum_tile_bytes(size_t bytes) {      // test hook: several tiles per run on small inputs
  const size_t t = bytes ? (bytes > CK_TILE_MAX ? CK_TILE_MAX : bytes) & ~(size_t)15 : CK_TILE_DEFAULT;
  g_checksum_tile.store((uint32_t)(t < 16 ? 16 : t));
}

// One upload (the run table, the prefix sum of the runs' tile counts, the crc32 constants), the tile kernel, the combine kernel, one
// download of 4 bytes per run, one synchronisation - whatever the number of runs and their sizes.
int engine_checksum_batch(int kind, int n, const Job* runs, uint32_t* digests, hipStream_t stream) {
  if (n <= 0) return 0;
  CtxGuard ctx; EngineState& st = *ctx.st;
  if (ensure_device(st)) return -1;
  const uint32_t tile = g_checksum_tile.load();
  static uint32_t consts[CK_NCONST];
  static std::once_flag consts_once;
  std::call_once(consts_once, [] { ck_constants(consts); });
  Carver tv;                                  // the same layout in the pinned arena and at the front of the device arena
  const size_t o_runs = tv.take(sizeof(CkRun) * (size_t)n);
  const size_t o_tile0 = tv.take(sizeof(uint64_t) * ((size_t)n + 1));
  const size_t o_consts = tv.take(sizeof consts);
  const size_t table_bytes = tv.off;
  const size_t o_digests = tv.take(sizeof(uint32_t) * (size_t)n);
  if (st.pin.ensure(tv.off)) return -1;
  uint8_t* P = st.pin.base;
  CkRun* hr = (CkRun*)(P + o_runs);
  uint64_t* ht = (uint64_t*)(P + o_tile0);
  uint64_t ntiles = 0;
  for (int i = 0; i < n; i++) {
    hr[i] = CkRun{(const uint8_t*)runs[i].src, (uint64_t)runs[i].srcsize};
    ht[i] = ntiles;
    ntiles += ((uint64_t)runs[i].srcsize + tile - 1) / tile;
  }
  ht[n] = ntiles;
  memcpy(P + o_consts, consts, sizeof consts);
  const size_t o_partials = tv.take(sizeof(uint32_t) * (size_t)(ntiles ? ntiles : 1));
  if (st.dev.ensure(tv.off)) return -1;
  uint8_t* D = st.dev.base;
  HIP_TRY(hipMemcpyAsync(D, P, table_bytes, hipMemcpyHostToDevice, stream));
  const CkRun* d_runs = (const CkRun*)(D + o_runs);
  const uint64_t* d_tile0 = (const uint64_t*)(D + o_tile0);
  const uint32_t* d_consts = (const uint32_t*)(D + o_consts);
  uint32_t* d_partials = (uint32_t*)(D + o_partials);
  uint32_t* d_digests = (uint32_t*)(D + o_digests);
  if (ntiles) {
    ProfScope ps(st, stream, "k_checksum_tiles");
    const uint64_t want = (ntiles + CK_WAVES - 1) / CK_WAVES, most = (uint64_t)(st.cus > 0 ? st.cus : 256) * CK_WGS_PER_CU;
    hipLaunchKernelGGL(k_checksum_tiles, dim3((unsigned)(want < most ? want : most)), dim3(CK_THREADS), 0, stream,
                       kind, d_runs, d_tile0, (uint32_t)n, ntiles, tile, d_consts, d_partials);
  }
  {
    ProfScope ps(st, stream, "k_checksum_combine");
    hipLaunchKernelGGL(k_checksum_combine, grid1((size_t)n, CK_WAVES), dim3(CK_THREADS), 0, stream,
                       kind, d_runs, d_tile0, (uint32_t)n, d_consts, d_partials, d_digests);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(P + o_digests, d_digests, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  prof_collect(st);
  memcpy(digests, P + o_digests, sizeof(uint32_t) * (size_t)n);
  return 0;
}

// ---------------------------------------------------------------------------------------------
// stand-alone filter calls on host buffers (the reference exports blosc_internal_* for its own
// tests under BLOSC_TESTING, blosc/shuffle.h:34-61 + blosc/blosc-export.h:38-43)
// kind: 0 shuffle, 1 unshuffle, 2 bitshuffle, 3 bitunshuffle
// ---------------------------------------------------------------------------------------------
int engine_filter(int kind, size_t typesize, size_t blocksize, const void* src, void* dst) {
  CtxGuard ctx;
  EngineState& st = *ctx.st;
  if (ensure_device(st)) return -1;
  if (blocksize == 0) return 0;
  if (typesize == 0 || typesize > 255 || blocksize > (size_t)kMaxBlockSize) return -1;
  hipStream_t stream = 0;
  const int32_t T = (int32_t)typesize, bs = (int32_t)blocksize;
  Carver cv;
  const size_t o_chunk = cv.take(sizeof(ChunkDesc));
  const size_t o_block = cv.take(sizeof(BlockDesc));
  const size_t o_in = cv.take(blocksize + 256);
  const size_t o_out = cv.take(blocksize + 256);
  if (st.dev.ensure(cv.off)) return -1;
  uint8_t* D = st.dev.base;
  ChunkDesc c;
  memset(&c, 0, sizeof c);
  c.nbytes = bs; c.blocksize = bs; c.typesize = T; c.nblocks = 1; c.leftover = 0; c.nsplits = 1;
  const bool fwd = (kind == 0 || kind == 2);
  c.mode = (kind < 2) ? CH_SHUFFLE : CH_BITSHUFFLE;
  // forward kernels read c.src and write c.filt; inverse kernels read c.filt and write c.dst
  if (fwd) { c.src = D + o_in; c.filt = D + o_out; c.dst = nullptr; }
  else { c.filt = D + o_in; c.dst = D + o_out; c.src = nullptr; }
  BlockDesc b{0, 0, 0, 1, bs, 0};
  HIP_TRY(hipMemcpyAsync(D + o_chunk, &c, sizeof c, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(D + o_block, &b, sizeof b, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(D + o_in, src, blocksize, hipMemcpyHostToDevice, stream));
  const int tiles = filter_tile_count(bs / T, kind < 2 ? shuffle_tile_elems(T) : bitshuffle_tile_elems(T));
  const ChunkDesc* dc = (const ChunkDesc*)(D + o_chunk);
  const BlockDesc* db = (const BlockDesc*)(D + o_block);
  switch (kind) {
    case 0: hipLaunchKernelGGL(k_shuffle, dim3(1, (unsigned)tiles), dim3(FT_THREADS), 0, stream, dc, db); break;
    case 1: hipLaunchKernelGGL(k_unshuffle, dim3(1, (unsigned)tiles), dim3(FT_THREADS), 0, stream, dc, db); break;
    case 2: hipLaunchKernelGGL(k_bitfilter_fast<0>, dim3(1, (unsigned)tiles), dim3(FT_THREADS), 0, stream, dc, db);
            hipLaunchKernelGGL(k_bitshuffle, dim3(1, (unsigned)tiles), dim3(FT_THREADS), 0, stream, dc, db, 1); break;
    default: hipLaunchKernelGGL(k_bitfilter_fast<1>, dim3(1, (unsigned)tiles), dim3(FT_THREADS), 0, stream, dc, db);
             hipLaunchKernelGGL(k_bitunshuffle, dim3(1, (unsigned)tiles), dim3(FT_THREADS), 0, stream, dc, db, 1); break;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(dst, D + o_out, blocksize, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return 0;
}

// ---------------------------------------------------------------------------------------------
// misc
// ---------------------------------------------------------------------------------------------
int engine_set_device(int dev) {
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess || dev < 0 || dev >= cnt) return -1;
  g_device.store(dev);
  // ensure_device() probes the topology of THIS device (per-XCD queues are only valid where the probe says so) and resets
  // everything a context cached about the previous one; the other contexts do the same the next time they are used
  CtxGuard ctx;
  return ensure_device(*ctx.st);
}

// Binds the calling thread's calls to `dev` (-1: back to the process-wide device).  Used by the multi-GPU entry points
// (blosc_api.hip: one host thread per GPU); a context that lives on `dev` is preferred, so every GPU keeps its own arenas.
int engine_thread_device(int dev) {
  if (dev >= 0) { int cnt = 0; if (hipGetDeviceCount(&cnt) != hipSuccess || dev >= cnt) return -1; }
  tl_device = dev;
  return 0;
}
int engine_device_count() { int cnt = 0; if (hipGetDeviceCount(&cnt) != hipSuccess) { (void)hipGetLastError(); return 0; } return cnt; }

void engine_release() {
  if (hosttime_on()) {
    const char* nm[2] = {"compress", "decompress"};
    for (int d = 0; d < 2; d++) if (g_ht.calls[d])
      fprintf(stderr, "blosc_amd host time per %s call (ms, %ld calls): phase0 %.3f  phase1 %.3f  phase2 %.3f  launches %.3f  wait %.3f\n", nm[d], g_ht.calls[d],
              g_ht.t[d][0] / g_ht.calls[d], g_ht.t[d][1] / g_ht.calls[d], g_ht.t[d][2] / g_ht.calls[d], g_ht.t[d][3] / g_ht.calls[d], g_ht.t[d][4] / g_ht.calls[d]);
  }
  if (g_forked) return;
  for (int i = 0; i < kMaxCtx; i++) {
    EngineState& st = g_ctx[i];
    std::lock_guard<std::mutex> lock(st.mu);
    if (!st.device_ok) continue;
    st.dev.release(); st.io.release(); st.pin.release(); st.put_pin.release(); st.enc_tabs.drop(); st.dec_tabs.drop();
    if (st.own) { (void)hipStreamDestroy(st.own); st.own = nullptr; }
  }
}

bool engine_is_device_pointer(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

void engine_prof_enable(int on) { g_prof.store((on & 1) != 0); sched_override_off().store((on & 2) != 0); }      // bit 1: plain queue order for the calls that follow (queue_order.h)
void engine_prof_reset() {
  for (int i = 0; i < kMaxCtx; i++) { std::lock_guard<std::mutex> lock(g_ctx[i].mu); g_ctx[i].prof_acc.clear(); }
}
int engine_prof_get(const char* kernel, double* total_ms, int* launches) {      // summed over the contexts
  double ms = 0; int n = 0; bool found = false;
  for (int i = 0; i < kMaxCtx; i++) {
    std::lock_guard<std::mutex> lock(g_ctx[i].mu);
    auto it = g_ctx[i].prof_acc.find(kernel);
    if (it == g_ctx[i].prof_acc.end()) continue;
    ms += it->second.ms; n += it->second.launches; found = true;
  }
  if (total_ms) *total_ms = ms;
  if (launches) *launches = n;
  return found ? 0 : -1;
}

}  // namespace bamd
