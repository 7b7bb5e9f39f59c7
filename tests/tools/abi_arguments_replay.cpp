// tests/tools/abi_arguments_replay.cpp — the unusable and edge arguments of tests/test_abi_arguments.py once more, from C++, as a stand-alone program
// for a host sanitizer: it links a build of the emulated library (tests/tools/blosc_emu_lib.cpp) made with the same -fsanitize flags, calls every
// batch entry point with the same kinds of arguments (counts -1 and 0, every checked pointer NULL in turn, alignments, codec names, parameter
// rows, offset tables that fall / end outside / hold spans of 0 and 15 bytes, lengths beyond their span, runs given as a size alone) and checks the
// whole-call return values the golden file records.  What it is for is the sanitizer's silence; the answers in full are the Python test's.
//   CXX=/opt/rocm/lib/llvm/bin/clang++; S="-fsanitize=address,undefined -fno-omit-frame-pointer -g"
//   $CXX -std=c++17 -O1 -shared -fPIC -w $S -I tests/tools/wave_emu -I c-blosc_amd/csrc -I include -x c++ tests/tools/blosc_emu_lib.cpp -o /tmp/libblosc_amd_emu_san.so -lpthread
//   $CXX -std=c++17 -O1 $S -I include tests/tools/abi_arguments_replay.cpp -o /tmp/abi_arguments_replay /tmp/libblosc_amd_emu_san.so -Wl,-rpath,/tmp && /tmp/abi_arguments_replay
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "blosc.h"
#include "blosc_gpu.h"
#include "blosc_gpu_checksum.h"
#include "blosc_gpu_getitem.h"
#include "blosc_gpu_packed.h"
#include "blosc_gpu_params.h"

static int g_failed = 0, g_calls = 0;
#define EXPECT(want, call)                                                                   \
  do {                                                                                       \
    const long long got_ = (long long)(call);                                                \
    g_calls++;                                                                               \
    if (got_ != (long long)(want)) { g_failed++; printf("line %d: %s answered %lld, recorded %lld\n", __LINE__, #call, got_, (long long)(want)); } \
  } while (0)

static const int N = 3, T = 8;
static const size_t SIZES[N] = {2048, 4096, 3000}, BS = 512;

int main() {
  blosc_set_compressor("lz4");
  // plain data: noise for the compress calls (stored chunks), a counter for the chunks the reading calls take
  std::vector<uint8_t> noise[N], soft[N], chunk[N], dst[N];
  uint32_t x = 12345;
  for (int i = 0; i < N; i++) {
    noise[i].resize(SIZES[i]); soft[i].resize(SIZES[i]); chunk[i].resize(SIZES[i] + 16); dst[i].assign(SIZES[i] + 16, 0xEE);
    for (size_t k = 0; k < SIZES[i]; k++) { x = x * 1664525u + 1013904223u; noise[i][k] = (uint8_t)(x >> 24); soft[i][k] = (uint8_t)((k / 8) & 0x3f); }
    const int r = blosc_compress_ctx(5, 1, T, SIZES[i], soft[i].data(), chunk[i].data(), chunk[i].size(), "lz4", BS, 1);
    if (r <= 16 || (size_t)r >= SIZES[i]) { printf("set-up: chunk %d compressed to %d\n", i, r); return 2; }
    chunk[i].resize((size_t)r);
  }
  const void* src[N] = {noise[0].data(), noise[1].data(), noise[2].data()};
  const void* csrc[N] = {chunk[0].data(), chunk[1].data(), chunk[2].data()};
  size_t csize[N] = {chunk[0].size(), chunk[1].size(), chunk[2].size()};
  void* dest[N] = {dst[0].data(), dst[1].data(), dst[2].data()};
  size_t room[N] = {dst[0].size(), dst[1].size(), dst[2].size()};
  int res[16];
  size_t off[16];
  std::vector<uint8_t> big(40000, 0xEE);
  const char* names[4] = {"lz4", "snappy", "nosuch", nullptr};

  // ---- include/blosc_gpu.h ----
  for (int host = 0; host < 2; host++) {
    for (const char* name : names) {
      EXPECT(0, host ? blosc_gpu_compress_batch_host(5, 1, T, name, BS, N, src, SIZES, dest, room, res)
                     : blosc_gpu_compress_batch(5, 1, T, name, BS, N, src, SIZES, dest, room, res, nullptr));
      EXPECT((name && strcmp(name, "lz4")) ? -5 : (int)SIZES[2] + 16, res[2]);
    }
    for (int n : {-1, 0}) {
      EXPECT(0, host ? blosc_gpu_compress_batch_host(5, 1, T, "lz4", BS, n, nullptr, nullptr, nullptr, nullptr, nullptr)
                     : blosc_gpu_compress_batch(5, 1, T, "lz4", BS, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
      EXPECT(0, host ? blosc_gpu_decompress_batch_host(n, nullptr, nullptr, nullptr, nullptr, nullptr)
                     : blosc_gpu_decompress_batch(n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    }
    EXPECT(0, host ? blosc_gpu_compress_batch_host(11, 1, T, "lz4", BS, N, src, SIZES, dest, room, res)
                   : blosc_gpu_compress_batch(11, 1, T, "lz4", BS, N, src, SIZES, dest, room, res, nullptr));
    EXPECT(-10, res[0]);
    for (const size_t* given : {(const size_t*)csize, (const size_t*)nullptr}) {
      EXPECT(0, host ? blosc_gpu_decompress_batch_host(N, csrc, given, dest, room, res) : blosc_gpu_decompress_batch(N, csrc, given, dest, room, res, nullptr));
      EXPECT(SIZES[1], res[1]);
    }
  }
  const int dev0 = 0, dev7 = 7;
  EXPECT(0, blosc_gpu_compress_batch_multi(1, nullptr, 5, 1, T, nullptr, BS, N, src, SIZES, dest, room, res));
  EXPECT(0, blosc_gpu_compress_batch_multi(1, &dev0, 5, 1, T, "snappy", BS, N, src, SIZES, dest, room, res));
  EXPECT(0, blosc_gpu_decompress_batch_multi(1, &dev0, N, csrc, csize, dest, room, res));
  for (int ndev : {0, -1, 65}) {
    EXPECT(-1, blosc_gpu_compress_batch_multi(ndev, nullptr, 5, 1, T, "lz4", BS, N, src, SIZES, dest, room, res));
    EXPECT(-1, blosc_gpu_decompress_batch_multi(ndev, nullptr, N, csrc, csize, dest, room, res));
    EXPECT(0, blosc_gpu_decompress_batch_multi(ndev, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr));
  }
  EXPECT(-1, blosc_gpu_compress_batch_multi(1, &dev7, 5, 1, T, "lz4", BS, N, src, SIZES, dest, room, res));

  // ---- include/blosc_gpu_packed.h, include/blosc_gpu_params.h ----
  EXPECT(0, blosc_gpu_packed_bound(-1, SIZES, 1)); EXPECT(0, blosc_gpu_packed_bound(0, SIZES, 1)); EXPECT(0, blosc_gpu_packed_bound(N, nullptr, 1));
  EXPECT(9192, blosc_gpu_packed_bound(N, SIZES, 0)); EXPECT(0, blosc_gpu_packed_bound(N, SIZES, 3)); EXPECT(16384, blosc_gpu_packed_bound(N, SIZES, 4096));
  EXPECT(0, blosc_gpu_packed_bound(N, SIZES, 8192));
  blosc_gpu_cparams rows[N];
  for (int i = 0; i < N; i++) { memset(&rows[i], 0, sizeof rows[i]); rows[i].clevel = 5; rows[i].doshuffle = 1; rows[i].compcode = BLOSC_LZ4; rows[i].typesize = T; rows[i].blocksize = BS; }
  for (int per_chunk = 0; per_chunk < 2; per_chunk++) {
    auto call = [&](int n, const void* const* s, const size_t* nb, void* d, size_t dsize, size_t align, size_t* o, int* r, const char* name = "lz4", int clevel = 5) {
      return per_chunk ? blosc_gpu_compress_packed_params(n, rows, s, nb, d, dsize, align, o, r, nullptr)
                       : blosc_gpu_compress_packed(clevel, 1, T, name, BS, n, s, nb, d, dsize, align, o, r, nullptr);
    };
    for (size_t align : {(size_t)0, (size_t)16, (size_t)4096}) { EXPECT(0, call(N, src, SIZES, big.data(), big.size(), align, off, res)); EXPECT(SIZES[0] + 16, res[0]); }
    for (size_t align : {(size_t)3, (size_t)8192}) { EXPECT(-1, call(N, src, SIZES, big.data(), big.size(), align, off, res)); EXPECT(-1, call(0, src, SIZES, big.data(), big.size(), align, off, res)); }
    EXPECT(-1, call(-1, src, SIZES, big.data(), big.size(), 1, off, res)); EXPECT(-1, call(-1, src, SIZES, big.data(), big.size(), 1, nullptr, res));
    EXPECT(0, call(0, nullptr, nullptr, nullptr, 0, 1, off, nullptr)); EXPECT(-1, call(0, src, SIZES, big.data(), big.size(), 1, nullptr, res));
    EXPECT(-1, call(2, nullptr, SIZES, big.data(), big.size(), 1, off, res)); EXPECT(-1, call(2, src, nullptr, big.data(), big.size(), 1, off, res));
    EXPECT(-1, call(2, src, SIZES, big.data(), big.size(), 1, nullptr, res)); EXPECT(-1, call(2, src, SIZES, big.data(), big.size(), 1, off, nullptr));
    EXPECT(0, call(2, src, SIZES, nullptr, 0, 1, off, res)); EXPECT(6176, off[2]);
    EXPECT(-1, call(2, src, SIZES, nullptr, 4096, 1, off, res)); EXPECT(0, call(2, src, SIZES, big.data(), 0, 1, off, res));
    if (!per_chunk) {
      for (const char* name : {"snappy", "nosuch"}) { EXPECT(0, call(N, src, SIZES, big.data(), big.size(), 1, off, res, name)); EXPECT(-5, res[1]); EXPECT(0, off[N]); }
      EXPECT(-1, call(N, src, SIZES, big.data(), big.size(), 1, off, nullptr, "snappy"));
      EXPECT(0, call(N, src, SIZES, big.data(), big.size(), 1, off, res, nullptr)); EXPECT(0, call(N, src, SIZES, big.data(), big.size(), 1, off, res, "lz4", 11)); EXPECT(-10, res[0]);
    } else {
      EXPECT(-1, blosc_gpu_compress_packed_params(2, nullptr, src, SIZES, big.data(), big.size(), 1, off, res, nullptr));
    }
  }
  EXPECT(0, blosc_gpu_compress_batch_params(-1, rows, src, SIZES, dest, room, res, nullptr)); EXPECT(0, blosc_gpu_compress_batch_params(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  EXPECT(-1, blosc_gpu_compress_batch_params(2, nullptr, src, SIZES, dest, room, res, nullptr)); EXPECT(-1, blosc_gpu_compress_batch_params(2, rows, nullptr, SIZES, dest, room, res, nullptr));
  EXPECT(-1, blosc_gpu_compress_batch_params(2, rows, src, nullptr, dest, room, res, nullptr)); EXPECT(-1, blosc_gpu_compress_batch_params(2, rows, src, SIZES, nullptr, room, res, nullptr));
  EXPECT(-1, blosc_gpu_compress_batch_params(2, rows, src, SIZES, dest, nullptr, res, nullptr)); EXPECT(-1, blosc_gpu_compress_batch_params(2, rows, src, SIZES, dest, room, nullptr, nullptr));
  struct { int code[N], split[N], clevel[N], want[N]; } edge[] = {
      {{-1, 3, 6}, {0, 0, 0}, {5, 5, 5}, {2064, -5, -5}}, {{1, 1, 1}, {-1, 0, 5}, {5, 5, 5}, {-10, 4112, -10}}, {{1, 1, 1}, {1, 2, 4}, {11, -1, 0}, {-10, -10, 3016}}};
  for (auto& e : edge) {
    blosc_gpu_cparams r2[N];
    for (int i = 0; i < N; i++) { r2[i] = rows[i]; r2[i].compcode = e.code[i]; r2[i].splitmode = e.split[i]; r2[i].clevel = e.clevel[i]; }
    EXPECT(0, blosc_gpu_compress_batch_params(N, r2, src, SIZES, dest, room, res, nullptr));
    for (int i = 0; i < N; i++) EXPECT(e.want[i], res[i]);
    EXPECT(0, blosc_gpu_compress_packed_params(N, r2, src, SIZES, big.data(), big.size(), 1, off, res, nullptr));
    for (int i = 0; i < N; i++) EXPECT(e.want[i], res[i]);
  }

  // ---- containers for the reading calls: the chunks back to back; with 15 bytes of junk behind chunk 0 ----
  std::vector<uint8_t> cont, gap;
  size_t o[N + 1] = {0}, og[N + 1] = {0};
  for (int i = 0; i < N; i++) { cont.insert(cont.end(), chunk[i].begin(), chunk[i].end()); o[i + 1] = cont.size(); }
  gap = chunk[0]; gap.insert(gap.end(), 15, 0xA5); gap.insert(gap.end(), chunk[1].begin(), chunk[1].end());
  og[1] = chunk[0].size(); og[2] = og[1] + 15; og[3] = gap.size();
  const size_t falls[N + 1] = {o[0], o[2], o[1], o[3]}, span0[N + 1] = {o[0], o[1], o[1], o[2]}, none[N + 1] = {0, 0, 0, 0};
  std::vector<uint8_t> out(SIZES[0] + SIZES[1] + SIZES[2], 0xEE);
  EXPECT(0, blosc_gpu_decompress_packed(N, cont.data(), cont.size(), o, out.data(), out.size(), off, res, nullptr)); EXPECT(SIZES[2], res[2]);
  EXPECT(0, blosc_gpu_decompress_packed(N, cont.data(), cont.size(), o, nullptr, 0, off, res, nullptr)); EXPECT(out.size(), off[N]);
  EXPECT(0, blosc_gpu_decompress_packed(N, cont.data(), cont.size(), o, nullptr, 77, off, res, nullptr)); EXPECT(0, blosc_gpu_decompress_packed(N, cont.data(), cont.size(), o, out.data(), 0, off, res, nullptr));
  EXPECT(-1, blosc_gpu_decompress_packed(-1, cont.data(), cont.size(), o, out.data(), out.size(), off, res, nullptr)); EXPECT(0, blosc_gpu_decompress_packed(0, nullptr, 0, nullptr, nullptr, 0, off, nullptr, nullptr));
  EXPECT(-1, blosc_gpu_decompress_packed(0, cont.data(), cont.size(), o, out.data(), out.size(), nullptr, res, nullptr)); EXPECT(-1, blosc_gpu_decompress_packed(2, nullptr, cont.size(), o, out.data(), out.size(), off, res, nullptr));
  EXPECT(-1, blosc_gpu_decompress_packed(2, cont.data(), cont.size(), nullptr, out.data(), out.size(), off, res, nullptr)); EXPECT(-1, blosc_gpu_decompress_packed(2, cont.data(), cont.size(), o, out.data(), out.size(), nullptr, res, nullptr));
  EXPECT(-1, blosc_gpu_decompress_packed(2, cont.data(), cont.size(), o, out.data(), out.size(), off, nullptr, nullptr)); EXPECT(-1, blosc_gpu_decompress_packed(N, cont.data(), cont.size(), falls, out.data(), out.size(), off, res, nullptr));
  EXPECT(-1, blosc_gpu_decompress_packed(N, cont.data(), cont.size() - 1, o, out.data(), out.size(), off, res, nullptr)); EXPECT(-1, blosc_gpu_decompress_packed(2, nullptr, 0, none, out.data(), out.size(), off, res, nullptr));
  EXPECT(0, blosc_gpu_decompress_packed(N, cont.data(), cont.size(), span0, out.data(), out.size(), off, res, nullptr)); EXPECT(-1, res[1]); EXPECT(SIZES[1], res[2]);
  EXPECT(0, blosc_gpu_decompress_packed(N, gap.data(), gap.size(), og, out.data(), out.size(), off, res, nullptr)); EXPECT(-1, res[1]); EXPECT(SIZES[1], res[2]);
  size_t nb[N], cb[N], bs[N];
  EXPECT(0, blosc_gpu_cbuffer_sizes_batch(N, csrc, nb, cb, bs, nullptr)); EXPECT(SIZES[2], nb[2]); EXPECT(BS, bs[0]); EXPECT(csize[1], cb[1]);
  EXPECT(0, blosc_gpu_cbuffer_sizes_batch(2, csrc, nullptr, nullptr, nullptr, nullptr)); EXPECT(-1, blosc_gpu_cbuffer_sizes_batch(2, nullptr, nb, cb, bs, nullptr));
  EXPECT(-1, blosc_gpu_cbuffer_sizes_batch(-1, csrc, nb, cb, bs, nullptr)); EXPECT(0, blosc_gpu_cbuffer_sizes_batch(0, nullptr, nb, cb, bs, nullptr));

  // ---- include/blosc_gpu_getitem.h ----
  const int NR = 9, rc[NR] = {0, 2, 1, 3, -1, 1, 1, 0, 0}, rs[NR] = {0, 100, 500, 0, 0, 512, -1, 250, 256}, rn[NR] = {10, 50, 12, 1, 1, 1, 2, 6, 0}, want[NR] = {80, 400, 96, -1, -1, -1, -1, 48, 0};
  std::vector<uint8_t> slices[NR]; void* rdest[NR];
  for (int r = 0; r < NR; r++) { slices[r].assign((size_t)rn[r] * T + 8, 0xEE); rdest[r] = slices[r].data(); }
  EXPECT(0, blosc_gpu_getitem_batch(N, csrc, NR, rc, rs, rn, rdest, res, nullptr));
  for (int r = 0; r < NR; r++) EXPECT(want[r], res[r]);
  EXPECT(-1, blosc_gpu_getitem_batch(-1, csrc, NR, rc, rs, rn, rdest, res, nullptr)); EXPECT(-1, blosc_gpu_getitem_batch(N, csrc, -1, rc, rs, rn, rdest, res, nullptr));
  EXPECT(0, blosc_gpu_getitem_batch(N, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)); EXPECT(0, blosc_gpu_getitem_batch(0, nullptr, 2, rc, rs, rn, rdest, res, nullptr));
  EXPECT(-1, res[0]);
  EXPECT(-1, blosc_gpu_getitem_batch(2, nullptr, 2, rc, rs, rn, rdest, res, nullptr)); EXPECT(-1, blosc_gpu_getitem_batch(2, csrc, 2, nullptr, rs, rn, rdest, res, nullptr));
  EXPECT(-1, blosc_gpu_getitem_batch(2, csrc, 2, rc, nullptr, rn, rdest, res, nullptr)); EXPECT(-1, blosc_gpu_getitem_batch(2, csrc, 2, rc, rs, nullptr, rdest, res, nullptr));
  EXPECT(-1, blosc_gpu_getitem_batch(2, csrc, 2, rc, rs, rn, nullptr, res, nullptr)); EXPECT(-1, blosc_gpu_getitem_batch(2, csrc, 2, rc, rs, rn, rdest, nullptr, nullptr));
  auto gp = [&](int nchunks, const void* c, size_t csz, const size_t* table, int nranges, const int* a, const int* b, const int* d, void* dp, size_t dsz, size_t* oo, int* rr) {
    return blosc_gpu_getitem_packed(nchunks, c, csz, table, nranges, a, b, d, dp, dsz, oo, rr, nullptr);
  };
  EXPECT(0, gp(N, cont.data(), cont.size(), o, NR, rc, rs, rn, out.data(), out.size(), off, res)); EXPECT(624, off[NR]);
  for (int r = 0; r < NR; r++) EXPECT(want[r], res[r]);
  EXPECT(0, gp(N, cont.data(), cont.size(), o, NR, rc, rs, rn, nullptr, 0, off, res)); EXPECT(0, gp(N, cont.data(), cont.size(), o, NR, rc, rs, rn, nullptr, 99, off, res));
  EXPECT(0, gp(N, cont.data(), cont.size(), o, NR, rc, rs, rn, out.data(), 0, off, res)); EXPECT(-1, gp(-1, cont.data(), cont.size(), o, NR, rc, rs, rn, out.data(), out.size(), off, res));
  EXPECT(-1, gp(N, cont.data(), cont.size(), o, -1, rc, rs, rn, out.data(), out.size(), off, res)); EXPECT(0, gp(N, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, off, nullptr));
  EXPECT(-1, gp(N, cont.data(), cont.size(), o, 0, rc, rs, rn, out.data(), out.size(), nullptr, res)); EXPECT(0, gp(N, cont.data(), cont.size(), falls, 0, rc, rs, rn, out.data(), out.size(), off, res));
  EXPECT(0, gp(0, nullptr, 0, nullptr, 2, rc, rs, rn, out.data(), out.size(), off, res)); EXPECT(-1, gp(2, nullptr, 0, none, 2, rc, rs, rn, out.data(), out.size(), off, res));
  EXPECT(-1, gp(2, cont.data(), cont.size(), nullptr, 2, rc, rs, rn, out.data(), out.size(), off, res)); EXPECT(-1, gp(2, cont.data(), cont.size(), o, 2, nullptr, rs, rn, out.data(), out.size(), off, res));
  EXPECT(-1, gp(2, cont.data(), cont.size(), o, 2, rc, nullptr, rn, out.data(), out.size(), off, res)); EXPECT(-1, gp(2, cont.data(), cont.size(), o, 2, rc, rs, nullptr, out.data(), out.size(), off, res));
  EXPECT(-1, gp(2, cont.data(), cont.size(), o, 2, rc, rs, rn, out.data(), out.size(), nullptr, res)); EXPECT(-1, gp(2, cont.data(), cont.size(), o, 2, rc, rs, rn, out.data(), out.size(), off, nullptr));
  EXPECT(-1, gp(N, cont.data(), cont.size(), falls, NR, rc, rs, rn, out.data(), out.size(), off, res)); EXPECT(-1, gp(N, cont.data(), cont.size() - 1, o, NR, rc, rs, rn, out.data(), out.size(), off, res));
  EXPECT(0, gp(N, cont.data(), cont.size(), span0, NR, rc, rs, rn, out.data(), out.size(), off, res)); EXPECT(-1, res[2]); EXPECT(400, res[1]);
  EXPECT(0, gp(N, gap.data(), gap.size(), og, NR, rc, rs, rn, out.data(), out.size(), off, res)); EXPECT(-1, res[2]); EXPECT(400, res[1]);

  // ---- include/blosc_gpu_checksum.h ----
  uint8_t runs[64];
  for (int k = 0; k < 64; k++) runs[k] = (uint8_t)k;
  const void* rp[N] = {runs, runs + 10, runs + 10}; const void* rnull[N] = {runs, nullptr, runs + 10}; const void* rbad[N] = {runs, runs, nullptr};
  const size_t rsz[N] = {10, 0, 20}, huge[N] = {10, (size_t)INT32_MAX + 17, 20}, table[N + 1] = {0, 10, 10, 30}, tfalls[N + 1] = {0, 10, 9, 30}, t15[N + 1] = {5, 5, 20, 64};
  const size_t lens[N] = {10, 0, 7}, lbad[N] = {10, 1, 20}, same[N + 1] = {7, 7, 7, 7}, far[2] = {0, (size_t)INT32_MAX + 17};
  unsigned dig[N];
  const unsigned adler[N] = {11468846u, 1u, 226099591u}, crc[N] = {1164760902u, 0u, 2818760320u};
  for (int kind : {1, 2}) {
    const unsigned* w = kind == 1 ? adler : crc;
    EXPECT(0, blosc_gpu_checksum_batch(kind, N, rp, rsz, dig, nullptr)); for (int i = 0; i < N; i++) EXPECT(w[i], dig[i]);
    EXPECT(0, blosc_gpu_checksum_batch(kind, N, rnull, rsz, dig, nullptr)); for (int i = 0; i < N; i++) EXPECT(w[i], dig[i]);
    EXPECT(0, blosc_gpu_checksum_packed(kind, N, runs, 64, table, nullptr, dig, nullptr)); for (int i = 0; i < N; i++) EXPECT(w[i], dig[i]);
    EXPECT(0, blosc_gpu_checksum_packed(kind, N, runs, 30, table, lens, dig, nullptr)); EXPECT(w[0], dig[0]);
    EXPECT(0, blosc_gpu_checksum_packed(kind, N, runs, 64, t15, nullptr, dig, nullptr)); EXPECT(w[1], dig[0]);
    EXPECT(0, blosc_gpu_checksum_packed(kind, 2, nullptr, 0, none, nullptr, dig, nullptr)); EXPECT(w[1], dig[1]);
    EXPECT(0, blosc_gpu_checksum_packed(kind, 2, nullptr, 64, same, nullptr, dig, nullptr)); EXPECT(w[1], dig[0]);
  }
  for (int kind : {0, 3, -1})
    for (int n : {N, 0, -1}) { EXPECT(-1, blosc_gpu_checksum_batch(kind, n, rp, rsz, dig, nullptr)); EXPECT(-1, blosc_gpu_checksum_packed(kind, n, runs, 64, table, nullptr, dig, nullptr)); }
  for (int n : {0, -1}) { EXPECT(0, blosc_gpu_checksum_batch(1, n, nullptr, nullptr, nullptr, nullptr)); EXPECT(0, blosc_gpu_checksum_packed(2, n, nullptr, 0, nullptr, nullptr, nullptr, nullptr)); }
  EXPECT(-1, blosc_gpu_checksum_batch(1, 2, nullptr, rsz, dig, nullptr)); EXPECT(-1, blosc_gpu_checksum_batch(1, 2, rp, nullptr, dig, nullptr)); EXPECT(-1, blosc_gpu_checksum_batch(1, 2, rp, rsz, nullptr, nullptr));
  EXPECT(-1, blosc_gpu_checksum_batch(1, N, rbad, rsz, dig, nullptr)); EXPECT(-1, blosc_gpu_checksum_batch(1, N, rnull, huge, dig, nullptr));      // a size alone: nothing is read
  EXPECT(-1, blosc_gpu_checksum_packed(1, 2, nullptr, 64, table, nullptr, dig, nullptr)); EXPECT(-1, blosc_gpu_checksum_packed(1, 2, runs, 64, nullptr, nullptr, dig, nullptr));
  EXPECT(-1, blosc_gpu_checksum_packed(1, 2, runs, 64, table, nullptr, nullptr, nullptr)); EXPECT(-1, blosc_gpu_checksum_packed(1, N, runs, 64, tfalls, nullptr, dig, nullptr));
  EXPECT(-1, blosc_gpu_checksum_packed(1, N, runs, 29, table, nullptr, dig, nullptr)); EXPECT(-1, blosc_gpu_checksum_packed(1, N, runs, 64, table, lbad, dig, nullptr));
  EXPECT(-1, blosc_gpu_checksum_packed(1, 2, nullptr, 64, table, none, dig, nullptr)); EXPECT(-1, blosc_gpu_checksum_packed(1, 1, nullptr, far[1], far, nullptr, dig, nullptr));

  blosc_destroy();
  printf("%d calls and checks, %d differ\n", g_calls, g_failed);
  return g_failed ? 1 : 0;
}
