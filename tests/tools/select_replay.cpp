// tests/tools/select_replay.cpp — the two calls of include/blosc_gpu_select.h from C++, as a stand-alone program for a host sanitizer: it links a build of
// the emulated library (tests/tools/blosc_emu_lib.cpp) made with the same -fsanitize flags and runs ragged candidate tables (ranges of 0, 1, 3 and 70
// rows, bad rows among good ones, a chunk whose rows all fail), both forms, the sizing call and the unusable tables, with exactly sized output arrays
// between guard words.  It checks the winner against the candidate answers of the same call; what it is for is the sanitizer's silence over the
// host side (one table entry per candidate, the fold into the caller's arrays).  The answers in full are tests/select_checks.py's.
//   CXX=/opt/rocm/lib/llvm/bin/clang++; S="-fsanitize=address,undefined -fno-omit-frame-pointer -g"
//   $CXX -std=c++17 -O1 -shared -fPIC -w $S -I tests/tools/wave_emu -I c-blosc_amd/csrc -I include -x c++ tests/tools/blosc_emu_lib.cpp -o /tmp/libblosc_amd_emu_san.so -lpthread
//   $CXX -std=c++17 -O1 $S -I include tests/tools/select_replay.cpp -o /tmp/select_replay /tmp/libblosc_amd_emu_san.so -Wl,-rpath,/tmp && /tmp/select_replay
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "blosc.h"
#include "blosc_gpu_select.h"

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    g_checks++;                                                                \
    if (!(cond)) { g_failed++; printf("line %d: %s\n", __LINE__, #cond); }    \
  } while (0)

static blosc_gpu_cparams row(int clevel, int shuffle, int code, size_t T, size_t bs) { return blosc_gpu_cparams{clevel, shuffle, code, 0, T, bs}; }

int main() {
  const int N = 5;
  const size_t SIZES[N] = {6000, 3000, 4000, 0, 2048};
  std::vector<uint8_t> src[N], dst[N];
  uint32_t x = 777;
  for (int i = 0; i < N; i++) {
    src[i].resize(SIZES[i] + 1); dst[i].assign(SIZES[i] + 16, 0xEE);
    for (size_t k = 0; k < SIZES[i]; k++) { x = x * 1664525u + 1013904223u; src[i][k] = i == 1 ? (uint8_t)(x >> 24) : (uint8_t)(((k / 4) & 0x7f) + ((x >> 30) & 1)); }
  }
  // chunk 0: three good rows between two bad ones | chunk 1 (noise): one row | chunk 2: 70 rows | chunk 3 (empty): no rows | chunk 4: rows that all fail
  std::vector<blosc_gpu_cparams> rows;
  std::vector<int> first{0};
  rows.push_back(row(10, 1, BLOSC_LZ4, 4, 512)); rows.push_back(row(5, 0, BLOSC_LZ4, 1, 512)); rows.push_back(row(5, 1, BLOSC_LZ4, 4, 512));
  rows.push_back(row(5, 1, BLOSC_SNAPPY, 4, 512)); rows.push_back(row(3, 2, BLOSC_ZSTD, 4, 512));
  first.push_back((int)rows.size());
  rows.push_back(row(5, 1, BLOSC_BLOSCLZ, 8, 512));
  first.push_back((int)rows.size());
  for (int k = 0; k < 70; k++) rows.push_back(row(k % 10, 1 + k % 2, BLOSC_LZ4, 4, (size_t)128 << (k / 10 % 6)));
  first.push_back((int)rows.size());
  first.push_back((int)rows.size());
  rows.push_back(row(5, 1, BLOSC_SNAPPY, 4, 512)); rows.push_back(row(5, 7, BLOSC_LZ4, 4, 512));
  first.push_back((int)rows.size());
  const int E = (int)rows.size();
  const void* sp[N]; void* dp[N]; size_t cap[N];
  for (int i = 0; i < N; i++) { sp[i] = src[i].data(); dp[i] = dst[i].data(); cap[i] = SIZES[i] + 16; }

  auto winner = [&](const std::vector<int>& cand, int i) {
    int best = -1;
    for (int e = first[i]; e < first[i + 1]; e++) if (cand[e] > 0 && (best < 0 || cand[e] < cand[best])) best = e;
    return best;
  };
  // the batch form: exactly sized outputs (the sanitizer sees a write behind them)
  std::vector<int> res(N, -777), choice(N, -777), cand(E, -777);
  CHECK(blosc_gpu_compress_batch_select(N, first.data(), rows.data(), sp, SIZES, dp, cap, res.data(), choice.data(), cand.data(), nullptr) == 0);
  for (int i = 0; i < N; i++) {
    const int w = winner(cand, i);
    CHECK(choice[i] == (w < 0 ? -1 : w - first[i]));
    CHECK(res[i] == (first[i] == first[i + 1] ? -10 : cand[w < 0 ? first[i] : w]));
    if (w >= 0) { int32_t cb; memcpy(&cb, dst[i].data() + 12, 4); CHECK(cb == res[i]); }
    else CHECK(dst[i].empty() || (dst[i][0] == 0xEE && dst[i][dst[i].size() - 1] == 0xEE));
  }
  CHECK(cand[0] == -10 && cand[3] == -5 && res[3] == -10 && res[4] == -5 && choice[4] == -1);
  // without the candidate answers
  std::vector<int> res2(N, -777), choice2(N, -777);
  CHECK(blosc_gpu_compress_batch_select(N, first.data(), rows.data(), sp, SIZES, dp, cap, res2.data(), choice2.data(), nullptr, nullptr) == 0);
  CHECK(res2 == res && choice2 == choice);
  // the packed form: the sizing call, then a container of exactly that size
  std::vector<size_t> off(N + 1, 99), off2(N + 1, 99);
  std::vector<int> res3(N, -777), choice3(N, -777), cand3(E, -777);
  CHECK(blosc_gpu_compress_packed_select(N, first.data(), rows.data(), sp, SIZES, nullptr, 0, 16, off.data(), res3.data(), choice3.data(), cand3.data(), nullptr) == 0);
  CHECK(choice3 == choice && cand3 == cand && off[0] == 0 && off[4] == off[3] && off[5] == off[4]);
  std::vector<uint8_t> cont(off[N]);
  CHECK(blosc_gpu_compress_packed_select(N, first.data(), rows.data(), sp, SIZES, cont.data(), cont.size(), 16, off2.data(), res3.data(), choice3.data(), nullptr, nullptr) == 0);
  CHECK(off2 == off && res3 == res);
  for (int i = 0; i < N; i++) if (res[i] > 0) CHECK(memcmp(cont.data() + off[i], dst[i].data(), (size_t)res[i]) == 0);
  // every chunk without rows
  std::vector<int> none(N + 1, 0);
  CHECK(blosc_gpu_compress_packed_select(N, none.data(), rows.data(), sp, SIZES, nullptr, 0, 1, off2.data(), res3.data(), choice3.data(), nullptr, nullptr) == 0);
  CHECK(res3 == std::vector<int>(N, -10) && choice3 == std::vector<int>(N, -1) && off2 == std::vector<size_t>(N + 1, 0));
  // unusable tables: a negative answer, nothing written
  std::vector<int> falls(first); falls[2] = 0;
  std::vector<int> from_one(first); from_one[0] = 1;
  res3.assign(N, -777);
  CHECK(blosc_gpu_compress_batch_select(N, falls.data(), rows.data(), sp, SIZES, dp, cap, res3.data(), choice3.data(), nullptr, nullptr) < 0);
  CHECK(blosc_gpu_compress_batch_select(N, from_one.data(), rows.data(), sp, SIZES, dp, cap, res3.data(), choice3.data(), nullptr, nullptr) < 0);
  CHECK(blosc_gpu_compress_packed_select(N, first.data(), nullptr, sp, SIZES, nullptr, 0, 16, off2.data(), res3.data(), choice3.data(), nullptr, nullptr) < 0);
  CHECK(blosc_gpu_compress_packed_select(N, first.data(), rows.data(), sp, SIZES, nullptr, 0, 24, off2.data(), res3.data(), choice3.data(), nullptr, nullptr) < 0);
  CHECK(res3 == std::vector<int>(N, -777));
  blosc_destroy();
  printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed != 0;
}
