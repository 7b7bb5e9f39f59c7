// tests/tools/enc_lookahead_check.cpp — CPU check of the lead a block's shuffle task has over its streams in the encode queues
// (c-blosc_amd/csrc/queue_order.h: build_encode_queues, enc_lookahead()).  The kernel's waves sleep through whatever part of a shuffle
// task is not over when they draw one of its block's streams, so the lead is sized to the task (96 blocks, round 7) and must be the SAME
// for every block, with and without cost feedback: in an XCD's queue, the first stream of its k-th block has exactly
// min(k + 1 + lookahead, blocks of the XCD) shuffle entries in front of it (the queue opens with the first lookahead + 1 of them).
//   g++ -O1 -std=c++17 -I c-blosc_amd/csrc tests/tools/enc_lookahead_check.cpp -o /tmp/enc_lookahead_check && /tmp/enc_lookahead_check
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include "queue_order.h"

using namespace bamd;

static int fail(const char* what, int a, int b) { printf("FAIL: %s (%d, %d)\n", what, a, b); return 1; }

int main() {
  const int LA = (int)enc_lookahead();
  if (LA != 96) return fail("enc_lookahead() is not the 96 blocks the measurements of round 7 chose", LA, 96);
  for (int nblocks : {1, 7, 8, 9, 8 * LA - 1, 8 * LA, 8 * LA + 8, 8 * LA + 13, 8192}) {
    for (int feedback = 0; feedback < 2; feedback++) {
      const int T = 8;
      std::vector<ChunkDesc> chunks(1); memset(&chunks[0], 0, sizeof chunks[0]);
      chunks[0].typesize = T; chunks[0].mode = CH_SHUFFLE | CH_FUSED_SHUF;
      std::vector<BlockDesc> blocks((size_t)nblocks);
      for (int j = 0; j < nblocks; j++) { memset(&blocks[(size_t)j], 0, sizeof(BlockDesc)); blocks[(size_t)j].blk = j; blocks[(size_t)j].first_stream = j * T; blocks[(size_t)j].nstreams = T; }
      uint32_t cost[256] = {0};
      for (int k = 0; k < T; k++) cost[k] = 100;
      cost[1] = 4000; cost[5] = 3900;      // two expensive planes, as in the benchmark's data
      std::vector<int32_t> q; size_t sh_at = 0;
      build_encode_queues(blocks, chunks, cost, feedback != 0, q, 8, &sh_at);
      for (int x = 0; x < 8; x++) {
        const int mine = nblocks / 8 + (x < nblocks % 8 ? 1 : 0);      // blocks x, x + 8, ... belong to queue x
        int shuffles = 0, opening = -1;
        std::vector<int> before((size_t)std::max(mine, 1), -1);        // shuffle entries in front of the first stream of the XCD's k-th block
        for (int i = q[(size_t)x]; i < q[(size_t)x + 1]; i++) {
          const int32_t t = q[9 + (size_t)i];
          if (t < 0) { shuffles++; continue; }
          if (opening < 0) opening = shuffles;
          const int g = t / T;
          if (g % 8 != x) return fail("a stream on another XCD's queue", g, x);
          if (before[(size_t)(g / 8)] < 0) before[(size_t)(g / 8)] = shuffles;
        }
        if (shuffles != mine) return fail("shuffle entries of a queue", shuffles, mine);
        if (mine && opening != std::min(LA + 1, mine)) return fail("the queue does not open with the lookahead's shuffle tasks", opening, std::min(LA + 1, mine));
        for (int k = 0; k < mine; k++)
          if (before[(size_t)k] != std::min(k + 1 + LA, mine)) return fail("lead of a block's shuffle task", before[(size_t)k], std::min(k + 1 + LA, mine));
      }
    }
  }
  printf("enc_lookahead_check OK (lookahead %d blocks)\n", LA);
  return 0;
}
