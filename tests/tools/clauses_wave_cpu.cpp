// tests/tools/clauses_wave_cpu.cpp — where_terms_test (c-blosc_amd/csrc/row_prims.h), the per-row evaluation of a term list, on its own on
// the wavefront emulator: the SAME source k_where_mark_terms and k_aggregate_tiles_terms run.  TEST INFRASTRUCTURE ONLY
// (tests/test_wave_emu_clauses.py builds it).
//   /opt/rocm/lib/llvm/bin/clang++ -std=c++17 -O1 -shared -fPIC -w -I tests/tools/wave_emu -I c-blosc_amd/csrc -x c++ \
//       tests/tools/clauses_wave_cpu.cpp -o tests/tools/libclauses_wave_cpu.so
#define WAVE_EMU_IMPLEMENTATION
#include <hip/hip_runtime.h>
#include "dev_types.h"
#include "row_prims.h"

namespace {
struct Job { const bamd::WhereTerms* q; const uint8_t* rows; uint32_t row_bytes, nrows; uint8_t* pass; uint64_t* v0; };
// lane l takes rows l, l + 64, ...; like the kernels, a lane without a row sits out and the ballot is taken by all
void body(int lane, void* arg) {
  Job* j = (Job*)arg;
  using namespace bamd;
  for (uint32_t r0 = 0; r0 < j->nrows; r0 += 64u) {
    const uint32_t r = r0 + (uint32_t)lane;
    bool hit = false;
    uint64_t v[WH_MAX_FIELDS] = {};
    if (r < j->nrows) hit = where_terms_test(j->q, (const gu8*)(j->rows + (size_t)r * j->row_bytes), v);
    const uint64_t m = __ballot(hit);
    if (r < j->nrows) { j->pass[r] = (uint8_t)((m >> lane) & 1ull); j->v0[r] = v[0]; }
  }
}
}  // namespace

extern "C" unsigned emu_terms_sizeof() { return (unsigned)sizeof(bamd::WhereTerms); }
// pass_out[r] = the list lets row r through; v0_out[r] = what it loaded for field 0
extern "C" void emu_terms_test(const void* terms, const uint8_t* rows, unsigned row_bytes, unsigned nrows, uint8_t* pass_out, uint64_t* v0_out) {
  Job j = {(const bamd::WhereTerms*)terms, rows, row_bytes, nrows, pass_out, v0_out};
  wave_emu::run(body, &j);
}
