// Stand-alone check of regenie_amd/csrc/l1_stage.h (the level-1 staging area: shape tables, ridge values, results) on the host, built with
// -fsanitize=address,undefined by tests/test_l1_stage_cpu.py.  The allocators are malloc / free with guard-free exact sizes, so a write past
// any section of the area, a use of a released area or a leak of one fails the run.
#include <stdio.h>
#include <stdlib.h>
#include <set>
#include "../../regenie_amd/csrc/l1_stage.h"

static int n_host = 0, n_dev = 0, fail_after = -1;
static void* h_alloc(size_t b) { if (fail_after == 0) return nullptr; if (fail_after > 0) --fail_after; ++n_host; return malloc(b); }
static void h_free(void* p) { --n_host; free(p); }
static void* d_alloc(size_t b) { if (fail_after == 0) return nullptr; if (fail_after > 0) --fail_after; ++n_dev; return malloc(b); }
static void d_free(void* p) { --n_dev; free(p); }

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static int check_tables(const L1Stage& s, int n64, int K, int nslice, int world, int rank, const std::vector<int32_t>& cols,
                        const std::vector<int32_t>& chrom) {
  // every macro tile (mr >= mc) of every (fold, slice) that belongs to this rank exactly once; the rest padding (fold = -1)
  const int T2 = (n64 + 127) / 128;
  std::set<long> seen;
  const L1Item* it = s.h<L1Item>(s.off_items);
  CHECK(s.n_items % 8 == 0);
  for (size_t i = 0; i < s.n_items; ++i) {
    if (it[i].fold < 0) continue;
    CHECK(it[i].fold < K && it[i].slice >= 0 && it[i].slice < nslice && it[i].mr < T2 && it[i].mc >= 0 && it[i].mc <= it[i].mr);
    CHECK((it[i].mr * (it[i].mr + 1) / 2 + it[i].mc) % world == rank);
    const long key = (((long)it[i].fold * nslice + it[i].slice) * T2 + it[i].mr) * T2 + it[i].mc;
    CHECK(seen.insert(key).second);
  }
  long want = 0;
  for (int mr = 0; mr < T2; ++mr)
    for (int mc = 0; mc <= mr; ++mc) want += ((mr * (mr + 1) / 2 + mc) % world == rank);
  CHECK((long)seen.size() == want * K * nslice);
  const int32_t* col0 = s.h<int32_t>(s.off_col0);
  int32_t run = 0;
  for (size_t c = 0; c < cols.size(); ++c) { CHECK(col0[c] == run); run += cols[c]; }
  CHECK(col0[cols.size()] == run);
  for (size_t c = 0; c < chrom.size(); ++c) CHECK(s.h<int32_t>(s.off_chrom)[c] == chrom[c]);
  // the sections do not overlap and lie inside the area
  CHECK(s.off_items + sizeof(L1Item) * s.n_items <= s.off_col0);
  CHECK(s.off_col0 + sizeof(int32_t) * (cols.size() + 1) <= s.off_chrom);
  CHECK(s.off_chrom + sizeof(int32_t) * chrom.size() <= s.table_bytes && s.table_bytes == s.off_tau);
  CHECK(s.off_tau + sizeof(double) * s.P * s.R1 <= s.off_res);
  CHECK(s.off_res + sizeof(L1Res) * s.P <= s.total && s.total <= s.capacity);
  return 0;
}

int main() {
  const L1StageAlloc a{h_alloc, h_free, d_alloc, d_free};
  L1Stage s;
  int up = 0;
  // the flagship's shape: order 576, 5 folds, 22 chromosomes of 23, one trait
  std::vector<int32_t> cols = {40, 40, 35, 30, 30, 30, 25, 25, 20, 20, 25, 20, 20, 15, 15, 15, 15, 15, 10, 10, 10, 80};
  std::vector<int32_t> chrom(cols.size());
  for (size_t c = 0; c < chrom.size(); ++c) chrom[c] = (int32_t)c + 1;
  CHECK(l1_stage_prepare(s, a, 576, 5, 16, 1, 0, (int)cols.size(), cols.data(), (int)chrom.size(), chrom.data(), 1, 5, &up) == 0 && up == 1);
  CHECK(check_tables(s, 576, 5, 16, 1, 0, cols, chrom) == 0);
  // every byte of the tau and result sections is writable (what a call does); the device image has the same size
  for (size_t b = s.off_tau; b < s.total; ++b) { s.host[b] = 1; s.dev[b] = 2; }
  for (size_t b = 0; b < s.table_bytes; ++b) s.dev[b] = s.host[b];
  const uint8_t* h0 = s.host;
  // the same shape again: nothing rebuilt, nothing uploaded, same memory
  CHECK(l1_stage_prepare(s, a, 576, 5, 16, 1, 0, (int)cols.size(), cols.data(), (int)chrom.size(), chrom.data(), 1, 5, &up) == 0 && up == 0);
  CHECK(s.host == h0 && n_host == 1 && n_dev == 1);
  CHECK(check_tables(s, 576, 5, 16, 1, 0, cols, chrom) == 0);
  // another chromosome layout of the same size: rebuilt in place
  std::swap(cols[0], cols[21]);
  CHECK(l1_stage_prepare(s, a, 576, 5, 16, 1, 0, (int)cols.size(), cols.data(), (int)chrom.size(), chrom.data(), 1, 5, &up) == 0 && up == 1);
  CHECK(s.host == h0 && check_tables(s, 576, 5, 16, 1, 0, cols, chrom) == 0);
  // no LOCO ids, three traits, eight ridge values, rank 1 of 3, a larger order: the area grows, the old one is freed
  CHECK(l1_stage_prepare(s, a, 2624, 7, 3, 3, 1, (int)cols.size(), cols.data(), 0, nullptr, 3, 8, &up) == 0 && up == 1);
  CHECK(n_host == 1 && n_dev == 1 && check_tables(s, 2624, 7, 3, 3, 1, cols, {}) == 0);
  for (size_t b = s.off_tau; b < s.total; ++b) s.host[b] = 3;
  // back to a small one: no reallocation
  const size_t cap = s.capacity;
  std::vector<int32_t> one = {5};
  CHECK(l1_stage_prepare(s, a, 64, 2, 1, 1, 0, 1, one.data(), 1, one.data(), 1, 1, &up) == 0 && up == 1 && s.capacity == cap);
  CHECK(check_tables(s, 64, 2, 1, 1, 0, one, one) == 0);
  // allocation failure while growing (host, then device): an error, nothing leaked, the stage usable again afterwards
  for (int k = 0; k < 2; ++k) {
    fail_after = k;
    CHECK(l1_stage_prepare(s, a, 8192, 5, 1, 1, 0, (int)cols.size(), cols.data(), 0, nullptr, 2, 5, &up) == -1);
    fail_after = -1;
    CHECK(n_host == 0 && n_dev == 0 && s.host == nullptr && s.capacity == 0);
    CHECK(l1_stage_prepare(s, a, 576, 5, 16, 1, 0, (int)cols.size(), cols.data(), 0, nullptr, 1, 5, &up) == 0 && up == 1);
  }
  l1_stage_release(s, a);
  CHECK(n_host == 0 && n_dev == 0 && s.host == nullptr && s.dev == nullptr);
  l1_stage_release(s, a);      // releasing an empty stage is a no-op
  printf("l1_stage ok\n");
  return 0;
}
