// Host-side staging of the K-fold level 1 (l1.hip): the tables that depend only on the problem's shape, the ridge values of a
// call and the small results that come back from it, in ONE page-locked host area with ONE device image, owned by the context.
//
//   tables  | work items of k_l1_gram128 | first column of every chromosome (+ the total) | chromosome id of every cols_per_chr entry |
//   inputs  | ridge values tau [P][R1] |
//   results | L1Res [P] |                                    (device -> host, one copy per phenotype, read after the call's single wait)
//
// The tables are rebuilt (and uploaded again by the caller) only when their key changes: padded order, folds, K slices, rank / world,
// the columns per chromosome and the LOCO chromosome ids.  Between rg_set_problem calls a driver runs level 1 once per trait on the
// same shape, so every call after the first uploads the ridge values alone.  Page-locked memory makes those copies truly asynchronous:
// no stream wait is needed to keep the source alive, the area outlives the call.
//
// Plain C++ (no HIP): the allocators are passed in, so that tests/hipcpu/l1_stage_host.cpp runs this file under AddressSanitizer.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <algorithm>
#include <vector>

#define L1_R1MAX 8                       // ridge values of level 1 (rg_l1_qt: n_ridge_l1 in [1, 8])
#define L1_NPART (L1_R1MAX * 3 + 2)      // sums a chunk of positions contributes: (Sx, Sx2, Sxy) per ridge value, Sy, Sy2

struct L1Item { int16_t mr, mc, fold, slice; };

// what one phenotype's level 1 hands back: the chunk sums reduced in chunk order, the selected ridge index, the "not SPD" flag
struct L1Res {
  double tot[L1_NPART];
  int32_t best, info;
};

// Work table of k_l1_gram128 for one rank (see the kernel): macro tiles (mr >= mc) of the padded order n64, K folds, nslice K
// slices.  Groups = the macro tiles of one 4 x 4 super tile of one (fold, slice); the groups are dealt to the eight XCDs and
// workgroup id 8 j + x is the j-th item of XCD x's list (ids are dispatched to XCD id mod 8).  Lists are padded with fold = -1.
static inline std::vector<L1Item> l1_build_items(int n64, int K, int nslice, int world, int rank) {
  const int T2 = (n64 + 127) / 128, S = 4, TS = (T2 + S - 1) / S;
  std::vector<std::vector<L1Item>> xl(8);
  int gi = 0;
  for (int f = 0; f < K; ++f)
    for (int sl = 0; sl < nslice; ++sl)
      for (int Mr = 0; Mr < TS; ++Mr)
        for (int Mc = 0; Mc <= Mr; ++Mc) {
          std::vector<L1Item>& dst = xl[gi % 8];
          bool any = false;
          for (int mr = Mr * S; mr < std::min(T2, (Mr + 1) * S); ++mr)
            for (int mc = Mc * S; mc < std::min(T2, (Mc + 1) * S); ++mc) {
              if (mc > mr) continue;
              if ((mr * (mr + 1) / 2 + mc) % world != rank) continue;
              dst.push_back(L1Item{(int16_t)mr, (int16_t)mc, (int16_t)f, (int16_t)sl});
              any = true;
            }
          if (any) ++gi;
        }
  size_t mx = 0;
  for (auto& v : xl) mx = std::max(mx, v.size());
  std::vector<L1Item> items(mx * 8, L1Item{0, 0, -1, 0});
  for (int x = 0; x < 8; ++x)
    for (size_t j = 0; j < xl[x].size(); ++j) items[8 * j + x] = xl[x][j];
  return items;
}

struct L1StageAlloc {
  void* (*host_alloc)(size_t bytes);     // page-locked host memory (nullptr on failure)
  void (*host_free)(void* p);
  void* (*dev_alloc)(size_t bytes);      // device memory (nullptr on failure)
  void (*dev_free)(void* p);
};

struct L1Stage {
  // key of the tables
  int n64 = 0, K = 0, nslice = 0, world = 0, rank = 0, P = 0, R1 = 0;
  std::vector<int32_t> cols, chrom;
  // the area: byte offsets are the same on the host and on the device
  uint8_t* host = nullptr;
  uint8_t* dev = nullptr;
  size_t capacity = 0;                   // bytes allocated on each side (grows only)
  size_t n_items = 0, off_items = 0, off_col0 = 0, off_chrom = 0, off_tau = 0, off_res = 0, table_bytes = 0, total = 0;

  template <class T> T* h(size_t off) const { return reinterpret_cast<T*>(host + off); }
  template <class T> T* d(size_t off) const { return reinterpret_cast<T*>(dev + off); }
};

static inline size_t l1_stage_align(size_t x) { return (x + 63) / 64 * 64; }

static inline void l1_stage_release(L1Stage& s, const L1StageAlloc& a) {
  if (s.host) a.host_free(s.host);
  if (s.dev) a.dev_free(s.dev);
  s = L1Stage();
}

// Makes the area hold the tables of this shape.  Returns 0, or -1 when memory could not be had (the area is then released).
// *upload = 1: the tables were (re)built and bytes [0, table_bytes) of the host side must be copied to the device side.
// The caller must not have copies from or to the area in flight (every level-1 call ends with a stream wait).
static inline int l1_stage_prepare(L1Stage& s, const L1StageAlloc& a, int n64, int K, int nslice, int world, int rank, int nchr,
                                   const int32_t* cols_per_chr, int nloco, const int32_t* loco_chrom, int P, int R1, int* upload) {
  *upload = 0;
  const bool same = s.host && s.n64 == n64 && s.K == K && s.nslice == nslice && s.world == world && s.rank == rank && s.P == P &&
                    s.R1 == R1 && (int)s.cols.size() == nchr && std::equal(s.cols.begin(), s.cols.end(), cols_per_chr) &&
                    (int)s.chrom.size() == nloco && std::equal(s.chrom.begin(), s.chrom.end(), loco_chrom);
  if (same) return 0;
  const std::vector<L1Item> items = l1_build_items(n64, K, nslice, world, rank);
  size_t off = 0;
  const size_t off_items = off;  off = l1_stage_align(off + sizeof(L1Item) * items.size());
  const size_t off_col0 = off;   off = l1_stage_align(off + sizeof(int32_t) * ((size_t)nchr + 1));
  const size_t off_chrom = off;  off = l1_stage_align(off + sizeof(int32_t) * (size_t)std::max(1, nloco));
  const size_t table_bytes = off;
  const size_t off_tau = off;    off = l1_stage_align(off + sizeof(double) * (size_t)P * R1);
  const size_t off_res = off;    off = l1_stage_align(off + sizeof(L1Res) * (size_t)P);
  if (off > s.capacity) {
    uint8_t* nh = (uint8_t*)a.host_alloc(off);
    uint8_t* nd = nh ? (uint8_t*)a.dev_alloc(off) : nullptr;
    if (!nh || !nd) {
      if (nh) a.host_free(nh);
      l1_stage_release(s, a);
      return -1;
    }
    if (s.host) a.host_free(s.host);
    if (s.dev) a.dev_free(s.dev);
    s.host = nh; s.dev = nd; s.capacity = off;
  }
  s.n64 = n64; s.K = K; s.nslice = nslice; s.world = world; s.rank = rank; s.P = P; s.R1 = R1;
  s.cols.assign(cols_per_chr, cols_per_chr + nchr);
  s.chrom.assign(loco_chrom, loco_chrom + nloco);
  s.n_items = items.size(); s.off_items = off_items; s.off_col0 = off_col0; s.off_chrom = off_chrom; s.off_tau = off_tau;
  s.off_res = off_res; s.table_bytes = table_bytes; s.total = off;
  memset(s.host, 0, s.total);
  if (!items.empty()) memcpy(s.h<L1Item>(off_items), items.data(), sizeof(L1Item) * items.size());
  int32_t* col0 = s.h<int32_t>(off_col0);
  col0[0] = 0;
  for (int c = 0; c < nchr; ++c) col0[c + 1] = col0[c] + cols_per_chr[c];
  if (nloco > 0) memcpy(s.h<int32_t>(off_chrom), loco_chrom, sizeof(int32_t) * (size_t)nloco);
  *upload = 1;
  return 0;
}
