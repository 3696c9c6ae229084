"""The pure pieces of the Step-2 driver (regenie_amd/host/driver_step2.h, driver_step2_bgen.cpp), compiled with g++ into a small harness (no GPU involved):
  plan_groups          blocks -> the groups the BGEN read-ahead prepares, and the share of each group the device decodes;
  repack_analysed      the 2-bit codes of the analysed samples, four to a byte;
  below_min_mac        compute_mac's rule (Geno.cpp:3077-3108, autosomes);
  info_score           compute_aaf_info (Geno.cpp:3132-3141): IMPUTE info for .bgen, MaCH r2 for .pgen dosages.
Every expected value is worked out here in Python."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = r'''
#include "driver_step2.h"
using namespace rgdrv;
// blocks (chrom, j0, bs) -> per group: chrom, j0, rows, dev_rows, first block; per block: its group, its first row there; returns the number of groups
extern "C" int plan(const int32_t* chrom, const int64_t* j0, const int32_t* bs, int nb, int bsize, int target, double share, int has_device,
                    int32_t* g_chrom, int64_t* g_j0, int32_t* g_rows, int32_t* g_dev, int64_t* g_first, int64_t* b_group, int32_t* b_row) {
  std::vector<BlkRef> blocks;
  for (int b = 0; b < nb; ++b) blocks.push_back({chrom[b], nullptr, j0[b], bs[b]});
  const GroupPlan pl = plan_groups(blocks, bsize, target, share, has_device != 0);
  if (pl.block_group.size() != (size_t)nb) return -1;
  for (size_t g = 0; g < pl.groups.size(); ++g) {
    g_chrom[g] = pl.groups[g].ref.chrom; g_j0[g] = pl.groups[g].ref.j0; g_rows[g] = pl.groups[g].ref.bs; g_dev[g] = pl.groups[g].dev_rows; g_first[g] = (int64_t)pl.groups[g].first_block;
  }
  for (int b = 0; b < nb; ++b) { b_group[b] = (int64_t)pl.block_group[b].first; b_row[b] = pl.block_group[b].second; }
  return (int)pl.groups.size();
}
extern "C" int64_t repack(const uint8_t* rows, int64_t bpr, int bs, const int64_t* file_idx, int64_t n, int nthreads, uint8_t* out) {
  std::vector<uint8_t> packed;
  const int64_t ld = repack_analysed(rows, bpr, bs, file_idx, n, nthreads, packed);
  if ((int64_t)packed.size() != ld * bs) return -1;
  memcpy(out, packed.data(), packed.size());
  return ld;
}
extern "C" int below(double total, double ns, double min_mac) { return below_min_mac(total, ns, min_mac) ? 1 : 0; }
extern "C" double info(int bgen, double info_num, double ns, double af) { return info_score(bgen != 0, info_num, ns, af); }
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("s2plan")
    src = d / "h.cpp"
    src.write_text(HARNESS)
    so = d / "libs2plan.so"
    host = os.path.join(ROOT, "regenie_amd", "host")
    libdir = os.path.join(ROOT, "regenie_amd", "lib")
    if not os.path.exists(os.path.join(libdir, "librg_step1_hip.so")):
        import __graft_entry__ as g
        g.build()
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + host, os.path.join(host, "driver_step2_bgen.cpp"), str(src), "-o", str(so),
                        "-L" + libdir, "-lrg_step1_hip", "-Wl,-rpath," + libdir, "-lz", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lb = C.CDLL(str(so))
    lb.info.restype = C.c_double
    lb.info.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double]
    lb.below.argtypes = [C.c_double, C.c_double, C.c_double]
    lb.repack.restype = C.c_int64
    return lb


def _blocks(chrom_sizes, bsize):
    out = []
    for c, m in chrom_sizes:
        out += [(c, j0, min(bsize, m - j0)) for j0 in range(0, m, bsize)]
    return out


P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731


@pytest.mark.parametrize("has_device", [True, False])
@pytest.mark.parametrize("share", [0.0, 0.25, 0.5, 0.9])
@pytest.mark.parametrize("target", [100, 3072])
@pytest.mark.parametrize("chrom_sizes", [[(1, 280)], [(1, 120), (2, 57)]], ids=["one_chr_7_blocks", "two_chr_3_2_blocks_last_short"])
def test_group_planning(lib, chrom_sizes, target, share, has_device):
    """A group is a run of consecutive blocks of ONE chromosome.  With a device its limit is max(bsize, target) / (1 - share) variants (at
    most 65,536): the device's part of a group keeps the size `target`, what the host threads take comes on top.  It is filled greedily, so
    it is larger than the limit only when a single block is, and the device's rows end at the block boundary nearest to (1 - share) x size."""
    bsize = 40
    blocks = _blocks(chrom_sizes, bsize)
    assert [b[2] for b in blocks] == ([40] * 7 if len(chrom_sizes) == 1 else [40, 40, 40, 40, 17])
    nb = len(blocks)
    chrom = np.array([b[0] for b in blocks], np.int32); j0 = np.array([b[1] for b in blocks], np.int64); bs = np.array([b[2] for b in blocks], np.int32)
    g_chrom = np.zeros(nb, np.int32); g_j0 = np.zeros(nb, np.int64); g_rows = np.zeros(nb, np.int32); g_dev = np.zeros(nb, np.int32); g_first = np.zeros(nb, np.int64)
    b_group = np.zeros(nb, np.int64); b_row = np.zeros(nb, np.int32)
    ng = lib.plan(P(chrom), P(j0), P(bs), nb, bsize, target, C.c_double(share), int(has_device), P(g_chrom), P(g_j0), P(g_rows), P(g_dev), P(g_first), P(b_group), P(b_row))
    assert 1 <= ng <= nb
    limit = int(min(65536.0, max(bsize, target) / (1.0 - share))) if has_device else bsize
    # the groups cut the block list into consecutive runs, each inside one chromosome
    assert g_first[0] == 0 and (np.diff(g_first[:ng]) > 0).all()
    bounds = list(g_first[:ng]) + [nb]
    for g in range(ng):
        mine = blocks[bounds[g]:bounds[g + 1]]
        assert {b[0] for b in mine} == {g_chrom[g]}                                     # never spans two chromosomes
        assert g_j0[g] == mine[0][1] and g_rows[g] == sum(b[2] for b in mine)
        assert all(mine[k][1] + mine[k][2] == mine[k + 1][1] for k in range(len(mine) - 1))     # contiguous
        assert g_rows[g] <= limit or len(mine) == 1
        if bounds[g + 1] < nb and blocks[bounds[g + 1]][0] == g_chrom[g]:              # it ended because the next block did not fit
            assert g_rows[g] + blocks[bounds[g + 1]][2] > limit
        starts = np.cumsum([0] + [b[2] for b in mine])                                  # block boundaries, the group's end included
        for k in range(len(mine)):
            assert b_group[bounds[g] + k] == g and b_row[bounds[g] + k] == starts[k]
        if not has_device:
            assert len(mine) == 1 and g_dev[g] == 0                                     # one block per group, all of it on the host threads
        elif share == 0.0 or len(mine) == 1:
            assert g_dev[g] == g_rows[g]                                                # whole
        else:
            want = (1.0 - share) * g_rows[g]
            assert g_dev[g] in starts[1:] and g_dev[g] > 0
            assert abs(g_dev[g] - want) == min(abs(s - want) for s in starts[1:])
    if has_device and target == 3072:
        assert ng == len(chrom_sizes)                                                   # a chromosome of a few blocks is one group
    if has_device and target == 100 and share == 0.0:
        assert list(g_rows[:ng]) == ([80, 80, 80, 40] if len(chrom_sizes) == 1 else [80, 40, 57])


@pytest.mark.parametrize("n_file", [9, 64, 65, 257])
def test_repack_analysed(lib, n_file):
    """Every third sample dropped: sample k of the analysis is sample file_idx[k] of the file; its 2-bit code sits at bits 2 (i mod 4) of byte
    i // 4 of the row (a partial last byte, an exact word, a word plus one)."""
    rng = np.random.default_rng(n_file)
    bs, bpr = 3, (n_file + 3) // 4
    rows = rng.integers(0, 256, size=(bs, bpr), dtype=np.uint8)
    file_idx = np.array([i for i in range(n_file) if i % 3 != 2], np.int64)
    n = len(file_idx)
    ld = (n + 3) // 4
    want = np.zeros((bs, ld), np.uint8)
    for j in range(bs):
        for k in range(n):
            i = int(file_idx[k])
            code = (int(rows[j, i // 4]) >> (2 * (i % 4))) & 3
            want[j, k // 4] |= code << (2 * (k % 4))
    for nthreads in (1, 2):
        got = np.full((bs, ld), 0xAA, np.uint8)
        assert lib.repack(P(rows), C.c_int64(bpr), bs, P(file_idx), C.c_int64(n), nthreads, P(got)) == ld
        assert (got == want).all()


def test_below_min_mac_and_info_score(lib):
    rng = np.random.default_rng(11)
    ns = rng.integers(1, 5000, size=400).astype(np.float64)
    total = np.round(rng.random(400) * 2 * ns * 255) / 255
    total[:40] = np.round(total[:40])
    cases = list(zip(total, ns)) + [(0.0, 10.0), (20.0, 10.0), (5.0, 10.0), (15.0, 10.0), (4.999999, 10.0), (15.000001, 10.0)]
    for min_mac in (0.5, 5.0, 50.0):
        for t, m in cases:
            assert lib.below(t, m, min_mac) == int(min(t, 2.0 * m - t) < min_mac), (t, m, min_mac)
    assert lib.below(5.0, 10.0, 5.0) == 0 and lib.below(15.0, 10.0, 5.0) == 0          # a count that EQUALS --minMAC is kept
    af = total / (2.0 * ns)
    num = rng.random(400) * 2 * ns
    with np.errstate(divide="ignore", invalid="ignore"):
        impute = 1.0 - num / (2.0 * ns * af * (1.0 - af))
        mach = (num / ns - 4.0 * af * af) / (2.0 * af * (1.0 - af))
    for k in range(400):
        if af[k] in (0.0, 1.0):
            continue
        assert lib.info(1, num[k], ns[k], af[k]) == impute[k] and lib.info(0, num[k], ns[k], af[k]) == mach[k]
    assert (impute < 0).any()                                                            # very uncertain dosages: the IMPUTE score is negative, and printed as NA
    for bgen in (0, 1):
        assert lib.info(bgen, 3.0, 100.0, 0.0) == 1.0 and lib.info(bgen, 3.0, 100.0, 1.0) == 1.0      # a monomorphic variant
    assert lib.info(1, 30.0, 10.0, 0.25) == 1.0 - 30.0 / (2.0 * 10.0 * 0.25 * 0.75) < 0
