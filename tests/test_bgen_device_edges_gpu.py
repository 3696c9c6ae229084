"""The device BGEN decoder (regenie_amd/csrc/bgen_inflate.hip) at its DEFLATE and kernel edges, on the hand-built streams of
tests/deflate_cases.py: what zlib's compressor never writes but an inflater must read (codes of 15 bits, distance 32,768, 258 as 284 + 31, a
one-code distance alphabet, empty stored blocks, repeats across the alphabet boundary), the emit_match regimes at their boundaries, blocks
below and at the 322 bytes where the window loop starts, every stream at the four byte alignments of its first byte, input that ends at a
256-byte chunk edge -- and the refusals, each built on purpose with the status traced from the code.  The arbiter of the bytes is zlib
(tests/test_deflate_cases_cpu.py pins the corpus against it without a GPU); the walk's rows and sums are held to tests/bgen_restate.py.
Then the walk and the Adler-32 kernels at their own edges, on streams from zlib level 6.  Bytes and integers: every comparison is exact."""
import zlib

import numpy as np
import pytest

from regenie_amd.bgen import BgenDevice
from tests import deflate_cases as dc
from tests.bgen_restate import check, expect

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    with BgenDevice(0) as d:
        yield d


def _by_n():
    out = {}
    for c in dc.valid_cases():
        out.setdefault(c.n, []).append(c)
    return out


def test_valid_corpus_at_four_alignments(dev):
    """One decode per sample count N: all its streams, each at off % 4 = 0, 1, 2, 3."""
    ran = 0
    for n, cs in sorted(_by_n().items()):
        comp, off, clen, which = dc.lay_out([c.stream for c in cs])
        assert set((off % 4).tolist()) == {0, 1, 2, 3}
        ulen = np.full(off.size, 10 + 3 * n, dtype=np.int32)
        blocks = np.stack([np.frombuffer(zlib.decompress(cs[i].stream), dtype=np.uint8) for i in which])
        dev.set_samples(n)
        res = dev.decode(comp, off, clen, ulen, fetch_raw=True)
        names = [(cs[i].name, int(o % 4)) for i, o in zip(which, off)]
        assert (res["status"] == 0).all(), [(nm, int(s)) for nm, s in zip(names, res["status"]) if s]
        wrong = [nm for k, nm in enumerate(names) if not np.array_equal(res["raw"][k, :10 + 3 * n], blocks[k])]
        assert not wrong, wrong
        check(res, expect(blocks, n, None, False))
        ran += off.size
    assert ran == 4 * len(dc.valid_cases())


def test_malformed_corpus_between_good_neighbours(dev):
    """Every refusal once, in one batch per N, a known-good stream before, between and after: each malformed stream gets the status its `why`
    traces, the neighbours their bytes and sums."""
    by_name = {c.name: c for c in dc.valid_cases()}
    seen = 0
    for n, goods in ((200, ("hdist1_zero_length_window", "repeat16_across_boundary_window")), (50, ("hdist1_zero_length_serial", "code15_serial_n50"))):
        bad = [c for c in dc.malformed_cases() if c.n == n]
        goods = [by_name[g] for g in goods]
        assert all(g.n == n for g in goods)
        order = []
        for k, c in enumerate(bad):
            if k % 4 == 0:
                order.append(goods[(k // 4) % 2])
            order.append(c)
        order.append(goods[1])
        comp, off, clen, which = dc.lay_out([c.stream for c in order], aligns=(1,), pad=0)      # zeros behind every stream: what `why` assumes
        ulen = np.array([c.ulen for c in order], dtype=np.int32)
        dev.set_samples(n)
        res = dev.decode(comp, off, clen, ulen, fetch_raw=True)
        got = {c.name: int(s) for c, s in zip(order, res["status"]) if c.payload is None}
        assert got == {c.name: dc.expected_status(c) for c in bad}
        keep = np.array([c.payload is not None for c in order])
        assert keep.sum() >= 2
        blocks = np.stack([np.frombuffer(c.payload, dtype=np.uint8) for c in order if c.payload is not None])
        assert (res["status"][keep] == 0).all()
        assert np.array_equal(res["raw"][keep, :10 + 3 * n], blocks)
        want = expect(blocks, n, None, False)
        for k in ("g16", "sum_q", "sum_info", "n_obs", "max_q"):
            assert np.array_equal(res[k][keep], want[k]), k
        seen += len(bad)
    assert seen == len(dc.malformed_cases())


def _zlib_batch(rng, m, n, miss_rate=0.05, ff=False):
    """m blocks of n samples as zlib level-6 streams: (comp, off, clen, ulen, blocks)."""
    blocks, streams = [], []
    for _ in range(m):
        pl = np.where(rng.random(n) < miss_rate, 0x82, 0x02).astype(np.uint8)
        pr = np.full(2 * n, 0xFF, dtype=np.uint8) if ff else rng.integers(0, 256, 2 * n).astype(np.uint8)
        blk = int(n).to_bytes(4, "little") + bytes([2, 0, 2, 2]) + pl.tobytes() + bytes([0, 8]) + pr.tobytes()
        blocks.append(np.frombuffer(blk, dtype=np.uint8))
        streams.append(zlib.compress(blk, 6))
    comp, off, clen, _ = dc.lay_out(streams, aligns=(0,))
    return comp, off, clen, np.full(m, 10 + 3 * n, dtype=np.int32), np.stack(blocks)


@pytest.mark.parametrize("n", [1, 3, 1023, 1024, 1025])
def test_walk_grid_edges(dev, n):
    """n at the walk's grid edge (1,024 samples per workgroup) and at the padding of ld16 = ceil(n / 8) * 8, both allele orders."""
    comp, off, clen, ulen, blocks = _zlib_batch(np.random.default_rng(n), 5, n)
    dev.set_samples(n)
    for ref_first in (False, True):
        check(dev.decode(comp, off, clen, ulen, ref_first=ref_first), expect(blocks, n, None, ref_first))


@pytest.mark.parametrize("P", [1, 64, 65, 130])
def test_walk_trait_masks(dev, P):
    """P traits with masks (W = 1, 2, 3 words per sample), ~10 % missing, over a file_idx with repeats and out of order: traits 0, 63, 64 and
    129 (where they exist) each miss at least one observed sample."""
    rng = np.random.default_rng(100 + P)
    n_file, n = 1100, 1025
    comp, off, clen, ulen, blocks = _zlib_batch(rng, 4, n_file)
    fi = rng.integers(0, n_file, n)
    fi[:3] = fi[3]                                        # a sample four times over
    assert np.unique(fi).size < n and (np.diff(fi) < 0).any()
    mask = (rng.random((P, n)) > 0.1).astype(np.uint8)
    observed = (blocks[:, 8:8 + n_file][:, fi] & 0x80) == 0
    for p in {0, 63, 64, 129} & set(range(P)):
        assert ((mask[p] == 0) & observed).any(axis=1).all()
    dev.set_samples(n_file, file_idx=fi, mask=mask)
    for ref_first in (False, True):
        check(dev.decode(comp, off, clen, ulen, ref_first=ref_first), expect(blocks, n_file, fi, ref_first, mask))


@pytest.mark.parametrize("coding", [0, 1, 2])
def test_walk_coded_rows_at_1025(dev, coding):
    rng = np.random.default_rng(7)
    n = 1025
    comp, off, clen, ulen, blocks = _zlib_batch(rng, 4, n)
    mask = (rng.random((3, n)) > 0.1).astype(np.uint8)
    dev.set_samples(n, mask=mask)
    dev.set_coding(coding)
    try:
        for ref_first in (False, True):
            check(dev.decode(comp, off, clen, ulen, ref_first=ref_first), expect(blocks, n, None, ref_first, mask, coding))
    finally:
        dev.set_coding(0)


def test_adler_edges(dev):
    """Payloads of all 0xFF at 20,000 samples (the modular reduction on the largest sums, max_q = 765), a block of 13 bytes (one 16-byte piece,
    15 empty segments) and a ulen of 16 k + 1; a wrong trailer on each is ST_ADLER."""
    for n, ff in ((20000, True), (1, False), (1, True), (13, True), (2, True)):
        assert n != 13 or (10 + 3 * n) % 16 == 1
        comp, off, clen, ulen, blocks = _zlib_batch(np.random.default_rng(n), 3, n, miss_rate=0.0 if ff else 0.05, ff=ff)
        dev.set_samples(n)
        res = dev.decode(comp, off, clen, ulen, fetch_raw=True)
        assert np.array_equal(res["raw"][:, :10 + 3 * n], blocks)
        check(res, expect(blocks, n, None, False))
        if ff:
            assert (res["max_q"] == 765).all()
        c2 = comp.copy()
        c2[off[1] + clen[1] - 1] ^= 0x01                  # the Adler-32 trailer's last byte
        res = dev.decode(c2, off, clen, ulen)
        assert res["status"].tolist() == [0, dc.ST_ADLER, 0]
