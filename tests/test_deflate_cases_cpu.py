"""Pins the hand-built DEFLATE corpus of tests/deflate_cases.py without a GPU: zlib accepts every valid stream and returns the intended bytes,
refuses every malformed one, and the corpus holds, by name, each construct the device decoder's tests rely on (computed from the token lists and
code lengths of the cases, not from any decoder).  The valid corpus also goes through the host reader (inflate_fast.h, then zlib) as BGEN files."""
import struct
import zlib

import numpy as np
import pytest

from tests import deflate_cases as dc


def test_valid_streams_are_what_zlib_inflates():
    for c in dc.valid_cases():
        assert zlib.decompress(c.stream) == c.payload == dc.apply(dc.block_tokens(c.blocks)), c.name
        assert len(c.payload) == c.ulen == 10 + 3 * c.n and dc.is_bgen_block(c.payload, c.n), c.name
        assert c.ulen <= 70 * 1024 and c.stream[:2] == b"\x78\x01", c.name
        assert "hip:" in c.why, c.name


def test_malformed_streams_are_refused_by_zlib():
    for c in dc.malformed_cases():
        try:
            out = zlib.decompress(c.stream)
        except zlib.error:
            continue
        assert len(out) != c.ulen, c.name              # a sound stream, of another length than the file states
    for c in dc.malformed_cases():
        assert dc.expected_status(c) in range(1, 12) and "hip:" in c.why, c.name


def _dyn_blocks():
    return [(c, b) for c in dc.valid_cases() for b in c.blocks if b["kind"] == "dyn"]


def _used(blk):
    """(lit/len symbols, distance symbols) a Huffman block's tokens use, the end-of-block symbol included."""
    lits, dists = {256}, set()
    for t in blk["tokens"]:
        if isinstance(t, int):
            lits.add(t)
        else:
            lits.add(257 + dc.len_symbol(t[0], blk.get("long258", False))[0])
            dists.add(dc.dist_symbol(t[1])[0])
    return lits, dists


def test_corpus_covers_the_deflate_constructs():
    valid = dc.valid_cases()
    matches = {t for c in valid for t in dc.block_tokens(c.blocks) if not isinstance(t, int)}
    cover = {}
    dyn = _dyn_blocks()
    cover["lit/len code of 15 bits in use"] = any(b["lit_lens"][s] == 15 for _, b in dyn for s in _used(b)[0])
    cover["distance code of 15 bits in use"] = any(b["dist_lens"][s] == 15 for _, b in dyn for s in _used(b)[1])
    cover["lit/len codes of every length 11..15 in one block (second-level tables of 1 to 5 bits)"] = any(
        set(range(11, 16)) <= set(b["lit_lens"]) for _, b in dyn)
    cover["distance codes of every length 10..15 in one block (second-level tables of 1 to 6 bits)"] = any(
        set(range(10, 16)) <= set(b["dist_lens"]) for _, b in dyn)
    cover["distance 32768"] = any(d == 32768 for _, d in matches)
    for d in dc.REGIME_DISTS:
        cover["match (258, %d)" % d] = (258, d) in matches
    for m in ((64, 64), (65, 65), (3, 4032), (258, 4032), (3, 4033), (258, 4033)):
        cover["match %r" % (m,)] = m in matches
    for k in range(29):
        cover["length symbol %d" % (257 + k)] = any(dc.len_symbol(l)[0] == k for l, _ in matches)
    for k in range(30):
        cover["distance symbol %d" % k] = any(dc.dist_symbol(d)[0] == k for _, d in matches)
    cover["258 as symbol 284 + 31, fixed"] = any(b["kind"] == "fixed" and b.get("long258") and (258 in [t[0] for t in b["tokens"] if not isinstance(t, int)])
                                                 for c in valid for b in c.blocks)
    cover["258 as symbol 284 + 31, dynamic"] = any(b.get("long258") and (258 in [t[0] for t in b["tokens"] if not isinstance(t, int)]) for _, b in dyn)
    cover["distance alphabet of one 1-bit code, used"] = any(b["dist_lens"] == [1] and _used(b)[1] == {0} for _, b in dyn)
    cover["HDIST = 1 with a zero length"] = any(b["dist_lens"] == [0] and len(b["tokens"]) > 100 for _, b in dyn)
    cover["fixed block of the end-of-block symbol alone"] = any(b["kind"] == "fixed" and not b["tokens"] for c in valid for b in c.blocks)
    cover["dynamic block of the end-of-block symbol alone"] = any(not b["tokens"] for _, b in dyn)
    kinds = [[b["kind"] + ("0" if b["kind"] == "stored" and not b["data"] else "") for b in c.blocks] for c in valid]
    cover["empty stored block between Huffman blocks"] = any(
        any(k[i] == "stored0" and k[i - 1] in ("fixed", "dyn") and {"fixed", "dyn"} & set(k[i + 1:]) for i in range(1, len(k))) for k in kinds)
    cover["final stored block after a Huffman block"] = any(k[-1] == "stored" and {"fixed", "dyn"} & set(k[:-1]) for k in kinds)
    for sym in (16, 17):
        cover["repeat code %d across the literal / distance boundary" % sym] = any(
            it[0] == sym and it[3] < len(b["lit_lens"]) < it[3] + it[4]
            for _, b in dyn for it in dc.cl_rle(b["lit_lens"] + b["dist_lens"], len(b["lit_lens"]), b.get("rle", "split")))
    cover["HLIT = 286 and HDIST = 30, every length non-zero"] = any(len(b["lit_lens"]) == 286 and len(b["dist_lens"]) == 30 and all(b["lit_lens"])
                                                                   and all(b["dist_lens"]) for _, b in dyn)
    cover["every length 5..15 in each of the five ballot chunks of 64 symbols"] = any(
        all(set(range(5, 16)) <= set(b["lit_lens"][ch * 64:ch * 64 + 64]) for ch in range(5)) for _, b in dyn)
    names = {c.name for c in valid}
    for n in (1, 2, 5, 103, 104, 105):
        for kind in ("fixed", "dyn", "stored"):
            cover["N = %d as a %s stream" % (n, kind)] = "size_n%d_%s" % (n, kind) in names
    sizes = {c.ulen for c in valid}
    for u in (13, 16, 49, 319, 322, 325, 2044, 2047, 2050, 4093, 4096, 4099):
        cover["ulen %d" % u] = u in sizes
    clens = {len(c.stream) for c in valid}
    for cl in (255, 256, 257, 511, 512, 513):
        cover["stream of %d bytes" % cl] = cl in clens
    cover["far match right after a ring flush and as its trigger"] = "far_match_at_flush_fixed" in names and "far_match_at_flush_dyn" in names
    cover["distance 4096 right after an end-of-block"] = any(
        len(c.blocks) > 1 and c.blocks[1]["tokens"][:1] == [(3, 4096)] for c in valid if c.blocks[0]["kind"] == "fixed")
    missing = [k for k, v in cover.items() if not v]
    assert not missing, missing


def test_corpus_covers_the_refusals():
    bad = {c.name: dc.expected_status(c) for c in dc.malformed_cases()}
    want = {"lit_code_oversubscribed": 4, "dist_code_oversubscribed": 4, "codelength_code_oversubscribed": 4, "lit_code_incomplete": 4,
            "dist_code_incomplete_two_codes": 4, "codelength_code_incomplete": 4, "btype_3": 2, "stored_nlen_mismatch": 3, "repeat16_first": 4,
            "no_end_of_block_code": 4, "repeat_past_hlit_hdist": 4, "stored_overrun": 7, "literal_after_258_to_cap": 7}
    for stem, st in (("fixed_symbol_286", 5), ("fixed_symbol_287", 5), ("fixed_distance_code_30", 5), ("fixed_distance_code_31", 5),
                     ("distance_before_start_first_symbol", 6), ("distance_before_start_by_one", 6), ("one_byte_more_by_literal", 7),
                     ("one_byte_more_by_match", 7), ("one_byte_fewer", 8), ("input_ends_inside_block", 9)):
        want[stem + "_window"] = want[stem + "_serial"] = st
    for k, st in want.items():
        assert bad.get(k) == st, k
    for c in dc.malformed_cases():                       # `_window` means the damage lies where the window loop decodes, `_serial` below 322 bytes
        if c.name.endswith("_window"):
            assert c.ulen >= 322, c.name
        if c.name.endswith("_serial"):
            assert c.ulen < 322, c.name


def test_lay_out_places_every_stream_at_the_four_alignments():
    streams = [c.stream for c in dc.valid_cases()[:7]]
    comp, off, clen, which = dc.lay_out(streams)
    assert sorted(zip(which.tolist(), (off % 4).tolist())) == [(i, a) for i in range(7) for a in range(4)]
    for o, l, i in zip(off, clen, which):
        assert comp[o:o + l].tobytes() == streams[i]
    assert (np.diff(off) >= clen[:-1] + 4).all()


def _write_bgen(path, n, cases):
    """BGEN v1.2, layout 2, zlib: one variant per case, its stream stored as it is."""
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", 20))
        fh.write(struct.pack("<IIII", 20, len(cases), n, 0x6e656762))
        fh.write(struct.pack("<I", 1 | (2 << 2)))
        for j, c in enumerate(cases):
            rs = ("rs%d" % j).encode()
            fh.write(struct.pack("<H", 0) + struct.pack("<H", len(rs)) + rs + struct.pack("<H", 1) + b"1" + struct.pack("<IH", 100 + j, 2))
            fh.write(struct.pack("<I", 1) + b"A" + struct.pack("<I", 1) + b"G")
            fh.write(struct.pack("<II", len(c.stream) + 4, c.ulen) + c.stream)


def test_valid_corpus_through_the_host_reader(tmp_path):
    """The host route (bgen_reader.h: inflate_fast.h first, zlib behind it) returns every payload byte for byte, and hands the stored streams
    over unchanged (rg_bgen_read_compressed: what the device path is given)."""
    from regenie_amd.bgen import BgenFile
    by_n = {}
    for c in dc.valid_cases():
        by_n.setdefault(c.n, []).append(c)
    for n, cs in sorted(by_n.items()):
        path = str(tmp_path / ("n%d.bgen" % n))
        _write_bgen(path, n, cs)
        with BgenFile(path) as f:
            assert (f.n_samples, f.n_variants) == (n, len(cs))
            blocks = f.read_blocks(np.arange(len(cs)))
            comp, off, clen, ulen = f.read_compressed(np.arange(len(cs)))
        for j, c in enumerate(cs):
            assert blocks[j].tobytes() == c.payload, c.name
            assert comp[off[j]:off[j] + clen[j]].tobytes() == c.stream and ulen[j] == c.ulen, c.name
