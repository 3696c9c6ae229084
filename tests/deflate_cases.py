"""A token-level DEFLATE writer (RFC 1951 / 1950) and the corpus of hand-built zlib streams that pins the device BGEN inflate kernels
(regenie_amd/csrc/bgen_inflate.hip) at their DEFLATE and kernel edges.  Plain Python: the writer takes the tokens and the code lengths as they are
given and optimises nothing, so a stream holds exactly the construct its name says -- codes of 15 bits, distance 32,768, length 258 as symbol 284
with 31 extra bits, a distance alphabet of one 1-bit code, empty stored blocks, ... -- which zlib's own compressor never writes.

Every VALID case inflates to a well-formed BGEN layout-2 block of some N (10 + 3 N bytes: N, K = 2, ploidy 2 / 2, N ploidy bytes, 0, 8, 2 N
probability bytes), so the decoder's status is 0 on it and the walk's outputs can be checked too.  A MALFORMED case has payload None; its `why`
names the status the kernel reaches and the line of bgen_inflate.hip that sets it, traced by reading the code.  zlib (python's module) is the
arbiter of both kinds: tests/test_deflate_cases_cpu.py.

`hip:NNN` in a `why` is a line of regenie_amd/csrc/bgen_inflate.hip."""
from __future__ import annotations

import collections
import functools
import random
import zlib

import numpy as np

# RFC 1951, section 3.2.5 / 3.2.7
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32

# the kernel's status values (bgen_inflate.hip: enum ST_*)
ST_OK, ST_HEADER, ST_BTYPE, ST_STORED, ST_TABLE, ST_CODE, ST_DIST, ST_OVERRUN, ST_SHORT, ST_INPUT, ST_ADLER, ST_FORMAT = range(12)

Case = collections.namedtuple("Case", "name stream ulen payload why n blocks")


# ---------------------------------------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------------------------------------
class BitWriter:
    """LSB-first: the first bit written is bit 0 of the first byte."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        """A Huffman code goes out first bit first, i.e. bit-reversed."""
        self.put(int(format(code, "0%db" % length)[::-1], 2), length)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def nbits(self):
        return 8 * len(self.out) + self.n

    def getvalue(self):
        self.align()
        return bytes(self.out)


def canonical(lengths):
    """Canonical Huffman codes (RFC 1951, 3.2.2) of a list of code lengths; None for a symbol of length 0."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        if l:
            out.append(nxt[l])
            nxt[l] += 1
        else:
            out.append(None)
    return out


def kraft(lengths):
    """Sum of 2^-l as a multiple of 2^-15: 32,768 = complete."""
    return sum(1 << (15 - l) for l in lengths if l)


def len_symbol(length, long258=False):
    """(symbol index 0..28, extra value, extra bits) of a match length; long258 writes 258 as symbol 284 + 31."""
    if length == 258 and long258:
        return 27, 31, 5
    k = max(i for i in range(29) if LBASE[i] <= length)
    if k == 28 and length != 258:
        k = 27
    return k, length - LBASE[k], LEXT[k]


def dist_symbol(dist):
    k = max(i for i in range(30) if DBASE[i] <= dist)
    return k, dist - DBASE[k], DEXT[k]


def _tokens(w, tokens, lit_lens, dist_lens, long258):
    """Tokens: int = literal; (len, dist) = match; ("sym", s) = literal / length symbol s alone; ("bits", v, n) = raw bits."""
    lc, dc = canonical(lit_lens), canonical(dist_lens)
    for t in tokens:
        if isinstance(t, int):
            w.code(lc[t], lit_lens[t])
        elif t[0] == "sym":
            w.code(lc[t[1]], lit_lens[t[1]])
        elif t[0] == "bits":
            w.put(t[1], t[2])
        else:
            k, ev, eb = len_symbol(t[0], long258)
            w.code(lc[257 + k], lit_lens[257 + k])
            w.put(ev, eb)
            k, ev, eb = dist_symbol(t[1])
            w.code(dc[k], dist_lens[k])
            w.put(ev, eb)


def cl_rle(seq, hlit, mode):
    """The code-length sequence as (symbol, extra value, extra bits, start, count) items.  mode "plain": one item per length; "split": runs
    (16 / 17 / 18) inside each alphabet; "joint": runs over the whole sequence, so one may cross the literal / distance boundary."""
    if mode == "plain":
        return [(l, 0, 0, i, 1) for i, l in enumerate(seq)]
    parts = [(0, len(seq))] if mode == "joint" else [(0, hlit), (hlit, len(seq))]
    items = []
    for lo, hi in parts:
        i = lo
        while i < hi:
            j = i
            while j < hi and seq[j] == seq[i]:
                j += 1
            run, v = j - i, seq[i]
            if v == 0:
                while run >= 11:
                    r = min(run, 138)
                    items.append((18, r - 11, 7, i, r)); i += r; run -= r
                if run >= 3:
                    items.append((17, run - 3, 3, i, run)); i += run; run = 0
            else:
                items.append((v, 0, 0, i, 1)); i += 1; run -= 1
                while run >= 3:
                    r = min(run, 6)
                    items.append((16, r - 3, 2, i, r)); i += r; run -= r
            for _ in range(run):
                items.append((v, 0, 0, i, 1)); i += 1
    return items


CL_LENS = [4] * 13 + [5] * 6          # a complete code over all 19 code-length symbols (13 / 16 + 6 / 32 = 1); not optimised


def write_block(w, blk, final):
    """blk: dict(kind = "stored" | "fixed" | "dyn" | "raw", ...).  Fields beyond the tokens override what a well-formed block would hold."""
    kind = blk["kind"]
    final = blk.get("final", final)
    if kind == "raw":                                   # ("bits" tuples only): a block written bit by bit
        for _, v, n in blk["bits"]:
            w.put(v, n)
        return
    w.put(1 if final else 0, 1)
    if kind == "stored":
        data = blk["data"]
        w.put(0, 2)
        w.align()
        w.put(len(data), 16)
        w.put(blk.get("nlen", len(data) ^ 0xFFFF), 16)
        for b in data:
            w.put(b, 8)
        return
    long258 = blk.get("long258", False)
    if kind == "fixed":
        w.put(1, 2)
        _tokens(w, blk["tokens"], FIXED_LIT, FIXED_DIST, long258)
        if blk.get("eob", True):
            w.code(0, 7)
        return
    lit_lens, dist_lens = blk["lit_lens"], blk["dist_lens"]
    w.put(2, 2)
    w.put(blk.get("hlit_field", len(lit_lens) - 257), 5)
    w.put(blk.get("hdist_field", len(dist_lens) - 1), 5)
    cl_lens = blk.get("cl_lens", CL_LENS)
    w.put(19 - 4, 4)
    for s in CLORDER:
        w.put(cl_lens[s], 3)
    cc = canonical(cl_lens)
    items = blk.get("cl_items")
    if items is None:
        items = cl_rle(list(lit_lens) + list(dist_lens), len(lit_lens), blk.get("rle", "split"))
    for it in items:
        w.code(cc[it[0]], cl_lens[it[0]])
        w.put(it[1], it[2])
    if blk.get("header_only"):
        return
    _tokens(w, blk["tokens"], lit_lens, dist_lens, long258)
    if blk.get("eob", True):
        w.code(canonical(lit_lens)[256], lit_lens[256])


def block_tokens(blocks):
    """The literal / match tokens of a list of blocks, stored bytes as literals."""
    out = []
    for b in blocks:
        if b["kind"] == "stored":
            out += list(b["data"])
        elif b["kind"] in ("fixed", "dyn"):
            out += [t for t in b.get("tokens", []) if isinstance(t, int) or isinstance(t[0], int)]
    return out


def apply(tokens):
    """The plain definition: a literal is a byte, a match copies `len` bytes from `dist` back, byte by byte."""
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            ln, dist = t
            assert 1 <= dist <= len(out)
            for _ in range(ln):
                out.append(out[-dist])
    return bytes(out)


def deflate(blocks):
    w = BitWriter()
    for i, b in enumerate(blocks):
        write_block(w, b, i == len(blocks) - 1)
    return w.getvalue()


def zwrap(raw, payload):
    """RFC 1950: CMF / FLG 78 01 and the big-endian Adler-32 of the payload."""
    return b"\x78\x01" + raw + (zlib.adler32(payload) & 0xFFFFFFFF).to_bytes(4, "big")


# ---------------------------------------------------------------------------------------------------------
# code lengths
# ---------------------------------------------------------------------------------------------------------
def complete_lens(n, top, seed=None):
    """A complete code of n symbols whose longest codes have `top` bits: the ladder 1, 2, ..., top - 1, top, top, a code of it split in two
    until there are n -- the shortest each time (a flat code with a long tail), or with `seed` one drawn at random among those below 15 bits
    (a ragged tree with many codes of every length).  Sorted ascending."""
    ls = list(range(1, top)) + [top, top]
    rng = random.Random(seed)
    while len(ls) < n:
        ls.sort()
        x = ls.pop(0 if seed is None else rng.randrange(sum(1 for l in ls if l < 15)))
        assert x < 15
        ls += [x + 1, x + 1]
    assert len(ls) == n and kraft(ls) == 32768
    return sorted(ls)


def spread(ls, mult, long_at=()):
    """Length of symbol s = ls[s * mult mod n] (mult coprime to n): every chunk of 64 symbols gets every length.  long_at: symbols that must
    hold one of the longest codes."""
    n = len(ls)
    out = [ls[(s * mult) % n] for s in range(n)]
    assert sorted(out) == sorted(ls)
    for i, s in enumerate(long_at):                     # the longest codes (15, 15, 14, 13, ...) go to long_at in its order
        j = max((k for k in range(n) if k not in long_at[:i]), key=lambda k: out[k])
        out[s], out[j] = out[j], out[s]
    return out


FLAT_LIT = complete_lens(286, 9)[::1]                  # symbol order: 226 codes of 8 bits, then 60 of 9
FLAT_DIST = complete_lens(30, 5)
LIT15 = spread(complete_lens(286, 15, seed=1), 37, long_at=(285, 256, 0x82, 258))
DIST15 = spread(complete_lens(30, 15), 7, long_at=(0, 29))
DIST_HEAD9 = complete_lens(30, 9)[::-1]                # 9, 9, 8, ...: a repeat of the literals' 9s can run into it


# ---------------------------------------------------------------------------------------------------------
# payloads: BGEN layout-2 blocks built token by token
# ---------------------------------------------------------------------------------------------------------
RING = 4096


class Builder:
    """Builds the payload of N samples and its token list together.  Literals at the positions the format fixes take the fixed value; free bytes
    come from a seeded generator (ploidy bytes 0x02, one in ten 0x82 = missing; probability bytes anything).  A match that would put a wrong
    byte on a fixed position raises.  `flushed` follows the kernel's ring_flush rule (hip:509, hip:556) so that a case can place a token
    directly after or before a flush."""

    def __init__(self, n, seed):
        self.n, self.ulen = n, 10 + 3 * n
        self.rng = random.Random(seed)
        self.out, self.toks = bytearray(), []
        self.fixed = dict(enumerate(int(n).to_bytes(4, "little") + bytes([2, 0, 2, 2])))
        self.fixed[8 + n], self.fixed[9 + n] = 0, 8
        self.flushed, self.just_flushed = 0, False

    @property
    def pos(self):
        return len(self.out)

    def _after(self):
        self.just_flushed = self.pos - self.flushed >= RING // 2
        if self.just_flushed:
            self.flushed = self.pos & ~15

    def lit(self, v=None):
        p = self.pos
        assert p < self.ulen
        if p in self.fixed:
            assert v is None or v == self.fixed[p]
            v = self.fixed[p]
        elif v is None:
            v = (0x82 if self.rng.random() < 0.1 else 0x02) if p < 8 + self.n else self.rng.randrange(256)
        self.out.append(v)
        self.toks.append(v)
        self._after()

    def lits(self, upto, v=None):
        while self.pos < upto:
            self.lit(v if self.pos not in self.fixed else None)

    def ok(self, ln, dist):
        p = self.pos
        if not (3 <= ln <= 258 and 1 <= dist <= p and p + ln <= self.ulen):
            return False
        tmp = self.out[p - dist:p]
        return all(tmp[(q - p) % dist] == self.fixed[q] for q in range(p, p + ln) if q in self.fixed)

    def match(self, ln, dist):
        assert self.ok(ln, dist), (self.n, self.pos, ln, dist)
        for _ in range(ln):
            self.out.append(self.out[-dist])
        self.toks.append((ln, dist))
        self._after()

    def auto(self, upto, p_match=0.3, max_len=24):
        """Literals and matches of random length and distance up to `upto`."""
        while self.pos < upto:
            ln, dist = self.rng.randint(3, max_len), self.rng.randint(1, max(1, min(self.pos, 300)))
            if self.rng.random() < p_match and self.pos + ln <= upto and self.ok(ln, dist):
                self.match(ln, dist)
            else:
                self.lit()

    def cut(self):
        t, self.toks = self.toks, []
        return t

    def payload(self):
        assert self.pos == self.ulen
        return bytes(self.out)


def is_bgen_block(payload, n):
    return (len(payload) == 10 + 3 * n and payload[:8] == int(n).to_bytes(4, "little") + bytes([2, 0, 2, 2])
            and payload[8 + n] == 0 and payload[9 + n] == 8)


def fixed(tokens, **kw):
    return dict(kind="fixed", tokens=tokens, **kw)


def dyn(tokens, lit_lens=FLAT_LIT, dist_lens=FLAT_DIST, **kw):
    return dict(kind="dyn", tokens=tokens, lit_lens=list(lit_lens), dist_lens=list(dist_lens), **kw)


def stored(data, **kw):
    return dict(kind="stored", data=bytes(data), **kw)


def _valid(name, n, blocks, why):
    payload = apply(block_tokens(blocks))
    assert is_bgen_block(payload, n), name
    assert len(payload) <= 70 * 1024
    return Case(name, zwrap(deflate(blocks), payload), len(payload), payload, why, n, blocks)


def _bad(name, n, blocks, why, ulen=None, payload_for_adler=b"", cut=None):
    s = zwrap(deflate(blocks), payload_for_adler)
    if cut is not None:
        s = s[:cut]
    return Case(name, s, 10 + 3 * n if ulen is None else ulen, None, why, n, blocks)


# ---------------------------------------------------------------------------------------------------------
# the corpus
# ---------------------------------------------------------------------------------------------------------
SMALL_N = (1, 2, 5, 13, 18, 103, 104, 105, 106)
EDGE_N = (678, 679, 680, 1361, 1362, 1363)            # ulen 2,044 / 2,047 / 2,050 (RING / 2) and 4,093 / 4,096 / 4,099 (RING)
REGIME_DISTS = (1, 2, 37, 63, 64, 65, 257)


def _streams_of_deflate():
    out = []
    # --- codes of 15 bits, all 286 + 30 symbols, lengths spread over the ballot chunks
    for n, tag in ((200, "window"), (50, "serial")):
        b = Builder(n, 1)
        b.lits(8 + n + 2)
        for v in [s for s in range(256) if LIT15[s] >= 11][:8]:      # probability bytes with codes of 11 to 14 bits
            b.lit(v)
        b.lits(b.pos + 6)
        b.match(258 if n == 200 else 40, 1)            # length symbol 285 / distance symbol 0: both 15 bits in LIT15 / DIST15
        b.match(3, 2)
        b.auto(b.ulen - 20, 0.4)
        b.lits(b.ulen)
        out.append(_valid("code15_%s_n%d" % (tag, n), n, [dyn(b.cut(), LIT15, DIST15)],
                          "lit/len and distance codes of 15 bits: second-level tables of 5 and 6 bits (hip:146-181), looked up in the %s loop (%s); "
                          "286 + 30 lengths permuted over the five ballot chunks (hip:122-142)" % (tag, "hip:459-475" if n == 200 else "hip:523-542")))
    # --- every length symbol, every distance symbol, distance 32,768, HLIT = 286 / HDIST = 30 in full
    n = 11100
    b = Builder(n, 2)
    b.lits(24700)
    for k in range(29):
        b.match(LBASE[k] + ((1 << LEXT[k]) - 1 if k < 28 else 0) - (1 if k == 27 else 0), DBASE[k] + (1 << DEXT[k]) - 1)
    b.match(9, DBASE[29])
    b.lits(32768)
    b.match(3, 32768)
    b.match(258, 32768)
    b.match(64, 32768)
    b.lits(b.ulen - 100)
    b.match(3, 32768)                                  # in the serial loop
    b.match(70, 32768)
    b.lits(b.ulen)
    out.append(_valid("all_symbols_dist32768_code15", n, [dyn(b.cut(), LIT15, DIST15)],
                      "every length symbol 257..285 and distance symbol 0..29 with their largest extra bits; distance 32,768 = 24,577 + 8,191 "
                      "(hip:479 window, hip:546 serial; far path hip:314-323); HLIT = 286, HDIST = 30, all lengths non-zero (hip:414)"))
    b = Builder(n, 3)
    b.lits(32768)
    b.match(258, 32768)
    b.match(3, 32768)
    b.lits(b.ulen - 3)
    b.match(3, 32768)
    out.append(_valid("dist32768_fixed", n, [fixed(b.cut())],
                      "distance 32,768 on the fixed code (30 five-bit distance codes, hip:376), the first possible position and the last three bytes"))
    # --- 258 as symbol 284 + 31
    for kind in ("fixed", "dyn"):
        n = 300
        b = Builder(n, 4)
        b.lits(8 + n + 4)
        b.match(258, 1)                                 # pos 312 <= cap - 322 = 588: window loop
        b.lits(600)
        b.match(258, 3)                                 # pos 600: serial loop
        b.lits(b.ulen)
        t = b.cut()
        out.append(_valid("len258_as_284_31_%s" % kind, n, [fixed(t, long258=True) if kind == "fixed" else dyn(t, long258=True)],
                          "length 258 written as symbol 284 with extra bits 31 (227 + 31), once in the window loop (hip:469), once behind the "
                          "hand-over in the serial loop (hip:535)"))
    # --- distance alphabets of one code or none
    for n, tag in ((200, "window"), (50, "serial")):
        b = Builder(n, 5)
        b.lits(8 + n + 3)
        b.match(17, 1)
        b.lit()
        b.match(64 if n == 50 else 258, 1)
        b.lits(b.ulen)
        out.append(_valid("dist_one_1bit_code_%s" % tag, n, [dyn(b.cut(), FLAT_LIT, [1])],
                          "HDIST = 1 with one code of 1 bit: the incomplete set build_table_impl admits (hip:115); its other half stays K_BAD"))
        b = Builder(n, 6)
        b.lits(b.ulen)
        out.append(_valid("hdist1_zero_length_%s" % tag, n, [dyn(b.cut(), FLAT_LIT, [0])],
                          "HDIST = 1 with length 0: a block of literals, an empty distance table (hip:115: maxl = 0)"))
    # --- blocks that are only an end-of-block symbol; empty stored blocks; a final stored block
    b = Builder(200, 7)
    b.auto(300)
    t1 = b.cut()
    b.auto(b.ulen)
    t2 = b.cut()
    out.append(_valid("eob_only_blocks", 200, [fixed([]), dyn([]), fixed(t1), fixed([]), dyn([], [0] * 256 + [1], [0]), dyn(t2), fixed([])],
                      "blocks of the end-of-block symbol alone, first, between and last (fixed, dynamic, and a dynamic one whose only code is the "
                      "1-bit end-of-block: hip:506 stop = 1, hip:516)"))
    b = Builder(200, 8)
    b.auto(250)
    t1 = b.cut()
    b.auto(500)
    t2 = b.cut()
    b.lits(b.ulen)
    t3 = b.cut()
    out.append(_valid("empty_stored_between_final_stored", 200, [stored(b""), fixed(t1), stored(b""), stored(b""), dyn(t2), stored(b""), stored(bytes(t3))],
                      "empty stored blocks before and between Huffman blocks (hip:355-369 after bits_seek, hip:515), a final stored block after a "
                      "Huffman block"))
    b = Builder(50, 9)
    b.auto(80)
    t1 = b.cut()
    b.lits(b.ulen)
    out.append(_valid("final_stored_after_huffman_serial", 50, [dyn(t1), stored(b""), stored(bytes(b.cut()))],
                      "the same below 322 bytes: the stored block follows the serial loop's end-of-block (hip:552-554)"))
    # --- a repeat across the literal / distance boundary
    for n, tag in ((200, "window"), (50, "serial")):
        b = Builder(n, 10)
        b.auto(b.ulen, 0.4)
        t = b.cut()
        out.append(_valid("repeat16_across_boundary_%s" % tag, n, [dyn(t, FLAT_LIT, DIST_HEAD9, rle="joint")],
                          "a code-16 repeat of the literals' trailing 9s runs on into the distance lengths (hip:402-409: one index over both alphabets)"))
        lit = list(FLAT_LIT)                           # six 9-bit codes dropped free 6 / 512, six others shortened to 8 bits use them
        lit[280:286] = [0] * 6
        lit[270:276] = [8] * 6
        assert kraft(lit) == 32768
        dist = [0, 0] + complete_lens(28, 6)
        b = Builder(n, 11)
        b.lits(8 + n + 4)
        while b.pos + 40 < b.ulen:
            b.match(5, 3) if b.ok(5, 3) else b.lit()
            b.lit()
        b.lits(b.ulen)
        out.append(_valid("zero_repeat_across_boundary_%s" % tag, n, [dyn(b.cut(), lit, dist, rle="joint")],
                          "a zero run (code 17) over the last six literal/length lengths and the first two distance lengths (hip:403-409)"))
    # --- plain (unrepeated) code lengths: 316 items through the code-length table
    b = Builder(200, 12)
    b.auto(b.ulen, 0.4)
    out.append(_valid("lengths_without_repeats", 200, [dyn(b.cut(), LIT15, DIST15, rle="plain")],
                      "316 code lengths one by one, none by 16 / 17 / 18 (hip:394-410)"))
    return out


def _streams_of_matches():
    out = []
    n = 1300
    for order, tag in ((REGIME_DISTS, "up"), (REGIME_DISTS[::-1], "down")):
        for kind in ("fixed", "dyn"):
            b = Builder(n, 20)
            b.lits(8 + n + 12)
            for d in order:
                b.match(258, d)
                b.lit()
            for ln, d in ((64, 64), (65, 65), (63, 64), (64, 63), (65, 64), (66, 65), (129, 64), (130, 65), (5, 2), (3, 1), (4, 3), (3, 3)):
                b.match(ln, d)
                b.lit()
            b.lits(b.ulen)
            t = b.cut()
            out.append(_valid("match_regimes_%s_%s" % (tag, kind), n, [fixed(t) if kind == "fixed" else dyn(t)],
                              "emit_match from the window loop: dist < 64 overlapping (float-quotient modulo, hip:298-307), 64 <= dist < len (chunks "
                              "that read earlier chunks, hip:290-296), len <= 64 <= dist on the one-instruction path (hip:496) at 64 / 65 and "
                              "just off it (63, 64), (65, 64); distances in order '%s'" % tag))
    for d in REGIME_DISTS:                                  # the same regimes called from the serial loop: the match starts behind cap - 322
        b = Builder(200, 24)
        b.lits(b.ulen - 300)
        b.match(258, d)
        b.lits(b.ulen - 10)
        b.match(10, d) if d < 100 else b.match(10, 64)
        out.append(_valid("match_serial_258_dist%d" % d, 200, [fixed(b.cut())],
                          "emit_match(258, %d) called by the serial loop (hip:550) after the hand-over stop = 2 (hip:499); the stream ends on a match" % d))
    n = 3000
    b = Builder(n, 21)
    b.lits(4100)
    for ln, d in ((3, 4032), (258, 4032), (3, 4033), (258, 4033), (64, 4032), (64, 4033), (65, 4032), (3, 4095), (258, 4096), (3, 4097), (100, 4031)):
        b.match(ln, d)
        b.lit()
    b.lits(b.ulen - 300)
    for ln, d in ((3, 4032), (3, 4033), (258, 4033)):      # the same in the serial loop
        b.match(ln, d)
    b.lits(b.ulen)
    t = b.cut()
    for kind in ("fixed", "dyn"):
        out.append(_valid("ring_edge_4032_4033_%s" % kind, n, [fixed(t) if kind == "fixed" else dyn(t)],
                          "dist = RING - 64 = 4,032 is the last match read from the LDS ring, 4,033 the first read from flushed memory "
                          "(hip:288, hip:482 `slow`, hip:314-323)"))
    # far matches directly after and directly before a ring flush
    n = 5000
    b = Builder(n, 22)
    b.lits(5100)
    while not b.just_flushed:
        b.lit()
    b.match(258, 4033)                                      # the flush of the symbol before has just been issued
    b.match(3, 4033)
    while not b.just_flushed:
        b.lit()
    b.match(200, b.pos)                                     # as far back as the block goes
    while b.pos - b.flushed < RING // 2 - 3:
        b.lit()
    assert b.pos - b.flushed == RING // 2 - 3
    b.match(3, 4033)                                        # this match triggers the flush
    assert b.just_flushed
    b.match(258, 4040)
    while b.pos - b.flushed < RING // 2 - 1:
        b.lit()
    b.match(258, 5000)                                      # the largest overshoot of the trigger
    assert b.just_flushed
    b.match(258, 4033)
    b.lits(b.ulen)
    t = b.cut()
    for kind in ("fixed", "dyn"):
        out.append(_valid("far_match_at_flush_%s" % kind, n, [fixed(t) if kind == "fixed" else dyn(t)],
                          "a far match as the first symbol after ring_flush and as the symbol that triggers it (hip:509, hip:311: the bytes read "
                          "were flushed at least RING / 2 - 600 bytes ago)"))
    # dist = 4,096 right after an end-of-block taken in the window loop: that path writes a byte at ring[pos] without advancing (hip:504)
    b = Builder(n, 23)
    b.lits(4600)
    while b.out[b.pos - 4096] == 1 or b.out[b.pos - 4095] == 1:
        b.lit()
    t1 = b.cut()
    b.match(3, 4096)
    b.match(258, 4095)
    b.lits(b.ulen)
    out.append(_valid("dist4096_after_window_eob", n, [fixed(t1), fixed(b.cut())],
                      "the window loop's end-of-block leaves the byte 0x01 at ring[pos & 4095], the slot of output byte pos - 4,096 (hip:504-506): a "
                      "match of distance 4,096 that follows must not be served from the ring (hip:288)"))
    return out


def _small(n, kind, seed):
    b = Builder(n, seed)
    if kind == "stored":
        b.lits(b.ulen)
        t = b.cut()
        h = len(t) // 2
        return [stored(bytes(t[:h])), stored(bytes(t[h:]))]
    b.auto(b.ulen, 0.35, 12)
    return [fixed(b.cut())] if kind == "fixed" else [dyn(b.cut())]


def _streams_of_sizes():
    out = []
    for n in SMALL_N + EDGE_N:
        for kind in ("fixed", "dyn", "stored"):
            ulen = 10 + 3 * n
            why = ("ulen = %d %s 322: %s (hip:435-437)" % (ulen, "<" if ulen < 322 else ">=", "serial loop only" if ulen < 322 else
                   "window loop while pos <= %d, then the hand-over stop = 2 (hip:499, hip:513)" % (ulen - 322)))
            if n in EDGE_N:
                why = "ulen = %d at a multiple of RING / 2 = 2,048: the last ring_flush and its tail of %d bytes (hip:273-281, hip:561)" % (ulen, ulen % 16)
            elif ulen % 16 in (0, 1):
                why += "; ulen = 16 k + %d (ring_flush tail hip:276, Adler piece hip:581-592)" % (ulen % 16)
            out.append(_valid("size_n%d_%s" % (n, kind), n, _small(n, kind, 30 + n), why))
    # literals only up to the end: the window loop is left at its top (stop stays 0)
    b = Builder(200, 31)
    b.lits(b.ulen)
    out.append(_valid("literals_only_tail", 200, [dyn(b.cut())], "no match near the end: the window loop ends by its own test, stop = 2 at hip:513"))
    return out


def _fixed_literals_exact(n, nbytes_block, seed):
    """A fixed block of literals whose end-of-block code ends exactly `nbytes_block` bytes into the zlib stream: 16 + 3 + 8 L + (number of 9-bit
    literals) + 7 bits with L = nbytes_block - 4 literals, six of them >= 144 (ploidy bytes 0x82)."""
    b = Builder(n, seed)
    L = nbytes_block - 4
    assert 8 + 6 < L <= 8 + n
    b.lits(8)
    for _ in range(6):
        b.lit(0x82)
    b.lits(L, 0x02)
    return b, b.cut()


def _streams_of_framing():
    out = []
    # end of input next to a 256-byte chunk edge: stored streams of exactly clen bytes (16 + 3 N + 5 k with k blocks)
    for clen, n, k in ((255, 78, 1), (256, 75, 3), (257, 77, 2), (511, 160, 3), (512, 162, 2), (513, 164, 1)):
        b = Builder(n, 40 + k)
        b.lits(b.ulen)
        t = bytes(b.cut())
        cutp = [len(t) * i // k for i in range(k + 1)]
        c = _valid("clen%d_stored" % clen, n, [stored(t[cutp[i]:cutp[i + 1]]) for i in range(k)],
                   "a stream of %d bytes: with mis = 0..3 the input ends at, before and after a chunk edge of the serial reader "
                   "(hip:235-238 the cur / nxt swap, hip:212 zeros past ndw)" % clen)
        assert len(c.stream) == clen
        out.append(c)
    # the same with Huffman blocks: a fixed block of literals (some of 9 bits) padded to the bit
    for clen, n in ((255, 79), (256, 79), (257, 79), (511, 164), (512, 164), (513, 164)):
        b = Builder(n, 50)
        ulen = 10 + 3 * n
        n9 = 8 * (clen - 4) - (26 + 8 * ulen)
        b.lits(10 + n, 0x02)
        n9 -= sum(v >= 144 for v in b.out)               # (the sample count's own byte)
        assert 0 <= n9 <= 2 * n, (clen, n, n9)
        k9 = 0
        while b.pos < ulen:
            b.lit(200 if k9 < n9 else 17)
            k9 += 1
        c = _valid("clen%d_fixed" % clen, n, [fixed(b.cut())],
                   "a stream of %d bytes whose end-of-block code ends on its last bit before the trailer: serial reader (n = %d) at the chunk edge "
                   "(hip:230-238)" % (clen, n) if ulen < 322 else
                   "a stream of %d bytes: window loop, then bits_seek (hip:251-259) and the serial reader up to the chunk edge" % clen)
        assert len(c.stream) == clen, (clen, len(c.stream))
        out.append(c)
    # bits_seek landing in the last dwords of a chunk: the first block ends T bytes into the stream
    for T in (248, 252, 253, 255, 256, 260):
        b, t1 = _fixed_literals_exact(300, T, 60)
        b.auto(b.ulen, 0.3)
        out.append(_valid("seek_after_block_at_byte_%d" % T, 300, [fixed(t1), dyn(b.cut())],
                          "the first block's end-of-block ends at byte %d of the stream: with mis = 0..3 bits_seek (hip:251-259) lands in dwords "
                          "62, 63 and 64, i.e. takes and skips the branch `(b.w >> 6) != chunk`; the window loop of the second block starts on "
                          "`base + 4 >= 64` (hip:451)" % T))
    return out


def _streams_malformed():
    out = []
    good = Builder(200, 70)
    good.auto(good.ulen, 0.3)
    gt = good.cut()
    gp = good.payload()
    small = Builder(50, 71)
    small.auto(small.ulen, 0.3)
    st = small.cut()
    sp = small.payload()

    def both(name, mk, why_w, why_s=None):
        """mk(n, tokens, payload) -> (blocks, ulen or None, payload for the trailer): once over the window loop, once over the serial loop"""
        for n, t, p, tag, why in ((200, gt, gp, "window", why_w), (50, st, sp, "serial", why_s or why_w)):
            blocks, ulen, pay = mk(n, t, p)
            out.append(_bad("%s_%s" % (name, tag), n, blocks, why, ulen, pay))

    def table(name, why, **kw):
        kw["header_only"] = True                        # the block's header, then the trailer: the tables are refused before a symbol is read
        out.append(_bad(name, 200, [dyn(gt, **kw)], why + " -> ST_TABLE (4)", None, gp))

    over = list(FLAT_LIT); over[100] = 7
    table("lit_code_oversubscribed", "build_table_impl: left < 0 (hip:105, hip:111), hip:414", lit_lens=over)
    over = list(FLAT_DIST); over[5] = 3
    table("dist_code_oversubscribed", "build_table_impl: left < 0 (hip:111), second call of hip:414", dist_lens=over)
    table("codelength_code_oversubscribed", "build_table_impl of the 19 lengths: left < 0 (hip:111), hip:390", cl_lens=[4] * 14 + [5] * 5, header_only=True)
    inc = list(FLAT_LIT); inc[100] = 10
    table("lit_code_incomplete", "build_table_impl: left > 0 with maxl = 10 (hip:115), hip:414", lit_lens=inc)
    table("dist_code_incomplete_two_codes", "build_table_impl: left > 0, maxl = 2 (hip:115)", dist_lens=[2, 2] + [0] * 28)
    table("dist_code_incomplete_one_2bit_code", "build_table_impl: left > 0, ONE code but of 2 bits: maxl != 1 (hip:115)", dist_lens=[2])
    table("codelength_code_incomplete", "build_table_impl mode 2: left > 0 (hip:115), hip:390", cl_lens=[4] * 12 + [5] * 7, header_only=True)
    noeob = [0 if s == 256 else 9 for s in range(286)]
    for s in range(227):                               # a complete code over the other 285 symbols: x of 8 bits, 285 - x of 9, 2 x + 285 - x = 512
        noeob[s] = 8
    assert kraft(noeob) == 32768
    table("no_end_of_block_code", "lens[32 + 256] == 0 (hip:413)", lit_lens=noeob, header_only=True)
    seq = list(FLAT_LIT) + list(FLAT_DIST)
    table("repeat16_first", "code 16 with i == 0 (hip:402), hip:411", cl_items=[(16, 0, 2, 0, 3)] + cl_rle(seq, 286, "split"), header_only=True)
    items = cl_rle(seq, 286, "plain")[:-2] + [(18, 127, 7, 314, 138)]
    table("repeat_past_hlit_hdist", "i + rep > ntot (hip:405), hip:411", cl_items=items, header_only=True)
    table("hlit_287", "hlit > 286 (hip:380)", hlit_field=30, header_only=True)
    table("hdist_31", "hdist > 30 (hip:380)", hdist_field=30, header_only=True)
    out.append(_bad("btype_3", 200, [dict(kind="raw", bits=[("bits", 1, 1), ("bits", 3, 2), ("bits", 0, 29)])], "btype == 3 (hip:371) -> ST_BTYPE (2)", None, gp))
    out.append(_bad("btype_3_after_block", 200, [fixed(gt[:100]), dict(kind="raw", bits=[("bits", 1, 1), ("bits", 3, 2), ("bits", 0, 29)])],
                    "btype == 3 in the second block, after bits_seek (hip:371) -> ST_BTYPE (2)", None, gp))
    out.append(_bad("stored_nlen_mismatch", 200, [stored(gp, nlen=(len(gp) ^ 0xFFFF) ^ 0x0100)], "len ^ 0xFFFF != nlen (hip:360) -> ST_STORED (3)", None, gp))
    out.append(_bad("stored_overrun", 200, [fixed(gt), stored(b"\x00")], "stored block of one byte at pos = cap (hip:361) -> ST_OVERRUN (7)", None, gp + b"\x00"))

    def sym(s):
        def mk(n, t, p):
            k = 40
            return [fixed(t[:k] + [("sym", s)] + t[k:])], None, p
        return mk
    for s in (286, 287):
        both("fixed_symbol_%d" % s, sym(s), "the fixed code's symbol %d is K_BAD (hip:75): A = 0x80 in the window, stop = 16 + ST_CODE (hip:506) -> ST_CODE (5)" % s,
             "the fixed code's symbol %d is K_BAD (hip:75): serial loop's last branch (hip:555) -> ST_CODE (5)" % s)

    def dcode(d):
        def mk(n, t, p):
            k = 40
            return [fixed(t[:k] + [("sym", 257), ("bits", int(format(d, "05b")[::-1], 2), 5)] + t[k:])], None, p
        return mk
    for d in (30, 31):
        both("fixed_distance_code_%d" % d, dcode(d),
             "distance code %d of the fixed code has no entry (hip:77, hip:161): the window's A stays 0x80 (hip:464, hip:477) -> ST_CODE (5)" % d,
             "distance code %d of the fixed code has no entry: dk is not K_LEN (hip:544) -> ST_CODE (5)" % d)
    both("dist_one_1bit_code_other_half",
         lambda n, t, p: ([dyn(list(p[:30]) + [("sym", 257), ("bits", 1, 1)] + list(p[30:]), FLAT_LIT, [1])], None, p),
         "the unused half of a one-code distance alphabet is K_BAD (hip:161): window A = 0x80 (hip:477) -> ST_CODE (5)",
         "the unused half of a one-code distance alphabet is K_BAD: hip:544 -> ST_CODE (5)")
    both("distance_before_start_first_symbol", lambda n, t, p: ([fixed([(3, 1)] + t)], None, p),
         "a match at pos = 0: dist > o.pos with pos <= lim (hip:494, hip:499) -> ST_DIST (6)", "dist > o.pos (hip:548) -> ST_DIST (6)")
    both("distance_before_start_by_one", lambda n, t, p: ([fixed(list(p[:20]) + [(3, 21)] + t)], None, p),
         "20 literals, then distance 21 (hip:494, hip:499) -> ST_DIST (6)", "20 literals, then distance 21 (hip:548) -> ST_DIST (6)")
    both("one_byte_more_by_literal", lambda n, t, p: ([fixed(t + [7])], None, p + b"\x07"),
         "ulen + 1 bytes: the window loop stops at pos > cap - 322, the serial loop refuses the literal at pos = cap (hip:530) -> ST_OVERRUN (7)",
         "ulen + 1 bytes: the literal at pos = cap (hip:530) -> ST_OVERRUN (7)")
    both("one_byte_more_by_match", lambda n, t, p: ([fixed(list(p[:-2]) + [(3, 1)])], None, p[:-2] + p[-3:-2] * 3),
         "a match of 3 with 2 bytes left: pos + len > cap (hip:549) -> ST_OVERRUN (7)")
    both("one_byte_fewer", lambda n, t, p: ([fixed(list(p[:-1]))], None, p[:-1]),
         "the final block ends at pos = cap - 1 (hip:562) -> ST_SHORT (8)")
    # ulen = 610: a match of 258 at pos = cap - 258 (behind the hand-over at cap - 322), then one literal too many
    p = gp
    out.append(_bad("literal_after_258_to_cap", 200, [fixed(list(p[:352]) + [(258, 300), 9])], "a match of 258 that ends at cap, taken by the serial loop "
                    "because pos = cap - 258 > cap - 322 (hip:499), then a literal at pos = cap (hip:530) -> ST_OVERRUN (7); a window loop that "
                    "ran to cap - 258 would write it", None, p[:352] + bytes(p[52:310]) + b"\x09"))
    # the input ends inside a block: on FLAT_LIT the all-zero code is the literal 0, so the zeros read past the end decode as literals
    for n, t, p, tag, why in ((200, gt, gp, "window", "zeros past the end decode as literal 0: the window loop reaches w0 > ndw + 2 (hip:440) -> ST_INPUT (9)"),
                              (50, st, sp, "serial", "zeros past the end decode as literal 0: the serial loop is about to read past ndw + 2 dwords "
                               "(hip:520) -> ST_INPUT (9)")):
        full = zwrap(deflate([dyn(t)]), p)
        hdr = 2 + (len(deflate([dyn([], header_only=True)])))
        out.append(Case("input_ends_inside_block_%s" % tag, full[:hdr + (len(full) - hdr) // 4], 10 + 3 * n, None, why, n, [dyn(t)]))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """All cases, valid ones first.  Names are unique."""
    out = _streams_of_deflate() + _streams_of_matches() + _streams_of_sizes() + _streams_of_framing() + _streams_malformed()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def valid_cases():
    return [c for c in cases() if c.payload is not None]


def malformed_cases():
    return [c for c in cases() if c.payload is None]


def expected_status(case):
    """The status a malformed case's `why` ends on, e.g. '-> ST_CODE (5)'."""
    return int(case.why.rsplit("(", 1)[1].split(")")[0])


def lay_out(streams, aligns=(0, 1, 2, 3), pad=0xFF):
    """The streams laid into one buffer the way rg_bgen_read_compressed hands them over, each once per alignment: off % 4 runs through `aligns`.
    Returns (comp, off, clen, which) with which[i] = index into `streams`."""
    buf, off, clen, which = bytearray(), [], [], []
    for a in aligns:
        for i, s in enumerate(streams):
            buf += bytes([pad]) * (4 + (a - len(buf)) % 4)
            assert len(buf) % 4 == a
            off.append(len(buf)); clen.append(len(s)); which.append(i)
            buf += s
    buf += bytes([pad]) * 8
    return np.frombuffer(bytes(buf), dtype=np.uint8).copy(), np.array(off, dtype=np.int64), np.array(clen, dtype=np.int32), np.array(which)
