"""Kernel parity of Step 1's narrow-precision paths (GPU), each against a plain high-precision reference of the same operation.

* G~X / G~Y of level 0 (rg_k_xy_i8): route 0 is the digit-plane contraction on the i8 matrix cores (k_v_split, k_xy_i8,
  k_xy_combine), route 1 the fp64 kernel of RG_XY_F64=1 (k_geno_xy).  Reference: the exact sum of g0 * V and M * V per (block,
  fold, row, column); V is cut into three pieces on fixed grids of 2^-21, 2^-42 and 2^-63 of the column's scale plus a remainder,
  so that every piece's products and sums are integers below 2^53 (exact in any order), and the pieces are added in extended
  precision.
  Bar of route 0: |got - exact| <= 4e-15 sum|terms| + 2^-52 n_fold max|V_c|.  k_v_split rounds q = V 2^(54-e) to an integer
  (2^e = twice the column's largest power of two at most): a term g V moves by at most 2 * 2^-55 * 2^e <= 2^-53 * 2 max|V_c|,
  n_fold of them 2^-52 n_fold max|V_c|.  The digit sums are exact int32, k_xy_combine adds eight of them in fp64 with partial sums
  no larger than 1.01 sum|terms| (balanced digits): 8 * 1.01 * 2^-53 < 1e-15 of sum|terms|, inside the 4e-15.
  Bar of route 1: n_chunk 2^-53 / (1 - n_chunk 2^-53) sum|terms| (n_chunk <= 4,096, the sequential fp64 sum of one chunk; the test
  adds the chunk partials of a fold in extended precision).  The 4e-15 of route 0 does NOT hold for it: on a constant column (the
  intercept column of V in level 0) the chunk's roundings are correlated and reach about ten times that.
  The two routes must agree within the sum of their bars.
* The weighted Gram of the logistic ridge (rg_k_wgram), H = sum over a chain's training positions of w x_r x_c:
  fmt 0 (fp64, k_wgram128 + k_wg_reduce) against H: 1e-13 sum|w x_r x_c|.  The kernel adds four products per fp64 matrix instruction
  into one accumulator per K slice: at most n_seq = N / (4 nslice) sequential roundings (7,800 at 500,000 positions); the
  probabilistic bound 3 sqrt(n_seq) 2^-53 is 3e-14, the reference (2,048-position matmuls added with TwoSum) adds about 1e-14.
  fmt 1 (fp16) and 2 (bf16 hi + lo) against H_emul, the fp64 sum of the very products the kernel forms from its rounded operands:
  2^-14 sum|v_r v_c|.  One flush of the fp32 accumulators spans 4,096 positions = 256 accumulating instructions of K = 16 (fp16;
  bf16: 128 stages x 2 x 3 or 4 = 1,024 instructions of smaller products), each rounding once at 2^-24 of what the accumulator holds:
  2^-16 (bf16 worst case 2^-14), and a margin for the instruction's internal order.  Truncating the fp16 operands instead of
  rounding them moves every diagonal entry by about 2^-11 of itself.  In the 500,000-position case one predictor row holds a
  spike (64 positions of v = 32, a sum of 2^16) and small values v^2 = 0.99 * 2^-12 after it: sixteen of them are below half an
  fp32 ulp of 2^16, so an accumulator that is not flushed drops all of them for the rest of its K slice (31,000 positions:
  1.9 x the bar), while a flushed one loses at most the 4,032 after the spike in its first window (0.25 x the bar).
  Sanity of the emulation: |H_emul - H| within the format's own bound (fp16: rounding 2^-11 + 2^-24 relative, 2^-25 absolute
  in the subnormal range, per operand).
* The level-0 routes (VALU / digit-plane / fp64-MFMA predictions, one and two phenotype groups, R0 from 1 to 8, K up to 32, the
  block width at which the i8 prediction route ends) through Step1Engine against the oracle (1e-8, as tests/test_step1_gpu.py),
  and W of the default routes against RG_PRED_F64=1 and RG_XY_F64=1 at 1e-12 relative.

Worst observed ratio to the bar on an MI355X: G~X / G~Y route 0 0.023, route 1 0.012; weighted Gram fmt 0 0.034, fmt 1 0.24 and
fmt 2 0.24 (both the 500,000-position spike case, as designed; 0.016 and 0.046 elsewhere)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import regenie_step1 as orc  # noqa: E402
from regenie_amd.engine import load_library  # noqa: E402
from tests.test_step1_gpu import _compare  # noqa: E402
from tests.util import gpu_step1, rel_err, synth_dosages, write_plink  # noqa: E402

U = 2.0 ** -53


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _layout(fold_len):
    plen = [(n + 255) // 256 * 256 for n in fold_len]
    start = np.concatenate([[0], np.cumsum(plen)[:-1]]).astype(np.int64)
    return start, np.array(plen, np.int64), int(sum(plen))


def _i64(a):
    return np.ascontiguousarray(np.asarray(a, np.int64))


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, np.int32))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _ratio(err, bar):
    """max err / bar (entries with bar = 0 must have err = 0, which the caller asserts)."""
    return float(np.max(err / np.where(bar > 0, bar, 1.0)))


# ---- G~X / G~Y ------------------------------------------------------------------------------------------------------------------

def _v_columns(rng, Cv, Np, kinds):
    """V [Cv][Np]: column c of kind kinds[c % len(kinds)]."""
    V = np.zeros((Cv, Np))
    for c in range(Cv):
        k = kinds[c % len(kinds)]
        x = rng.standard_normal(Np)
        if k == "normal":
            V[c] = x
        elif k == "pow2_pos":            # maximum exactly 2^3, positive
            V[c] = np.clip(x, -7.9, 7.9)
            V[c, rng.integers(Np)] = 8.0
        elif k == "pow2_neg":            # maximum exactly 2^-5, negative
            V[c] = np.clip(x, -0.99, 0.99) * 2.0 ** -5
            V[c, rng.integers(Np)] = -(2.0 ** -5)
        elif k == "neg_max":             # maximum attained by a negative entry
            V[c] = np.clip(x, -2.5, 2.5)
            V[c, rng.integers(Np)] = -3.7
        elif k == "lowdigit":            # maximum 1, every other entry an odd multiple of 2^-47: the lowest digit is -64 everywhere
            V[c] = (2 * rng.integers(-3, 3, size=Np) + 1) * 2.0 ** -47
            V[c, rng.integers(Np)] = 1.0
        elif k == "zero":
            pass
        elif k == "tiny":                # entries at 2^-60 of the maximum, and subnormals
            V[c] = x
            i = rng.random(Np) < 0.2
            V[c, i] = np.sign(x[i]) * 2.0 ** -60 * np.abs(x).max()
            j = rng.random(Np) < 0.1
            V[c, j] = np.sign(x[j]) * 5e-320
        elif k.startswith("scale"):      # column scales from 1e-150 to 1e150
            V[c] = x * 10.0 ** float(k[5:])
        else:
            raise ValueError(k)
    return V


def _exact_sums(G, V):
    """sum_pos G[j, pos] V[c, pos] for integer G in 0..2, exactly (returned in extended precision): [rows][Cv]."""
    out = np.zeros((G.shape[0], V.shape[0]), np.longdouble)
    for c in range(V.shape[0]):
        v = V[c]
        mx = np.abs(v).max()
        if mx == 0.0:
            continue
        e = np.frexp(mx)[1]
        rest = v.copy()
        for sh in (21, 42, 63):
            piece = np.rint(np.ldexp(rest, sh - e))             # an integer, |piece| <= 2^21
            rest = rest - np.ldexp(piece, e - sh)                # exact
            out[:, c] += np.ldexp((G @ piece).astype(np.longdouble), e - sh)
        out[:, c] += (G @ rest).astype(np.longdouble)          # below 2^-64 of the column's scale
    return out


def _xy_call(pk, pk_ld, n128, bs, nmiss, fold_len, V, route, Np):
    lib = load_library()
    nblk, Cv = len(bs), V.shape[0]
    bs_h, nm_h, fl_h = _i32(bs), _i32(nmiss), _i64(fold_len)
    nchunk = C.c_int32(0)
    assert lib.rg_k_xy_i8(_stream(), pk.data_ptr(), pk_ld, n128 * pk_ld, nblk, n128, _ptr(bs_h), _ptr(nm_h), len(fold_len),
                          _ptr(fl_h), V.data_ptr(), Np, Cv, route, None, 0, None, 0, C.byref(nchunk)) == 0
    nch = nchunk.value
    part = torch.full((nblk, nch, n128, 2, Cv), float("nan"), dtype=torch.float64, device="cuda")
    s32n = nblk * 2 * len(fold_len) * n128 * 128
    S32 = torch.full((s32n,), 0x7FC00000, dtype=torch.int32, device="cuda")     # the bits of a float NaN
    rc = lib.rg_k_xy_i8(_stream(), pk.data_ptr(), pk_ld, n128 * pk_ld, nblk, n128, _ptr(bs_h), _ptr(nm_h), len(fold_len), _ptr(fl_h),
                        V.data_ptr(), Np, Cv, route, S32.data_ptr(), s32n, part.data_ptr(), part.numel(), C.byref(nchunk))
    assert rc == 0
    torch.cuda.synchronize()
    return part.cpu().numpy(), nch


def _xy_case(seed, fold_len, bs, n128, miss_blocks, Cv, kinds, const_row=None):
    rng = np.random.default_rng(seed)
    start, plen, Np = _layout(fold_len)
    nblk = len(bs)
    pk_ld = Np // 4
    codes = rng.integers(0, 4, size=(nblk, n128, Np), dtype=np.uint8)      # rows past bs keep anything
    if const_row is not None:
        codes[0, const_row] = 0                                  # dosage 2 at every position
    nmiss = []
    for b in range(nblk):
        live = codes[b, :bs[b]]
        live[live == 1] = 3                                      # dosages 2, 1, 0 at 1/4, 1/4, 1/2
        if miss_blocks[b]:
            m = rng.random((bs[b], Np)) < 0.05
            if const_row is not None and b == 0:
                m[const_row] = False
            codes[b, :bs[b]][m] = 1
        nmiss.append(int((codes[b, :bs[b]] == 1).sum()))
    V = _v_columns(rng, Cv, Np, kinds)
    if const_row is not None:
        V[0] = -1.968996062992126                                # q = -(31 * 2^49 + 64 (2^49 - 1) / 127): digits -64 in planes 0..6
    c4 = codes.reshape(nblk, n128, Np // 4, 4).astype(np.uint8)
    pk = (c4[..., 0] | (c4[..., 1] << 2) | (c4[..., 2] << 4) | (c4[..., 3] << 6)).astype(np.uint8)
    pk_d = _dev(np.concatenate([pk.reshape(-1), np.zeros(16, np.uint8)]))     # 16 bytes of slack, as level 0 allocates
    del c4, pk
    V_d = _dev(V)
    got0, nch0 = _xy_call(pk_d, pk_ld, n128, bs, nmiss, fold_len, V_d, 0, Np)
    got1, nch1 = _xy_call(pk_d, pk_ld, n128, bs, nmiss, fold_len, V_d, 1, Np)
    assert nch0 == len(fold_len)
    cseg = np.concatenate([[f] * ((plen[f] + 4095) // 4096) for f in range(len(fold_len))])
    assert nch1 == cseg.size
    absV = np.abs(V)
    worst = [0.0, 0.0]
    for b in range(nblk):
        for f in range(len(fold_len)):
            sl = slice(start[f], start[f] + plen[f])
            cb = codes[b, :bs[b], sl]
            g0 = np.select([cb == 0, cb == 2], [2.0, 1.0], 0.0)
            mi = (cb == 1).astype(np.float64)
            r1 = got1[b, cseg == f].astype(np.longdouble).sum(axis=0)      # the chunk partials of the fold
            for st, Gm in ((0, g0), (1, mi)):
                if st == 1 and nmiss[b] == 0:
                    continue                                     # set 1 is neither written nor read for a block without missing calls
                ex = _exact_sums(Gm, V[:, sl])
                tabs = Gm @ absV[:, sl].T
                bar0 = 4e-15 * tabs + 2.0 ** -52 * plen[f] * absV.max(axis=1)[None, :]
                nc = min(4096, int(plen[f]))
                bar1 = nc * U / (1 - nc * U) * tabs
                e0 = np.abs((got0[b, f, :bs[b], st, :].astype(np.longdouble) - ex)).astype(np.float64)
                e1 = np.abs((r1[:bs[b], st, :] - ex)).astype(np.float64)
                assert np.all(np.isfinite(got0[b, f, :, st, :])) and np.all(np.isfinite(r1[:, st, :].astype(np.float64)))
                assert np.all(e0 <= bar0), ("route 0", b, f, st, _ratio(e0, bar0))
                assert np.all(e1 <= bar1), ("route 1", b, f, st, _ratio(e1, bar1))
                d01 = np.abs(got0[b, f, :bs[b], st, :].astype(np.longdouble) - r1[:bs[b], st, :]).astype(np.float64)
                assert np.all(d01 <= bar0 + bar1)
                # rows past bs read nothing: zeros on both routes
                assert np.all(got0[b, f, bs[b]:, st, :] == 0.0) and np.all(got1[b, cseg == f][:, bs[b]:, st, :] == 0.0)
                worst[0] = max(worst[0], _ratio(e0, bar0))
                worst[1] = max(worst[1], _ratio(e1, bar1))
    print("xy worst ratio to bar: route 0 %.3g, route 1 %.3g" % tuple(worst))


_KINDS = ["normal", "pow2_pos", "pow2_neg", "neg_max", "zero", "tiny", "lowdigit", "scale-150", "scale150", "scale-40", "scale75"]


@pytest.mark.parametrize("Cv,fold_len,bs,n128,miss", [
    (1, [1301, 2222], [77], 128, [True]),
    (13, [700, 1, 2049, 913, 300], [300, 129, 256], 384, [True, False, True]),
    (16, [123 + 37 * f for f in range(32)], [128], 128, [False]),
    (17, [999, 3001, 257, 1800, 640], [100, 250, 1], 256, [False, True, False]),
    (53, [4500, 2900], [200, 31, 384], 384, [True, True, False]),
])
def test_xy_i8_both_routes_match_exact_sums(Cv, fold_len, bs, n128, miss):
    kinds = _KINDS[2:] if Cv == 1 else _KINDS
    _xy_case(1000 + Cv, fold_len, bs, n128, miss, Cv, kinds)


def test_xy_i8_long_fold_near_the_int32_bound():
    """A fold of 4,194,401 samples with a row of dosage 2 against a constant column whose digits are -64 in planes 0..6: each of those
    per-plane sums is -128 n_fold, within a factor of 4 of the int32 bound 64 * 2 * n_fold < 2^31 that xy_i8.hip states."""
    fold_len = [4194401, 3000]
    assert 128 * ((fold_len[0] + 255) // 256 * 256) >= 2 ** 29
    _xy_case(7, fold_len, [5], 128, [True], 3, ["normal", "neg_max", "tiny"], const_row=0)


# ---- the weighted Gram ----------------------------------------------------------------------------------------------------------

def _bf16_rne(x32):
    u = x32.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32)


def _sum_chunks(f, n, step=2048):
    """sum over position chunks of f(slice) (L x L), added with TwoSum: the chunks' fp64 matmuls are the only rounding of note."""
    s = c = None
    for p0 in range(0, n, step):
        t = f(slice(p0, min(n, p0 + step)))
        if s is None:
            s, c = t, np.zeros_like(t)
            continue
        a = s + t
        bp = a - s
        c += (s - (a - bp)) + (t - bp)
        s = a
    return s + c


def _wgram_call(W_d, Np, L, w_d, nchain, fold_len, slots, excl_own, fmt):
    lib = load_library()
    n64 = (L + 63) // 64 * 64
    out = torch.full((len(slots), n64 + 64, n64), float("nan"), dtype=torch.float64, device="cuda")
    fl, sc = _i64(fold_len), _i32(slots)
    ns = C.c_int32(-1)
    rc = lib.rg_k_wgram(_stream(), W_d.data_ptr(), Np, L, 1, 0, w_d.data_ptr(), nchain, len(fold_len), _ptr(fl), _ptr(sc), len(slots),
                        excl_own, fmt, out.data_ptr(), C.byref(ns))
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()[:, :L, :L], ns.value


def _wgram_case(N, L, K, slots, excl_own, seed, spike=False):
    rng = np.random.default_rng(seed)
    fold_len = [int(x) for x in np.diff(np.round(np.linspace(0, N, K + 1)).astype(int))]
    if K > 1 and not spike:                                      # unequal folds, not multiples of 256
        fold_len[0] += 77
        fold_len[-1] -= 77
    start, plen, Np = _layout(fold_len)
    nchain = K if excl_own else max(slots) + 1
    X = rng.standard_normal((L, Np))
    pad = np.ones(Np, bool)
    for f in range(K):
        pad[start[f]:start[f] + fold_len[f]] = False
    if spike:
        w = np.full((nchain, Np), 0.25)
        X *= 0.5
        R = min(200, L - 1)
        X[R] = 2.0 * 1019 * 2.0 ** -16                             # v = 1019 * 2^-16, v^2 = 0.99 * 2^-12
        X[R, :64] = 64.0                                          # v = 32: sum 2^16 in the first chunk
    else:
        w = np.exp(rng.uniform(np.log(1e-10), np.log(0.25), size=(nchain, Np)))
        w[rng.random((nchain, Np)) < 0.05] = 0.0                 # masked samples
    w[:, pad] = 0.0                                               # padding positions carry zero weights
    W_d, w_d = _dev(X), _dev(w)
    res = {fmt: _wgram_call(W_d, Np, L, w_d, nchain, fold_len, slots, excl_own, fmt) for fmt in (0, 1, 2)}
    del W_d, w_d
    lower = (np.arange(L)[:, None] // 64) >= (np.arange(L)[None, :] // 64)      # the lower 64 x 64 tiles
    diag_tile = (np.arange(L)[:, None] // 256) == (np.arange(L)[None, :] // 256)
    worst = {}
    for s, ch in enumerate(slots):
        keep = np.ones(Np, bool)
        if excl_own:
            keep[start[ch]:start[ch] + plen[ch]] = False
        Xk, wk = X[:, keep], w[ch, keep]
        n = Xk.shape[1]
        Xw = Xk * wk
        H = _sum_chunks(lambda q: Xw[:, q] @ Xk[:, q].T, n)
        Habs = np.abs(Xw) @ np.abs(Xk).T
        del Xw
        v = Xk * np.sqrt(wk)
        del Xk
        v32 = v.astype(np.float32)
        v16 = v32.astype(np.float16).astype(np.float64)
        hi = _bf16_rne(v32)
        lo = _bf16_rne((v32 - hi).astype(np.float32)).astype(np.float64)
        hi = hi.astype(np.float64)
        for fmt in (0, 1, 2):
            got, ns = res[fmt]
            g = got[s]
            assert np.all(np.isfinite(g[lower]))
            if fmt == 0:
                err, bar = np.abs(g - H), 1e-13 * Habs
            else:
                if fmt == 1:
                    He = v16 @ v16.T
                    Sa = np.abs(v16) @ np.abs(v16).T
                    av = np.abs(v).sum(axis=1)
                    sanity = (2.0 ** -10 + 2.0 ** -20) * (np.abs(v) @ np.abs(v).T) + 2.0 ** -24 * (av[:, None] + av[None, :]) + n * 2.0 ** -48
                else:
                    He = hi @ hi.T + hi @ lo.T + lo @ hi.T + np.where(diag_tile, lo @ lo.T, 0.0)
                    Sa = np.abs(hi) @ np.abs(hi).T + np.abs(hi) @ np.abs(lo).T + np.abs(lo) @ np.abs(hi).T
                    sanity = 2.0 * 2.0 ** -11 * (np.abs(v) @ np.abs(v).T)
                assert np.all(np.abs(He - H) <= sanity), ("emulation", fmt, _ratio(np.abs(He - H), sanity))
                err, bar = np.abs(g - He), 2.0 ** -14 * Sa
            ok = err[lower] <= bar[lower]
            assert np.all(ok), ("fmt", fmt, "slot", s, _ratio(err[lower], bar[lower]))
            if fmt:
                assert ns >= 1
                if N >= 500000:
                    assert ns > 1, "the largest case must take more than one K slice"
            worst[fmt] = max(worst.get(fmt, 0.0), _ratio(err[lower], bar[lower]))
    print("wgram N=%d L=%d worst ratio to bar:" % (N, L), worst)


@pytest.mark.parametrize("N,L,K,slots,excl_own", [
    (6500, 64, 2, [1], 1),
    (6500, 300, 5, [3, 0, 4], 1),
    (6500, 513, 10, [7, 2, 9, 0, 5], 1),
    (6500, 513, 1, [0], 0),              # leave-one-out form: one chain over every position
    (6500, 2560, 5, [4, 1], 1),
    (50000, 300, 5, [2, 4, 0], 1),
    (50000, 64, 10, [9, 3], 1),
])
def test_weighted_gram_formats(N, L, K, slots, excl_own):
    _wgram_case(N, L, K, slots, excl_own, seed=N + L + K)


def test_weighted_gram_500k_flush():
    """500,000 positions, L = 256, two chains over all positions: 16 K slices; the spike row makes a missing fp32 flush visible."""
    _wgram_case(500000, 256, 2, [1, 0], 0, seed=5, spike=True)


# ---- level-0 route sweep --------------------------------------------------------------------------------------------------------

def _sweep_data(tmp_path, N, M, chroms, P, miss_blocks, seed):
    g = synth_dosages(M, N, miss_rate=0.0, seed=seed)
    r0 = 0
    for (nb, miss) in miss_blocks:                                # missing calls in some blocks only
        if miss:
            g[r0:r0 + nb] = synth_dosages(nb, N, miss_rate=0.03, seed=seed + 1 + r0)
        r0 += nb
    pre = str(tmp_path / "sw")
    write_plink(pre, g, chroms, P=P, ncov=2, seed=seed, missing_pheno=0.04)
    return pre


@pytest.mark.parametrize("R0,P,K,bs,N,blocks", [
    (8, 2, 5, 300, 1500, [(300, True), (300, False), (150, False)]),       # P R0 = 16: VALU route
    (8, 3, 2, 300, 1500, [(300, False), (200, True)]),                     # 24 rows: digit route, one group
    (8, 9, 10, 256, 2000, [(256, True), (256, False), (100, True)]),       # 72 rows: two groups, the last with one phenotype
    (1, 17, 32, 300, 4000, [(300, False), (250, True)]),                   # P R0 = 17
    (3, 22, 5, 200, 1800, [(200, True), (200, False), (120, False)]),      # pg = 21: two groups
    (7, 10, 3, 280, 1600, [(280, False), (280, True), (33, False)]),
    (5, 4, 5, 1024, 1200, [(1024, True), (1024, False), (300, False)]),    # n128 = 1024: the last width of the i8 prediction route
    (5, 4, 5, 1025, 1200, [(1025, False), (1025, True)]),                  # n128 = 1152: past it
    (2, 9, 2, 400, 2500, [(400, False), (400, True), (400, False)]),
    (4, 6, 32, 350, 5000, [(350, True), (200, False)]),
])
def test_level0_route_sweep(tmp_path, monkeypatch, R0, P, K, bs, N, blocks):
    sizes = [nb for nb, _ in blocks]
    M = sum(sizes)
    chroms = np.repeat(np.arange(1, len(sizes) + 1), sizes)         # one block per chromosome
    pre = _sweep_data(tmp_path, N, M, chroms, P, blocks, seed=R0 * 100 + P)
    # R0 = 1 only through an explicit --l0 value (a count of ridge values must be at least 2)
    ridge = dict(setl0=[0.5]) if R0 == 1 else dict(n_ridge_l0=R0)
    opt = orc.Step1Options(bed=pre, pheno_file=pre + ".pheno", covar_file=pre + ".covar", bsize=bs, cv_folds=K, **ridge)
    ref, got = _compare(opt)
    for env in ("RG_PRED_F64", "RG_XY_F64"):
        monkeypatch.setenv(env, "1")
        other = gpu_step1(opt)
        monkeypatch.delenv(env)
        for ph in range(P):
            e = rel_err(got["W"][ph], other["W"][ph])
            assert e < 1e-12, (env, ph, e)
