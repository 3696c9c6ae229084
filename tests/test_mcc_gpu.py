"""rg_s2_qt_moments (include/rg_step2.h, regenie_amd/csrc/step2_mcc.hip) through regenie_amd.step2 against np.longdouble sums of the vector formed
in NumPy: S_k = sum_i mask_t(i) r(i)^k (k = 1..6) and r . yres_t, r = the mean-imputed raw genotype of a variant check_sparse_G calls sparse,
(g~ - X X^T g~) / scale_fac otherwise -- with the mean, verdict and scale_fac the score call returned.

Bound (derived, not measured): for S_k, 4 (n + k (C + 4)) 2^-53 sum_i mask |r_i|^k -- first-order summation error (n terms) plus the propagation of
the rounding of c = X b (C FMAs, b itself a rounded sum) and of the subtraction, scale division and powers (the + 4) into r^k (factor k), with 4x
headroom; for r . yres the same with k = 1 and sum |r_i yres_i|.  The bound is asserted for the kernel as it stands.  The same sums in plain
float64 NumPy (another order) are printed next to it: they use at most 0.02 of the bound on every row but one kind -- the singleton counted on the
other allele (flip: all calls 2 but one, a dense row that lies almost in the span of the intercept), where |r| is a 1 / n share of |g~| and the
rounding of g~ - X b is relative to |g~|, not to |r| as the bound assumes: float64 NumPy is 0.99 to 13 times the bound there (n = 259 to 4100),
the kernel 0.06 to 0.11 of it (MI355X).  For such rows the bound is too tight by the ratio |g~| / |r|; it is not loosened here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LD = np.longdouble
EPS = 2.0 ** -53


def _pack(G):
    """hard calls (NaN missing) -> .bed rows: 00 -> 2, 01 -> missing, 10 -> 1, 11 -> 0"""
    bs, n = G.shape
    code = np.where(np.isnan(G), 1, np.where(G == 2, 0, np.where(G == 1, 2, 3))).astype(np.uint8)
    code = np.concatenate([code, np.zeros((bs, (-n) % 4), np.uint8)], axis=1).reshape(bs, -1, 4)
    return (code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6)).astype(np.uint8)


def _problem(n, C, P, bs, masked, seed):
    rng = np.random.default_rng(seed)
    X = np.linalg.qr(np.column_stack([np.ones(n), rng.normal(size=(n, C - 1))]))[0].T.copy()      # [C][n]
    mask = np.ones((P, n), np.uint8)
    if masked:
        for t in range(P):
            mask[t, rng.random(n) < 0.04 * (t + 1)] = 0
    Y = rng.normal(size=(P, n)) * mask
    maf = rng.uniform(0.05, 0.5, size=bs)
    maf[::3] = rng.uniform(0.3, 0.5, size=len(maf[::3]))       # dense rows (more than n / 2 non-zero calls) among the sparse ones
    G = rng.binomial(2, maf[:, None], size=(bs, n)).astype(np.float64)
    G[rng.random(G.shape) < 0.01] = np.nan                     # rows with missing calls
    if bs >= 8:
        G[1] = 0.0                                             # monomorphic (ignored)
        G[2] = np.nan                                          # all missing (ignored)
        G[3] = 0.0; G[3, n // 3] = 1.0                         # a singleton
        G[4] = 0.0; G[4, rng.choice(n, n // 2, replace=False)] = 1.0      # floor(n * 0.5) non-zero entries; at the even n = 4100 exactly n * 0.5: the boundary of the rule (<=: sparse)
        G[5] = 0.0; G[5, rng.choice(n, n // 2 + 1, replace=False)] = 2.0  # one more: dense
    return X, Y, mask, G


def _reference(G, X, Y, mask, mean, sf, sparse):
    """-> sums [bs][P][7] and their absolute-value counterparts, np.longdouble"""
    bs, n = G.shape
    P = Y.shape[0]
    Xl, out, mag = X.astype(LD), np.zeros((bs, P, 7), LD), np.zeros((bs, P, 7), LD)
    for j in range(bs):
        g = np.where(np.isnan(G[j]), LD(mean[j]), G[j].astype(LD))
        r = g if sparse[j] else (g - Xl.T @ (Xl @ g)) / LD(sf[j])
        for t in range(P):
            m = mask[t].astype(LD)
            for k in range(1, 7):
                out[j, t, k - 1] = (m * r ** k).sum()
                mag[j, t, k - 1] = (m * np.abs(r) ** k).sum()
            out[j, t, 6] = (r * Y[t].astype(LD)).sum()
            mag[j, t, 6] = np.abs(r * Y[t].astype(LD)).sum()
    return out, mag


def _check(res, sums, G, X, Y, mask, flip=False):
    bs, n = G.shape
    C = X.shape[0]
    Gc = np.where(np.isnan(G), np.nan, 2.0 - G) if flip else G
    keep = np.flatnonzero(res["ignored"] == 0)
    assert 0 < len(keep)
    if bs >= 8:
        assert res["ignored"][2] == 1      # (the monomorphic row is ignored only where it is dense: all calls 2 after the flip)
    sparse = res["scale_fac"] == 1.0
    nz = np.array([np.count_nonzero(np.where(np.isnan(Gc[j]), res["mean"][j], Gc[j])) for j in range(bs)])
    assert np.array_equal(sparse[keep], (nz <= n * 0.5)[keep])
    want, mag = _reference(Gc, X, Y, mask, res["mean"], res["scale_fac"], sparse)
    worst, worst64, fails = 0.0, 0.0, []
    for j in keep:
        rf = np.where(np.isnan(Gc[j]), res["mean"][j], Gc[j])
        r64 = rf if sparse[j] else (rf - X.T @ (X @ rf)) / res["scale_fac"][j]
        for t in range(Y.shape[0]):
            for k in range(7):
                kk = 1 if k == 6 else k + 1
                bound = 4 * (n + kk * (C + 4)) * EPS * float(mag[j, t, k])
                err = abs(float(LD(sums[j, t, k]) - want[j, t, k]))
                np64 = (r64 * Y[t]).sum() if k == 6 else (mask[t] * r64 ** kk).sum()
                e64 = abs(float(LD(np64) - want[j, t, k]))
                if bound > 0:
                    worst, worst64 = max(worst, err / bound), max(worst64, e64 / bound)
                if err > bound:
                    fails.append((int(j), t, k, err, bound, e64))
    print("  float64 NumPy in another order: worst error / bound %.3f (above 0.25 the bound itself is too tight for the row, see the docstring)" % worst64)
    assert not fails, fails[:5]
    return worst


@pytest.mark.parametrize("n,C,P,bs,masked", [(259, 1, 1, 1, False), (259, 6, 3, 37, True), (1003, 33, 3, 37, True), (1003, 6, 1, 37, False),
                                             (4100, 6, 3, 37, True)])
@pytest.mark.parametrize("flip", [False, True])
def test_moments_packed(n, C, P, bs, masked, flip):
    from regenie_amd.step2 import Step2QT
    X, Y, mask, G = _problem(n, C, P, bs, masked, seed=n + C + bs)
    with Step2QT(n, C, P) as s2:
        s2.set_null(X, Y, mask, np.ones(P))
        res = s2.score_block_packed(_pack(G), flip=flip)
        a = s2.qt_moments(np.arange(bs))["sums"]
        b = s2.qt_moments(np.arange(bs))["sums"]
        sub = s2.qt_moments(np.arange(bs)[::-1][:3])["sums"]
    assert a.tobytes() == b.tobytes()                                # two identical calls, identical bits
    assert sub.tobytes() == a[::-1][:3].tobytes()                    # a row's sums do not depend on the list
    worst = _check(res, a, G, X, Y, mask, flip)
    print("packed n=%d C=%d P=%d bs=%d flip=%d: worst error / bound %.3f" % (n, C, P, bs, flip, worst))


@pytest.mark.parametrize("n,C,P,bs,masked", [(259, 6, 3, 37, True), (1003, 33, 3, 37, True), (1003, 1, 1, 1, False)])
def test_moments_fp64_rows(n, C, P, bs, masked):
    from regenie_amd.step2 import Step2QT
    X, Y, mask, G = _problem(n, C, P, bs, masked, seed=7 * n + C)
    with Step2QT(n, C, P) as s2:
        s2.set_null(X, Y, mask, np.ones(P))
        res = s2.score_block(G)
        a = s2.qt_moments(np.arange(bs))["sums"]
        b = s2.qt_moments(np.arange(bs))["sums"]
    assert a.tobytes() == b.tobytes()
    print("fp64 n=%d C=%d: worst error / bound %.3f" % (n, C, _check(res, a, G, X, Y, mask)))


@pytest.mark.parametrize("n,C,P,bs,masked,scale", [(259, 6, 3, 37, True, 255), (1003, 33, 3, 37, True, 16384), (1003, 6, 1, 1, False, 255)])
def test_moments_integer_dosages(n, C, P, bs, masked, scale):
    from regenie_amd.step2 import Step2QT
    X, Y, mask, G = _problem(n, C, P, bs, masked, seed=11 * n + C)
    rng = np.random.default_rng(5)
    q = np.where(np.isnan(G), 0xFFFF, np.clip(np.nan_to_num(G) * scale - (rng.integers(0, scale // 4, G.shape) * (np.nan_to_num(G) == 1)), 0, 2 * scale)).astype(np.uint16)
    Gd = np.where(q == 0xFFFF, np.nan, q.astype(np.float64) / scale)
    with Step2QT(n, C, P) as s2:
        s2.set_null(X, Y, mask, np.ones(P))
        res = s2.score_block_int(q, scale)
        a = s2.qt_moments(np.arange(bs))["sums"]
        b = s2.qt_moments(np.arange(bs))["sums"]
    assert a.tobytes() == b.tobytes()
    print("int n=%d C=%d scale=%d: worst error / bound %.3f" % (n, C, scale, _check(res, a, Gd, X, Y, mask)))


def test_moments_need_a_scored_block():
    from regenie_amd.engine import RgError
    from regenie_amd.step2 import Step2QT
    X, Y, mask, G = _problem(259, 3, 1, 4, False, seed=1)
    with Step2QT(259, 3, 1) as s2:
        s2.set_null(X, Y, mask, np.ones(1))
        with pytest.raises(RgError):
            s2.qt_moments([0])
        s2.score_block_packed(_pack(G))
        with pytest.raises(RgError):
            s2.qt_moments([4])
        assert s2.qt_moments([3])["sums"].shape == (1, 1, 7)
        s2.set_columns(X)                      # another entry reuses the staging buffers: the scored block is gone
        s2.contract_packed(_pack(G))
        with pytest.raises(RgError):
            s2.qt_moments([0])
        s2.score_block_packed(_pack(G))
        s2.set_null(X, Y, mask, np.ones(1))    # ... and so it is under a new null model
        with pytest.raises(RgError):
            s2.qt_moments([0])
