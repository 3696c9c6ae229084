"""rg_s2_qt_rerint (include/rg_step2.h, regenie_amd/csrc/step2_rerint.hip) through regenie_amd.step2 against the NumPy restatement
(tests/rerint_restate.py).

Shapes: n = 63 (below a sort tile of 2,048 keys and below a wave), 257, 1,031, 4,099 (three tiles after padding to 8,192: the global steps and the
merge kernel run) -- none a multiple of 64 or 256; P = 1 and 3 with a mask per trait; C = 1, 5, 33.  Traits: 0 all values distinct but for a -0.0 and a +0.0, which tie, 1 distinct but
for ONE block of tied values, 2 values on a grid of 7 (many blocks).

Tolerance (profiles/rerint.md): SciPy's and the standard library's normal quantile -- two fp64 routines for the same function -- differ by at most
1.04e-15 relative over every rank and half-rank at n = 500,000 (7.8e-16 at n = 4,099); the device gets one decimal order over that: 1.04e-14.
  ranks                     exact
  --apply-rerint values     elementwise relative (a quantile divided by two norms)
  --apply-rerint-cov values relative to the trait's largest |value|: res - X beta cancels, the rounding is that of the operands
  scale_Y, scf_sv           relative"""
import numpy as np
import pytest

from tests import rerint_restate as rr

pytestmark = pytest.mark.gpu
TOL = 1.04e-14


def _problem(n, C, P, seed=0):
    """-> X [C][n], res0 [P][n] (masked), mask [P][n]"""
    rng = np.random.default_rng(seed + 1000 * n + 10 * C + P)
    X = np.linalg.qr(np.column_stack([np.ones(n), rng.normal(size=(n, C - 1))]))[0].T.copy()
    mask = np.ones((P, n), np.uint8)
    for t in range(P):
        mask[t, rng.random(n) < 0.03 * (t + 1)] = 0
    Y = rng.normal(size=(P, n))
    obs0 = np.flatnonzero(mask[0])
    Y[0, obs0[1]], Y[0, obs0[-2]] = -0.0, 0.0                                  # a signed zero is a zero: the two tie (the reference compares with ==)
    if P > 1:
        obs = np.flatnonzero(mask[1])
        Y[1, rng.choice(obs, max(3, n // 10), replace=False)] = 0.25         # one block of ties
    if P > 2:
        Y[2] = rng.integers(-3, 4, n) / 4.0                                   # every value tied with many others
    return X, Y * mask, mask


_cache = {}


def _restated(n, C, P, mode):
    key = (n, C, P, mode)
    if key not in _cache:
        X, res0, mask = _problem(n, C, P)
        _cache[key] = (X, res0, mask, rr.transform(res0.T, X.T, mask.T, mode))
        for a in _cache[key][:3]:
            a.setflags(write=False)
    return _cache[key]


def _device(n, C, P, mode, X, res0, mask):
    from regenie_amd.step2 import Step2QT
    with Step2QT(n, C, P) as s2:
        s2.set_null(X, res0, mask, np.zeros(P))
        return s2.rerint(mode)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("P,C", [(1, 1), (3, 5), (3, 33)])
@pytest.mark.parametrize("n", [63, 257, 1031, 4099])
def test_entry_against_restatement(n, P, C, mode):
    X, res0, mask, want = _restated(n, C, P, mode)
    got = _device(n, C, P, mode, X, res0, mask)
    assert np.array_equal(got["ranks"], want["ranks"].T)
    for key in ("scale_Y", "scf_sv"):
        dev = float(np.max(np.abs(got[key] - want[key]) / np.abs(want[key])))
        print("n=%d P=%d C=%d mode=%d %s: max relative deviation %.3g" % (n, P, C, mode, key, dev))
        assert dev <= TOL, (key, dev)
    w = want["res"].T
    assert not got["res"][mask == 0].any()
    if mode == 1:
        nz = w != 0
        assert not got["res"][~nz].any()                                       # the median of an odd count: u = 1 / 2 exactly
        dev = float(np.max(np.abs(got["res"][nz] - w[nz]) / np.abs(w[nz])))
    else:
        dev = float(np.max(np.abs(got["res"] - w) / np.abs(w).max(axis=1, keepdims=True)))
    print("n=%d P=%d C=%d mode=%d res: max deviation %.3g" % (n, P, C, mode, dev))
    assert dev <= TOL, dev


@pytest.mark.parametrize("n", [257, 4099])
def test_a_second_call_gives_the_same_bytes_and_sample_order_does_not_matter(n):
    X, res0, mask, _ = _restated(n, 5, 3, 2)
    a, b = _device(n, 5, 3, 2, X, res0, mask), _device(n, 5, 3, 2, X, res0, mask)
    for key in ("res", "ranks", "scale_Y", "scf_sv"):
        assert a[key].tobytes() == b[key].tobytes(), key
    perm = np.random.default_rng(3).permutation(n)
    c = _device(n, 5, 3, 1, np.ascontiguousarray(X[:, perm]), np.ascontiguousarray(res0[:, perm]), np.ascontiguousarray(mask[:, perm]))
    d = _device(n, 5, 3, 1, X, res0, mask)
    assert np.array_equal(c["ranks"], d["ranks"][:, perm])


@pytest.mark.parametrize("n", [63, 4099])
def test_a_constant_trait_is_the_sd_error_not_a_fault(n):
    from regenie_amd.engine import RgError
    from regenie_amd.step2 import Step2QT
    X, res0, mask = (a.copy() for a in _problem(n, 5, 3))
    res0[1] = 0.75 * mask[1]                                                  # every observed value of trait 1 equal
    with Step2QT(n, 5, 3) as s2:
        s2.set_null(X, res0, mask, np.zeros(3))
        with pytest.raises(RgError, match="some phenotype residuals has sd=0."):
            s2.rerint(1)
        with pytest.raises(RgError, match="rg_s2_set_null has not been called"):      # the null model is gone until the next set_null
            s2.score_block(np.zeros((1, n)))
        s2.set_null(X, _problem(n, 5, 3)[1], mask, np.zeros(3))
        assert np.isfinite(s2.rerint(1)["res"]).all()


def _pack(G):
    bs, n = G.shape
    code = np.where(np.isnan(G), 1, np.where(G == 2, 0, np.where(G == 1, 2, 3))).astype(np.uint8)
    code = np.concatenate([code, np.zeros((bs, (-n) % 4), np.uint8)], axis=1).reshape(bs, -1, 4)
    return (code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6)).astype(np.uint8)


@pytest.mark.parametrize("mode", [1, 2])
def test_a_block_scored_after_the_call(mode):
    """The three block entries after rg_s2_qt_rerint against the same entries on a fresh context whose set_null was handed (a) the residuals and
    scf_sv the call returned: the same bytes -- the context holds what it reported, res^T X included; (b) the restatement's: stats and bhat within
    1e-13 of the largest |value|.  The residuals may differ by 1.04e-14 of theirs (TOL); were every one off by that much, a statistic -- n = 1,031
    products with a unit-norm vector -- would move by sqrt(n) x 1.04e-14 x max |res| ~ 4 = 1.4e-12.  The residuals measured at 1.5e-15, seven times
    below TOL, put that at 2e-13; the bound sits under it, near enough to the 5e-16 measured to catch a res^T X that is off in a small entry."""
    from regenie_amd.step2 import Step2QT
    n, C, P, bs = 1031, 5, 3, 24
    X, res0, mask, want = _restated(n, C, P, mode)
    rng = np.random.default_rng(11)
    G = rng.binomial(2, rng.uniform(0.05, 0.5, size=bs)[:, None], size=(bs, n)).astype(np.float64)
    G[rng.random(G.shape) < 0.01] = np.nan
    rows = _pack(G)
    G16 = np.where(np.isnan(G), 0xFFFF, G * 255).astype(np.uint16)

    def score(s2):
        return [s2.score_block(G), s2.score_block_packed(rows), s2.score_block_int(G16, 255)]

    with Step2QT(n, C, P) as s2:
        s2.set_null(X, res0, mask, np.zeros(P))
        t = s2.rerint(mode)
        after = score(s2)
    with Step2QT(n, C, P) as s2:
        s2.set_null(X, t["res"], mask, t["scf_sv"])
        same = score(s2)
        s2.set_null(X, want["res"].T, mask, want["scf_sv"])
        restated = score(s2)
    for a, b, c in zip(after, same, restated):
        for key in ("stats", "bhat", "scale_fac", "ignored"):
            assert a[key].tobytes() == b[key].tobytes(), key
        for key in ("stats", "bhat"):
            assert np.array_equal(np.isnan(a[key]), np.isnan(c[key]))
            dev = float(np.nanmax(np.abs(a[key] - c[key])) / np.nanmax(np.abs(c[key])))
            print("mode %d %s: deviation from the restatement's block %.3g of the largest value" % (mode, key, dev))
            assert dev <= 1e-13, (key, dev)


def test_arguments_are_checked():
    """The entry needs a null model, and a mode outside the two is refused."""
    from regenie_amd.engine import RgError
    from regenie_amd.step2 import Step2QT
    with Step2QT(63, 1, 1) as s2:
        with pytest.raises(RgError, match="rg_s2_set_null has not been called"):
            s2.rerint(1)
        X, res0, mask = _problem(63, 1, 1)
        s2.set_null(X, res0, mask, np.zeros(1))
        with pytest.raises(RgError, match="mode must be"):
            s2.rerint(3)
