"""rg_s2_set_coding (include/rg_step2.h: `--test dominant | recessive` behind the C ABI) through regenie_amd.step2, against the NumPy fp64
restatement of tests/dom_rec_cases.py (recode, then the formulas in the header of rg_step2.h; tests/test_dom_rec_cpu.py holds it to regenie's own
files) and, for binary traits, the oracle's score test on the recoded vector.  Shapes: the smallest that reach every decode path -- 257 samples (no
multiple of 4 or 64), 70 rows, 3 covariates, 3 traits with different masks, rows that are all missing, rows without a homozygote, a row without a
non-reference call, both values of flip.  Tolerances: those of the additive path (tests/test_step2_qt_gpu.py RTOL, tests/test_step2_bt_gpu.py)."""
import numpy as np
import pytest

from tests import dom_rec_cases as dc

pytestmark = pytest.mark.gpu
RTOL = 1e-9         # tests/test_step2_qt_gpu.py
N, BS, C, P = 257, 70, 3, 3


def _pack(G):
    bs, n = G.shape
    code = np.where(np.isnan(G), 1, np.where(G == 2, 0, np.where(G == 1, 2, 3))).astype(np.uint8)
    code = np.concatenate([code, np.zeros((bs, (-n) % 4), np.uint8)], axis=1).reshape(bs, -1, 4)
    return (code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6)).astype(np.uint8)


@pytest.fixture(scope="module")
def problem():
    from oracle import regenie_step2_qt as s2o
    rng = np.random.default_rng(31)
    X = np.linalg.qr(np.column_stack([np.ones(N), rng.normal(size=(N, C - 1))]))[0]
    mask = (rng.random((N, P)) > np.array([0.0, 0.08, 0.2])).astype(np.float64)      # trait 0 complete, the others differ
    Y = rng.normal(size=(N, P))
    Y = (Y - X @ (X.T @ Y)) * mask
    res, _, scf = s2o.compute_res(Y, 0.1 * rng.normal(size=(N, P)) * mask, mask, mask.sum(axis=0), C, np.ones(P))
    maf = np.concatenate([rng.uniform(0.15, 0.9, size=BS // 2), rng.uniform(0.01, 0.08, size=BS - BS // 2)])      # rows that are dense and rows that are sparse under every coding and flip
    G = rng.binomial(2, maf[:, None], size=(BS, N)).astype(np.float64)
    G[rng.random(G.shape) < 0.03] = np.nan
    G[3, :] = np.nan                                      # all missing
    G[40, :] = np.nan
    G[5] = np.where(G[5] == 2, 1.0, G[5])                 # no homozygote of the counted allele (recessive: an all-zero vector)
    G[41] = np.where(G[41] == 2, 0.0, G[41])
    G[6] = np.where(np.isnan(G[6]), np.nan, 0.0)          # no non-reference call at all
    G[7] = np.where(np.isnan(G[7]), np.nan, 2.0)          # every call homozygous (with flip: the all-zero row)
    return X, res, mask, scf, G


def _check_qt(got, counts, want, bs):
    assert np.array_equal(counts[:, :3], want["counts"][:, :3])
    assert np.array_equal(got["n_obs"], N - want["counts"][:, 2])
    assert np.array_equal(got["n_obs_p"], want["n_obs_p"]) and np.array_equal(got["total_p"], want["total_p"])
    obs = got["n_obs"] > 0
    assert np.array_equal(got["ignored"][~obs], np.ones((~obs).sum(), np.int32))
    assert np.allclose(got["mean"][obs], want["mean"][obs], rtol=1e-13)
    ok = obs & (got["ignored"] == 0)
    assert np.array_equal(ok, ~np.isnan(want["scale_fac"]) & ~(want["scale_fac"] < 1e-6))
    assert np.allclose(got["scale_fac"][ok], want["scale_fac"][ok], rtol=1e-11)
    for k, w in (("stats", "stats_all"), ("bhat", "bhat_all")):
        scale = np.nanmax(np.abs(want[w][ok]))
        assert np.allclose(got[k][ok], want[w][ok], rtol=RTOL, atol=RTOL * scale, equal_nan=True), k      # NaN: an all-zero vector on the sparse branch (0 / 0)
    # not vacuous: most rows are scored (a rare variant counted from the other allele is all ones under the dominant coding: ignored), on both branches
    assert ok.sum() > bs // 2 and want["sparse"][ok].any() and not want["sparse"][ok].all()


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("coding", [1, 2])
def test_qt_packed_under_a_coding_against_the_restatement(problem, coding, flip):
    from regenie_amd.step2 import Step2QT
    X, res, mask, scf, G = problem
    want = dc.qt_block(2.0 - G if flip else G, coding, X, res, mask, scf, filters=False)
    with Step2QT(N, C, P) as s2:
        s2.set_null(X.T, res.T, mask.T, scf)
        s2.set_coding(coding)
        got = s2.score_block_packed(_pack(G), flip=flip)
        counts = s2.packed_counts(BS)
    _check_qt(got, counts, want, BS)
    hom = counts[:, 1]                                    # the count `--minHOMs` compares: homozygotes of the allele counted under flip
    assert np.array_equal(hom, ((2.0 - G if flip else G) == 2).sum(axis=1)) and (hom == 0).any() and (hom > 0).any()


@pytest.mark.parametrize("coding", [1, 2])
def test_qt_packed_under_a_coding_with_every_trait_observed(problem, coding):
    """Masks of ones: the library takes the per-trait counts from the variant's (no pass over the masks)."""
    from regenie_amd.step2 import Step2QT
    X, res, mask, scf, G = problem
    ones = np.ones_like(mask)
    res1 = res * 1.0          # (any residual is a valid input: the statistic is compared with the restatement on the same numbers)
    want = dc.qt_block(G, coding, X, res1, ones, scf, filters=False)
    with Step2QT(N, C, P) as s2:
        s2.set_null(X.T, res1.T, ones.T, scf)
        s2.set_coding(coding)
        got = s2.score_block_packed(_pack(G))
        counts = s2.packed_counts(BS)
    _check_qt(got, counts, want, BS)


def test_additive_bits_do_not_depend_on_the_new_entry(problem):
    """A context that never calls rg_s2_set_coding, one that sets RG_S2_ADDITIVE, and one that comes back to it from another coding: identical bits."""
    from regenie_amd.step2 import ADDITIVE, RECESSIVE, Step2QT
    X, res, mask, scf, G = problem
    rows = _pack(G)
    out = []
    for mode in ("never", "set", "back"):
        with Step2QT(N, C, P) as s2:
            s2.set_null(X.T, res.T, mask.T, scf)
            if mode == "set":
                s2.set_coding(ADDITIVE)
            if mode == "back":
                s2.set_coding(RECESSIVE)
                s2.score_block_packed(rows)
                s2.set_coding(ADDITIVE)
            out.append((s2.score_block_packed(rows), s2.score_block_packed(rows, flip=True)))
    for other in out[1:]:
        for a, b in zip(out[0], other):
            for k in ("stats", "bhat", "scale_fac", "mean", "n_obs", "ignored", "total_p", "n_obs_p"):
                assert a[k].tobytes() == b[k].tobytes(), k
    want = dc.qt_block(G, 0, X, res, mask, scf, filters=False)                      # and they are the additive test
    _check_qt(out[0][0], np.column_stack([(G == 1).sum(1), (G == 2).sum(1), np.isnan(G).sum(1), np.zeros(BS)]).astype(np.int32), want, BS)


@pytest.mark.parametrize("coding", [1, 2])
def test_contract_packed_under_a_coding(problem, coding):
    """sums / sq of the recoded row, counts additive; the bound is tests/test_step2_qt_gpu.py's for the additive contraction."""
    from regenie_amd.step2 import Step2QT
    _, _, _, _, G = problem
    rng = np.random.default_rng(9)
    ncol, nsq = 21, 3
    cols = rng.normal(size=(ncol, N)) * np.exp(rng.uniform(-6, 6, size=(ncol, 1)))
    with Step2QT(N, C, P) as s2:
        s2.set_columns(cols, nsq)
        s2.set_coding(coding)
        for flip in (False, True):
            Ge = 2.0 - G if flip else G
            got = s2.contract_packed(_pack(G), flip=flip)
            miss = np.isnan(Ge).astype(np.float64)
            g0 = np.nan_to_num(dc.recode(Ge, coding))
            assert np.array_equal(got["counts"][:, 0], (Ge == 1).sum(axis=1)) and np.array_equal(got["counts"][:, 1], (Ge == 2).sum(axis=1))
            assert np.array_equal(got["counts"][:, 2], miss.sum(axis=1).astype(np.int32)) and g0.max() == 1.0
            for name, want, have in (("g0", g0 @ cols.T, got["sums"][:, 0]), ("miss", miss @ cols.T, got["sums"][:, 1]), ("sq", (g0 * g0) @ cols[:nsq].T, got["sq"])):
                bound = (np.abs(g0) + miss) @ np.abs(cols[: want.shape[1]]).T + 1e-300
                assert (np.abs(have - want) <= 4e-15 * bound + 2.0 ** -52 * N * np.abs(cols[: want.shape[1]]).max(axis=1)[None, :]).all(), name


@pytest.mark.parametrize("coding", [1, 2])
def test_bt_score_and_corrections_under_a_coding(coding):
    """The binary-trait score test and both corrections on the recoded, mean-imputed vector (no flip_geno: Data.cpp:2108), against the oracle; counts,
    total_p and n_obs_p stay additive."""
    from oracle import regenie_step2_bt as bt
    from regenie_amd.step2 import BT_FIRTH_APPROX, BT_SPA, Step2QT
    from tests.test_step2_bt_gpu import _nulls, _problem
    n, bs = 1001, 24
    X, off, G, y, mask = _problem(17, n=n, C=3, P=2, bs=bs)
    G[:4] = np.where(np.isnan(G[:4]), np.nan, 2.0 - G[:4])            # rows whose additive mean exceeds 1: the additive test would flip them
    nulls, fo = _nulls(X, off, y, mask)
    fitted = np.array([nl["p"] for nl in nulls])
    R = dc.recode(G, coding)
    with Step2QT(n, 3, 2) as s2:
        s2.set_sparse_rule(n, 0.5, False)
        s2.bt_set_null(X.T, y.T, mask.T, fitted, firth_offset=fo)
        s2.set_coding(coding)
        got = s2.bt_score_packed(_pack(G))
        obs = ~np.isnan(G)
        assert np.array_equal(got["counts"][:, 0], (G == 1).sum(1)) and np.array_equal(got["counts"][:, 1], (G == 2).sum(1)) and np.array_equal(got["counts"][:, 2], (~obs).sum(1))
        pairs, gi = [], []
        for j in range(bs):
            mu = np.nanmean(R[j])
            g = np.where(obs[j], R[j], mu)
            gi.append(g)
            assert got["mean"][j] == pytest.approx(mu, rel=1e-12)
            sparse = int((g != 0).sum()) <= 0.5 * n
            assert bool(got["sparse"][j]) == sparse
            for q in range(2):
                m = mask[:, q]
                assert got["total_p"][j, q] == np.nansum(G[j][m]) - np.nansum(G[j]) and got["n_obs_p"][j, q] == int((obs[j] & m).sum()) - int(obs[j].sum())
                if mu == 0:
                    continue
                ref = bt.score_bt(g, X, y[:, q], m.astype(float), nulls[q], sparse=sparse)
                if ref is None:                          # (a denominator below numtol: ignored on both sides)
                    assert got["test_ignored"][j, q]
                    continue
                assert not got["test_ignored"][j, q]
                assert got["stats"][j, q] == pytest.approx(ref["stats"], rel=1e-9, abs=1e-10)
                assert got["bhat"][j, q] == pytest.approx(ref["bhat"], rel=1e-9, abs=1e-12)
                assert got["denum"][j, q] == pytest.approx(ref["denum"], rel=1e-9)
                pairs.append((j, q, ref))
        var = np.array([p[0] for p in pairs] * 2, np.int32)
        tr = np.array([p[1] for p in pairs] * 2, np.int32)
        fast = np.array([0] * len(pairs) + [int(got["sparse"][p[0]]) for p in pairs], np.uint8)
        fc = s2.bt_correct(BT_FIRTH_APPROX, var, tr, fast)
        sc = s2.bt_correct(BT_SPA, var, tr, fast)
    nfirth = nspa = 0
    for t, (j, q, ref) in enumerate(pairs + pairs):
        g, m = gi[j], mask[:, q].astype(float)
        is_fast = bool(fast[t])
        want = bt.approx_firth(g, X, y[:, q], m, nulls[q], fo[q], sparse=is_fast, mac=0 if is_fast else None)
        if want is None:
            assert fc["fail"][t] == 1
        else:
            assert fc["fail"][t] == 0
            assert fc["beta"][t] == pytest.approx(want["bhat"], rel=1e-6, abs=1e-8) and fc["se"][t] == pytest.approx(want["se"], rel=1e-6)
            assert fc["chisq"][t] == pytest.approx(want["chisq"], rel=1e-6, abs=1e-9)
            nfirth += 1
        if abs(ref["stats"]) < 0.1:
            continue
        wsp = bt.spa_test(ref["stats"], ref["denum"], ref["Gres"], nulls[q], m, carriers=np.flatnonzero(g != 0) if is_fast else None)
        if wsp is None:
            assert sc["fail"][t] == 1
        else:
            assert sc["fail"][t] == 0
            assert sc["logp"][t] == pytest.approx(wsp["logp"], rel=1e-6, abs=1e-9) and sc["chisq"][t] == pytest.approx(wsp["chisq"], rel=1e-6, abs=1e-9)
            assert sc["beta"][t] == pytest.approx(wsp["bhat"], rel=1e-6, abs=1e-10) and sc["se"][t] == pytest.approx(wsp["se"], rel=1e-9)
            nspa += 1
    assert nfirth > len(pairs) // 2 and nspa > len(pairs) // 2


def test_int_rows_whose_coded_maximum_is_the_scale(problem):
    """Integer dosages are taken as they come: coded 8-bit probabilities (at most `scale`, reached) score as the NumPy restatement scores the same
    numbers (its additive formulas on the coded values), whatever the context's coding is."""
    from regenie_amd.step2 import DOMINANT, Step2QT
    X, res, mask, scf, G = problem
    rng = np.random.default_rng(5)
    q = np.where(np.isnan(G), 0xFFFF, np.where(G >= 1, rng.integers(0, 256, size=G.shape), 0)).astype(np.uint16)
    q[0, :8] = 255                                        # the coded maximum
    assert q[q != 0xFFFF].max() == 255
    Gd = np.where(q == 0xFFFF, np.nan, q / 255.0)
    want = dc.qt_block(Gd, 0, X, res, mask, scf, filters=False)
    with Step2QT(N, C, P) as s2:
        s2.set_null(X.T, res.T, mask.T, scf)
        s2.set_coding(DOMINANT)
        got = s2.score_block_int(q, 255)
    ok = got["ignored"] == 0
    assert np.array_equal(ok, ~np.isnan(want["scale_fac"]) & ~(want["scale_fac"] < 1e-6)) and ok.sum() > BS - 8
    assert np.array_equal(got["scale_fac"][ok] == 1.0, want["sparse"][ok]) and want["sparse"][ok].any() and not want["sparse"][ok].all()
    assert np.allclose(got["scale_fac"][ok], want["scale_fac"][ok], rtol=1e-11) and np.allclose(got["mean"][ok], want["mean"][ok], rtol=1e-13)
    assert np.allclose(got["stats"][ok], want["stats_all"][ok], rtol=RTOL, atol=1e-10, equal_nan=True)
    assert np.allclose(got["bhat"][ok], want["bhat_all"][ok], rtol=RTOL, atol=1e-13, equal_nan=True)
