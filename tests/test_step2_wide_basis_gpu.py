"""The Step-2 quantitative-trait kernels at covariate bases of 16 to 64 columns -- the widths a conditional analysis produces, where every
conditioning variant is one more column of X (rg_s2_qt_block, rg_s2_qt_block_packed, rg_s2_qt_block_int behind regenie_amd.step2.Step2QT)
-- against the reference-pinned oracle (oracle/regenie_step2_qt.py: score_qt_block_ref).  The basis is built as the driver builds it
(intercept, covariates, mean-imputed conditioning variants, orthonormalised), and the tested block holds what such an analysis tests:
exact copies of conditioning variants (the reference drops them: scale_fac < numtol), near copies (a tested variant in strong LD with a
conditioning one: the residual sum of squares is a small share of sum g^2), an all-missing and a monomorphic row beside ordinary
variants on both sides of check_sparse_G.  Every (variant, trait) is held to RTOL of its OWN reference value, not of the block's largest.

The fixtures are checked without a GPU (test_fixture_preconditions); the other tests are marked gpu."""
import functools

import numpy as np
import pytest

from oracle import regenie_step2_qt as s2o
from tests.test_step2_qt_gpu import RTOL, _compare, _pack_bed, _run, _run_packed

gpu = pytest.mark.gpu

LD_RTOL = 1e-11                       # float64 oracle against its longdouble restatement on the near copies (set by the issue)
K_CANDIDATES = (1, 2, 3, 5, 8, 13, 21)
# fixed rows of the tested block (bs >= 20)
ROW_MONO, ROW_ALL_MISSING, ROW_EXACT_A, ROW_NEAR_DENSE, ROW_NEAR_SPARSE, ROW_EXACT_B = 2, 3, 5, 9, 12, 17
SPECIAL_ROWS = (ROW_MONO, ROW_ALL_MISSING, ROW_EXACT_A, ROW_NEAR_DENSE, ROW_NEAR_SPARSE, ROW_EXACT_B)


def _variant_longdouble(g_raw, X, res, mask, scf, n_samples):
    """One variant of score_qt_block_ref (mean imputation, check_sparse_G, then the sparse or the dense branch of compute_score_qt) with
    every sum in numpy.longdouble; the inputs are the float64 values taken as exact.  -> stats [P], bhat [P], scale_fac."""
    L = np.longdouble
    n, C = X.shape
    obs = ~np.isnan(g_raw)
    g = np.where(obs, g_raw, 0.0).astype(L)
    g[~obs] = g.sum() / L(int(obs.sum()))
    Xl, rl, ml, sl = (np.asarray(a, dtype=L) for a in (X, res, mask, scf))
    beta = Xl.T @ g
    if np.count_nonzero(g) <= n_samples * 0.5:
        num = rl.T @ g - (rl.T @ Xl) @ beta
        gm = g[:, None] * ml
        den = (gm * gm).sum(axis=0) - 2 * ((Xl.T @ gm).T @ beta) + beta @ beta
        sf = L(1)
    else:
        r = g - Xl @ beta
        sf = np.sqrt(r @ r) / np.sqrt(L(n - C))
        gs = r / sf
        num = (rl.T @ gs) * sf
        den = sf * sf * (ml.T @ (gs * gs))
    stats = num / np.sqrt(den)
    return stats, stats * sl / np.sqrt(den), sf


def _longdouble_gap(g_raw, X, res, mask, scf):
    """The largest relative distance of the float64 oracle's stats, bhat and scale_fac of one variant from the longdouble restatement,
    and the oracle's `ignored` flag."""
    ref = s2o.score_qt_block_ref(g_raw[None, :], X, res, mask, scf)
    stats, bhat, sf = _variant_longdouble(g_raw, X, res, mask, scf, X.shape[0])
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = max(float(np.max(np.abs(ref["stats"][0] - stats) / np.abs(stats))), float(np.max(np.abs(ref["bhat"][0] - bhat) / np.abs(bhat))),
                  float(abs(ref["scale_fac"][0] - sf) / abs(sf)))
    return gap, int(ref["ignored"][0])


def _near_copy(column_calls, k, rng_seed):
    """The conditioning variant's hard calls with k observed calls changed (c -> (c + 1) mod 3); the positions of a smaller k are a prefix."""
    g = column_calls.copy()
    pos = np.random.default_rng(rng_seed).permutation(np.flatnonzero(~np.isnan(g)))[:k]
    g[pos] = (g[pos] + 1) % 3
    return g


def wide_problem(seed, n, C, P, bs, n_cond, miss_y):
    """The basis as the driver builds it -- intercept, C - 1 - n_cond normal covariates, n_cond conditioning variants (mean-imputed hard
    calls; MAF 0.33 - 0.5 for the first two and every second one after them, which check_sparse_G calls dense, 0.05 - 0.2 for the others),
    orthonormalised by QR -- residuals, masks and scf as tests/test_step2_qt_gpu.py::_problem takes them, and the tested block G [bs][n] of
    hard calls (NaN = missing, about 1 % of them).  -> dict; "k_dense" / "k_sparse": the number of calls changed in the two near copies, the
    smallest of K_CANDIDATES at which the float64 oracle stays within LD_RTOL of its longdouble restatement and does not ignore the variant
    ("gap_dense" / "gap_sparse": that distance)."""
    assert 3 <= n_cond <= C - 1 and bs >= 20
    rng = np.random.default_rng(seed)
    dense_col = np.array([q < 2 or q % 2 == 1 for q in range(n_cond)])
    maf = np.where(dense_col, rng.uniform(0.33, 0.5, size=n_cond), rng.uniform(0.05, 0.2, size=n_cond))
    cond = rng.binomial(2, maf[:, None], size=(n_cond, n)).astype(np.float64)
    cond[rng.random(cond.shape) < 0.01] = np.nan
    imputed = np.array([s2o.mean_impute(c)[0] for c in cond])
    cov = np.column_stack([np.ones(n), rng.normal(size=(n, C - 1 - n_cond)), imputed.T])
    X = np.linalg.qr(cov)[0]
    Y = rng.normal(size=(n, P)) + 0.3 * rng.normal(size=(n, 1))
    mask = np.ones((n, P))
    if miss_y:
        mask[rng.random((n, P)) < miss_y] = 0
    Y = (Y - X @ (X.T @ Y)) * mask
    neff = mask.sum(axis=0)
    scale_Y = np.sqrt((Y ** 2).sum(axis=0) / (neff - C))
    Y = Y / scale_Y
    blup = 0.1 * rng.normal(size=(n, P)) * mask
    res, _, scf = s2o.compute_res(Y, blup, mask, neff, C, scale_Y)
    G = rng.binomial(2, np.exp(rng.uniform(np.log(0.01), np.log(0.5), size=bs))[:, None], size=(bs, n)).astype(np.float64)
    G[rng.random(G.shape) < 0.01] = np.nan
    G[ROW_MONO] = 2.0
    G[ROW_ALL_MISSING] = np.nan
    G[ROW_EXACT_A], G[ROW_EXACT_B] = cond[0], cond[1]                      # dense conditioning variants, missing calls and all
    sparse_col = int(np.flatnonzero(~dense_col)[0])
    out = {"X": X, "res": res, "mask": mask, "scf": scf, "G": G, "dense_col": dense_col, "cond": cond}
    for name, row, src in (("dense", ROW_NEAR_DENSE, 0), ("sparse", ROW_NEAR_SPARSE, sparse_col)):
        for k in K_CANDIDATES:
            g = _near_copy(cond[src], k, seed + 7919 * (src + 1))
            gap, ign = _longdouble_gap(g, X, res, mask, scf)
            if gap <= LD_RTOL and not ign:
                break
        G[row] = g
        out["k_" + name], out["gap_" + name] = k, gap
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _integer_dosages(case, scale):
    """The hard calls of the block in units of 1 / scale with the perturbation of test_integer_dosage_route_against_oracle (four in ten
    entries moved by up to scale / 3, three in ten set to exactly zero) on the ordinary rows; the copies, the monomorphic and the all-missing
    row stay what they are.  -> uint16 [bs][n] (0xFFFF = missing), the same values as float64 dosages."""
    G = case["G"]
    bs, n = G.shape
    rng = np.random.default_rng(scale + n + bs)
    miss = np.isnan(G)
    hard = np.nan_to_num(G).astype(np.int64) * scale
    Gi = np.clip(hard + (rng.random((bs, n)) < 0.4) * rng.integers(-scale // 3, scale // 3 + 1, size=(bs, n)), 0, 2 * scale)
    Gi[rng.random((bs, n)) < 0.3] = 0
    for j in SPECIAL_ROWS:
        Gi[j] = hard[j]
    return np.where(miss, 0xFFFF, Gi).astype(np.uint16), np.where(miss, np.nan, Gi / float(scale))


@functools.lru_cache(maxsize=None)
def wide_case(seed, n, C, P, bs, n_cond, miss_y):
    """wide_problem with its three references, computed once per process and shared read-only: "ref" for the hard calls (the fp64 and the
    packed route), "ref255" / "ref16384" for the integer dosages "Gi255" / "Gi16384"."""
    case = wide_problem(seed, n, C, P, bs, n_cond, miss_y)
    null = (case["X"], case["res"], case["mask"], case["scf"])
    case["ref"] = s2o.score_qt_block_ref(case["G"], *null)
    for scale in (255, 16384):
        Gi, Gf = _integer_dosages(case, scale)
        Gi.setflags(write=False)
        case["Gi%d" % scale], case["ref%d" % scale] = Gi, s2o.score_qt_block_ref(Gf, *null)
    for key in ("ref", "ref255", "ref16384"):
        for a in case[key].values():
            a.setflags(write=False)
    return case


def _check_fixture(case):
    """What the inputs must be for the GPU tests to mean what they say (no GPU needed)."""
    bs = case["G"].shape[0]
    assert case["gap_dense"] <= LD_RTOL and case["gap_sparse"] <= LD_RTOL, (case["k_dense"], case["gap_dense"], case["k_sparse"], case["gap_sparse"])
    assert case["dense_col"][0] and case["dense_col"][1]
    for key in ("ref", "ref255", "ref16384"):
        ref = case[key]
        assert 0 < ref["sparse"].sum() < bs, key                                         # both branches of check_sparse_G
        assert ref["ignored"][[ROW_EXACT_A, ROW_EXACT_B, ROW_MONO, ROW_ALL_MISSING]].all(), key   # residualize_geno drops the exact copies
        assert not ref["sparse"][[ROW_EXACT_A, ROW_EXACT_B, ROW_NEAR_DENSE]].any() and ref["sparse"][ROW_NEAR_SPARSE], key
        assert not ref["ignored"][[ROW_NEAR_DENSE, ROW_NEAR_SPARSE]].any(), key
        assert ref["ignored"].sum() == 4, key
        ok = ref["ignored"] == 0
        assert np.isfinite(ref["stats"][ok]).all() and np.isfinite(ref["bhat"][ok]).all(), key


def _ss_over_gg(case, j):
    """|g - X X^T g|^2 / |g|^2 of the mean-imputed hard calls of row j: how much of the variant the basis leaves."""
    g = s2o.mean_impute(case["G"][j])[0]
    r = g - case["X"] @ (case["X"].T @ g)
    return float(r @ r) / float(g @ g)


def _hold(got, ref, case, route):
    """_compare of tests/test_step2_qt_gpu.py, then every non-ignored (variant, trait) on its own: |got - ref| <= RTOL |ref| + the absolute
    floors that file uses (1e-10 for the statistic, 1e-13 for bhat)."""
    _compare(got, ref)
    ok = ref["ignored"] == 0
    for key, floor in (("stats", 1e-10), ("bhat", 1e-13)):
        g, r = got[key], ref[key]
        excess = np.where(ok[:, None], np.abs(g - r) - (RTOL * np.abs(r) + floor), -1.0)
        j, p = np.unravel_index(np.argmax(excess), excess.shape)
        assert excess[j, p] <= 0, "%s %s[%d, %d]: got %.17g, reference %.17g (relative %.3e), ss / gg of the row %.3e" % (
            route, key, j, p, g[j, p], r[j, p], abs(g[j, p] - r[j, p]) / abs(r[j, p]), _ss_over_gg(case, j))


def _null(case):
    return case["X"], case["res"], case["mask"], case["scf"]


def _int_routes(case, route_tag):
    """rg_s2_qt_block_int at two (scale 255) and three (scale 16384) digit planes against the oracle; and the same rows read in place from
    a device tensor whose pitch exceeds n (k_s2_int_rows without the 16-byte loads when the pitch is no multiple of 8; garbage beyond the
    row): bit-identical, the sums of the rows being exact integers."""
    import torch
    from regenie_amd.step2 import Step2QT
    X, res, mask, scf = _null(case)
    n, C = X.shape
    for scale in (255, 16384):
        Gi, ref = case["Gi%d" % scale], case["ref%d" % scale]
        with Step2QT(n, C, res.shape[1]) as s2:
            s2.set_null(X.T, res.T, mask.T, scf)
            got = s2.score_block_int(Gi, scale)
            pad = 5 if (n + 5) % 8 else 3
            big = torch.randint(-32768, 32767, (Gi.shape[0], n + pad), dtype=torch.int16, device="cuda")
            big[:, :n] = torch.from_numpy(Gi.view(np.int16).copy()).cuda()
            dev = s2.score_block_int(big[:, :n], scale)
        _hold(got, ref, case, "%s int scale %d" % (route_tag, scale))
        for key in ("stats", "bhat", "scale_fac", "mean", "n_obs", "ignored"):
            assert np.array_equal(got[key], dev[key], equal_nan=True), (scale, key)


# ---- 1. three routes over the basis width -----------------------------------------------------------------------------------------------
# Both sides of every width-dependent branch: one / two column tiles of k_s2_masked_int_mfma (16 | 17), its last width and the first of
# k_s2_masked_int (32 | 33), the middle of that kernel's four-sweep regime and the limit; ngc = ceil(C / 16) = 1 .. 4 covariate groups on the
# packed route's compact axis.  n is no multiple of 64 and bs none of 16.
SWEEP = {16: (2503, 21), 17: (3001, 27), 31: (3533, 35), 32: (4001, 41), 33: (4099, 45), 48: (5003, 53), 64: (6001, 67)}
SWEEP_CASES = [(100 + C, n, C, 3, bs, min(C - 1, 10), miss_y) for C, (n, bs) in SWEEP.items() for miss_y in (0.0, 0.06)]
# ---- 2. many traits with many covariates: ngrp = ceil((C + P) / 16) = 8 column groups, two contraction launches on the compact axis ------
# 3 % missing values in 64 and in 40 traits list 1.92 n and 1.2 n masked samples: above n, the packed route carries C P + P mask columns
# (4,288 contraction columns at 64 x 64) and RG_S2_MASK_COLS=1 asks for the same route; 2 % in 40 traits list 0.8 n: the compact axis with
# ngc = 3 and launches of 32 + 8 traits.
MANY = [(64, 64, 0.03), (33, 40, 0.03), (33, 40, 0.02)]
MANY_CASES = [(200 + C + P, 4099, C, P, 33, min(C - 1, 10), miss_y) for C, P, miss_y in MANY]
# ---- 3. the tile fallback of the fp64 route (rg_s2_qt_block) ------------------------------------------------------------------------------
# With RG_S2_TILE=16x4 (vpb = 16) the two launches ask for
#   lds1 = 8 B * 4 vpb (2 + 2 C)                    = 512 (2 + 2 C) B
#   lds2 = 8 B * (vpb C + vpb + 4 vpb (2 + 2 P))    = 128 (C + 9 + 8 P) B
# and fall back to the default tile when either exceeds 60 KB = 61,440 B:
#   (C, P) = (64, 2): lds1 = 66,560 B  > 61,440                  -> the default tile
#   (C, P) = (60, 2): lds1 = 62,464 B  > 61,440                  -> the default tile (the first width that falls back)
#   (C, P) = (59, 2): lds1 = 61,440 B, not above                 -> 16x4 at its largest footprint
#   (C, P) = (58, 2): lds1 = 60,416 B                            -> 16x4
#   (C, P) = (4, 64): lds1 = 5,120 B, lds2 = 128 * 525 = 67,200 B > 61,440 -> the default tile
TILE = [(64, 2, True), (60, 2, True), (59, 2, False), (58, 2, False), (4, 64, True)]
TILE_CASES = [(300 + C + P, 2999, C, P, 23, min(C - 1, 10), 0.03) for C, P, _ in TILE]


def _id(args):
    return "C%d-P%d-n%d-bs%d-miss%g" % (args[2], args[3], args[1], args[4], args[6])


@pytest.mark.parametrize("args", SWEEP_CASES + MANY_CASES + TILE_CASES, ids=_id)
def test_fixture_preconditions(args):
    """No GPU: the near copies are variants the float64 oracle itself resolves (within 1e-11 of its longdouble restatement, not ignored),
    both branches of check_sparse_G occur in each of the three blocks, the exact copies are what the reference drops."""
    case = wide_case(*args)
    print("near copies: dense k = %d (gap %.2e, ss / gg %.2e), sparse k = %d (gap %.2e, ss / gg %.2e)" % (
        case["k_dense"], case["gap_dense"], _ss_over_gg(case, ROW_NEAR_DENSE), case["k_sparse"], case["gap_sparse"], _ss_over_gg(case, ROW_NEAR_SPARSE)))
    _check_fixture(case)


@gpu
@pytest.mark.parametrize("args", SWEEP_CASES, ids=_id)
def test_three_routes_over_the_basis_width(args):
    case = wide_case(*args)
    _check_fixture(case)
    null = _null(case)
    _hold(_run(*null, case["G"]), case["ref"], case, "fp64")
    _hold(_run_packed(*null, _pack_bed(case["G"])), case["ref"], case, "packed")
    _int_routes(case, "sweep")


@gpu
@pytest.mark.parametrize("args", MANY_CASES, ids=_id)
def test_many_traits_with_many_covariates(args, monkeypatch):
    """64 x 64 and 33 x 40 covariates x traits with phenotypes that differ in their missing values.  The near copy of a dense conditioning
    variant (ss / gg = 2.4e-4) is the row that decides the hard-call route here: its dense-branch denominator sum mask_p g^2 -
    2 (X^T (g o mask_p)) . beta + beta^T Q_p beta is three terms of the size of gg for a result of the size of ss, and at 33 x 40 it was
    1.8e-9 (statistic) and 3.5e-9 (bhat) from the oracle in both the compact-axis and the mask-column form (the same formula in numpy
    float64: 4.5e-9 from its longdouble value).  rg_s2_qt_block_packed now sends a dense variant with ss < gg / 64 through the fp64 route,
    which forms the residual itself."""
    from regenie_amd.step2 import Step2QT
    case = wide_case(*args)
    _check_fixture(case)
    X, res, mask, scf = null = _null(case)
    n, C = X.shape
    P = res.shape[1]
    assert (C + P + 15) // 16 == (8 if (C, P) == (64, 64) else 5)          # column groups of [X | res]
    assert (int((mask == 0).sum()) > n) == (args[6] == 0.03)          # which of the two packed routes the library itself picks
    _hold(_run(*null, case["G"]), case["ref"], case, "fp64")
    rows = _pack_bed(case["G"])
    out = {}
    for name, env in (("compact", None), ("columns", "1")):
        if env is None:
            monkeypatch.delenv("RG_S2_MASK_COLS", raising=False)
        else:
            monkeypatch.setenv("RG_S2_MASK_COLS", env)
        with Step2QT(n, C, P) as s2:
            s2.set_null(X.T, res.T, mask.T, scf)
            out[name] = s2.score_block_packed(rows)
    monkeypatch.delenv("RG_S2_MASK_COLS", raising=False)
    a, b = out["compact"], out["columns"]
    for k in ("n_obs", "ignored", "n_obs_p", "total_p"):      # as test_packed_masked_compact_axis_equals_mask_columns requires
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    for k in ("stats", "bhat"):
        ok = ~np.isnan(b[k])
        assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), k
        assert np.allclose(a[k][ok], b[k][ok], rtol=1e-10, atol=1e-12), (k, np.abs(a[k][ok] - b[k][ok]).max())
    _hold(a, case["ref"], case, "packed")
    _hold(b, case["ref"], case, "packed, RG_S2_MASK_COLS=1")
    obs = ~np.isnan(case["G"])
    assert np.array_equal(a["n_obs_p"], (obs[:, :, None] & (mask[None] > 0)).sum(axis=1))
    _int_routes(case, "many traits")


@gpu
@pytest.mark.parametrize("C,P,falls_back", TILE, ids=["C%d-P%d" % t[:2] for t in TILE])
def test_tile_16x4_and_its_fallback_to_the_default_tile(C, P, falls_back, monkeypatch):
    """The widths around the 60 KB bound of the two streaming kernels' dynamic LDS (arithmetic above TILE): all against the oracle; where
    the launch falls back, it IS the default tile and gives the default tile's numbers bit for bit."""
    case = wide_case(*TILE_CASES[[t[:2] for t in TILE].index((C, P))])
    _check_fixture(case)
    assert (max(512 * (2 + 2 * C), 128 * (C + 9 + 8 * P)) > 60 * 1024) == falls_back
    null = _null(case)
    monkeypatch.setenv("RG_S2_TILE", "16x4")
    got = _run(*null, case["G"])
    _hold(got, case["ref"], case, "fp64, RG_S2_TILE=16x4")
    if falls_back:
        monkeypatch.delenv("RG_S2_TILE")
        default = _run(*null, case["G"])
        for key in ("stats", "bhat", "scale_fac", "mean", "n_obs", "ignored"):
            assert np.array_equal(got[key], default[key], equal_nan=True), key
