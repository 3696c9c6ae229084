"""The LD-matrix library (include/rg_ld.h, regenie_amd/csrc/ld_corr.hip) through regenie_amd/ld.py on the GPU: the exact integer
sums of panel pairs against numpy integer products, covariance / correlation against the longdouble restatement of print_ld
(tests/ld_restate.py), the device-side 16-bit quantisation, one size run, the error paths."""
import numpy as np
import pytest

from tests import ld_restate as lr

pytestmark = pytest.mark.gpu


def _calls(rng, bs, n, miss):
    maf = rng.uniform(0.02, 0.5, size=bs)
    G = rng.binomial(2, maf[:, None], size=(bs, n)).astype(np.float32)      # (float32 holds 0 / 1 / 2 / nan; a 1,000 x 200,001 panel stays at 0.8 GB)
    if miss:
        G[rng.random(G.shape, dtype=np.float32) < miss] = np.nan
    return G


def _ints(G, flip):
    """g0 (0 at a missing entry) and the indicator [bs][n], as integers held in float64: their products are integers below 2^53, so
    the BLAS product is the exact integer product (numpy's int64 matmul is the same number, a thousand times slower)."""
    m = np.isnan(G)
    return np.where(m, 0.0, (2 - G) if flip else G).astype(np.float64), m.astype(np.float64)


@pytest.mark.parametrize("n", [1, 63, 500, 4099, 200001])
@pytest.mark.parametrize("miss", [0.0, 0.03])
def test_pair_sums_are_exact(n, miss):
    import torch
    from regenie_amd.ld import LDMatrix, pack_bed_rows
    rng = np.random.default_rng(1000 + n)
    sizes = [1, 37, 256, 1000]
    for flip in (False, True):
        panels = [_calls(rng, bs, n, miss) for bs in sizes]
        with LDMatrix(n, 1, sum(sizes)) as ld:
            starts, c0 = [], 0
            for k, G in enumerate(panels):
                rows = pack_bed_rows(G)
                if k % 2:      # device pointer, with a row pitch wider than the row
                    t = torch.zeros((rows.shape[0], rows.shape[1] + 5), dtype=torch.uint8, device="cuda")
                    t[:, :rows.shape[1]] = torch.from_numpy(rows).cuda()
                    rows = t
                ld.append(rows, np.arange(c0, c0 + G.shape[0]), flip=flip)
                starts.append(c0)
                c0 += G.shape[0]
            for a in range(len(panels)):
                ga, ma = _ints(panels[a], flip)
                for b in (a, (a + 1) % len(panels)):     # a panel with itself and with another one
                    gb, mb = (ga, ma) if b == a else _ints(panels[b], flip)
                    got = ld.pair_sums(starts[a], len(ga), starts[b], len(gb))
                    assert np.array_equal(got["A"], ga @ gb.T), (n, miss, flip, a, b, "A")
                    assert np.array_equal(got["B"], ga @ mb.T), (n, miss, flip, a, b, "B")
                    assert np.array_equal(got["Bt"], ma @ gb.T), (n, miss, flip, a, b, "Bt")
                    assert np.array_equal(got["D"], ma @ mb.T), (n, miss, flip, a, b, "D")


def _basis(rng, n, C):
    return np.linalg.qr(np.column_stack([np.ones(n), rng.normal(size=(n, C - 1))]))[0]


def _rel_dist(a, ref):
    d = np.sqrt(np.abs(np.diag(ref)).astype(np.float64))
    d[d == 0] = 1.0
    return float(np.max(np.abs(np.asarray(a, dtype=np.longdouble) - ref) / (d[:, None] * d[None, :])))


@pytest.mark.parametrize("C", [1, 12, 33, 64])
def test_cov_and_corr_against_longdouble_restatement(C):
    """Tolerance (set by the issue): the library may be at most 4 x as far from the longdouble restatement as numpy's float64
    restatement is (max over entries, relative to sqrt(LD_ii LD_jj)).  C = 33 and 64: the basis of a conditional analysis (the
    projection of k_ld_combine over three groups of 16 columns and one more, and over all of RG_S2_MAX_COV), on a smaller matrix:
    the longdouble restatement takes one pass over the calls per basis column."""
    from regenie_amd.ld import COV_F64, CORR_F64, R2_U16, LDMatrix, pack_bed_rows
    rng = np.random.default_rng(77 + C)
    n, M, nforced = (20000, 1500, 7) if C <= 12 else (1031, 263, 7)
    sizes = [600, 500, M - nforced - 1100] if C <= 12 else [100, 90, M - nforced - 190]
    order = rng.permutation(M)                    # scrambled column order
    forced, filled = order[:nforced], order[nforced:]
    Gfull = np.zeros((n, M))
    X = _basis(rng, n, C)
    with LDMatrix(n, C, M) as ld:
        ld.set_basis(X.T)
        ld.force_columns(forced)
        c0 = 0
        for k, bs in enumerate(sizes):
            G = _calls(rng, bs, n, 0.02 if k != 1 else 0.0)       # the middle panel has no missing call
            cols = filled[c0:c0 + bs]
            ld.append(pack_bed_rows(G), cols)
            Gfull[:, cols] = G.T
            c0 += bs
        cov = ld.finish(COV_F64)
        cor = ld.finish(CORR_F64)
        r2 = ld.finish(R2_U16)
    ref_cov = lr.ld_cov(Gfull, X, np.longdouble)
    ref_cor = lr.ld_corr(Gfull, X, np.longdouble)
    d_np_cov, d_lib_cov = _rel_dist(lr.ld_cov(Gfull, X), ref_cov), _rel_dist(cov, ref_cov)
    d_np_cor = float(np.max(np.abs(lr.ld_corr(Gfull, X) - ref_cor)))
    d_lib_cor = float(np.max(np.abs(cor - ref_cor)))
    print("C=%d covariance: numpy fp64 %.3e, library %.3e from longdouble; correlation: numpy %.3e, library %.3e"
          % (C, d_np_cov, d_lib_cov, d_np_cor, d_lib_cor))
    assert d_lib_cov <= 4 * d_np_cov, (d_lib_cov, d_np_cov)
    assert d_lib_cor <= 4 * d_np_cor, (d_lib_cor, d_np_cor)
    assert np.array_equal(cov, cov.T) and np.array_equal(cor, cor.T)
    assert np.all(cor[forced][:, filled] == 0) and np.allclose(np.diag(cor)[forced], 1.0, rtol=0, atol=1e-15)
    # the triangle quantised on the device is the quantisation of the library's own correlations, bit for bit
    assert np.array_equal(r2, lr.quantise(cor)[0])


def _copy_basis(rng, n, C, imputed):
    """[1, C - 1 - k normal covariates, the k mean-imputed variants] orthonormalised: the basis of an analysis conditional on them."""
    return np.linalg.qr(np.column_stack([np.ones(n), rng.normal(size=(n, C - 1 - imputed.shape[1])), imputed]))[0]


def check_copied_columns(cov, cor, r2, Gfull, X, ref_cov, np_cov, copies):
    """Columns `copies` of the matrix are exact copies of basis columns (a variant of the region that the analysis conditions on): their
    projected variance is rounding noise around zero.  What is asserted is what does not depend on the sign of that noise:
      - among the OTHER columns the rule of test_cov_and_corr_against_longdouble_restatement;
      - a copy's row of the covariance is zero up to the rounding of its two terms, |LD_ij| <= 4 n eps |g_i| |g_j| (each of g_i . g_j and
        (X^T g_i) . (X^T g_j) is a sum of n, resp. C products bounded by |g_i| |g_j|, with the worst-case bound n eps of a length-n sum;
        the factor 4 covers the two terms and the sums inside X^T g);
      - print_ld's diagonal rules (tests/ld_dosage_restate.py: corr_of) on the library's own covariance give the library's correlations:
        finite, unit diagonal -- sqrt(numtol) stands in for a non-positive variance -- and never NaN;
      - R^2 of a copy with any other column quantises to 0, in the library as in both restatements (the copy-copy pair is noise over noise
        and is left out), and the device-side quantisation is that of the library's own correlations."""
    from tests import ld_dosage_restate as dr
    M = cov.shape[0]
    others = np.setdiff1d(np.arange(M), copies)
    sub = np.ix_(others, others)
    d_np, d_lib = _rel_dist(np_cov[sub], ref_cov[sub]), _rel_dist(cov[sub], ref_cov[sub])
    ref_cor, np_cor = dr.corr_of(ref_cov, np.longdouble), dr.corr_of(np_cov)
    d_np_cor, d_lib_cor = float(np.max(np.abs(np_cor[sub] - ref_cor[sub]))), float(np.max(np.abs(cor[sub] - ref_cor[sub])))
    print("copied columns: diagonal %s (library), %s (numpy); others: covariance numpy %.3e, library %.3e; correlation numpy %.3e, library %.3e"
          % (np.diag(cov)[copies], np.diag(np_cov)[copies], d_np, d_lib, d_np_cor, d_lib_cor))
    assert d_lib <= 4 * d_np, (d_lib, d_np)
    assert d_lib_cor <= 4 * d_np_cor, (d_lib_cor, d_np_cor)
    norm = np.sqrt((lr.mean_impute(Gfull) ** 2).sum(axis=0))
    n = Gfull.shape[0]
    assert (np.abs(cov[copies]) <= 4 * n * np.finfo(np.float64).eps * norm[copies][:, None] * norm[None, :]).all()
    assert np.isfinite(cov).all() and np.isfinite(cor).all()
    assert np.array_equal(cov, cov.T) and np.array_equal(cor, cor.T)
    np.testing.assert_allclose(cor, dr.corr_of(cov), rtol=1e-14, atol=0)
    np.testing.assert_allclose(np.diag(cor), 1.0, rtol=0, atol=1e-15)
    iu = np.triu_indices(M, 1)
    pair_with_other = np.isin(iu[0], copies) ^ np.isin(iu[1], copies)
    for name, c in (("library", cor), ("numpy", np_cor), ("longdouble", ref_cor)):
        assert (lr.quantise(c)[0][pair_with_other] == 0).all(), name
    assert (r2[pair_with_other] == 0).all()
    assert np.array_equal(r2, lr.quantise(cor)[0])


def test_columns_that_copy_basis_columns():
    """Two columns of the LD matrix are the conditioning variants themselves (C = 33: intercept, 30 covariates, the two variants)."""
    from regenie_amd.ld import COV_F64, CORR_F64, R2_U16, LDMatrix, pack_bed_rows
    rng = np.random.default_rng(433)
    n, C, M, copies = 2051, 33, 200, np.array([17, 151])
    G = _calls(rng, M, n, 0.02)
    G[copies] = rng.binomial(2, 0.4, size=(2, n))
    G[copies[0], rng.random(n) < 0.02] = np.nan
    Gfull = G.T.astype(np.float64)
    X = _copy_basis(rng, n, C, lr.mean_impute(Gfull[:, copies]))
    with LDMatrix(n, C, M) as ld:
        ld.set_basis(X.T)
        ld.append(pack_bed_rows(G[:130]), np.arange(130))
        ld.append(pack_bed_rows(G[130:]), np.arange(130, M))
        cov, cor, r2 = ld.finish(COV_F64), ld.finish(CORR_F64), ld.finish(R2_U16)
    check_copied_columns(cov, cor, r2, Gfull, X, lr.ld_cov(Gfull, X, np.longdouble), lr.ld_cov(Gfull, X), copies)


TILE_MISS = {"none": (), "middle": (1,), "outer_two": (0, 2), "all": (0, 1, 2)}


@pytest.mark.parametrize("which", list(TILE_MISS))
def test_three_row_tiles_with_and_without_missing_calls(which):
    """The smallest shape at which the Gram kernel takes every branch of its four sums: 257 rows are row tiles of 128, 128 and 1 (appended
    as three panels, so a panel is a tile), 65 samples are two K-steps, and the tiles named by `which` hold missing calls (about 10 %,
    allele frequencies of 0.2 to 0.5: a B or D tile that is skipped wrongly, or computed from the wrong tile, moves entries by a tenth
    of their size).  The sums of panel pairs and of the whole matrix against itself are the exact integer products; covariance and
    correlation obey the rule of test_cov_and_corr_against_longdouble_restatement."""
    from regenie_amd.ld import COV_F64, CORR_F64, R2_U16, LDMatrix, pack_bed_rows
    rng = np.random.default_rng(257)
    n, C, sizes = 65, 2, [128, 128, 1]
    R = sum(sizes)
    M = R + 1
    order = rng.permutation(M)                    # shuffled column order, one forced column
    forced, filled = order[:1], order[1:]
    X = _basis(rng, n, C)
    panels = []
    for t, bs in enumerate(sizes):
        G = rng.binomial(2, rng.uniform(0.2, 0.5, size=bs)[:, None], size=(bs, n)).astype(np.float32)
        if t in TILE_MISS[which]:
            G[rng.random(G.shape) < 0.1] = np.nan
            G[0, 3] = np.nan
        panels.append(G)
    Gfull = np.zeros((n, M))
    with LDMatrix(n, C, M) as ld:
        ld.set_basis(X.T)
        ld.force_columns(forced)
        starts, c0 = [], 0
        for G in panels:
            cols = filled[c0:c0 + len(G)]
            ld.append(pack_bed_rows(G), cols)
            Gfull[:, cols] = G.T
            starts.append(c0)
            c0 += len(G)
        ints = [_ints(G, False) for G in panels]
        ints.append(tuple(np.concatenate(x) for x in zip(*ints)))      # all rows against themselves: 3 x 3 tiles
        for a, b in [(0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (2, 0), (3, 3)]:
            (ga, ma), (gb, mb) = ints[a], ints[b]
            got = ld.pair_sums(starts[a % 3], len(ga), starts[b % 3], len(gb))
            for key, want in (("A", ga @ gb.T), ("B", ga @ mb.T), ("Bt", ma @ gb.T), ("D", ma @ mb.T)):
                assert np.array_equal(got[key], want), (which, a, b, key)
        cov = ld.finish(COV_F64)
        cor = ld.finish(CORR_F64)
        r2 = ld.finish(R2_U16)
    ref_cov = lr.ld_cov(Gfull, X, np.longdouble)
    ref_cor = lr.ld_corr(Gfull, X, np.longdouble)
    d_np_cov, d_lib_cov = _rel_dist(lr.ld_cov(Gfull, X), ref_cov), _rel_dist(cov, ref_cov)
    d_np_cor = float(np.max(np.abs(lr.ld_corr(Gfull, X) - ref_cor)))
    d_lib_cor = float(np.max(np.abs(cor - ref_cor)))
    print("%s covariance: numpy fp64 %.3e, library %.3e from longdouble; correlation: numpy %.3e, library %.3e" % (which, d_np_cov, d_lib_cov, d_np_cor, d_lib_cor))
    assert d_lib_cov <= 4 * d_np_cov, (d_lib_cov, d_np_cov)
    assert d_lib_cor <= 4 * d_np_cor, (d_lib_cor, d_np_cor)
    assert np.array_equal(cov, cov.T) and np.array_equal(cor, cor.T)
    assert np.all(cov[forced][:, filled] == 0) and np.all(cor[forced][:, filled] == 0)
    assert np.array_equal(r2, lr.quantise(cor)[0])


def test_size_run_200k_by_4096():
    """n = 200,000, M = 4,096: a row store of 200 MB, 32 tile rows, int32 sums up to 8e5; 64 sampled rows against the restatement."""
    import torch
    from regenie_amd.ld import COV_F64, LDMatrix
    n, M, C, bs = 200000, 4096, 3, 1024
    g = torch.Generator(device="cuda").manual_seed(5)
    rng = np.random.default_rng(5)
    X = _basis(rng, n, C)
    nb = (n + 3) // 4
    sample = np.sort(rng.choice(M, 64, replace=False))
    with LDMatrix(n, C, M) as ld:
        ld.set_basis(X.T)
        keep = {}
        for p in range(M // bs):
            maf = torch.rand((bs, 1), device="cuda", generator=g) * 0.48 + 0.02
            u = torch.rand((bs, 4 * nb), device="cuda", generator=g)
            gt = (u < maf * maf).to(torch.uint8) + (u < 1 - (1 - maf) ** 2).to(torch.uint8)      # 0 / 1 / 2
            code = torch.where(gt == 2, 0, torch.where(gt == 1, 2, 3)).to(torch.uint8)
            if p % 2 == 0:
                code[torch.rand((bs, 4 * nb), device="cuda", generator=g) < 0.01] = 1               # missing
            code = code.view(bs, nb, 4)
            rows = (code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6)).contiguous()
            ld.append(rows, np.arange(p * bs, (p + 1) * bs))
            keep[p] = rows.cpu().numpy()
        cov = ld.finish(COV_F64)
        print("size run: Gram kernel %.2f ms for %d tiles" % (ld.kernel_ms, ld.tiles))
    allrows = np.concatenate([keep[p] for p in range(M // bs)])

    def decode(r):
        c = np.stack([(r >> s) & 3 for s in (0, 2, 4, 6)], axis=-1).reshape(r.shape[0], -1)[:, :n]
        return np.where(c == 1, np.nan, np.where(c == 0, 2.0, np.where(c == 2, 1.0, 0.0)))

    diag = np.sqrt(np.diag(cov))
    worst_np = worst_lib = 0.0
    Gs = decode(allrows[sample]).T                 # [n][64]
    cb = 256
    for c0 in range(0, M, cb):
        Gp = decode(allrows[c0:c0 + cb]).T
        ref = lr.ld_cov(Gs, X, np.longdouble, Gb=Gp)
        f64 = lr.ld_cov(Gs, X, Gb=Gp)
        sc = diag[sample][:, None] * diag[c0:c0 + cb][None, :]
        worst_np = max(worst_np, float(np.max(np.abs(f64 - ref) / sc)))
        worst_lib = max(worst_lib, float(np.max(np.abs(cov[sample][:, c0:c0 + cb] - ref) / sc)))
    print("size run: numpy fp64 %.3e, library %.3e from longdouble" % (worst_np, worst_lib))
    assert worst_lib <= 4 * worst_np, (worst_lib, worst_np)


def test_error_paths():
    from regenie_amd.engine import RgError
    from regenie_amd.ld import LDMatrix, pack_bed_rows
    rng = np.random.default_rng(3)
    n = 100
    rows = pack_bed_rows(_calls(rng, 4, n, 0.0))
    X = np.full((1, n), 1 / np.sqrt(n))
    for bad in ((0, 1, 4), (n, 1, 0), (n, 0, 4)):
        with pytest.raises(RgError):
            LDMatrix(*bad)
    with LDMatrix(n, 1, 6) as ld:
        ld.set_basis(X)
        with pytest.raises(RgError, match="used twice"):
            ld.append(rows, [0, 1, 1, 2])
        ld.append(rows, [0, 1, 2, 3])
        with pytest.raises(RgError, match="used twice"):
            ld.append(rows[:1], [2])
        with pytest.raises(RgError, match="more rows"):
            ld.append(rows, [4, 5, 6, 7])
        with pytest.raises(RgError, match="out of range"):
            ld.append(rows[:1], [6])
        with pytest.raises(RgError, match="neither appended nor forced"):
            ld.finish()
        with pytest.raises(RgError, match="row range"):
            ld.pair_sums(0, 5, 0, 1)
        ld.force_columns([4])
        ld.append(rows[:1], [5])
        assert ld.finish().shape == (6, 6)
    with LDMatrix(n, 1, 2) as ld:
        ld.append(rows[:2], [0, 1])
        with pytest.raises(RgError, match="set_basis"):
            ld.finish()
