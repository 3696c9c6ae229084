"""Integer-dosage panels of the LD-matrix library (rg_ld_append_int, regenie_amd/csrc/ld_corr.hip) through regenie_amd/ld.py on the
GPU: the exact 64-bit sums of panel pairs against float64 BLAS products of the integer arrays, the flush of the int32 accumulators
past 2^19 samples, covariance / correlation against the longdouble restatement (tests/ld_dosage_restate.py), hard calls handed
over as dosages against the 2-bit path, the error paths."""
import numpy as np
import pytest

from tests import ld_dosage_restate as dr
from tests import ld_restate as lr

pytestmark = pytest.mark.gpu


def _dosages(rng, bs, n, scale, miss):
    """[bs][n] uint16 uniform on [0, 2 * scale], with 0 and 2 * scale forced in and a share `miss` of 0xFFFF."""
    G = rng.integers(0, 2 * scale + 1, size=(bs, n)).astype(np.uint16)
    G.flat[0] = 0
    G.flat[-1] = 2 * scale
    if miss:
        G[rng.random(G.shape) < miss] = dr.MISSING
    return G


def _device(rows, pad=5):
    """The rows as a device tensor with a pitch wider than the row."""
    import torch
    t = torch.zeros((rows.shape[0], rows.shape[1] + pad), dtype=torch.int16, device="cuda")
    t[:, :rows.shape[1]] = torch.from_numpy(rows.view(np.int16)).cuda()
    return t


def _check_pairs(ld, panels, starts, tag):
    for a in range(len(panels)):
        ga, ma = dr.ints(panels[a].T)
        for b in sorted({a, (a + 1) % len(panels)}):      # a panel with itself and with the next one
            gb, mb = (ga, ma) if b == a else dr.ints(panels[b].T)
            got = ld.pair_sums_int(starts[a], ga.shape[1], starts[b], gb.shape[1])
            assert got["A"].dtype == np.int64
            assert np.array_equal(got["A"], dr.exact_product(ga, gb)), tag + (a, b, "A")
            assert np.array_equal(got["B"], dr.exact_product(ga, mb)), tag + (a, b, "B")
            assert np.array_equal(got["Bt"], dr.exact_product(ma, gb)), tag + (a, b, "Bt")
            assert np.array_equal(got["D"], dr.exact_product(ma, mb)), tag + (a, b, "D")


@pytest.mark.parametrize("n", [1, 63, 500, 4099])
@pytest.mark.parametrize("scale", [255, 16384])
@pytest.mark.parametrize("miss", [0.0, 0.03])
def test_pair_sums_are_exact(n, scale, miss):
    from regenie_amd.ld import LDMatrix
    rng = np.random.default_rng(2000 + n + scale)
    sizes = [1, 37, 256]
    panels = [_dosages(rng, bs, n, scale, miss) for bs in sizes]
    with LDMatrix(n, 1, sum(sizes)) as ld:
        starts, c0 = [], 0
        for k, G in enumerate(panels):
            ld.append_int(_device(G) if k % 2 else G, np.arange(c0, c0 + G.shape[0]), scale)
            starts.append(c0)
            c0 += G.shape[0]
        _check_pairs(ld, panels, starts, (n, scale, miss))


def test_accumulators_are_flushed_past_2_to_19_samples():
    """n = 600,001 > 2^19, scale 16384: half of the rows are constant -- at 24512 = -64 - 64 * 128 + 2 * 128^2, whose balanced digits
    are extreme in every plane, at 2 * scale, or at 0 -- so a digit product sits at 4,096 for every sample and an int32 accumulator
    that is never flushed overflows; 16384^2 * 4 * 6e5 < 2^53, so the float64 product is the exact integer."""
    from regenie_amd.ld import LDMatrix
    n, scale, bs = 600001, 16384, 64
    rng = np.random.default_rng(19)
    panels = []
    for k in range(2):
        G = rng.integers(0, 2 * scale + 1, size=(bs, n)).astype(np.uint16)
        G[rng.random(G.shape) < 0.01] = dr.MISSING
        G[0:bs // 2:3] = 24512
        G[1:bs // 2:3] = 2 * scale
        G[2:bs // 2:3] = 0
        panels.append(G)
    with LDMatrix(n, 1, 2 * bs) as ld:
        ld.append_int(panels[0], np.arange(bs), scale)
        ld.append_int(_device(panels[1], 3), np.arange(bs, 2 * bs), scale)
        _check_pairs(ld, panels, [0, bs], (n, scale))


def _basis(rng, n, C):
    return np.linalg.qr(np.column_stack([np.ones(n), rng.normal(size=(n, C - 1))]))[0]


def _rel_dist(a, ref):
    d = np.sqrt(np.abs(np.diag(ref)).astype(np.float64))
    d[d == 0] = 1.0
    return float(np.max(np.abs(np.asarray(a, dtype=np.longdouble) - ref) / (d[:, None] * d[None, :])))


@pytest.mark.parametrize("C", [1, 12, 33, 64])
@pytest.mark.parametrize("scale", [255, 16384])
def test_cov_and_corr_against_longdouble_restatement(scale, C):
    """The rule of tests/test_ld_gpu.py: the library may be at most 4 x as far from the longdouble restatement as numpy's float64
    restatement is (max over entries, relative to sqrt(LD_ii LD_jj)): both round the same fp64 sums, in a different order.  C = 33 and
    64: the basis of a conditional analysis, X^T g from rg_s2_contract_int over three and four column groups."""
    from regenie_amd.ld import COV_F64, CORR_F64, R2_U16, LDMatrix
    rng = np.random.default_rng(500 + scale + C)
    n, M, nforced = (5000, 600, 7) if C <= 12 else (1031, 263, 7)      # (the longdouble restatement takes two passes over the dosages per basis column)
    sizes = [256, 200, M - nforced - 456] if C <= 12 else [128, 70, M - nforced - 198]
    order = rng.permutation(M)
    forced, filled = order[:nforced], order[nforced:]
    Gfull = np.zeros((n, M), dtype=np.uint16)
    X = _basis(rng, n, C)
    with LDMatrix(n, C, M) as ld:
        ld.set_basis(X.T)
        ld.force_columns(forced)
        c0 = 0
        for k, bs in enumerate(sizes):
            G = _dosages(rng, bs, n, scale, 0.02 if k != 1 else 0.0)      # the middle panel has no missing value
            cols = filled[c0:c0 + bs]
            ld.append_int(_device(G) if k == 2 else G, cols, scale)
            Gfull[:, cols] = G.T
            c0 += bs
        cov = ld.finish(COV_F64)
        cor = ld.finish(CORR_F64)
        r2 = ld.finish(R2_U16)
    ref_cov = dr.ld_cov(Gfull, scale, X, np.longdouble)
    ref_cor = dr.corr_of(ref_cov, np.longdouble)
    np_cov = dr.ld_cov(Gfull, scale, X)
    d_np_cov, d_lib_cov = _rel_dist(np_cov, ref_cov), _rel_dist(cov, ref_cov)
    d_np_cor = float(np.max(np.abs(dr.corr_of(np_cov) - ref_cor)))
    d_lib_cor = float(np.max(np.abs(cor - ref_cor)))
    print("scale=%d C=%d covariance: numpy fp64 %.3e, library %.3e from longdouble; correlation: numpy %.3e, library %.3e"
          % (scale, C, d_np_cov, d_lib_cov, d_np_cor, d_lib_cor))
    assert d_lib_cov <= 4 * d_np_cov, (d_lib_cov, d_np_cov)
    assert d_lib_cor <= 4 * d_np_cor, (d_lib_cor, d_np_cor)
    assert np.array_equal(cov, cov.T) and np.array_equal(cor, cor.T)
    assert np.all(cor[forced][:, filled] == 0) and np.allclose(np.diag(cor)[forced], 1.0, rtol=0, atol=1e-15)
    assert np.array_equal(r2, lr.quantise(cor)[0])


@pytest.mark.parametrize("scale", [255, 16384])
def test_columns_that_copy_basis_columns(scale):
    """tests/test_ld_gpu.py::test_columns_that_copy_basis_columns for integer dosages: two columns of the matrix are the hard calls the
    analysis conditions on, handed over in units of 1 / scale (C = 33: intercept, 30 covariates, the two variants)."""
    from regenie_amd.ld import COV_F64, CORR_F64, R2_U16, LDMatrix
    from tests.test_ld_gpu import _copy_basis, check_copied_columns
    rng = np.random.default_rng(434 + scale)
    n, C, M, copies = 2051, 33, 200, np.array([17, 151])
    G = _dosages(rng, M, n, scale, 0.02)
    G[copies] = rng.binomial(2, 0.4, size=(2, n)) * scale
    G[copies[0], rng.random(n) < 0.02] = dr.MISSING
    Gf = dr.to_float(G.T, scale)
    X = _copy_basis(rng, n, C, lr.mean_impute(Gf[:, copies]))
    with LDMatrix(n, C, M) as ld:
        ld.set_basis(X.T)
        ld.append_int(G[:130], np.arange(130), scale)
        ld.append_int(_device(G[130:]), np.arange(130, M), scale)
        cov, cor, r2 = ld.finish(COV_F64), ld.finish(CORR_F64), ld.finish(R2_U16)
    check_copied_columns(cov, cor, r2, Gf, X, dr.ld_cov(G.T, scale, X, np.longdouble), dr.ld_cov(G.T, scale, X), copies)


TILE_MISS = {"none": (), "middle": (1,), "outer_two": (0, 2), "all": (0, 1, 2)}


@pytest.mark.parametrize("which", list(TILE_MISS))
def test_three_row_tiles_with_and_without_missing_values(which):
    """tests/test_ld_gpu.py::test_three_row_tiles_with_and_without_missing_calls for integer dosages of scale 255: 257 rows are row tiles
    of 128, 128 and 1 (a panel each), 65 samples are two K-steps, the tiles named by `which` hold about 10 % missing values; dosages
    uniform on [0, 510] have a mean near 1, so a B or D tile that is skipped wrongly moves entries by a tenth of their size."""
    from regenie_amd.ld import COV_F64, CORR_F64, R2_U16, LDMatrix
    rng = np.random.default_rng(258)
    n, C, scale, sizes = 65, 2, 255, [128, 128, 1]
    R = sum(sizes)
    M = R + 1
    order = rng.permutation(M)                    # shuffled column order, one forced column
    forced, filled = order[:1], order[1:]
    X = _basis(rng, n, C)
    panels = []
    for t, bs in enumerate(sizes):
        G = _dosages(rng, bs, n, scale, 0.1 if t in TILE_MISS[which] else 0.0)
        if t in TILE_MISS[which]:
            G[0, 3] = dr.MISSING
        panels.append(G)
    Gfull = np.zeros((n, M), dtype=np.uint16)
    with LDMatrix(n, C, M) as ld:
        ld.set_basis(X.T)
        ld.force_columns(forced)
        starts, c0 = [], 0
        for k, G in enumerate(panels):
            cols = filled[c0:c0 + len(G)]
            ld.append_int(_device(G) if k == 1 else G, cols, scale)
            Gfull[:, cols] = G.T
            starts.append(c0)
            c0 += len(G)
        _check_pairs(ld, panels, starts, (which,))
        _check_pairs(ld, [np.concatenate(panels)], [0], (which, "all rows"))      # all rows against themselves: 3 x 3 tiles
        cov = ld.finish(COV_F64)
        cor = ld.finish(CORR_F64)
        r2 = ld.finish(R2_U16)
    ref_cov = dr.ld_cov(Gfull, scale, X, np.longdouble)
    ref_cor = dr.corr_of(ref_cov, np.longdouble)
    np_cov = dr.ld_cov(Gfull, scale, X)
    d_np_cov, d_lib_cov = _rel_dist(np_cov, ref_cov), _rel_dist(cov, ref_cov)
    d_np_cor = float(np.max(np.abs(dr.corr_of(np_cov) - ref_cor)))
    d_lib_cor = float(np.max(np.abs(cor - ref_cor)))
    print("%s covariance: numpy fp64 %.3e, library %.3e from longdouble; correlation: numpy %.3e, library %.3e" % (which, d_np_cov, d_lib_cov, d_np_cor, d_lib_cor))
    assert d_lib_cov <= 4 * d_np_cov, (d_lib_cov, d_np_cov)
    assert d_lib_cor <= 4 * d_np_cor, (d_lib_cor, d_np_cor)
    assert np.array_equal(cov, cov.T) and np.array_equal(cor, cor.T)
    assert np.all(cov[forced][:, filled] == 0) and np.all(cor[forced][:, filled] == 0)
    assert np.array_equal(r2, lr.quantise(cor)[0])


@pytest.mark.parametrize("scale", [16384, 255])
def test_hard_calls_as_dosages_match_the_2bit_path(scale):
    """R2_U16 identical and the covariance within rtol 1e-13 of the 2-bit path's, entry by entry -- at scale 16384.  An entry is a
    difference of sums about 1e5 times its own size, so rtol 1e-13 on it asks for bit-identical summands; that is what fp64 gives when
    the scale is a power of two (every division by it is exact).  At scale 255 the integer sums A, B, D and the means are still exact
    multiples, but X^T g goes through rg_s2_contract_int's multiplication by fl(1 / 255), which rounds differently from the 2-bit
    path by an ulp of a summand: measured 1.4e-12 absolute, 7e-11 of an entry of size 2e-2.  There the covariance is held to 1e-13 of
    sqrt(LD_ii LD_jj), the scale the sibling test uses, and R2_U16 stays identical."""
    from regenie_amd.ld import COV_F64, R2_U16, LDMatrix, pack_bed_rows
    rng = np.random.default_rng(41)
    n, M, C = 4099, 300, 3
    maf = rng.uniform(0.05, 0.5, size=M)
    G = rng.binomial(2, maf[:, None], size=(M, n)).astype(np.float64)
    G[rng.random(G.shape) < 0.02] = np.nan
    Gi = np.where(np.isnan(G), dr.MISSING, np.nan_to_num(G) * scale).astype(np.uint16)
    X = _basis(rng, n, C)
    res = []
    for dosage in (False, True):
        with LDMatrix(n, C, M) as ld:
            ld.set_basis(X.T)
            if dosage:
                ld.append_int(Gi, np.arange(M), scale)
            else:
                ld.append(pack_bed_rows(G), np.arange(M))
            res.append((ld.finish(COV_F64), ld.finish(R2_U16)))
    assert np.array_equal(res[0][1], res[1][1])
    if scale == 16384:
        np.testing.assert_allclose(res[1][0], res[0][0], rtol=1e-13, atol=0)
    else:
        d = np.sqrt(np.diag(res[0][0]))
        assert np.max(np.abs(res[1][0] - res[0][0]) / (d[:, None] * d[None, :])) <= 1e-13


def test_error_paths():
    from regenie_amd.engine import RgError
    from regenie_amd.ld import LDMatrix, pack_bed_rows
    rng = np.random.default_rng(3)
    n, scale = 100, 255
    G = _dosages(rng, 4, n, scale, 0.05)
    X = np.full((1, n), 1 / np.sqrt(n))
    with LDMatrix(n, 1, 6) as ld:
        ld.set_basis(X)
        for bad in (0, 16385):
            with pytest.raises(RgError, match="rg error -1: .*scale"):
                ld.append_int(G, [0, 1, 2, 3], bad)
        over = G.copy()
        over[2, 17] = 2 * scale + 1
        with pytest.raises(RgError, match="rg error -1: .*above 2 \\* scale"):
            ld.append_int(over, [0, 1, 2, 3], scale)
        with pytest.raises(RgError, match="rg error -1: .*used twice"):
            ld.append_int(G, [0, 1, 1, 2], scale)
        ld.append_int(G, [0, 1, 2, 3], scale)
        with pytest.raises(RgError, match="rg error -1: .*cannot be mixed"):
            ld.append(pack_bed_rows(np.zeros((1, n))), [4])
        with pytest.raises(RgError, match="one scale"):
            ld.append_int(G[:1], [4], 16384)
        with pytest.raises(RgError, match="rg error -1: .*used twice"):
            ld.append_int(G[:1], [2], scale)
        with pytest.raises(RgError, match="integer-dosage"):
            ld.pair_sums(0, 1, 0, 1)
        # the context is usable after every refusal
        ld.force_columns([4])
        ld.append_int(G[:1], [5], scale)
        cor = ld.finish()
        assert cor.shape == (6, 6) and np.all(np.isfinite(cor))
        Gi = np.zeros((n, 6), dtype=np.uint16)
        Gi[:, [0, 1, 2, 3, 5]] = np.concatenate([G, G[:1]]).T
        np.testing.assert_allclose(cor, dr.ld_corr(Gi, scale, X.T), rtol=0, atol=1e-9)
    with LDMatrix(n, 1, 4) as ld:      # a first append that fails at scale 255 (two digit planes), then the retry at scale 16384 (three)
        ld.set_basis(X)
        with pytest.raises(RgError, match="rg error -1: .*above 2 \\* scale"):
            ld.append_int(over, [0, 1, 2, 3], scale)
        G3 = _dosages(rng, 4, n, 16384, 0.05)
        ld.append_int(G3, [0, 1, 2, 3], 16384)
        ga, ma = dr.ints(G3.T)
        got = ld.pair_sums_int(0, 4, 0, 4)
        assert np.array_equal(got["A"], dr.exact_product(ga, ga)) and np.array_equal(got["D"], dr.exact_product(ma, ma))
        assert np.array_equal(got["B"], dr.exact_product(ga, ma))
        np.testing.assert_allclose(ld.finish(), dr.ld_corr(G3.T, 16384, X.T), rtol=0, atol=1e-9)
    with LDMatrix(n, 1, 2) as ld:      # the other order of mixing
        ld.append(pack_bed_rows(np.zeros((1, n))), [0])
        with pytest.raises(RgError, match="rg error -1: .*cannot be mixed"):
            ld.append_int(G[:1], [1], scale)
