"""The unscaled LD matrix and its sparse form (RG_LD_GTG_F64, rg_ld_finish_sparse / rg_ld_sparse_fetch; regenie_amd/csrc/ld_corr.hip)
through regenie_amd/ld.py on the GPU, against the restatement of print_ld's `--skip-scaleG` branches (tests/ld_gtg_restate.py).

Shapes: the smallest at which the two sparse passes can go wrong -- no pair at all (M = 1), one pair (M = 2), a row of exactly 64
candidates (M = 65: one step of one wavefront), a row that crosses the 128-column tile of the Gram and takes a third step (M = 130),
three row tiles with n = 67 samples (no multiple of 4 or 64) and missing calls in some tiles only (M = 257), forced columns, integer
dosages.  The columns are near-copies of one variant at the head and at the tail of the matrix and independent variants
between them, and the threshold is put into the widest gap of the restated |r| values: the rows of the tail group keep every pair,
rows of independent variants keep none, row 0 keeps some (asserted per shape on the restatement).

Tolerance: that of tests/test_ld_gpu.py for RG_LD_CORR_F64 -- the library may be at most 4 x as far from the longdouble restatement
as numpy's float64 restatement is (max over the entries; sd relative to its value).  The kept pairs must be exactly the
restatement's: the threshold is at least 1e-9 away from every restated |r| (asserted), many orders above either side's error."""
import numpy as np
import pytest

from tests import ld_dosage_restate as dr
from tests import ld_gtg_restate as gr
from tests import ld_restate as lr

pytestmark = pytest.mark.gpu


def _basis(rng, n, C):
    return np.linalg.qr(np.column_stack([np.ones(n), rng.normal(size=(n, C - 1))]))[0]


def _groups(M):
    """Sizes of the head group, the independent middle and the tail group of near-copies."""
    if M <= 2:
        return M, 0, 0
    head = tail = min(5, M // 8 + 2)
    return head, M - head - tail, tail


def _calls(rng, M, n, miss_cols):
    """[M][n] hard calls (nan = missing, 8 % of the calls of the columns in miss_cols): see the module docstring."""
    head, mid, tail = _groups(M)

    def copies(k):
        base = rng.binomial(2, 0.4, size=n)
        out = np.repeat(base[None, :], k, axis=0)
        flip = rng.random((k, n)) < 0.04
        out[flip] = rng.binomial(2, 0.4, size=int(flip.sum()))
        return out
    grp = copies(head + tail)      # one group, split: a head row keeps pairs in its first step of 64 columns and in its last
    G = np.concatenate([grp[:head], rng.binomial(2, rng.uniform(0.2, 0.5, size=mid)[:, None], size=(mid, n)), grp[head:]]).astype(np.float64)
    for c in miss_cols:
        G[c, rng.random(n) < 0.08] = np.nan
    return G


def _thresholds(every, M):
    """The threshold(s) of a shape from its restated values: the middle of the widest gap between neighbouring |r| (M = 2: one below and
    one above its only pair)."""
    a = np.sort(np.abs(np.asarray(every, dtype=np.float64)))
    if len(a) == 0:
        return [0.5]
    if len(a) == 1:
        assert 0.01 < a[0] < 0.99
        return [a[0] / 2, (a[0] + 1) / 2]
    k = int(np.argmax(np.diff(a)))
    return [float((a[k] + a[k + 1]) / 2)]


def _check(ld, cov_ref, cov_np, M, forced=(), want_structure=True):
    """cov_ref / cov_np: the longdouble and the float64 restatement of LD (ld_cov) for what the context `ld` holds."""
    from regenie_amd.ld import COV_F64, GTG_F64
    gtg_ref, gtg_np = gr.gtg_of(cov_ref, np.longdouble), gr.gtg_of(cov_np)
    cov, gtg = ld.finish(COV_F64), ld.finish(GTG_F64)
    # no diagonal entry of these inputs lies in (-tol, 0): off the diagonal the two forms are the same numbers, on it max(diag, numtol)
    assert not ((np.diag(cov) < 0) & (np.abs(np.diag(cov)) < lr.TOL)).any()
    off = ~np.eye(M, dtype=bool)
    assert np.array_equal(gtg[off], cov[off])
    assert np.array_equal(np.diag(gtg), np.maximum(np.diag(cov), lr.NUMTOL))
    every_ref = gr.sparse_of(gtg_ref, np.longdouble(0.5))[4]
    every_np = gr.sparse_of(gtg_np, 0.5)[4]
    sd_ref = np.sqrt(np.diag(gtg_ref))
    d_np_sd = float(np.max(np.abs(np.sqrt(np.diag(gtg_np)) - sd_ref) / sd_ref))
    d_np = float(np.max(np.abs(every_np - every_ref))) if len(every_ref) else 0.0
    for thr in _thresholds(every_np, M):
        for e in (every_ref, every_np):
            assert len(e) == 0 or float(np.min(np.abs(np.abs(e) - thr))) > 1e-9
        _, row_w, col_w, _, _ = gr.sparse_of(gtg_np, thr)
        _, row_l, col_l, val_l, _ = gr.sparse_of(gtg_ref, np.longdouble(thr))
        assert np.array_equal(row_w, row_l) and np.array_equal(col_w, col_l)      # the two restatements keep the same pairs
        sd, row, col, val = ld.finish_sparse(thr)
        # the count, and the (i, j) sequence: strictly ascending in row-major order, the restatement's
        assert len(row) == len(col) == len(val) == len(row_w), (len(row), len(row_w))
        key = row.astype(np.int64) * M + col
        assert np.all(row < col) and np.all(np.diff(key) > 0)
        assert np.array_equal(row, row_w) and np.array_equal(col, col_w)
        d_lib_sd = float(np.max(np.abs(sd - sd_ref) / sd_ref))
        d_lib = float(np.max(np.abs(val - val_l))) if len(val) else 0.0
        print("M=%d thr=%.6f: %d of %d pairs kept; val: numpy fp64 %.3e, library %.3e from longdouble; sd: numpy %.3e, library %.3e"
              % (M, thr, len(row), len(every_np), d_np, d_lib, d_np_sd, d_lib_sd))
        assert d_lib <= 4 * d_np, (d_lib, d_np)
        assert d_lib_sd <= 4 * d_np_sd, (d_lib_sd, d_np_sd)
        np.testing.assert_allclose(sd, np.sqrt(np.diag(gtg)), rtol=4e-16, atol=0)      # the sd line is the square root of the dense form's diagonal
        for c in forced:      # a forced-in column: sd = sqrt(numtol), no pair
            assert sd[c] == np.sqrt(lr.NUMTOL) and not (row == c).any() and not (col == c).any()
        # a second run gives the same bytes
        sd2, row2, col2, val2 = ld.finish_sparse(thr)
        assert sd2.tobytes() == sd.tobytes() and row2.tobytes() == row.tobytes() and col2.tobytes() == col.tobytes() and val2.tobytes() == val.tobytes()
        if want_structure and M > 2:
            cand = M - 1 - np.arange(M)
            kept = np.bincount(row, minlength=M)
            assert ((kept == 0) & (cand > 0)).any(), "no row without a kept pair"
            assert ((kept == cand) & (cand > 0)).any(), "no row with every pair kept"
            assert 0 < kept[0] < cand[0]
    return gtg


@pytest.mark.parametrize("M, n, C, miss_cols", [
    (1, 501, 4, (0,)),
    (2, 501, 4, (1,)),
    (65, 200, 2, (3, 40)),
    (130, 200, 3, (129,)),
    (257, 67, 1, tuple(range(128, 257, 7))),       # missing calls in the second and third row tile only
    (257, 67, 4, tuple(range(0, 128, 5))),         # in the first row tile only
])
def test_sparse_and_gtg_against_the_restatement(M, n, C, miss_cols):
    from regenie_amd.ld import LDMatrix, pack_bed_rows
    rng = np.random.default_rng(9000 + M + C)
    G = _calls(rng, M, n, miss_cols)
    X = _basis(rng, n, C)
    with LDMatrix(n, C, M) as ld:
        ld.set_basis(X.T)
        for c0 in range(0, M, 128):      # a panel is a row tile
            ld.append(pack_bed_rows(G[c0:c0 + 128]), np.arange(c0, min(c0 + 128, M)))
        _check(ld, lr.ld_cov(G.T, X, np.longdouble), lr.ld_cov(G.T, X), M)


def test_two_forced_columns():
    """Columns 1 and 69 are forced in (no variant fills them) and the variants take the others in a scrambled order."""
    from regenie_amd.ld import LDMatrix, pack_bed_rows
    rng = np.random.default_rng(9100)
    M, n, C, forced = 72, 150, 2, np.array([1, 69])
    Gv = _calls(rng, M - 2, n, (5,))
    filled = np.setdiff1d(np.arange(M), forced)
    head, mid, tail = _groups(M - 2)
    filled = np.concatenate([filled[:head], rng.permutation(filled[head:head + mid]), filled[head + mid:]])      # (the groups stay at the head and the tail)
    Gfull = np.zeros((n, M))
    Gfull[:, filled] = Gv.T
    X = _basis(rng, n, C)
    with LDMatrix(n, C, M) as ld:
        ld.set_basis(X.T)
        ld.force_columns(forced)
        ld.append(pack_bed_rows(Gv), filled)
        gtg = _check(ld, lr.ld_cov(Gfull, X, np.longdouble), lr.ld_cov(Gfull, X), M, forced=forced)
    assert np.all(gtg[forced][:, filled] == 0) and np.all(np.diag(gtg)[forced] == lr.NUMTOL)


def test_integer_dosages_at_scale_255():
    from regenie_amd.ld import LDMatrix
    rng = np.random.default_rng(9200)
    M, n, C, scale = 70, 150, 3, 255
    calls = _calls(rng, M, n, ())
    Gi = np.clip(np.rint(calls * scale + rng.integers(-60, 61, size=calls.shape)), 0, 2 * scale).astype(np.uint16)      # [M][n]
    Gi[7, rng.random(n) < 0.08] = dr.MISSING
    Gi[66, rng.random(n) < 0.08] = dr.MISSING
    X = _basis(rng, n, C)
    with LDMatrix(n, C, M) as ld:
        ld.set_basis(X.T)
        ld.append_int(Gi[:40], np.arange(40), scale)
        ld.append_int(Gi[40:], np.arange(40, M), scale)
        _check(ld, dr.ld_cov(Gi.T, scale, X, np.longdouble), dr.ld_cov(Gi.T, scale, X), M)


def test_sparse_error_paths():
    from regenie_amd.engine import RgError
    from regenie_amd.ld import LDMatrix, pack_bed_rows
    rng = np.random.default_rng(9300)
    n, M = 100, 4
    G = _calls(rng, M, n, ())
    with LDMatrix(n, 1, M) as ld:
        ld.set_basis(np.full((1, n), 1 / np.sqrt(n)))
        ld.append(pack_bed_rows(G[:3]), [0, 1, 2])
        with pytest.raises(RgError, match="neither appended nor forced"):
            ld.finish_sparse(0.5)
        ld.append(pack_bed_rows(G[3:]), [3])
        for thr in (0.0, -0.25, 1.0, 1.5, float("nan")):
            with pytest.raises(RgError, match=r"\(0, 1\)") as e:
                ld.finish_sparse(thr)
            assert e.value.code == -1      # RG_LD_ERR_ARG
        sd, row, col, val = ld.finish_sparse(1e-12)
        assert len(sd) == M and len(row) == len(col) == len(val) <= M * (M - 1) // 2
