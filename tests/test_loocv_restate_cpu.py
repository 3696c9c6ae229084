"""Pins the yardstick of the leave-one-out level-0 kernel tests (tests/loocv_restate.py) on the CPU.

  * the shortcut formula means leave-one-out: at bs = 5, N = 40, P = 2 the restatement equals a refit of the ridge regression without
    sample i, for every i, in long double;
  * at every case of the GPU sweep (tests/test_loocv_tri_gpu.py draws the same inputs) the two fp64 routes -- the oracle's
    eigendecomposition and the fp64 run of the restatement -- agree with the long-double run closely enough that the bound the device is
    held to, 10 max(d64, 1.04e-14) per column, stays under its cap of 1e-11, and the inputs are well-posed;
  * the bound is tight enough to see a lost tail: dropping the terms k >= (bs & ~3) of the sums (the recurrence kernel's tail loop)
    puts the restatement itself outside it."""
import numpy as np
import pytest

from tests import loocv_restate as lr

LD = lr.LD
EPS_LD = float(np.finfo(LD).eps)


def test_long_double_is_extended_precision():
    assert lr.have_extended_precision(), np.finfo(LD)


def test_cholesky_and_solves_in_long_double():
    rng = np.random.default_rng(2)
    B = rng.standard_normal((9, 30)).astype(LD)
    M = B @ B.T + LD(0.5) * np.eye(9, dtype=LD)
    L = lr.cholesky(M)
    assert L.dtype == LD and not np.triu(L, 1).any()
    assert float(np.abs(L @ L.T - M).max() / np.abs(M).max()) < 50 * EPS_LD
    R = rng.standard_normal((9, 4)).astype(LD)
    assert float(np.abs(L @ lr.forward(L, R) - R).max()) < 1e3 * EPS_LD
    assert float(np.abs(L.T @ lr.backward_t(L, R) - R).max()) < 1e3 * EPS_LD
    with pytest.raises(np.linalg.LinAlgError):
        lr.cholesky(M - LD(1e6) * np.eye(9, dtype=LD))


def test_restatement_is_leave_one_out_by_refitting():
    """bs = 5, N = 40, P = 2, five ridge values: every predictor against the refit without its sample.  Both sides are long double; the
    refit solves a system whose condition number is at most (d_max + lambda) / lambda, so they may differ by that times a few hundred eps."""
    rng = np.random.default_rng(5)
    bs, N, P = 5, 40, 2
    raw = rng.binomial(2, rng.uniform(0.2, 0.5, (bs, 1)), (bs, N)).astype(np.float64)
    raw[1, 7] = raw[3, 20] = -3
    ain = np.ones(N, bool)
    ain[[4, 31]] = False
    X = np.linalg.qr(np.column_stack([np.ones(N), rng.standard_normal((N, 2))]) * ain[:, None])[0] * ain[:, None]
    mask = np.repeat(ain[:, None], P, axis=1)
    mask[11, 0] = mask[12, 1] = False
    Y = rng.standard_normal((N, P)) * mask
    neff = mask.sum(axis=0).astype(np.float64)
    lam = bs * (1 - np.array([0.01, 0.25, 0.5, 0.75, 0.99])) / np.array([0.01, 0.25, 0.5, 0.75, 0.99])
    G, _ = lr.standardise_genotypes(raw, ain, X, int(ain.sum()), LD)
    fast, H = lr.level0_raw(G, Y, lam, LD)
    slow = lr.brute_force_raw(G, Y, lam, LD)
    dmax = float(np.linalg.eigvalsh((G @ G.T).astype(np.float64)).max())
    for r in range(lam.size):
        tol = 500 * EPS_LD * (dmax + lam[r]) / lam[r]
        dev = float(np.abs(fast[:, :, r] - slow[:, :, r]).max() / np.abs(slow[:, :, r]).max())
        print("lambda %.3g: shortcut against refit %.3g (tolerance %.3g)" % (lam[r], dev, tol))
        assert dev <= tol, (r, dev, tol)
    # and the standardised columns (what the tests compare) follow from the same numbers
    a = lr.standardise_predictors(fast, mask, neff, LD)
    b = lr.standardise_predictors(slow, mask, neff, LD)
    assert float(np.abs(a - b).max()) <= 1e-15
    assert not a[0, 11].any() and not a[1, 12].any() and not a[:, 4].any()
    for p in range(P):       # each column: mean 0 over the observed samples, unit sample variance
        m = mask[:, p]
        assert float(np.abs(a[p][m].sum(axis=0)).max()) < 1e-15
        assert float(np.abs((a[p][m] ** 2).sum(axis=0) / (neff[p] - 1) - 1).max()) < 1e-15
    # the samples outside the analysis have no leverage
    assert not H[~ain].any()


@pytest.mark.parametrize("case_id", lr.CASE_IDS)
def test_fp64_routes_against_long_double_at_the_sweep_cases(case_id):
    pr = lr.problem(case_id)
    refs = lr.references(case_id)
    p = pr.prep
    assert (p.Neff >= 2).all()
    assert p.mask[~p.ind_in_analysis].sum() == 0
    for b, ref in enumerate(refs):
        print("%s block %d (order %d): d_orc %.3g  d_f64 %.3g  bound %.3g  min(1 - h) %.3g  min scale %.3g"
              % (case_id, b, pr.blocks[b], ref.d_orc.max(), ref.d_f64.max(), ref.bound.max(), ref.one_minus_h_min, ref.scale_min))
        assert ref.W_ld.dtype == LD and np.isfinite(ref.W_ld.astype(np.float64)).all()
        assert ref.scale_min > 0.1, "a SNP near the low-variance check"           # the check itself is at 1e-6
        assert ref.one_minus_h_min > 1e-3, "a leverage next to 1"
        for ph in range(len(ref.W_ld)):
            assert not ref.W_ld[ph][~p.mask[:, ph]].any()
        assert (ref.d_orc <= ref.bound).all() and (ref.d_f64 <= ref.bound).all()
        assert (ref.bound <= lr.CAP).all(), "the fp64 routes disagree by more than a tenth of the cap: the case is not well-posed"
        assert (ref.bound >= 10 * lr.FLOOR).all()


@pytest.mark.parametrize("case_id", [c["id"] for c in lr.CASES if any(bs & 3 for bs in c["blocks"]) and c["N"] <= 2000])
def test_the_bound_sees_a_lost_tail(case_id):
    """What the device computes when k_tri_rec's tail loop (k = n & ~3 .. n - 1) is lost, restated: the last n & 3 terms of the leverage
    and numerator sums dropped.  Every block whose order is no multiple of four must then leave its bound in every column (or stop being
    a number: an order below four loses every term)."""
    pr = lr.problem(case_id)
    refs = lr.references(case_id)
    for b, bs in enumerate(pr.blocks):
        if not bs & 3:
            continue
        dev = lr.column_dev(lr.restated(pr, b, np.float64, omit="tail")["W"], refs[b].W_ld)
        print("%s block %d (order %d): without the tail %.3g .. %.3g, bound %.3g" % (case_id, b, bs, dev.min(), dev.max(), refs[b].bound.max()))
        assert not (dev <= refs[b].bound).any(), (b, bs, dev, refs[b].bound)
