"""K-fold level 1 of quantitative traits at one-trait shapes, on injected level-0 predictors (`rg_l0_set_w`, the pattern of
tests/test_l1_full_width_gpu.py), against the oracle's ridge_level_1 / select_tau / make_predictions / loco_from_predictions.

What is exercised: the single pass over W that forms the CV sums and the candidate predictions of every ridge value (k_l1_cvpred), the
reduction of the sums and the choice of the ridge value on the device (k_l1_select, the host rule of Data.cpp:1025-1037: first strict
minimum), the LOCO assembly / the gather that read the chosen index from device memory, and the context's staging area (tables uploaded
once per shape, ridge values and results per call).

Shapes: 1,003 samples in five folds of uneven size (150 / 260 / 201 / 192 / 200; every fold is padded to a multiple of 256 positions, so
chunks with idle tails and folds of one and of two chunks occur); L = 5, 65, 130, 545 predictors (inside one 64-tile, one past a tile
boundary, one past a 128 macro tile, the flagship's order: three 256-column coefficient tiles with a 33-column tail, 16-column load groups
with a remainder); 1 and 3 traits; three chromosomes of which the first holds a single block, so chromosome boundaries fall inside load
groups and inside coefficient tiles.  One trait: LOCO rows assembled on the device (`set_loco_output`, what bench.py runs); three traits:
per-chromosome predictions returned, LOCO rows assembled by the oracle's function from them.

Bounds: those the existing level-1 tests hold the same quantities to -- CV sums 1e-10 of their largest entry, selected index equal, LOCO rows
1e-10 of their largest entry for L <= 130 (tests/test_step1_gpu.py::test_level1_on_injected_predictors, L <= 50 there) and 1e-9 at L = 545
(tests/test_l1_full_width_gpu.py, whose systems are of the flagship's kind)."""
import functools

import numpy as np
import pytest

from oracle import regenie_step1 as orc

N = 1003
CV_SIZES = np.array([150, 260, 201, 192, 200], np.int64)
CHROMS = (2, 7, 21)                     # chromosome ids of the three column groups
R1 = 5


def layout(L):
    """(R0, blocks, [(chrom, first column, columns)]): the first chromosome holds a single block."""
    R0 = 1 if L == 5 else 5
    B = L // R0
    nb = [1, (B - 1) // 2, B - 1 - (B - 1) // 2]
    ctr = np.concatenate([[0], np.cumsum(nb)]) * R0
    return R0, B, [(CHROMS[c], int(ctr[c]), nb[c] * R0) for c in range(3)]


@functools.lru_cache(maxsize=None)
def problem(L, P):
    """Predictors shaped like level-0 output (the columns of a block: one block score, shrunk by different amounts), traits that load on them,
    covariates projected out; and the oracle's level 1 for every trait.  Computed once per shape, never modified."""
    rng = np.random.default_rng(1000 * L + P)
    R0, B, cc = layout(L)
    liab = rng.standard_normal((N, P))
    W = []
    for ph in range(P):
        Z = rng.standard_normal((N, B)) + 0.15 * liab[:, [ph]]
        E = rng.standard_normal((N, B))
        w = np.empty((N, L))
        for r, s in enumerate((0.05, 0.12, 0.2, 0.3, 0.45)[:R0]):
            w[:, r::R0] = Z + s * E
        w -= w.mean(axis=0)
        w /= w.std(axis=0, ddof=1)
        W.append(np.asfortranarray(w))
    X = np.linalg.qr(np.column_stack([np.ones(N), rng.standard_normal((N, 2))]))[0]
    Y = liab - X @ (X.T @ liab)
    Y /= np.sqrt((Y ** 2).sum(axis=0) / (N - X.shape[1]))
    tau = np.stack([orc.tau_from_h(orc.set_ridge_params(R1), L, False)] * P)
    for a in W + [X, Y, tau]:
        a.setflags(write=False)
    return dict(L=L, P=P, R0=R0, B=B, cc=cc, W=W, X=X, Y=Y, tau=tau)


@functools.lru_cache(maxsize=None)
def reference(L, P, tau_key=None):
    pr = problem(L, P)
    tau = pr["tau"] if tau_key is None else np.array(tau_key).reshape(P, -1)
    out = []
    for ph in range(P):
        cs, betas = orc.ridge_level_1(pr["W"][ph], pr["Y"][:, ph], CV_SIZES, tau[ph])
        best = orc.select_tau(cs, float(N), False)
        pred = orc.make_predictions(pr["W"][ph], betas, best, CV_SIZES, pr["cc"])
        out.append((cs, best, orc.loco_from_predictions(pred, pr["cc"], 23)))
    return out


def engine(pr, Y=None):
    from regenie_amd.engine import Step1Engine
    Y = pr["Y"] if Y is None else Y
    P = Y.shape[1]
    eng = Step1Engine(0)
    eng.set_problem(X=pr["X"], Y=Y, mask=np.ones((N, P), bool), ind_in_analysis=np.ones(N, bool), cv_sizes=CV_SIZES,
                    lam=np.array([1e3, 3e3, 1e4, 3e4, 1e5][:pr["R0"]]), neff=np.full(P, float(N)), n_file=N, n_blocks_total=pr["B"],
                    max_block_size=16)
    for ph in range(P):
        for b in range(pr["B"]):
            eng.set_w(b, ph, pr["W"][min(ph, len(pr["W"]) - 1)][:, b * pr["R0"]:(b + 1) * pr["R0"]])
    return eng


def check(pr, ref, cs, best, loco, ph):
    rcs, rbest, rloco = ref[ph]
    e_cs = np.abs(cs[ph] - rcs[:5]).max() / np.abs(rcs[:5]).max()
    e_lo = np.abs(loco - rloco).max() / np.abs(rloco).max()
    print("L=%d P=%d trait %d: CV sums rel err %.3e, best %d (oracle %d), LOCO rel err %.3e" % (pr["L"], pr["P"], ph, e_cs, int(best[ph]), rbest, e_lo))
    assert e_cs <= 1e-10
    assert int(best[ph]) == rbest
    assert e_lo <= (1e-10 if pr["L"] <= 130 else 1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [5, 65, 130, 545])
@pytest.mark.parametrize("P", [1, 3])
def test_level1_against_the_oracle(L, P):
    pr, ref = problem(L, P), reference(L, P)
    eng = engine(pr)
    cols = [nn for (_, _, nn) in pr["cc"]]
    if P == 1:
        eng.set_loco_output([c for (c, _, _) in pr["cc"]])                 # LOCO rows assembled on the device
    cs, best, pred = eng.l1_qt(pr["tau"], cols)
    for ph in range(P):
        loco = pred[ph] if P == 1 else orc.loco_from_predictions(pred[ph], pr["cc"], 23)
        assert loco.shape == (N, 23)
        check(pr, ref, cs, best, loco, ph)
    eng.close()


def tied_grid(L):
    """The ridge grid with the oracle's best value written over a neighbour: two equal candidates, the best of the grid."""
    pr = problem(L, 1)
    b = reference(L, 1)[0][1]
    tau = pr["tau"].copy()
    other = b + 1 if b + 1 < R1 else b - 1
    tau[0, other] = tau[0, b]
    return tau, min(b, other), max(b, other)


def test_duplicated_ridge_value_ties_in_the_oracle():
    """CPU, oracle alone: with a duplicated ridge value the two CV criteria are EQUAL and minimal, and the rule (Data.cpp:1025-1037, strict '<')
    keeps the first of them -- the case test_tie_keeps_the_first_minimum holds the device's selection to."""
    tau, first, second = tied_grid(65)
    cs, _, _ = reference(65, 1, tuple(tau.ravel()))[0]
    perf = (cs[2] + cs[3] - 2 * cs[4]) / float(N)
    assert perf[first] == perf[second] == perf.min()
    assert orc.select_tau(cs, float(N), False) == first


@pytest.mark.gpu
def test_tie_keeps_the_first_minimum():
    tau, first, second = tied_grid(65)
    pr = problem(65, 1)
    ref = reference(65, 1, tuple(tau.ravel()))
    eng = engine(pr)
    eng.set_loco_output([c for (c, _, _) in pr["cc"]])
    cs, best, pred = eng.l1_qt(tau, [nn for (_, _, nn) in pr["cc"]])
    perf = cs[0][2] + cs[0][3] - 2 * cs[0][4]
    print("criteria", perf, "best", int(best[0]), "first / second of the tie", first, second)
    assert perf[first] == perf[second] == perf.min()                       # the device's two candidates tie as well ...
    assert int(best[0]) == first == ref[0][1]                              # ... and the first one is kept
    check(pr, ref, cs, best, pred[0], 0)
    eng.close()


@pytest.mark.gpu
def test_second_call_on_a_context_equals_a_fresh_context():
    """Level 1 of trait 0, then of trait 1 (another y) on the SAME context -- the staged tables are reused, the ridge values and the result
    slot rewritten -- against trait 1 alone on a fresh context: bit for bit."""
    pr = problem(130, 1)
    rng = np.random.default_rng(77)
    y2 = rng.standard_normal((N, 1))
    y2 -= pr["X"] @ (pr["X"].T @ y2)
    Y = np.column_stack([pr["Y"], y2])
    cols = [nn for (_, _, nn) in pr["cc"]]
    tau2 = pr["tau"] * np.array([[1.0, 0.5, 2.0, 1.5, 1.0]])               # other ridge values too
    got = []
    for warm in (True, False):
        eng = engine(pr, Y)
        eng.set_loco_output([c for (c, _, _) in pr["cc"]])
        if warm:
            eng.set_l1_view(None, 0, 1)
            cs0, best0, pred0 = eng.l1_qt(pr["tau"], cols)
            check(pr, reference(130, 1), cs0, best0, pred0[0], 0)
        eng.set_l1_view(None, 1, 1)
        cs, best, pred = eng.l1_qt(tau2, cols)
        got.append((cs.copy(), best.copy(), pred[0].copy()))
        eng.close()
    assert np.array_equal(got[0][0], got[1][0])
    assert np.array_equal(got[0][1], got[1][1])
    assert np.array_equal(got[0][2], got[1][2])
    assert np.abs(got[0][2]).max() > 0
