"""The leave-one-out level 0 (regenie_amd/csrc/loocv_tri.hip with k_decode_gt and k_loocv_std of loocv.hip) at its kernel edges, held to the
long-double restatement (tests/loocv_restate.py; pinned on the CPU by tests/test_loocv_restate_cpu.py, which draws the same cases).

Route: Step1Engine.set_problem(cv_sizes=None), every block of a case in ONE l0_blocks_host call (l0_blocks_f64_host for the dosage case),
sync, get_w.  What each case reaches:
  order1                 no reduction step at all, the recurrence's tail loop only (n & ~3 = 0), P = 1, no covariate beside the intercept
  orders2_3_1_5          order 2 (only the tau = 0 last step), 3 (the first real reflector), 1 and 5 in one batch (early returns for some
                         blocks of a launch); N one past 128
  slab_edges             63, 64, 65: the 64-wide slabs of the Qt update and the 64-tile of the transform; k_tri_rec<5> with padded table
                         rows (P = 3); eight ridge values (512-thread workgroups)
  singular130_1_66       a third slab; order 1 beside order 130; SNP 129 a copy of SNP 0 and SNP 65 the complement of SNP 1 (A exactly
                         singular); P = 5, two ridge values
  P6, P10, P11           k_tri_rec<TRI_PG>: a partial group, a full one, a second group with one trait; 48, 80, 88 threads in k_tri_tables
  C17, C33               one ridge value; the second and third group of sixteen covariates in k_decode_gt
  more_snps_than_samples 64 SNPs, 50 samples: the trailing matrix of the reduction is rounding noise
  second_chunk           65,729 samples: a second, partial chunk of sample positions on the TRI_PG path
  bt_missing_removed_ref_first  binary traits, phenotypes missing per trait, missing calls, samples outside the analysis, --ref-first
  dosages                the other caller (l0_blocks_f64_host): dosages in units of 1/255, a few missing

Bound, per column (block, ridge value, trait): dev = max_i |W_gpu - W_ld| / max_i |W_ld| <= 10 max(d64, 1.04e-14), d64 the larger of the same
quantity for the oracle's eigen route and for the fp64 run of the restatement -- one decimal order for a device fp64 routine over two host
ones, as tests/test_rerint_gpu.py gives; nothing in it comes from the device.  Measured: profiles/loocv_tri_tests.md."""
import numpy as np
import pytest

from tests import loocv_restate as lr

pytestmark = pytest.mark.gpu

_dev = {}


def _engine(pr, lam=None):
    from regenie_amd.engine import Step1Engine
    p = pr.prep
    eng = Step1Engine(0)
    eng.set_problem(X=p.X, Y=p.Y, mask=p.mask, ind_in_analysis=p.ind_in_analysis, cv_sizes=None, lam=pr.lam if lam is None else lam,
                    neff=p.Neff, n_file=p.n_file, n_blocks_total=len(pr.blocks), max_block_size=max(pr.blocks), ref_first=pr.ref_first)
    return eng


def _level0(eng, pr, order=None):
    """One level-0 call for the blocks in `order` (default: all, as listed); returns [block] -> (P, N, R0)."""
    order = list(range(len(pr.blocks))) if order is None else order
    call = eng.l0_blocks_f64_host if pr.dosage else eng.l0_blocks_host
    call(order, [pr.rows[b] for b in order])
    eng.sync()
    return {b: np.stack([eng.get_w(b, ph) for ph in range(pr.prep.Y.shape[1])]) for b in order}


def _device(case_id):
    """The case on the device, once per session: the first call's predictors and a second call's on the same engine."""
    if case_id not in _dev:
        pr = lr.problem(case_id)
        eng = _engine(pr)
        try:
            first = _level0(eng, pr)
            second = _level0(eng, pr)
        finally:
            eng.close()
        _dev[case_id] = (first, second)
    return _dev[case_id]


@pytest.mark.parametrize("case_id", lr.CASE_IDS)
def test_every_column_against_long_double(case_id):
    pr = lr.problem(case_id)
    refs = lr.references(case_id)
    got, _ = _device(case_id)
    bad = []
    for b, ref in enumerate(refs):
        dev = lr.column_dev(got[b], ref.W_ld)                      # (P, R0)
        print("%s block %d (order %d): dev %.3g  d64 %.3g  bound %.3g" % (case_id, b, pr.blocks[b], dev.max(), ref.d64.max(), ref.bound.max()))
        for ph, r in zip(*np.nonzero(~(dev <= ref.bound))):
            rows = np.argsort(-np.abs(got[b][ph, :, r] - ref.W_ld[ph, :, r]).astype(np.float64))[:4]
            bad.append("block %d (order %d) ridge value %d trait %d: dev %.3g > bound %.3g (d64 %.3g), worst samples %s"
                       % (b, pr.blocks[b], r, ph, dev[ph, r], ref.bound[ph, r], ref.d64[ph, r], rows.tolist()))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case_id", lr.CASE_IDS)
def test_masked_entries_are_zero_and_nothing_is_nan(case_id):
    pr = lr.problem(case_id)
    got, _ = _device(case_id)
    for b in range(len(pr.blocks)):
        assert np.isfinite(got[b]).all(), b
        for ph in range(got[b].shape[0]):
            assert not got[b][ph][~pr.prep.mask[:, ph]].any(), (b, ph)
            assert got[b][ph][pr.prep.mask[:, ph]].any(), (b, ph)


@pytest.mark.parametrize("case_id", lr.CASE_IDS)
def test_a_second_call_gives_the_same_bytes(case_id):
    first, second = _device(case_id)
    for b in first:
        assert first[b].tobytes() == second[b].tobytes(), b


def test_a_block_does_not_depend_on_its_neighbours_in_the_batch():
    """The blocks of singular130_1_66 submitted as [1, 66, 130], and the two small ones without the large one (a smaller largest order in
    the batch: fewer step launches, a narrower transform): the same bytes per block."""
    pr = lr.problem("singular130_1_66")
    want, _ = _device("singular130_1_66")
    eng = _engine(pr)
    try:
        got = _level0(eng, pr, [1, 2, 0])
        for b in (0, 1, 2):
            assert got[b].tobytes() == want[b].tobytes(), ("order [1, 66, 130]", b)
        got = _level0(eng, pr, [1, 2])
        for b in (1, 2):
            assert got[b].tobytes() == want[b].tobytes(), ("batch [1, 66]", b)
    finally:
        eng.close()


def test_nine_ridge_values_are_refused_and_the_engine_stays_usable():
    """The leave-one-out level 0 serves at most eight ridge values (one wave each in k_tri_rec's 512-thread workgroup).  rg_set_problem
    refuses a ninth for either cross-validation scheme, so the level-0 call's own check ("more than 8 ridge values") cannot be reached through
    the ABI; the refusal is asserted where it happens."""
    from regenie_amd.engine import RgError, Step1Engine
    pr = lr.problem("orders2_3_1_5")
    p = pr.prep
    eng = Step1Engine(0)
    try:
        with pytest.raises(RgError, match=r"n_ridge_l0 must be in \[1,8\]|more than 8 ridge values"):
            eng.set_problem(X=p.X, Y=p.Y, mask=p.mask, ind_in_analysis=p.ind_in_analysis, cv_sizes=None, lam=np.linspace(1.0, 9.0, 9),
                            neff=p.Neff, n_file=p.n_file, n_blocks_total=len(pr.blocks), max_block_size=max(pr.blocks))
            eng.l0_blocks_host(list(range(len(pr.blocks))), pr.rows)
        eng.set_problem(X=p.X, Y=p.Y, mask=p.mask, ind_in_analysis=p.ind_in_analysis, cv_sizes=None, lam=pr.lam, neff=p.Neff,
                        n_file=p.n_file, n_blocks_total=len(pr.blocks), max_block_size=max(pr.blocks))
        got = _level0(eng, pr)
    finally:
        eng.close()
    want, _ = _device("orders2_3_1_5")
    for b in want:
        assert got[b].tobytes() == want[b].tobytes(), b


def test_a_negative_ridge_value_is_reported():
    """lambda = -1e9 makes every pivot of T + lambda I negative: k_tri_tables flags it and sync() reports it -- never a silent matrix of
    garbage.  (rg_set_problem accepts the value: the check is the deferred one.)  The flag is cleared with the report: a second sync is clean."""
    from regenie_amd.engine import RgError
    pr = lr.problem("orders2_3_1_5")
    eng = _engine(pr, lam=np.array([-1e9]))
    try:
        eng.l0_blocks_host(list(range(len(pr.blocks))), pr.rows)
        with pytest.raises(RgError, match="not positive definite"):
            eng.sync()
        eng.sync()
    finally:
        eng.close()
