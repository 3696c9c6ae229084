"""The coded mode of the device BGEN decoder (rg_bgen_dev_set_coding, csrc/bgen_inflate.hip: `--test dominant | recessive`) against a NumPy decode of
the file's probability bytes: the uint16 rows hold P(het) + P(hom) or P(hom) of the counted allele in units of 1 / 255, 0xFFFF for a missing sample,
and every sum -- allele total, info numerator, observed samples, the per-trait ones -- is bit for bit what the additive mode returns.  A file with
genuine probabilities and missing samples, 203 samples (no multiple of the walk's 4 samples per thread), a sample subset with trait masks, both
allele orders; and the integer entries of the Step-2 library on such rows (binary traits: no minor-allele flip, values up to `scale`)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
M, N = 40, 203


@pytest.fixture(scope="module")
def soft(tmp_path_factory):
    from tests.util import synth_dosages, write_synth_bgen
    prefix = str(tmp_path_factory.mktemp("bgen_coded") / "soft")
    write_synth_bgen(prefix, synth_dosages(M, N, miss_rate=0.03, seed=5), [1] * M, seed=5, soft=0.5)
    return prefix + ".bgen"


def _bytes(f, idx):
    blocks = f.read_blocks(idx)
    n = f.n_samples
    miss = (blocks[:, 8:8 + n] & 0x80) != 0
    pr = blocks[:, 10 + n:10 + 3 * n].reshape(len(idx), n, 2).astype(np.int64)
    return miss, pr[:, :, 0], pr[:, :, 1]


@pytest.mark.parametrize("subset", [False, True])
@pytest.mark.parametrize("ref_first", [False, True])
def test_device_rows_are_coded_and_sums_stay_additive(soft, ref_first, subset):
    from regenie_amd.bgen import BgenDevice, BgenFile
    rng = np.random.default_rng(2)
    with BgenFile(soft) as f, BgenDevice() as d:
        idx = np.arange(M)
        comp, off, clen, ulen = f.read_compressed(idx)
        miss, b0, b1 = _bytes(f, idx)
        b2 = np.maximum(255 - b0 - b1, 0)
        assert ((b1 > 0) & (b1 < 255)).any() and miss.any()
        fi = np.sort(rng.choice(N, 150, replace=False)) if subset else None
        mask = (rng.random((3, 150)) > 0.1).astype(np.uint8) if subset else None
        d.set_samples(N, file_idx=fi, mask=mask)
        cols = fi if subset else np.arange(N)
        base = d.decode(comp, off, clen, ulen, ref_first=ref_first)
        for coding, want in ((1, b1 + b2 if ref_first else b0 + b1), (2, b2 if ref_first else b0), (0, None)):
            d.set_coding(coding)
            got = d.decode(comp, off, clen, ulen, ref_first=ref_first)
            assert (got["status"] == 0).all()
            for k in ("sum_q", "sum_info", "n_obs", "max_q") + (("sum_q_t", "sum_info_t", "n_obs_t") if subset else ()):
                assert np.array_equal(got[k], base[k]), (coding, k)
            if coding == 0:
                assert np.array_equal(got["g16"], base["g16"])
                continue
            exp = np.where(miss, 0xFFFF, want)[:, cols].astype(np.uint16)
            assert np.array_equal(got["g16"], exp), coding
            assert not got["g16_pad"].any() and exp[exp != 0xFFFF].max() == 255


@pytest.mark.parametrize("coding", [1, 2])
def test_integer_entries_on_coded_rows(soft, coding):
    """rg_s2_qt_block_int against the NumPy restatement's formulas on the coded values, and rg_s2_bt_score_int against the oracle: rows whose largest
    value is `scale`, mean at most 1, so flip_geno's branch is not taken (the statistic has the sign of the coding given)."""
    from oracle import regenie_step2_bt as bt
    from regenie_amd.bgen import BgenFile
    from regenie_amd.step2 import Step2QT
    from tests.test_step2_bt_gpu import _nulls
    with BgenFile(soft) as f:
        miss, b0, b1 = _bytes(f, np.arange(M))
    q = np.where(miss, 0xFFFF, b0 + b1 if coding == 1 else b0).astype(np.uint16)
    q[0] = np.where(miss[0], 0xFFFF, 255)                    # every observed value at the scale: mean exactly 1
    q[1, ~miss[1]] = np.where(np.arange((~miss[1]).sum()) % 5 == 0, 0, 255)      # mean 0.8
    G = np.where(q == 0xFFFF, np.nan, q / 255.0)
    rng = np.random.default_rng(4)
    X = np.linalg.qr(np.column_stack([np.ones(N), rng.normal(size=(N, 2))]))[0]
    off = 0.3 * rng.normal(size=(N, 2))
    y = (rng.random((N, 2)) < 1 / (1 + np.exp(-(-0.5 + off)))).astype(np.float64)
    mask = rng.random((N, 2)) > 0.05
    nulls, fo = _nulls(X, off, y, mask)
    with Step2QT(N, 3, 2) as s2:
        s2.set_sparse_rule(N, 0.5, False)
        s2.bt_set_null(X.T, y.T, mask.T, np.array([nl["p"] for nl in nulls]), firth_offset=fo)
        s2.set_coding(coding)
        got = s2.bt_score_int(q, 255)
    assert q[q != 0xFFFF].max() == 255 and np.nanmean(G[0]) == 1.0
    checked = 0
    for j in range(M):
        mu = np.nanmean(G[j])
        g = np.where(np.isnan(G[j]), mu, G[j])
        assert got["mean"][j] == pytest.approx(mu, rel=1e-12) and mu <= 1.0
        sparse = int((g != 0).sum()) <= 0.5 * N
        assert bool(got["sparse"][j]) == sparse
        for t in range(2):
            ref = bt.score_bt(g, X, y[:, t], mask[:, t].astype(float), nulls[t], sparse=sparse)
            if ref is None:
                assert got["test_ignored"][j, t]
                continue
            assert got["stats"][j, t] == pytest.approx(ref["stats"], rel=1e-9, abs=1e-10)
            assert got["bhat"][j, t] == pytest.approx(ref["bhat"], rel=1e-9, abs=1e-12)
            checked += 1
    assert checked > M
