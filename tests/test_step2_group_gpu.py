"""The library's counts of a block restricted to a sample group (include/rg_step2.h: rg_s2_set_group, rg_s2_group_counts_packed,
rg_s2_group_sums_int; csrc/step2_group.hip) through regenie_amd.step2, against NumPy: EXACT integer equality.  Shapes: n = 13 (less than one
16-sample word), 1003 (n % 16 != 0, n % 4 != 0), 4099 (one sample past a full 256-thread stride of 16-sample words); rows wider than ceil(n / 4)
with garbage in the padding; bs 1, 7, 65; P 1 and 3 with distinct masks, one of them all-zero; the group empty, full and random; flip; every
coding (the counts stay additive and the score outputs are those of a context without a group, bit for bit); a row that is entirely missing;
integer rows at scale 255 and 16384 with values up to 2 * scale and missing entries, host and device pointers."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = (13, 1003, 4099)


def _calls(rng, bs, n):
    g = rng.integers(0, 3, size=(bs, n)).astype(np.int8)
    g[rng.random((bs, n)) < 0.07] = -3
    g[bs // 2] = -3                                                  # a row that is entirely missing
    return g


def _pack(g, ld, rng):
    """.bed coding (00 -> 2, 01 -> missing, 10 -> 1, 11 -> 0), rows ld bytes apart, garbage in every padding bit and byte."""
    bs, n = g.shape
    code = rng.integers(0, 4, size=(bs, ld * 4)).astype(np.uint8)
    code[:, :n] = np.where(g == 2, 0, np.where(g == 1, 2, np.where(g < 0, 1, 3)))
    c = code.reshape(bs, ld, 4)
    return (c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)).astype(np.uint8)


def _masks(rng, P, n):
    m = (rng.random((P, n)) > 0.2).astype(np.uint8)
    if P > 1:
        m[1] = 0                                                     # a trait nobody is observed for
    return m


def _planes(member, masks):
    return np.concatenate([member[None, :] != 0, (member[None, :] != 0) & (masks != 0)], axis=0)      # [1 + P][n]


def _want_counts(g, planes, flip):
    gg = np.where(g < 0, g, 2 - g) if flip else g
    out = np.zeros((g.shape[0], planes.shape[0], 3), np.int64)
    for q, pl in enumerate(planes):
        out[:, q, 0] = ((gg == 1) & pl[None, :]).sum(axis=1)
        out[:, q, 1] = ((gg == 2) & pl[None, :]).sum(axis=1)
        out[:, q, 2] = ((gg >= 0) & pl[None, :]).sum(axis=1)
    return out


def _null(rng, n, C, P, masks):
    X = np.linalg.qr(np.column_stack([np.ones(n), rng.normal(size=(n, C - 1))]))[0]
    Y = rng.normal(size=(n, P)) * masks.T
    return X.T.copy(), Y.T.copy(), rng.uniform(0.5, 2.0, size=P)


def _group(rng, kind, n):
    return {"empty": np.zeros(n, np.uint8), "full": np.ones(n, np.uint8), "random": (rng.random(n) < 0.5).astype(np.uint8)}[kind]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("P", (1, 3))
def test_group_counts_packed(n, P):
    from regenie_amd.step2 import Step2QT
    rng = np.random.default_rng(1000 * n + P)
    C = 3
    masks = _masks(rng, P, n)
    X, Y, scf = _null(rng, n, C, P, masks)
    with Step2QT(n, C, P) as s2:
        s2.set_null(X, Y, masks, scf)
        for bs in (1, 7, 65):
            g = _calls(rng, bs, n)
            for ld in ((n + 3) // 4, (n + 3) // 4 + 5):              # the second: rows that do not start on a 4-byte boundary
                rows = _pack(g, ld, rng)
                for kind in ("empty", "full", "random"):
                    member = _group(rng, kind, n)
                    s2.set_group(member)
                    for flip in (False, True):
                        got = s2.group_counts(rows, flip=flip)
                        assert got.dtype == np.int32 and np.array_equal(got, _want_counts(g, _planes(member, masks), flip)), (n, P, bs, ld, kind, flip)
        # masks handed over with the group (a binary-trait caller), and the masks of a later set_null
        other = _masks(rng, P, n)[::-1].copy()
        member = _group(rng, "random", n)
        s2.set_group(member, mask=other)
        assert np.array_equal(s2.group_counts(rows), _want_counts(g, _planes(member, other), False))
        s2.set_group(member)
        s2.set_null(X, Y * other, other, scf)
        assert np.array_equal(s2.group_counts(rows), _want_counts(g, _planes(member, other), False))
        s2.set_group(None)
        with pytest.raises(Exception):
            s2.group_counts(rows)


def test_group_counts_device_rows():
    import torch
    from regenie_amd.step2 import Step2QT
    n, P, C, bs = 4099, 3, 3, 7
    rng = np.random.default_rng(5)
    masks = _masks(rng, P, n)
    X, Y, scf = _null(rng, n, C, P, masks)
    g = _calls(rng, bs, n)
    member = _group(rng, "random", n)
    with Step2QT(n, C, P) as s2:
        s2.set_null(X, Y, masks, scf)
        s2.set_group(member)
        for ld in ((n + 3) // 4 + 3, (n + 3) // 4 + 1):              # 4-byte aligned rows and rows that are not
            rows = _pack(g, ld, rng)
            t = torch.from_numpy(rows).cuda()
            for flip in (False, True):
                assert np.array_equal(s2.group_counts(t, flip=flip), _want_counts(g, _planes(member, masks), flip))
            assert np.array_equal(t.cpu().numpy(), rows)             # read in place, not written


@pytest.mark.parametrize("coding", (0, 1, 2))
def test_counts_stay_additive_and_scores_are_untouched(coding):
    """The same call sequence on a context with a group and on one without: bit-equal score outputs; the group's counts are the additive ones."""
    from regenie_amd.step2 import Step2QT
    n, P, C, bs = 1003, 3, 4, 65
    rng = np.random.default_rng(77 + coding)
    masks = _masks(rng, P, n)
    masks[1] = (rng.random(n) > 0.1)                                 # (every trait observed somewhere: the statistics are finite)
    X, Y, scf = _null(rng, n, C, P, masks)
    g = _calls(rng, bs, n)
    member = _group(rng, "random", n)
    rows = _pack(g, (n + 3) // 4 + 2, rng)
    out = []
    for with_group in (False, True):
        with Step2QT(n, C, P) as s2:
            s2.set_coding(coding)
            s2.set_null(X, Y, masks, scf)
            if with_group:
                s2.set_group(member)
            for flip in (False, True):
                res = s2.score_block_packed(rows, flip=flip)
                if with_group:
                    assert np.array_equal(s2.group_counts(rows, flip=flip), _want_counts(g, _planes(member, masks), flip))
                res["packed_counts"] = s2.packed_counts(bs)         # the staged block is still the score call's
                res["moments"] = s2.qt_moments(np.arange(0, bs, 9))["sums"]
                out.append(res)
    for a, b in zip(out[:2], out[2:]):
        for k in ("stats", "bhat", "scale_fac", "mean", "n_obs", "ignored", "total_p", "n_obs_p", "packed_counts", "moments"):
            assert a[k].tobytes() == b[k].tobytes(), (coding, k)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("scale", (255, 16384))
def test_group_sums_int(n, scale):
    import torch
    from regenie_amd.step2 import Step2QT
    P, C = 3, 3
    rng = np.random.default_rng(31 * n + scale)
    masks = _masks(rng, P, n)
    X, Y, scf = _null(rng, n, C, P, masks)
    with Step2QT(n, C, P) as s2:
        s2.set_null(X, Y, masks, scf)
        for bs in (1, 7, 65):
            G = rng.integers(0, 2 * scale + 1, size=(bs, n)).astype(np.uint16)
            G[:, :3] = 2 * scale
            G[rng.random((bs, n)) < 0.05] = 0xFFFF
            G[bs // 2] = 0xFFFF
            for kind in ("empty", "full", "random"):
                member = _group(rng, kind, n)
                s2.set_group(member)
                planes = _planes(member, masks)
                obs = G != 0xFFFF
                want = np.zeros((bs, 1 + P, 2), np.int64)
                for q, pl in enumerate(planes):
                    want[:, q, 0] = np.where(obs & pl[None, :], G, 0).astype(np.int64).sum(axis=1)
                    want[:, q, 1] = (obs & pl[None, :]).sum(axis=1)
                got = s2.group_sums_int(G)
                assert got.dtype == np.int64 and np.array_equal(got, want), (n, scale, bs, kind)
                wide = np.full((bs, n + 5), 0x1234, np.uint16)       # a row pitch above n, garbage behind the samples
                wide[:, :n] = G
                t = torch.from_numpy(wide.view(np.int16)).cuda()
                assert np.array_equal(s2.group_sums_int(t), want), (n, scale, bs, kind, "device")
