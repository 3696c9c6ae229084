"""The library's allele counts among the cases of each trait (include/rg_step2.h: rg_s2_set_cases, rg_s2_case_counts_packed, rg_s2_case_sums_int,
rg_s2_group_counts_last, rg_s2_group_sums_last; csrc/step2_group.hip) through regenie_amd.step2, against NumPy: EXACT integer equality.
Shapes: n = 1 / 15 / 16 / 17 (a partial plane word, a partial row byte, one word, one sample past it), 1023, 4099 (more than one pass of 256 lanes
over eight-sample groups and over 16-sample words); P = 1 / 7 / 8 / 9 / 64 (both sides of a chunk of eight planes, RG_S2_MAX_PHENO); bs 1 and 33;
row pitches that are exact, padded and odd (the byte-wise and value-wise read paths) and multiples of 4 bytes / 8 values (the word and 16-byte
loads); flip; host and device rows; a row that is all missing; a trait without cases; a trait whose mask is all zero; uint16 rows holding 0,
65534 and 0xFFFF."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = (1, 15, 16, 17, 1023, 4099)
PS = (1, 7, 8, 9, 64)
BSS = (1, 33)
C = 3


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


def _setup(rng, n, P):
    """masks [P][n] (trait 2, when there is one, all zero), is_case [P][n] (the last trait without cases), the null model's arrays."""
    masks = (rng.random((P, n)) > 0.2).astype(np.uint8)
    is_case = (rng.random((P, n)) < 0.35).astype(np.uint8)
    if P > 2:
        masks[2] = 0
    is_case[P - 1] = 0
    X = np.linalg.qr(np.column_stack([np.ones(n), rng.normal(size=(n, C - 1))]))[0] if n > C else np.zeros((n, C))
    Y = rng.normal(size=(n, P)) * masks.T
    return masks, is_case, X.T.copy(), Y.T.copy(), rng.uniform(0.5, 2.0, size=P)


def _want_counts(g, planes, flip):
    gg = np.where(g < 0, g, 2 - g) if flip else g
    pl = planes.astype(np.int64).T                                   # [n][Q]
    return np.stack([(gg == 1).astype(np.int64) @ pl, (gg == 2).astype(np.int64) @ pl, (gg >= 0).astype(np.int64) @ pl], axis=2)


def _want_sums(G, planes):
    obs = G != 0xFFFF
    pl = planes.astype(np.int64).T
    return np.stack([np.where(obs, G, 0).astype(np.int64) @ pl, obs.astype(np.int64) @ pl], axis=2)


def _dosages(rng, bs, n):
    G = rng.integers(0, 65535, size=(bs, n)).astype(np.uint16)
    G[rng.random((bs, n)) < 0.3] = 65534
    G[rng.random((bs, n)) < 0.1] = 0
    G[rng.random((bs, n)) < 0.05] = 0xFFFF
    G[bs // 2] = 0xFFFF
    return G


def _byte_pitches(n):
    nb = (n + 3) // 4
    return nb, (nb + 5) | 1, (nb + 7) // 4 * 4                       # exact, padded and odd, a multiple of 4


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("P", PS)
def test_case_counts_packed(n, P):
    import torch
    from regenie_amd.step2 import Step2QT
    rng = np.random.default_rng(1000 * n + P)
    masks, is_case, X, Y, scf = _setup(rng, n, P)
    planes = (is_case != 0) & (masks != 0)
    with Step2QT(n, 0, P) as s2:                                     # no covariate basis: a context for the count entries alone (n = 1 has no other)
        s2.set_cases(is_case, mask=masks)                            # (the masks handed over: such a context takes no null model)
        for bs in BSS:
            g = _calls(rng, bs, n)
            for ld in _byte_pitches(n):
                rows = _pack(g, ld, rng)
                t = torch.from_numpy(rows).cuda()
                for flip in (False, True):
                    want = _want_counts(g, planes, flip)
                    got = s2.case_counts(rows, flip=flip)
                    assert got.dtype == np.int32 and got.shape == (bs, P, 3) and np.array_equal(got, want), (n, P, bs, ld, flip, "host")
                    got_d = s2.case_counts(t, flip=flip)
                    assert np.array_equal(got_d, want), (n, P, bs, ld, flip, "device")
                    assert got_d.tobytes() == s2.case_counts(t, flip=flip).tobytes()
                assert np.array_equal(t.cpu().numpy(), rows)         # read in place, not written


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("P", PS)
def test_case_sums_int(n, P):
    import torch
    from regenie_amd.step2 import Step2QT
    rng = np.random.default_rng(77 * n + P)
    masks, is_case, X, Y, scf = _setup(rng, n, P)
    planes = (is_case != 0) & (masks != 0)
    with Step2QT(n, 0, P) as s2:                                     # no covariate basis: a context for the count entries alone (n = 1 has no other)
        s2.set_cases(is_case, mask=masks)                            # (the masks handed over: such a context takes no null model)
        for bs in BSS:
            G = _dosages(rng, bs, n)
            want = _want_sums(G, planes)
            got = s2.case_sums_int(G)
            assert got.dtype == np.int64 and got.shape == (bs, P, 2) and np.array_equal(got, want), (n, P, bs, "host")
            host_wide = np.full((bs, n + 3), 0x4321, np.uint16)
            host_wide[:, :n] = G
            assert np.array_equal(s2.case_sums_int(host_wide), want), (n, P, bs, "host, padded")
            for ld in ((n + 7) // 8 * 8, (n + 5) | 1):               # 16-byte loads; rows that do not start on a 16-byte boundary
                wide = np.full((bs, ld), 0x1234, np.uint16)
                wide[:, :n] = G
                t = torch.from_numpy(wide.view(np.int16)).cuda()
                got_d = s2.case_sums_int(t)
                assert np.array_equal(got_d, want), (n, P, bs, ld, "device")
                assert got_d.tobytes() == s2.case_sums_int(t).tobytes()
                assert np.array_equal(t.cpu().numpy().view(np.uint16), wide)
            # a pitch of a multiple of 8 values on a base address that is not a multiple of 16 bytes
            ld = (n + 7) // 8 * 8
            flat = torch.from_numpy(np.full(bs * ld + 1, 0x1234, np.uint16).view(np.int16)).cuda()
            off = flat[1:].view(bs, ld)
            off[:, :n] = torch.from_numpy(G.view(np.int16)).cuda()
            assert np.array_equal(s2.case_sums_int(off), want), (n, P, bs, "device, odd base")


@pytest.mark.parametrize("n,P", [(17, 1), (1023, 8), (4099, 9), (1023, 64)])
def test_with_a_group_both_outputs_are_those_of_the_separate_calls(n, P):
    """One launch over the group's and the cases' planes: the case entry returns what it returns without a group, and the group's part of that
    launch is what the group entries return for the same rows."""
    from regenie_amd.step2 import Step2QT
    rng = np.random.default_rng(5 * n + P)
    masks, is_case, X, Y, scf = _setup(rng, n, P)
    member = (rng.random(n) < 0.5).astype(np.uint8)
    bs = 33
    g = _calls(rng, bs, n)
    rows = _pack(g, (n + 3) // 4 + 2, rng)
    G = _dosages(rng, bs, n)
    gplanes = np.concatenate([member[None, :] != 0, (member[None, :] != 0) & (masks != 0)], axis=0)
    cplanes = (is_case != 0) & (masks != 0)
    with Step2QT(n, C, P) as a, Step2QT(n, C, P) as b, Step2QT(n, C, P) as c:
        for s2 in (a, b, c):
            s2.set_null(X, Y, masks, scf)
        a.set_cases(is_case)
        b.set_group(member)
        c.set_group(member)
        c.set_cases(is_case)                                         # both, in the order the driver sets them
        for flip in (False, True):
            cc, gc = a.case_counts(rows, flip=flip), b.group_counts(rows, flip=flip)
            assert np.array_equal(cc, _want_counts(g, cplanes, flip)) and np.array_equal(gc, _want_counts(g, gplanes, flip))
            assert c.case_counts(rows, flip=flip).tobytes() == cc.tobytes()
            assert c.group_counts_last(bs).tobytes() == gc.tobytes()
            assert c.group_counts(rows, flip=flip).tobytes() == gc.tobytes()
        cs, gs = a.case_sums_int(G), b.group_sums_int(G)
        assert np.array_equal(cs, _want_sums(G, cplanes)) and np.array_equal(gs, _want_sums(G, gplanes))
        assert c.case_sums_int(G).tobytes() == cs.tobytes()
        assert c.group_sums_last(bs).tobytes() == gs.tobytes()
        with pytest.raises(Exception, match="bs is not"):
            c.group_sums_last(bs - 1)                                # the buffer is sized by the case call's bs
        assert c.group_sums_int(G).tobytes() == gs.tobytes()
        with pytest.raises(Exception):
            c.group_counts_last(bs)                                  # the last case entry summed integer rows
        with pytest.raises(Exception):
            a.group_sums_last(bs)                                    # no group on that context
        # the other order of the set calls, and each set cleared on its own
        a.set_group(member)
        assert a.case_sums_int(G).tobytes() == cs.tobytes() and a.group_sums_last(bs).tobytes() == gs.tobytes()
        a.set_group(None)
        assert a.case_counts(rows).tobytes() == _want_counts(g, cplanes, False).astype(np.int32).tobytes()
        with pytest.raises(Exception):
            a.group_counts(rows)
        c.set_cases(None)
        assert c.group_sums_int(G).tobytes() == gs.tobytes()
        with pytest.raises(Exception):
            c.case_sums_int(G)


def test_masks_handed_over_new_masks_and_clearing():
    from regenie_amd.step2 import Step2QT
    n, P, bs = 1023, 7, 33
    rng = np.random.default_rng(11)
    masks, is_case, X, Y, scf = _setup(rng, n, P)
    other = (rng.random((P, n)) > 0.4).astype(np.uint8)
    g = _calls(rng, bs, n)
    rows = _pack(g, (n + 3) // 4, rng)
    G = _dosages(rng, bs, n)
    with Step2QT(n, C, P) as s2:
        with pytest.raises(Exception):
            s2.set_cases(is_case)                                    # no masks yet: rg_s2_set_null has not been called, none are handed over
        s2.set_cases(is_case, mask=other)                            # a binary-trait caller hands its masks over
        assert np.array_equal(s2.case_counts(rows), _want_counts(g, (is_case != 0) & (other != 0), False))
        s2.set_null(X, Y, masks, scf)                                # ... and the masks of rg_s2_set_null do not replace them
        assert np.array_equal(s2.case_sums_int(G), _want_sums(G, (is_case != 0) & (other != 0)))
        s2.set_cases(is_case)
        assert np.array_equal(s2.case_counts(rows), _want_counts(g, (is_case != 0) & (masks != 0), False))
        s2.set_null(X, Y * other, other, scf)                        # new masks: the planes are packed again
        assert np.array_equal(s2.case_counts(rows), _want_counts(g, (is_case != 0) & (other != 0), False))
        assert np.array_equal(s2.case_sums_int(G), _want_sums(G, (is_case != 0) & (other != 0)))
        s2.set_cases(None)
        with pytest.raises(Exception) as e:
            s2.case_counts(rows)
        assert "rg_s2_set_cases" in str(e.value)
        s2.set_cases(None)                                           # clearing twice is fine


def test_a_context_without_cases_reports_an_error():
    from regenie_amd.engine import RgError
    from regenie_amd.step2 import Step2QT
    n, P = 17, 3
    rng = np.random.default_rng(3)
    masks, is_case, X, Y, scf = _setup(rng, n, P)
    with Step2QT(n, C, P) as s2:
        s2.set_null(X, Y, masks, scf)
        for call in (lambda: s2.case_counts(_pack(_calls(rng, 2, n), 5, rng)), lambda: s2.case_sums_int(_dosages(rng, 2, n)),
                     lambda: s2.group_counts_last(2), lambda: s2.group_sums_last(2), s2.case_rows_staged):
            with pytest.raises(RgError):
                call()
        res = s2.score_block_packed(_pack(_calls(rng, 2, n), 5, rng))   # the context is as usable as before
        assert res["n_obs"].shape == (2,)
    with Step2QT(n, 0, P) as s2:                                     # without a covariate basis: models and columns are refused, the counts work
        with pytest.raises(RgError, match="n_cov = 0"):
            s2.set_null(X[:0], Y, masks, scf)
        with pytest.raises(RgError, match="n_cov = 0"):
            s2.set_columns(Y)
        s2.set_cases(is_case, mask=masks)
        assert s2.case_sums_int(_dosages(rng, 2, n)).shape == (2, P, 2)
    with pytest.raises(RgError):
        Step2QT(3, 3, P)                                             # n > n_cov as before


def test_the_staged_copy_of_host_rows_is_handed_on():
    """A case entry on host rows keeps its device copy: read in place (as device rows) it gives the same counts (the driver hands it to the score
    entry: tests/test_afcc_cli_gpu.py).  After a case entry on device rows, or a set call, there is no such copy."""
    import torch
    from regenie_amd.engine import RgError
    from regenie_amd.step2 import Step2QT
    n, P, bs = 4099, 9, 33
    rng = np.random.default_rng(21)
    masks, is_case, X, Y, scf = _setup(rng, n, P)
    g = _calls(rng, bs, n)
    rows = _pack(g, (n + 3) // 4 + 3, rng)                           # an odd host pitch: the copy has its own
    G = _dosages(rng, bs, n)
    with Step2QT(n, C, P) as s2:
        s2.set_null(X, Y, masks, scf)
        s2.set_cases(is_case)
        want = s2.case_counts(rows)
        ptr, ld = s2.case_rows_staged()
        assert ld >= (n + 3) // 4 and ld % 4 == 0
        got = np.zeros_like(want)
        s2._check(s2.lib.rg_s2_case_counts_packed(s2.h, ptr, ld, bs, 1, 0, got.ctypes.data))
        assert got.tobytes() == want.tobytes()
        with pytest.raises(RgError):
            s2.case_rows_staged()                                    # that call took device rows
        want = s2.case_sums_int(G)
        ptr, ld = s2.case_rows_staged()
        assert ld >= n and ld % 8 == 0 and ptr % 16 == 0
        got = np.zeros_like(want)
        s2._check(s2.lib.rg_s2_case_sums_int(s2.h, ptr, ld, bs, 1, got.ctypes.data))
        assert got.tobytes() == want.tobytes()
        s2.case_counts(torch.from_numpy(rows).cuda())
        with pytest.raises(RgError):
            s2.case_rows_staged()
        s2.case_counts(rows)
        s2.set_cases(is_case)                                        # a set call ends the copy's validity
        with pytest.raises(RgError):
            s2.case_rows_staged()
