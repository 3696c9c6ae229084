"""The panel-of-128 batched Cholesky (regenie_amd/csrc/chol_p128.h) on the device, through `rg_k_chol_solve_src`: the call level 0 makes --
systems formed from source matrices, one per (source, ridge shift), right-hand sides embedded below each system's order -- held to
numpy.linalg.cholesky / solve.  tests/test_chol_p128_emulated_cpu.py runs the same header on the host for its indexing; this file is
the device's turn: the counted waits of the ring, the copies, the matrix instruction itself.

Tolerance: 1e-12 of the largest reference entry for the factor, the forward-substituted right-hand sides and the inverses of the diagonal
64-tiles and 128-blocks -- what the emulated test uses for the same quantities of the same matrices (G G^T / n with G n x 3n, shifted by
>= 0.1: condition numbers of a few tens, so a backward-stable factorization of order 1,000 stays two orders of magnitude inside it).
The solved right-hand sides (solve = 1) take the 1e-10 that tests/test_kernels_gpu.py::test_chol_solve asks of the same quantity."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from regenie_amd.engine import load_library  # noqa: E402

SHIFTS = [0.5, 2.0, 7.0, 0.1, 20.0]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sources(n64, orders, embed, seed, with_F, indefinite=()):
    rng = np.random.default_rng(seed)
    nouter = len(orders)
    S = np.full((nouter, n64, n64), 1e30)                 # whatever lies outside a system's own rows / columns must never be used
    F = np.full((nouter, n64, n64), 3e29) if with_F else None
    A_, B_ = [], []
    for o, n in enumerate(orders):
        G = rng.standard_normal((n, 3 * n))
        A = G @ G.T / n
        if o in indefinite:
            A -= 3.0 * np.eye(n)                          # eigenvalues of G G^T / n lie in about [0.5, 7.5]: some end up on either side of 0
        b = rng.standard_normal((embed, n))
        if with_F:
            G2 = rng.standard_normal((n, n))
            A2, b2 = G2 @ G2.T / (4 * n), rng.standard_normal((embed, n))
            S[o, :n, :n], F[o, :n, :n] = A + A2, A2
            S[o, n:n + embed, :n], F[o, n:n + embed, :n] = b + b2, b2
        else:
            S[o, :n, :n] = A
            S[o, n:n + embed, :n] = b
        A_.append(A)
        B_.append(b)
    return S, F, A_, B_


def _launch(n64, orders, R, embed, solve, S, F):
    lib = load_library()
    nouter, batch, T = len(orders), len(orders) * R, n64 // 64
    Sd, Fd = _dev(S), (_dev(F) if F is not None else None)
    shift = _dev(np.array(SHIFTS[:R]))
    d_n = _dev(np.array(orders, dtype=np.int32))
    mats = torch.full((batch, n64, n64), float("nan"), dtype=torch.float64, device="cuda")
    ws = torch.full((batch * (T + 10 * ((T + 3) // 4)) * 4096,), float("nan"), dtype=torch.float64, device="cuda")
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    rc = lib.rg_k_chol_solve_src(_stream(), Sd.data_ptr(), Fd.data_ptr() if Fd is not None else None, shift.data_ptr(), R, d_n.data_ptr(),
                                 nouter, n64, embed, solve, mats.data_ptr(), ws.data_ptr(), info.data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    w = ws.cpu().numpy()
    dinv = w[:batch * T * 4096].reshape(batch, T, 4096)
    linv = w[batch * T * 4096:batch * T * 4096 + batch * (n64 // 128) * 16384].reshape(batch, n64 // 128, 16384)
    return mats.cpu().numpy(), dinv, linv, int(info[0].item())


CASES = [
    # n64, orders, R, embed, with_F
    # orders 128 .. 1,024 in steps of 128 with ragged orders beside them; no right-hand sides (a full order leaves no row for one)
    (128, [128, 77], 1, 0, False),
    (256, [256, 130], 5, 0, False),
    (384, [384, 300], 1, 0, False),
    (512, [512, 400], 5, 0, True),
    (640, [640, 577], 1, 0, False),
    (768, [768, 641, 100], 1, 0, False),
    (896, [896, 800], 5, 0, False),
    (1024, [1024, 960], 1, 0, False),
    # embedded right-hand sides
    (256, [127, 126, 200, 253], 1, 3, False),             # 127 + 3: the right-hand sides spill from panel 0 into panel 1
    (1024, [1000, 960, 1023], 5, 1, False),               # the flagship's shape (bsize 1000, one trait, five shifts); 15 systems: not 8 R
    (1024, [1000, 1000, 960, 700, 300, 1019, 129, 64, 1000], 1, 5, False),      # 9 systems, five right-hand sides, systems of 1 .. 8 panels
    (512, [500, 300, 120], 5, 3, True),                   # X = S - F
    (1152, [1024, 1100], 1, 2, False),                    # nine panels
]


@pytest.mark.parametrize("n64,orders,R,embed,with_F", CASES)
def test_panel128_factor_and_forward_substitution(n64, orders, R, embed, with_F):
    S, F, A_, B_ = _sources(n64, orders, embed, seed=n64 + 7 * R + embed, with_F=with_F)
    mats, dinv, linv, info = _launch(n64, orders, R, embed, 0, S, F)
    assert info == 0
    worst = {"L": 0.0, "y": 0.0, "tile inverse": 0.0, "block inverse": 0.0}
    for o, n in enumerate(orders):
        for r in range(R):
            k = o * R + r
            L = np.linalg.cholesky(A_[o] + SHIFTS[r] * np.eye(n))
            worst["L"] = max(worst["L"], np.abs(np.tril(mats[k, :n, :n]) - L).max() / np.abs(L).max())
            if embed:
                Y = np.linalg.solve(L, B_[o].T).T
                worst["y"] = max(worst["y"], np.abs(mats[k, n:n + embed, :n] - Y).max() / np.abs(Y).max())
            for t in range((n + 63) // 64):
                lo, hi = 64 * t, min(64 * t + 64, n)
                Ik = np.linalg.inv(L[lo:hi, lo:hi])
                worst["tile inverse"] = max(worst["tile inverse"], np.abs(dinv[k, t].reshape(64, 64)[:hi - lo, :hi - lo] - Ik).max() / np.abs(Ik).max())
            for pnl in range((n + 127) // 128):
                lo, hi = 128 * pnl, min(128 * pnl + 128, n)
                Ip = np.linalg.inv(L[lo:hi, lo:hi])
                got = np.tril(linv[k, pnl].reshape(128, 128)[:hi - lo, :hi - lo])
                worst["block inverse"] = max(worst["block inverse"], np.abs(got - Ip).max() / np.abs(Ip).max())
    print("panel128", n64, orders, R, embed, worst)
    for name, e in worst.items():
        assert e < 1e-12, (name, e)


@pytest.mark.parametrize("n64,orders,R,embed,with_F", [c for c in CASES if c[3] > 0])
def test_panel128_solve(n64, orders, R, embed, with_F):
    S, F, A_, B_ = _sources(n64, orders, embed, seed=n64 + 7 * R + embed, with_F=with_F)
    mats, _, _, info = _launch(n64, orders, R, embed, 1, S, F)
    assert info == 0
    worst = 0.0
    for o, n in enumerate(orders):
        for r in range(R):
            X = np.linalg.solve(A_[o] + SHIFTS[r] * np.eye(n), B_[o].T).T
            worst = max(worst, np.abs(mats[o * R + r, n:n + embed, :n] - X).max() / np.abs(X).max())
    print("panel128 solve", n64, orders, R, embed, worst)
    assert worst <= 1e-10


@pytest.mark.parametrize("n64,orders,R,embed,bad", [(256, [200, 256, 130], 1, 0, 1), (1024, [1000, 960, 1000], 5, 1, 2)])
def test_panel128_flags_an_indefinite_system(n64, orders, R, embed, bad):
    """One source of the batch is symmetric indefinite (G G^T / n - 3 I): its pivots turn negative part of the way down, which the
    factorization flags without a branch and carries on from a pivot of 1 -- finite garbage, nothing faults."""
    S, F, A_, B_ = _sources(n64, orders, embed, seed=5, with_F=False, indefinite=(bad,))
    assert np.linalg.eigvalsh(A_[bad] + SHIFTS[0] * np.eye(orders[bad])).min() < 0
    _, _, _, info = _launch(n64, orders, R, embed, 0, S, F)
    assert info != 0
