"""The two `--skip-scaleG` branches of Data::print_ld (reference src/Data.cpp:4386-4391, :4400, :4407-4427) restated on dense numpy arrays,
on top of tests/ld_restate.py: the unscaled matrix after the diagonal rules, and its sparse form under `--sparse-thr`.
tests/test_ld_gtg_restate_cpu.py holds it to the reference's own output files."""
import numpy as np

from tests import ld_restate as lr


def gtg_of(LD, dtype=np.float64, tol=lr.TOL, numtol=lr.NUMTOL):
    """A diagonal entry in (-tol, 0) zeroes its row and column; then diag = max(diag, numtol).  Nothing is scaled."""
    LD = np.array(LD, dtype=dtype)
    d = np.diag(LD).copy()
    z = (d < 0) & (np.abs(d) < tol)
    LD[z, :] = 0
    LD[:, z] = 0
    LD[np.diag_indices_from(LD)] = np.maximum(np.diag(LD), dtype(numtol))
    return LD


def gtg(G, X, dtype=np.float64):
    return gtg_of(lr.ld_cov(G, X, dtype), dtype)


def sparse_of(GTG, thr):
    """-> sd [M] = sqrt(diag); row, col, val of the pairs i < j with |val| >= thr, val = GTG[i][j] / sd[i] / sd[j] (the two divisions
    as written), in row-major order; and every pair's val (the same order, unthresholded)."""
    sd = np.sqrt(np.diag(GTG))
    iu = np.triu_indices(GTG.shape[0], 1)
    v = GTG[iu] / sd[iu[0]] / sd[iu[1]]
    keep = np.abs(v) >= thr
    return sd, iu[0][keep].astype(np.int32), iu[1][keep].astype(np.int32), v[keep], v


def header(M, n_samples):
    return "%d %d\n" % (M, n_samples)


def text_dense(GTG, n_samples):
    """The file of `--output-corr-text --skip-scaleG`: the header line, the matrix at six significant digits, no newline at the end."""
    R = np.asarray(GTG, dtype=np.float64)
    return header(R.shape[0], n_samples) + "\n".join(" ".join("%.6g" % v for v in row) for row in R)


def text_sparse(sd, row, col, val, n_samples):
    """The file with `--sparse-thr`: the header line, the sd line, one `i j value` line (1-based) per kept pair."""
    sd = np.asarray(sd, dtype=np.float64)
    return (header(len(sd), n_samples) + " ".join("%.6g" % v for v in sd) + "\n" +
            "".join("%d %d %g\n" % (i + 1, j + 1, v) for i, j, v in zip(row, col, np.asarray(val, dtype=np.float64))))


def split_sparse(text):
    """-> the header line, the sd line, the (i, j) pairs as written (1-based) [K][2], the values [K]."""
    lines = text.split("\n")
    assert lines[-1] == "", "the sparse file ends with a newline"
    trip = [ln.split(" ") for ln in lines[2:-1]]
    assert all(len(t) == 3 for t in trip)
    ij = np.array([[int(t[0]), int(t[1])] for t in trip], dtype=np.int64).reshape(-1, 2)
    return lines[0] + "\n", lines[1], ij, np.array([float(t[2]) for t in trip])


def check_sparse(got_text, ref_text):
    """The rules for a sparse file: header byte-identical; the sd line within one unit of the sixth printed digit (lr.check_text); the
    (i, j) columns exactly equal, in order; the values within one unit of the sixth printed digit."""
    gh, gs, gij, gv = split_sparse(got_text)
    rh, rs, rij, rv = split_sparse(ref_text)
    assert gh == rh, (gh, rh)
    lr.check_text(gs, rs)
    assert gij.shape == rij.shape and np.array_equal(gij, rij), "the kept pairs differ: %d against the reference's %d" % (len(gij), len(rij))
    if len(rv):
        err = np.abs(gv - rv) - (1e-5 * np.abs(rv) + 1e-12)
        print("sparse: %d pairs, worst excess over the bound %.3g" % (len(rv), err.max()))
        assert err.max() <= 0, (gij[err.argmax()], gv[err.argmax()], rv[err.argmax()])
    return len(rv)
