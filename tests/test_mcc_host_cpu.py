"""The closed-form host side of `--mcc` (regenie_amd/host/driver_models.cpp: gamma_q / gamma_p, chisq1_upper_quantile, mcc_setup_trait, mcc_pvalue),
compiled with g++ into a small harness (no GPU involved).

gamma_q / gamma_p against scipy.special.gammaincc / gammainc over shapes 0.01 to 1e8 and both tails.  Bound: the series and the continued fraction
stop at 1e-16 relative; the prefactor x^a e^-x / Gamma(a + 1) is exp() of a quantity of size up to ~40 (the tails asked for here reach 1e-17)
formed as a * (log1p(u) - u) with u = (x - a) / a rounded once: a relative error of about (|log p| + a |u| eps / |log p| ...) eps <= ~1e-12 at
a = 1e8, where the rounding of u alone moves the exponent by a u eps ~ 1e-12 * sqrt(a) / 1e4.  2e-10 relative holds that with two decimal digits of
room and is far inside the 2e-5 of the result files; scipy's own error (~1e-13) is below it -- except in its LOWER tail at shapes of 1e5 and more,
where scipy.special.gammainc (and the gammaincc next to it) is 4e-6 (a = 1e6, P = 3e-7) to 35 % (a = 1e8) off a 50-digit evaluation of the series;
those values are held to that evaluation (decimal, standard library) instead.

mcc_pvalue against tests/mcc_restate.mcc_one (the NumPy restatement, which forms every sum from the normalised vectors and takes scipy's gamma) from
power sums taken in np.longdouble, for genotype-like, rare and near-normal vectors (D = cor^2 is close to a scaled chi-square(1) whatever the
vectors, so the fitted shape stays between 0.06 and 0.6 here: large shapes are the gamma test's ground): 1e-9 relative, the cancellation of the
central sixth-power sum at |mean| / sd <= 3."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy import special

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = r'''
#include "driver.h"
extern "C" double t_gamma_q(double a, double x) { return rgdrv::gamma_q(a, x); }
extern "C" double t_gamma_p(double a, double x) { return rgdrv::gamma_p(a, x); }
extern "C" double t_chisq1(double p) { return rgdrv::chisq1_upper_quantile(p); }
extern "C" double t_mcc(const double* yres, const uint8_t* mask, int64_t n, int n_cov, const double* sums, int* ok) {
  const rgdrv::MccTrait t = rgdrv::mcc_setup_trait(yres, mask, n, n_cov);
  bool k = false;
  const double p = rgdrv::mcc_pvalue(t, sums, &k);
  *ok = k ? 1 : 0;
  return p;
}
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("mcchost")
    src = d / "h.cpp"
    src.write_text(HARNESS)
    so = d / "libmcchost.so"
    host = os.path.join(ROOT, "regenie_amd", "host")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + host, os.path.join(host, "driver_models.cpp"), str(src), "-o", str(so)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(str(so))
    for f in (L.t_gamma_q, L.t_gamma_p):
        f.restype, f.argtypes = C.c_double, [C.c_double, C.c_double]
    L.t_chisq1.restype, L.t_chisq1.argtypes = C.c_double, [C.c_double]
    L.t_mcc.restype = C.c_double
    L.t_mcc.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
    return L


def _lower_tail_50_digits(a, x):
    """P(a, x) for a >= 1e4 from x^a e^-x / Gamma(a + 1) * sum_k x^k / ((a + 1) .. (a + k)) in 50-digit decimal arithmetic (Stirling's series for
    log Gamma: its first omitted term is below 1e-30 there)."""
    from decimal import Decimal as D, localcontext
    with localcontext() as ctx:
        ctx.prec = 50
        a, x = D(repr(float(a))), D(repr(float(x)))
        pi = D("3.14159265358979323846264338327950288419716939937510582")
        lg = (a + D("0.5")) * a.ln() - a + (2 * pi).ln() / 2 + 1 / (12 * a) - 1 / (360 * a ** 3) + 1 / (1260 * a ** 5)
        term = total = D(1)
        k = 0
        while term > total * D("1e-40"):
            k += 1
            term *= x / (a + k)
            total += term
        return float((a * x.ln() - x - lg).exp() * total)


SHAPES = [0.01, 0.1, 0.5, 1.0, 2.5, 10.0, 29.9, 30.0, 31.0, 100.0, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8]
# x = a + z sqrt(a): both sides of the mode, from the bulk out to tails of about 1e-17
ZS = [-8.0, -5.0, -3.0, -1.0, -0.25, 0.0, 0.25, 1.0, 3.0, 5.0, 8.0]


@pytest.mark.parametrize("a", SHAPES)
def test_host_incomplete_gamma_against_scipy(lib, a):
    worst = 0.0
    xs = [a + z * np.sqrt(a) for z in ZS] + [a * f for f in (0.01, 0.3, 0.7, 1.0 + 1e-4, 1.3, 2.0)] + [a + 1.0, a + 0.999]
    n = 0
    for x in xs:
        if not x > 0:
            continue
        lower, upper = float(special.gammainc(a, x)), float(special.gammaincc(a, x))
        if a >= 1e5 and lower < 1e-4:
            lower = _lower_tail_50_digits(a, x)
            upper = 1.0 - lower
        for mine, ref in ((lib.t_gamma_q(a, x), upper), (lib.t_gamma_p(a, x), lower)):
            if ref < 1e-290:      # the prefactor underflows: the driver reports such a test as failed
                continue
            # the smaller of the two tails is computed directly; the larger one is 1 - it: absolute error relative to 1
            err = abs(mine - ref) / (ref if ref < 0.5 else 1.0)
            worst = max(worst, err)
            n += 1
            assert err < 2e-10, (a, x, mine, ref)
    assert n >= 20
    print("gamma a=%g: worst relative deviation from scipy %.2g over %d values" % (a, worst, n))


def test_host_incomplete_gamma_edges(lib):
    assert lib.t_gamma_q(2.0, 0.0) == 1.0 and lib.t_gamma_p(2.0, 0.0) == 0.0
    assert lib.t_gamma_q(2.0, -1.0) == 1.0
    assert lib.t_gamma_q(2.0, float("inf")) == 0.0
    assert np.isnan(lib.t_gamma_q(0.0, 1.0)) and np.isnan(lib.t_gamma_q(-1.0, 1.0))


@pytest.mark.parametrize("p", [0.9, 0.5, 0.05, 1e-3, 1e-8, 1e-20, 1e-100, 1e-300])
def test_chisq1_upper_quantile(lib, p):
    q = lib.t_chisq1(p)
    assert float(special.chdtrc(1.0, q)) == pytest.approx(p, rel=1e-10)


def _sums(r, y, mask):
    LD = np.longdouble
    m, rl = mask.astype(LD), r.astype(LD)
    return np.array([float((m * rl ** k).sum()) for k in range(1, 7)] + [float((rl * y.astype(LD)).sum())])


@pytest.mark.parametrize("kind,n,n_cov,seed", [("genotype", 459, 4, 1), ("genotype", 2000, 10, 2), ("rare", 1500, 4, 3),
                                               ("normal", 3000, 4, 4), ("normal", 20000, 8, 5), ("shifted", 5000, 4, 6)])
def test_mcc_pvalue_against_the_restatement(lib, kind, n, n_cov, seed):
    from tests import mcc_restate as mr
    rng = np.random.default_rng(seed)
    mask = (rng.random(n) > 0.07).astype(np.uint8)
    y = (np.exp(rng.normal(size=n)) if kind in ("genotype", "rare") else rng.normal(size=n)) * mask
    if kind == "genotype":
        r = rng.binomial(2, 0.3, n).astype(np.float64)
    elif kind == "rare":
        r = rng.binomial(2, 0.004, n).astype(np.float64)
    else:
        r = rng.normal(size=n) + (3.0 if kind == "shifted" else 0.0)      # shifted: the binomial expansion of the central sums cancels digits
    r = r + 0.02 * y                                                        # some association
    want, skew = mr.mcc_one(r, y, mask, n_cov)
    S = _sums(r, y, mask)
    ok = C.c_int(0)
    yc, mc_ = np.ascontiguousarray(y), np.ascontiguousarray(mask)
    got = lib.t_mcc(yc.ctypes.data, mc_.ctypes.data, n, n_cov, S.ctypes.data, C.byref(ok))
    print("mcc %s n=%d: skewness of D %.4g, shape %.4g, p %.6g (restatement %.6g)" % (kind, n, skew, 4 / skew ** 2, got, want))
    assert skew > 0 and ok.value == 1
    assert got == pytest.approx(want, rel=1e-9)
