"""Extended-precision references of the spectral kernels (csrc/spectral_kernels.h) in numpy long double (64-bit significand on
x86): the rbf affinities, the degrees, and a product against a given matrix.  The bounds of tests/test_gpu_spectral.py are written
against these.

Affinity.  The device forms s = sum_c (y_ic - y_jc)^2 in double (d differences, d squares, d - 1 sums: relative error at most
(d + 1) eps64 on s, every term being non-negative), multiplies by -gamma (one more rounding) and takes exp.  An error of delta on
the exponent is a relative error of delta on the result, so against the exact value
    |A0 - A_hp| <= ((d + 2) gamma d2_ij + C_EXP) eps64 A_hp,
the first term the roundings carried through the exponent, C_EXP the error of exp itself in units of eps64.  An entry whose exact
value is below the smallest normal double may come out as anything in [0, DBL_MIN].
C_EXP is calibrated, not derived: tests/test_spectral_cpu.py measures the worst |exp64(x) - exp_ld(x)| / (eps64 exp_ld(x)) of
numpy's double exp over the exponents x = -gamma s of every golden case (results in the normal range), rounds it up to the next
power of two and multiplies by 4, the way C_KLD was set.  Measured: 0.580, so C_EXP = 4 x 1 = 4.  The worst device ratio, the largest (|A0 - A_hp| / (eps64 A_hp) - (d + 2) gamma d2_ij)
over every entry of every golden case on an MI355X: DEVICE_RATIO below (tests/test_gpu_spectral.py prints it per case)."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
DBL_MIN = float(np.finfo(np.float64).tiny)
C_EXP = 4.0
DEVICE_RATIO = 0.249            # measured (k16); between 0.100 and 0.249 in every case with an entry in the normal range


def sqdist(Y):
    Y = np.asarray(Y, dtype=np.float64).astype(LD)
    s = np.zeros((Y.shape[0], Y.shape[0]), dtype=LD)
    for c in range(Y.shape[1]):
        t = Y[:, None, c] - Y[None, :, c]
        s += t * t
    return s


def affinity(Y, gamma=1.0):
    """(A_hp, d2_hp): exp(-gamma d2) with a zero diagonal, and the squared distances, long double."""
    d2 = sqdist(Y)
    A = np.exp(-LD(gamma) * d2)
    np.fill_diagonal(A, LD(0))
    return A, d2


def affinity_bound(A_hp, d2_hp, d, gamma=1.0):
    """The allowance of |A0 - A_hp| per entry (float64); entries below DBL_MIN get DBL_MIN."""
    A, d2 = A_hp.astype(np.float64), d2_hp.astype(np.float64)
    b = ((d + 2) * gamma * d2 + C_EXP) * EPS * A
    return np.where(A_hp < LD(DBL_MIN), DBL_MIN, b)


def exp_ratio(x):
    """|exp64(x) - exp_ld(x)| / (eps64 exp_ld(x)) for the doubles x whose result is a normal double (others dropped)."""
    x = np.asarray(x, dtype=np.float64).ravel()
    ref = np.exp(x.astype(LD))
    keep = ref >= LD(DBL_MIN)
    return (np.abs(np.exp(x[keep]).astype(LD) - ref[keep]) / (LD(EPS) * ref[keep])).astype(np.float64)


def calibrate(worst):
    """The next power of two at or above `worst`, times 4."""
    return 4.0 * 2.0 ** int(np.ceil(np.log2(worst)))


def degrees(A_hp):
    """Column sums of A_hp, long double."""
    return A_hp.sum(axis=0)


def product(M, Q):
    """M Q in long double from doubles."""
    return np.asarray(M, dtype=np.float64).astype(LD) @ np.asarray(Q, dtype=np.float64).astype(LD)
