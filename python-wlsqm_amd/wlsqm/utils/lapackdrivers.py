"""Dense linear solvers for many small systems, and small matrix helpers (the reference's wlsqm.utils.lapackdrivers).

The solvers run on the GPU (libwlsqm_hip.so, lapack_batched.hip): LU with partial pivoting with the semantics of
LAPACK's dgetrf / dgetrs, and the symmetric indefinite Bunch-Kaufman factorization U*D*U^T of dsytrf / dsytrs with
uplo = 'U' (only the upper triangle of a symmetric matrix is read or written).  They take host numpy arrays, work in
place exactly as the reference's LAPACK calls do, and return when the results are back in the caller's arrays:

    general, generals, generalsp, generalfactor, generalfactored,
    mgeneral, mgeneralp, mgeneralfactor, mgeneralfactorp, mgeneralfactored, mgeneralfactoredp,
    symmetric, symmetrics, symmetricsp, symmetricfactor, symmetricfactored,
    msymmetric, msymmetricp, msymmetricfactor, msymmetricfactorp, msymmetricfactored, msymmetricfactoredp

Matrices are Fortran-ordered float64: A (n, n) or (n, n, nlhs), b (n,), (n, nrhs) or (n, nlhs); pivot arrays are
Fortran-ordered np.intc with LAPACK's 1-based entries.  ``ntasks`` (OpenMP threads in the reference) is accepted and
ignored.  Like the reference, the solvers do not report singular matrices: as dgesv / dsysv, a system whose matrix has
an exactly zero pivot is not solved, and its right-hand side is left as it came (the factor and pivots are written); the
device-resident entry points wlsqm.hip.getrf_batched & co. return LAPACK's INFO per matrix.

The helpers that have no batch (scaling, the 2x2 and tridiagonal solvers, svd, copies, symmetrization) run on the host
with numpy and scipy.linalg.lapack, the same LAPACK routines the reference binds.
"""
import ctypes as C
from enum import IntEnum

import numpy as np
from scipy.linalg import lapack as _lapack

from .. import _binding as B

__all__ = ["distribute_items", "copygeneral", "copysymmu", "symmetrize", "msymmetrize", "msymmetrizep",
           "ScalingAlgo", "do_rescale", "rescale_columns", "rescale_rows", "rescale_twopass", "rescale_dgeequ",
           "rescale_ruiz2001", "rescale_scalgm", "tridiag", "symmetric2x2", "symmetric", "symmetricfactor",
           "symmetricfactored", "symmetrics", "symmetricsp", "msymmetric", "msymmetricp", "msymmetricfactor",
           "msymmetricfactored", "msymmetricfactorp", "msymmetricfactoredp", "general2x2", "general", "generalfactor",
           "generalfactored", "generals", "generalsp", "mgeneral", "mgeneralp", "mgeneralfactor", "mgeneralfactored",
           "mgeneralfactorp", "mgeneralfactoredp", "svd"]

_EPSILON = 1e-15          # convergence tolerance of the iterative scalings
_MAX_ITERS = 100


# ---- argument checks (the reference's typed memoryviews: exact dtype, exact rank, Fortran-contiguous) ----

def _farray(a, ndim, name, dtype=np.float64):
    if not isinstance(a, np.ndarray):
        raise ValueError("argument %s must be a numpy array" % name)
    if a.dtype != np.dtype(dtype):
        raise ValueError("Buffer dtype mismatch, expected '%s' but got '%s' (argument %s)"
                         % (np.dtype(dtype).name, a.dtype.name, name))
    if a.ndim != ndim:
        raise ValueError("Buffer has wrong number of dimensions (expected %d, got %d) (argument %s)" % (ndim, a.ndim, name))
    if not a.flags.f_contiguous:
        raise ValueError("ndarray is not Fortran contiguous (argument %s)" % name)
    if not a.flags.writeable:
        raise ValueError("buffer source array is read-only (argument %s)" % name)
    return a


def _ipiv(a, ndim, name="ipiv"):
    return _farray(a, ndim, name, dtype=np.intc)


def _ntasks(ntasks):
    if ntasks is None or int(ntasks) < 1:
        raise ValueError("ntasks must be >= 1, got %r" % (ntasks,))


def _square(A, name="A"):
    if A.shape[0] != A.shape[1]:
        raise ValueError("argument %s must be square, got shape %s" % (name, A.shape))
    return A.shape[0]


def _rhs(b, n, count, name="b"):
    if b.shape[0] != n or (b.ndim == 2 and count is not None and b.shape[1] != count):
        raise ValueError("argument %s has shape %s, expected (%d%s)" % (name, b.shape, n, "" if b.ndim == 1 else ", %d" % count))


def _pivshape(ipiv, n, count):
    want = (n,) if count is None else (n, count)
    if ipiv.shape != want:
        raise ValueError("argument ipiv has shape %s, expected %s" % (ipiv.shape, want))


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _run(fn, *args):
    B.check(fn(*args, B.default_device()))


# ---- the GPU families: one factorization (getrf / sytrf) and one solve (getrs / sytrs) each ----

def _factor(kind, A, ipiv, count, info=None):
    n = A.shape[0]
    fn = B.lib().wlsqm_hip_getrf_batched_host if kind == "ge" else B.lib().wlsqm_hip_sytrf_batched_host
    _run(fn, n, count, _p(A), _p(ipiv), _p(info))


def _solve(kind, A, ipiv, b, count, lhs_stride):
    n = A.shape[0]
    fn = B.lib().wlsqm_hip_getrs_batched_host if kind == "ge" else B.lib().wlsqm_hip_sytrs_batched_host
    _run(fn, n, count, lhs_stride, _p(A), _p(ipiv), _p(b))


def _factor_solve(kind, A, b, count):
    n = A.shape[0]
    ipiv = np.empty((n, count), dtype=np.intc, order="F")
    fn = B.lib().wlsqm_hip_gesv_batched_host if kind == "ge" else B.lib().wlsqm_hip_sysv_batched_host
    _run(fn, n, count, _p(A), _p(ipiv), None, _p(b))


def _one(kind, A, b):
    _farray(A, 2, "A"); _farray(b, 1, "b")
    n = _square(A); _rhs(b, n, None)
    _factor_solve(kind, A, b, 1)
    return 0


def _many_rhs(kind, A, b, keep_A):
    _farray(A, 2, "A"); _farray(b, 2, "b")
    n = _square(A); _rhs(b, n, None)
    F = np.array(A, order="F") if keep_A else A
    ipiv = np.empty(n, dtype=np.intc)
    info = np.zeros(1, dtype=np.intc)
    _factor(kind, F, ipiv, 1, info)
    if info[0] == 0:                    # dgesv / dsysv: a singular A leaves b as it came
        _solve(kind, F, ipiv, b, b.shape[1], 0)
    return 0


def _factor_one(kind, A):
    _farray(A, 2, "A")
    n = _square(A)
    ipiv = np.empty(n, dtype=np.intc)
    _factor(kind, A, ipiv, 1)
    return ipiv


def _factored_one(kind, A, ipiv, b):
    _farray(A, 2, "A"); _ipiv(ipiv, 1); _farray(b, 1, "b")
    n = _square(A); _pivshape(ipiv, n, None); _rhs(b, n, None)
    _solve(kind, A, ipiv, b, 1, 1)
    return 0


def _m(kind, A, b):
    _farray(A, 3, "A"); _farray(b, 2, "b")
    n = _square(A); _rhs(b, n, A.shape[2])
    _factor_solve(kind, A, b, A.shape[2])
    return 0


def _mfactor(kind, A, ipiv):
    _farray(A, 3, "A"); _ipiv(ipiv, 2)
    n = _square(A); _pivshape(ipiv, n, A.shape[2])
    _factor(kind, A, ipiv, A.shape[2])
    return 0


def _mfactored(kind, A, ipiv, b):
    _farray(A, 3, "A"); _ipiv(ipiv, 2); _farray(b, 2, "b")
    n = _square(A); _pivshape(ipiv, n, A.shape[2]); _rhs(b, n, A.shape[2])
    _solve(kind, A, ipiv, b, A.shape[2], 1)
    return 0


def general(A, b):
    """Solve A x = b for a general square A (LU with partial pivoting, as dgesv).
    A (n, n): overwritten by its LU factors.  b (n,): the right-hand side in, the solution out.  Returns 0."""
    return _one("ge", A, b)


def generals(A, b):
    """Like general() for the nrhs columns of b (n, nrhs): A is factored once and overwritten by its LU factors."""
    return _many_rhs("ge", A, b, keep_A=False)


def generalsp(A, b, ntasks):
    """Like generals(); A is left unchanged (a copy is factored).  ntasks is accepted and ignored."""
    _ntasks(ntasks)
    return _many_rhs("ge", A, b, keep_A=True)


def generalfactor(A):
    """LU factorization of A (n, n) in place (as dgetrf).  Returns the pivots (n,), np.intc, 1-based as LAPACK's."""
    return _factor_one("ge", A)


def generalfactored(A, ipiv, b):
    """Solve with the output of generalfactor(): A and ipiv are read, b (n,) is overwritten by the solution."""
    return _factored_one("ge", A, ipiv, b)


def mgeneral(A, b):
    """Solve nlhs independent systems A[:, :, k] x = b[:, k]; A (n, n, nlhs) is overwritten by the LU factors, b (n, nlhs)
    by the solutions."""
    return _m("ge", A, b)


def mgeneralp(A, b, ntasks):
    """mgeneral(); ntasks is accepted and ignored (the batch runs on the GPU)."""
    _ntasks(ntasks)
    return _m("ge", A, b)


def mgeneralfactor(A, ipiv):
    """LU-factor every A[:, :, k] in place; the pivots go to ipiv (n, nlhs), np.intc, Fortran order, 1-based."""
    return _mfactor("ge", A, ipiv)


def mgeneralfactorp(A, ipiv, ntasks):
    """mgeneralfactor(); ntasks is accepted and ignored."""
    _ntasks(ntasks)
    return _mfactor("ge", A, ipiv)


def mgeneralfactored(A, ipiv, b):
    """Solve with the output of mgeneralfactor(): b[:, k] is overwritten by the solution of system k."""
    return _mfactored("ge", A, ipiv, b)


def mgeneralfactoredp(A, ipiv, b, ntasks):
    """mgeneralfactored(); ntasks is accepted and ignored."""
    _ntasks(ntasks)
    return _mfactored("ge", A, ipiv, b)


def symmetric(A, b):
    """Solve A x = b for a symmetric A (Bunch-Kaufman U D U^T, as dsysv with uplo='U'): only the upper triangle of
    A (n, n) is read, and it is overwritten by the factor; the strict lower triangle is left alone.  b (n,): the
    right-hand side in, the solution out.  Returns 0."""
    return _one("sy", A, b)


def symmetrics(A, b):
    """Like symmetric() for the nrhs columns of b (n, nrhs); A is factored once."""
    return _many_rhs("sy", A, b, keep_A=False)


def symmetricsp(A, b, ntasks):
    """Like symmetrics(); A is left unchanged (a copy is factored).  ntasks is accepted and ignored."""
    _ntasks(ntasks)
    return _many_rhs("sy", A, b, keep_A=True)


def symmetricfactor(A):
    """U D U^T factorization of the upper triangle of A (n, n) in place (as dsytrf, uplo='U').  Returns the pivots (n,),
    np.intc, in dsytrf's encoding (positive: 1x1 block and the row it was exchanged with; a negative pair: 2x2 block)."""
    return _factor_one("sy", A)


def symmetricfactored(A, ipiv, b):
    """Solve with the output of symmetricfactor(): b (n,) is overwritten by the solution."""
    return _factored_one("sy", A, ipiv, b)


def msymmetric(A, b):
    """Solve nlhs independent symmetric systems (upper triangles of A (n, n, nlhs)); b (n, nlhs) gets the solutions."""
    return _m("sy", A, b)


def msymmetricp(A, b, ntasks):
    """msymmetric(); ntasks is accepted and ignored."""
    _ntasks(ntasks)
    return _m("sy", A, b)


def msymmetricfactor(A, ipiv):
    """Factor every A[:, :, k] (upper triangle) in place; the pivots go to ipiv (n, nlhs), np.intc, Fortran order."""
    return _mfactor("sy", A, ipiv)


def msymmetricfactorp(A, ipiv, ntasks):
    """msymmetricfactor(); ntasks is accepted and ignored."""
    _ntasks(ntasks)
    return _mfactor("sy", A, ipiv)


def msymmetricfactored(A, ipiv, b):
    """Solve with the output of msymmetricfactor(): b[:, k] is overwritten by the solution of system k."""
    return _mfactored("sy", A, ipiv, b)


def msymmetricfactoredp(A, ipiv, b, ntasks):
    """msymmetricfactored(); ntasks is accepted and ignored."""
    _ntasks(ntasks)
    return _mfactored("sy", A, ipiv, b)


# ---- host helpers ----

def distribute_items(nitems, ntasks):
    """Split items 0 .. nitems-1 into ntasks contiguous blocks of near-equal size (the first nitems % ntasks blocks get one
    more).  Returns (blocksizes, baseidxs), int32 arrays of length ntasks; with fewer items than tasks only the first
    nitems entries are used (the rest are 0)."""
    nitems, ntasks = int(nitems), int(ntasks)
    if ntasks < 1:
        raise ValueError("ntasks must be >= 1, got %d" % ntasks)
    base, rem = divmod(nitems, ntasks)
    used = rem if base == 0 else ntasks
    blocksizes = np.zeros(ntasks, dtype=np.int32)
    baseidxs = np.zeros(ntasks, dtype=np.int32)
    blocksizes[:used] = base
    blocksizes[:min(rem, used)] += 1
    if used > 1:
        baseidxs[1:used] = np.cumsum(blocksizes[:used - 1])
    return (blocksizes, baseidxs)


def copygeneral(O, I):
    """Copy I into O (both Fortran-ordered float64 arrays of the same shape, O allocated by the caller)."""
    _farray(O, 2, "O"); _farray(I, 2, "I")
    if O.shape != I.shape:
        raise ValueError("O and I must have the same shape")
    O[...] = I


def copysymmu(O, I):
    """Copy the upper triangle of the square I (diagonal included) into O; the strict lower triangle of O is untouched."""
    _farray(O, 2, "O"); _farray(I, 2, "I")
    if O.shape != I.shape:
        raise ValueError("O and I must have the same shape")
    n = _square(I, "I")
    iu = np.triu_indices(n)
    O[iu] = I[iu]


def _symm(A):
    n = A.shape[0]
    i, j = np.triu_indices(n, 1)
    t = 0.5 * (A[i, j, ...] + A[j, i, ...])
    A[i, j, ...] = t
    A[j, i, ...] = t


def symmetrize(A):
    """A <- (A + A^T) / 2 in place, for a square Fortran-ordered A (n, n)."""
    _farray(A, 2, "A"); _square(A)
    _symm(A)


def msymmetrize(A):
    """symmetrize() every A[:, :, k] of A (n, n, nlhs) in place."""
    _farray(A, 3, "A"); _square(A)
    _symm(A)


def msymmetrizep(A, ntasks):
    """msymmetrize(); ntasks is accepted and ignored."""
    _ntasks(ntasks)
    msymmetrize(A)


class ScalingAlgo(IntEnum):
    """Scaling algorithms of do_rescale() (plain ints work as well)."""
    ALGO_COLS_EUCL = 1
    ALGO_ROWS_EUCL = 2
    ALGO_TWOPASS = 3
    ALGO_RUIZ2001 = 4
    ALGO_SCALGM = 5
    ALGO_DGEEQU = 6


def _cols_eucl(A, rs, cs):
    return cs / np.sqrt(((A * (cs[None, :] * rs[:, None])) ** 2).sum(axis=0))


def _rows_eucl(A, rs, cs):
    return rs / np.sqrt(((A * (rs[:, None] * cs[None, :])) ** 2).sum(axis=1))


def _scale_columns(A):
    rs, cs = np.ones(A.shape[0]), np.ones(A.shape[1])
    return rs, _cols_eucl(A, rs, cs)


def _scale_rows(A):
    rs, cs = np.ones(A.shape[0]), np.ones(A.shape[1])
    return _rows_eucl(A, rs, cs), cs


def _scale_twopass(A):
    rs, cs = np.ones(A.shape[0]), np.ones(A.shape[1])
    cs = _cols_eucl(A, rs, cs)
    return _rows_eucl(A, rs, cs), cs


def _scale_dgeequ(A):
    r, c, rowcnd, colcnd, amax, info = _lapack.dgeequ(A)
    if info != 0:
        return None
    return np.array(r, dtype=np.float64), np.array(c, dtype=np.float64)


def _scale_ruiz(A):
    """Ruiz (2001): rows and columns equilibrated together in the max norm; keeps a symmetric matrix symmetric."""
    nr, nc = A.shape
    rs, cs = np.ones(nr), np.ones(nc)
    drp, dcp = np.ones(nr), np.ones(nc)
    absA = np.abs(A)
    for _ in range(_MAX_ITERS):
        dr = np.sqrt((absA / (drp[:, None] * dcp[None, :])).max(axis=1))
        dc = np.sqrt((absA / (dcp[None, :] * drp[:, None])).max(axis=0))
        drp *= dr; rs /= dr
        dcp *= dc; cs /= dc
        if np.abs(1.0 - dr * dr).max() < _EPSILON and np.abs(1.0 - dc * dc).max() < _EPSILON:
            break
    return rs, cs


def _smallest_nonzero(t, axis):
    m = np.where(t > 0.0, t, np.inf).min(axis=axis)
    return np.where(np.isinf(m), 0.0, m)


def _scale_scalgm(A):
    """Chiang and Chandler (2008): geometric-mean scaling up from the smallest entries, then down from the largest, in the
    max norm; the same fixed point as Ruiz's."""
    nr, nc = A.shape
    rs, cs = np.ones(nr), np.ones(nc)
    absA = np.abs(A)
    with np.errstate(divide="ignore"):
        def up_rows(rs, cs, mod_cs):
            f = cs if mod_cs is None else cs * mod_cs
            return 1.0 / _smallest_nonzero(absA * (rs[:, None] * f[None, :]), 1)

        def up_cols(rs, mod_rs, cs):
            f = rs if mod_rs is None else rs * mod_rs
            return 1.0 / _smallest_nonzero(absA * (cs[None, :] * f[:, None]), 0)

        def down_rows(rs, cs, mod_cs):
            f = cs if mod_cs is None else cs * mod_cs
            return 1.0 / (absA * (rs[:, None] * f[None, :])).max(axis=1)

        def down_cols(rs, mod_rs, cs):
            f = rs if mod_rs is None else rs * mod_rs
            return 1.0 / (absA * (cs[None, :] * f[:, None])).max(axis=0)

        mode = 1
        for _ in range(_MAX_ITERS):
            if mode == 1:
                dr1 = up_rows(rs, cs, None)
                dc1 = up_cols(rs, dr1, cs)
                dc2 = up_cols(rs, None, cs)
                dr2 = up_rows(rs, cs, dc2)
                rs = rs * np.sqrt(dr1 * dr2)
                cs = cs * np.sqrt(dc1 * dc2)
            dr1 = down_rows(rs, cs, None)
            dc1 = down_cols(rs, dr1, cs)
            dc2 = down_cols(rs, None, cs)
            dr2 = down_rows(rs, cs, dc2)
            rs = rs * np.sqrt(dr1 * dr2)
            cs = cs * np.sqrt(dc1 * dc2)
            S = absA * (rs[:, None] * cs[None, :])
            if np.abs(1.0 - S.max(axis=1)).max() < _EPSILON and np.abs(1.0 - S.max(axis=0)).max() < _EPSILON:
                if mode == 1:
                    mode = 2
                else:
                    break
    return rs, cs


_SCALERS = {ScalingAlgo.ALGO_COLS_EUCL: _scale_columns, ScalingAlgo.ALGO_ROWS_EUCL: _scale_rows,
            ScalingAlgo.ALGO_TWOPASS: _scale_twopass, ScalingAlgo.ALGO_RUIZ2001: _scale_ruiz,
            ScalingAlgo.ALGO_SCALGM: _scale_scalgm, ScalingAlgo.ALGO_DGEEQU: _scale_dgeequ}


def do_rescale(A, algo):
    """Scale the general matrix A (nrows, ncols) in place with the algorithm `algo` (a ScalingAlgo member or its int),
    to lower its condition number before a solve.  Returns (row_scale, col_scale): scale b by row_scale before solving
    (b[j] *= row_scale[j]) and the solution by col_scale after (x[m] *= col_scale[m]).
    Raises ValueError for an unknown algorithm and np.linalg.LinAlgError when the scaling fails (ALGO_DGEEQU on a
    matrix with a zero row or column)."""
    _farray(A, 2, "A")
    algo = int(algo)
    if algo not in _SCALERS:
        raise ValueError("Unknown algorithm identifier, got %d" % algo)
    got = _SCALERS[ScalingAlgo(algo)](A)
    if got is None:
        raise np.linalg.LinAlgError("Matrix scaling failed (e.g. singular row or column).")
    rs, cs = got
    A *= rs[:, None] * cs[None, :]
    return (rs, cs)


def rescale_columns(A):
    """Scale every column of A to unit Euclidean norm (changes the units of x; breaks symmetry).  See do_rescale()."""
    return do_rescale(A, ScalingAlgo.ALGO_COLS_EUCL)


def rescale_rows(A):
    """Scale every row of A to unit Euclidean norm (b must be scaled the same way; breaks symmetry).  See do_rescale()."""
    return do_rescale(A, ScalingAlgo.ALGO_ROWS_EUCL)


def rescale_twopass(A):
    """Columns to unit Euclidean norm, then rows of the result (no iteration; breaks symmetry).  See do_rescale()."""
    return do_rescale(A, ScalingAlgo.ALGO_TWOPASS)


def rescale_dgeequ(A):
    """Row and column scaling of LAPACK's dgeequ (max norm).  Raises np.linalg.LinAlgError on a zero row or column."""
    return do_rescale(A, ScalingAlgo.ALGO_DGEEQU)


def rescale_ruiz2001(A):
    """Iterative simultaneous row and column equilibration of Ruiz (2001) in the max norm; preserves symmetry."""
    return do_rescale(A, ScalingAlgo.ALGO_RUIZ2001)


def rescale_scalgm(A):
    """Iterative SCALGM equilibration of Chiang and Chandler (2008) in the max norm; preserves symmetry."""
    return do_rescale(A, ScalingAlgo.ALGO_SCALGM)


def tridiag(a, b, c, x):
    """Solve a tridiagonal system with LAPACK's dgtsv: a (n-1,) sub-diagonal, b (n,) diagonal, c (n-1,) super-diagonal,
    x (n,) the right-hand side in, the solution out.  a, b and c are overwritten as dgtsv leaves them.  Returns 0."""
    for v, name in ((a, "a"), (b, "b"), (c, "c"), (x, "x")):
        _farray(v, 1, name)
    du2, d, du, sol, info = _lapack.dgtsv(a, b, c, x)
    a[...] = du2                # (dgtsv leaves the second super-diagonal of U in the first n-2 entries of dl)
    b[...] = d
    c[...] = du
    x[...] = sol
    return 0


def general2x2(A, b):
    """Solve a general 2x2 system directly (Cramer's rule); b (2,) is overwritten by the solution.  Returns 0."""
    _farray(A, 2, "A"); _farray(b, 1, "b")
    a00, a10, a01, a11 = A[0, 0], A[1, 0], A[0, 1], A[1, 1]
    b0, b1 = b[0], b[1]
    dm1 = 1.0 / (a00 * a11 - a01 * a10)
    b[0] = dm1 * (a11 * b0 - a01 * b1)
    b[1] = dm1 * (a00 * b1 - a10 * b0)
    return 0


def symmetric2x2(A, b):
    """Solve a symmetric 2x2 system directly from the upper triangle of A; b (2,) is overwritten.  Returns 0."""
    _farray(A, 2, "A"); _farray(b, 1, "b")
    a00, a01, a11 = A[0, 0], A[0, 1], A[1, 1]
    b0, b1 = b[0], b[1]
    dm1 = 1.0 / (a00 * a11 - a01 * a01)
    b[0] = dm1 * (a11 * b0 - a01 * b1)
    b[1] = dm1 * (a00 * b1 - a01 * b0)
    return 0


def svd(A):
    """Singular values of the general A (m, n) in descending order (dgesvd without U and V; S[0] / S[-1] is the 2-norm
    condition number).  A is overwritten as dgesvd leaves it."""
    _farray(A, 2, "A")
    u, s, vt, info = _lapack.dgesvd(A, compute_uv=0, full_matrices=0, overwrite_a=1)
    return np.array(s, dtype=np.float64)
