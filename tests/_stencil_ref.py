"""Reference statements for the stencil operators (wlsqm.hip.StencilOperator, csrc/stencil.hip), in numpy and exact arithmetic.

The SELL-64 layout (include/wlsqm_hip.h): rows in slices of 64; len (nrows,), width (nslices,) = max len of the slice, soff (nslices + 1,)
with soff[s + 1] - soff[s] = 64 * width[s]; entry e of row i at soff[i // 64] + 64 * e + i % 64; col (total,), val (nop, total).
The row of case j: (hoods[j, k], slots[:, j, k]) for k < nk[j] in slot order, then, where own_mask[j], (pts[j], own[:, j]).
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53


def gamma(n):
    """gamma_n = n u / (1 - n u), u = 2^-53: the bound of any n-rounding sum, fused or not, in any order."""
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def frame(lens):
    """(len int32, width int32, soff int64) of rows with `lens` live entries."""
    lens = np.asarray(lens, np.int64)
    ns = (len(lens) + 63) // 64
    padded = np.zeros(ns * 64, np.int64)
    padded[:len(lens)] = lens
    width = padded.reshape(ns, 64).max(axis=1)
    soff = np.concatenate([[0], np.cumsum(64 * width)]).astype(np.int64)
    return lens.astype(np.int32), width.astype(np.int32), soff


def rows_of(hoods, nk, slots, own=None, own_mask=None, pts=None):
    """The matrix as per-row lists: rows[j] = [(column, values (nop,)), ...] in entry order."""
    nop, n, K = slots.shape
    pts = np.arange(n) if pts is None else pts
    out = []
    for j in range(n):
        r = [(int(hoods[j, k]), slots[:, j, k].copy()) for k in range(min(max(int(nk[j]), 0), K))]
        if own_mask is not None and own_mask[j]:
            r.append((int(pts[j]), own[:, j].copy()))
        out.append(r)
    return out


def pack(rows, nop):
    """rows (as rows_of gives them) in SELL-64: dict(len, width, soff, col, val); padding is zeros."""
    ln, width, soff = frame([len(r) for r in rows])
    col = np.zeros(int(soff[-1]), np.int32)
    val = np.zeros((nop, int(soff[-1])))
    for i, r in enumerate(rows):
        for e, (c, v) in enumerate(r):
            at = soff[i // 64] + 64 * e + i % 64
            col[at], val[:, at] = c, v
    return dict(len=ln, width=width, soff=soff, col=col, val=val)


def transpose_rows(rows, ncols):
    """The transposed matrix as per-row lists: a stable sort of the entries by column, ties in (case, entry) order."""
    out = [[] for _ in range(ncols)]
    for i, r in enumerate(rows):
        for c, v in r:
            out[c].append((i, v))
    return out


def exact_apply(rows, X, nop, alpha=1.0, beta=0.0, Y0=None):
    """(exact, mag): per (field r, operator o, row i) the exact alpha * sum of val * X[r, col] + beta * Y0[r, o, i] rounded once, and the
    sum of the magnitudes of its terms (the scale of the gamma bound).  X (R, ncols); entries of X that no live entry names are never
    read, and neither is Y0 when beta == 0."""
    R = X.shape[0]
    exact = np.zeros((R, nop, len(rows)))
    mag = np.zeros((R, nop, len(rows)))
    fa, fb = Fraction(float(alpha)), Fraction(float(beta))
    for i, row in enumerate(rows):
        for r in range(R):
            xs = [Fraction(float(X[r, c])) for c, _ in row]
            for o in range(nop):
                terms = [fa * Fraction(float(v[o])) * x for (_, v), x in zip(row, xs)]
                if beta != 0:
                    terms.append(fb * Fraction(float(Y0[r, o, i])))
                exact[r, o, i] = float(sum(terms, Fraction(0)))
                mag[r, o, i] = float(sum((abs(t) for t in terms), Fraction(0)))
    return exact, mag


def flatten_transposed(trows, nop, nrows):
    """The transposed matrix of nop operators, whose product sums over the operators, as ONE single-plane matrix over the columns
    o * nrows + i of a flattened g (nop * nrows,): operator by operator, each in entry order, as apply_transpose sums."""
    return [[(o * nrows + i, v[o:o + 1]) for o in range(nop) for i, v in tr] for tr in trows]


def exact_dot(a, b):
    """sum a_i b_i of two float arrays as a Fraction."""
    return sum((Fraction(float(x)) * Fraction(float(y)) for x, y in zip(np.ravel(a), np.ravel(b))), Fraction(0))


def dense(rows, ncols, o):
    """Operator o as a dense (nrows, ncols) array, the duplicates of a row summed in entry order."""
    return dense_bound(rows, ncols, o)[0]


def dense_bound(rows, ncols, o):
    """(A, tol): operator o dense, and per element the room of another summation order of its duplicates: 2 ulp per duplicate sum,
    in the scale sum |v| of the element's entries (0 for an element with one entry or none)."""
    A, mag, cnt = np.zeros((len(rows), ncols)), np.zeros((len(rows), ncols)), np.zeros((len(rows), ncols))
    for i, r in enumerate(rows):
        for c, v in r:
            A[i, c] += v[o]
            mag[i, c] += abs(v[o])
            cnt[i, c] += 1
    return A, 2 * np.finfo(np.float64).eps * np.maximum(cnt - 1, 0) * mag


def random_structure(nrows, npoints, K, nop, seed, empty_slice=True):
    """A random matrix, not a fit: ragged nk in 0 .. K with 0 and K present, rows 64 .. 127 empty (a slice of width 0) when there are
    that many, columns drawn from the even points (so that some point is never named), a duplicated column and a self column in every
    row that is long enough, an own entry on about half of the rows, column 7 in slot 0 of every row with one (one point named by every
    such row), hoods padded with -1 and npoints, slots padded with NaN."""
    rng = np.random.default_rng([seed, nrows, K, nop])
    nk = rng.integers(0, K + 1, nrows).astype(np.int32)
    nk[0] = K
    if nrows > 1:
        nk[1] = 0
    own_mask = rng.random(nrows) < 0.5
    own_mask[0] = True
    if nrows > 1:
        own_mask[1] = False                         # an empty row
    if empty_slice and nrows >= 128:
        nk[64:128] = 0
        own_mask[64:128] = False
    pts = rng.permutation(npoints)[:nrows].astype(np.int32) if npoints >= nrows else rng.integers(0, npoints, nrows).astype(np.int32)
    hoods = (2 * rng.integers(0, npoints // 2, (nrows, K))).astype(np.int32)
    hoods[:, 0] = 7 % npoints
    if K > 2:
        hoods[:, 2] = hoods[:, 1]                   # a duplicated column
    if K > 3:
        hoods[:, 3] = pts                           # the row's own point among its neighbours
    slots = rng.standard_normal((nop, nrows, K))
    own = rng.standard_normal((nop, nrows))
    pad = np.arange(K)[None, :] >= nk[:, None]
    hoods[pad] = np.where((np.arange(nrows)[:, None] + np.arange(K)[None, :]) % 2 == 0, -1, npoints)[pad]
    slots[:, pad] = np.nan
    own[:, ~own_mask] = np.nan
    return dict(hoods=hoods, nk=nk, slots=slots, own=own, own_mask=own_mask, pts=pts, npoints=npoints)


def named(rows, npoints):
    """bool (npoints,): the points that some live entry names."""
    m = np.zeros(npoints, bool)
    for r in rows:
        for c, _ in r:
            m[c] = True
    return m
