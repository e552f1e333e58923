"""Inputs and reference answers shared by tests/test_solve_adjoint_host.py and tests/test_gpu_solve_adjoint.py: the case generator of
test_gpu_round2.py::test_solve_many_operator_path (ragged nk within 7 of K, case 7 fully known, mixed weightings), a stack of
gradients g, and per field the answer of tests/_adjoint_ref.py.  A reference is computed once per shape and shared; nothing modifies it."""
import numpy as np

import _adjoint_ref as R
import _cases as K
import synth

_CACHE = {}


def classes(no, knowns):
    """(unknown, true-known, dropped) DOF lists of a case as effective_mask splits them (infra.pyx:119-121: stray high bits drop the
    last unknowns)."""
    kn = int(knowns)
    free = [a for a in range(no) if not (kn >> a) & 1]
    extra = bin(kn >> no).count("1")
    nun = max(len(free) - extra, 0)
    return free[:nun], [a for a in range(no) if (kn >> a) & 1], free[nun:]


def geometry(dim, order, Kn, knowns, n=333, seed=None):
    no = K.NDOF[dim][order]
    rng = np.random.default_rng(1000 * dim + 100 * order + Kn if seed is None else seed)
    if dim == 1:
        S = np.sort(rng.uniform(0, 1, 3000))
        hoods = synth.knn(S[:, None], Kn, workers=2)[:n]
    else:
        S = synth.halton(3000, dim, skip=1)
        hoods = synth.knn(S, Kn, workers=2)[:n]
    xk = S[hoods]; xi = S[:n].copy()
    nk = rng.integers(max(no + 2, Kn - 7), Kn + 1, n).astype(np.int32); nk[0] = Kn
    kn = np.full(n, knowns, np.int64); kn[7] = (1 << no) - 1                      # one case with nothing to solve
    wm = np.full(n, 2, np.int32); wm[::4] = 1
    # every case has at least unknowns + 2 neighbours: nothing is left out of any maximum
    ok, _ = R.resolvable(dim, np.full(n, order), nk, kn)
    assert ok.all()
    return dict(dim=dim, order=order, K=Kn, n=n, no=no, xk=xk, xi=xi, nk=nk, knowns=kn, wm=wm, mask=int(knowns),
                orders=np.full(n, order, np.int32))


def problem(dim, order, Kn, knowns, nfields, n=333):
    """geometry + g (nfields, n, no) + per field the reference: ref_fk (nfields, n, K), ref_fi (nfields, n, no), s (nfields, n)."""
    key = (dim, order, Kn, int(knowns), nfields, n)
    if key in _CACHE:
        return _CACHE[key]
    c = geometry(dim, order, Kn, knowns, n)
    rng = np.random.default_rng(7 + 13 * Kn + order)
    g = rng.uniform(-1.0, 1.0, (nfields, n, c["no"]))
    ref_fk, ref_fi, s = np.zeros((nfields, n, Kn)), np.zeros((nfields, n, c["no"])), np.zeros((nfields, n))
    sens = None
    for r in range(nfields):
        # (the oracle's sensitivities depend on the geometry only: computed by the first field's call and handed to the others)
        ref = R.adjoint_ref(dim, order, c["xk"], c["nk"], c["xi"], c["knowns"], c["wm"], g[r], sens=sens)
        ref_fk[r], ref_fi[r], s[r] = ref["grad_fk"], ref["grad_fi"], ref["s"]
        sens = ref["sens"]
    c.update(g=g, ref_fk=ref_fk, ref_fi=ref_fi, s=s, sens=sens)
    for a in (g, ref_fk, ref_fi, s):
        a.setflags(write=False)
    _CACHE[key] = c
    return c
