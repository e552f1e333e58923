"""CPU-only checks of the CONTRACTED numerics mode (mode 3: the accurate mode with its neighbour sums, LU update and substitutions
fused; csrc/fit_accurate.hip with FMA = true).

(1) The mode code travels: wlsqm.hip.set_strict / get_strict / strict() / contracted() and WLSQM_HIP_STRICT carry 3 (host state of the
    library: no device needed).
(2) The mode's accuracy claim, asserted where it is deterministic: its CPU statement — oracle/variants.c with V_SYM | V_FMA, which the GPU
    kernels must equal bit for bit (tests/test_gpu_contracted.py) — against the reference's own output on the full-density goldens, against
    the oracle with the function value known, and on the sweep goldens.  The bound is the north star's 1e-10 per column, without a spare
    factor: the measured values (printed; pytest -s) are 5.4e-11 on config_C2_1M, 5.3e-11 on config_C5_1M and 9.0e-11 on config_C5_16M.
"""
import os
import sys
import threading

import numpy as np
import pytest

import _cases as K
import _contracted as CT
import _parity as P

TOL = CT.TOL               # north star: 1e-10 relative, per column
DENSE = ("C2_1M", "C5_1M", "C5_16M")


@pytest.fixture(scope="module")
def whip():
    from wlsqm import _binding
    if not os.path.exists(_binding.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    import wlsqm.hip as h
    return h


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


_bits = CT.bits


def _in_new_thread(f):
    seen = {}

    def run():
        seen["v"] = f()
    t = threading.Thread(target=run); t.start(); t.join()
    return seen["v"]


# ---- (1) mode codes ----------------------------------------------------------------------------------------------------------

def test_mode_3_round_trips(whip):
    prev = whip.set_strict(False)
    try:
        assert whip.set_strict("contracted") is False and whip.get_strict() == 3
        assert whip.set_strict(3) == 3 and whip.get_strict() == 3
        assert whip.set_strict("3") == 3 and whip.get_strict() == 3
        assert whip.set_strict("accurate") == 3 and whip.get_strict() == 2
        assert whip.set_strict("Contracted") == 2 and whip.get_strict() == 3
        assert whip.set_strict(True) == 3 and whip.get_strict() is True
        assert whip.set_strict(0) is True and whip.get_strict() is False
        with whip.strict(3):
            assert whip.get_strict() == 3
        assert whip.get_strict() is False
        with whip.strict("contracted"):
            assert whip.get_strict() == 3
        assert whip.get_strict() is False
        with whip.contracted():
            assert whip.get_strict() == 3
        assert whip.get_strict() is False
        assert "contracted" in whip.__all__
        # the C ABI itself: 3 is stored as 3 (it used to fold to 1), values beyond the documented codes still mean strict
        from wlsqm import _binding
        L = _binding.lib()
        L.wlsqm_hip_set_strict(3)
        assert L.wlsqm_hip_get_strict() == 3
        assert L.wlsqm_hip_set_strict(7) == 3 and L.wlsqm_hip_get_strict() == 1
        assert L.wlsqm_hip_set_strict(0) == 1
    finally:
        whip.set_strict(prev)


def test_mode_3_nests_with_the_other_modes(whip):
    prev = whip.set_strict(False)
    try:
        with whip.contracted():
            assert whip.get_strict() == 3
            with whip.accurate():
                assert whip.get_strict() == 2
                with whip.contracted():
                    assert whip.get_strict() == 3
                    with whip.strict():
                        assert whip.get_strict() is True
                    assert whip.get_strict() == 3
                    with whip.strict(False):
                        assert whip.get_strict() is False
                    assert whip.get_strict() == 3
                    with whip.strict(None):                      # None: leave the mode alone
                        assert whip.get_strict() == 3
                assert whip.get_strict() == 2
            assert whip.get_strict() == 3
        assert whip.get_strict() is False
        with whip.strict():
            with whip.contracted():
                assert whip.get_strict() == 3
            assert whip.get_strict() is True
        with pytest.raises(RuntimeError):
            with whip.contracted():
                raise RuntimeError("body")
        assert whip.get_strict() is False
        with pytest.raises(ValueError):
            whip.set_strict("fastest")
        assert whip.get_strict() is False
    finally:
        whip.set_strict(prev)


@pytest.mark.parametrize("value,mode", [("3", 3), ("contracted", 3), ("C", 3), ("c", 3), ("2", 2), ("accurate", 2), ("1", True), ("yes", True),
                                        ("0", False), ("", False)])
def test_a_fresh_thread_takes_its_mode_from_the_environment(whip, monkeypatch, value, mode):
    """WLSQM_HIP_STRICT is read at a thread's first use: 3.. / c.. / C.. now select the contracted mode (they used to fall under "anything
    else: strict"); every other value keeps its meaning.  The mode is per thread: the new thread's does not leak into this one."""
    prev = whip.set_strict(False)
    try:
        monkeypatch.setenv("WLSQM_HIP_STRICT", value)
        got = _in_new_thread(whip.get_strict)
        assert got == mode and (got is mode or mode in (2, 3))
        assert whip.get_strict() is False
        # ... and a thread that sets mode 3 itself keeps it to itself
        assert _in_new_thread(lambda: (whip.set_strict(3), whip.get_strict())[1]) == 3
        assert whip.get_strict() is False
    finally:
        whip.set_strict(prev)


# ---- (2) the CPU statement against the goldens -----------------------------------------------------------------------------------

def _variant(oracle, c, fi0, kn, flags):
    return CT.statement(oracle, c["dim"], c["order"], c["xk"], c["fk"], c["nk_a"], c["xi"], fi0, kn, c["wm_a"], fl=flags)


@pytest.mark.parametrize("name", DENSE)
def test_cpu_statement_against_the_references_output(oracle, name):
    """V_SYM | V_FMA on the full-density goldens: every column within 1e-10 of what the reference itself returned."""
    c = K.config_dense(name)
    got = _variant(oracle, c, c["fi0"], c["knowns_a"], oracle.V_SYM | oracle.V_FMA)
    sym = _variant(oracle, c, c["fi0"], c["knowns_a"], oracle.V_SYM)
    E = P.column_metric(got, c["g"]["fi"]); Es = P.column_metric(sym, c["g"]["fi"])
    print("%s vs the reference: contracted E_max %.3e (%d of %d columns <= 1e-10), accurate %.3e" % (name, E.max(), int((E <= TOL).sum()), E.size, Es.max()))
    assert np.all(E <= TOL), "%s: E = %s" % (name, E)


@pytest.mark.parametrize("name", DENSE)
def test_cpu_statement_with_the_function_value_known(oracle, name):
    """knowns = b?_F on every case (the default of every fit_* function): the derivative columns within 1e-10 of the oracle's, the known
    column untouched."""
    c = K.config_dense(name)
    n = len(c["nk_a"])
    kn = np.ones(n, np.int64)
    got = _variant(oracle, c, c["fi0"], kn, oracle.V_SYM | oracle.V_FMA)
    sym = _variant(oracle, c, c["fi0"], kn, oracle.V_SYM)
    ora = c["fi0"].copy()
    oracle.fit_many(c["dim"], c["xk"], c["fk"], c["nk_a"], c["xi"], ora, None, 0, np.full(n, c["order"], np.int32), kn, c["wm_a"], ntasks=8)
    assert np.array_equal(_bits(got[:, 0]), _bits(c["fi0"][:, 0])), "the known value is not written"
    E = P.column_metric(got[:, 1:], ora[:, 1:]); Es = P.column_metric(sym[:, 1:], ora[:, 1:])
    print("%s, F known, vs the oracle: contracted E_max %.3e, accurate %.3e" % (name, E.max(), Es.max()))
    assert np.all(E <= TOL), "%s: E = %s" % (name, E)


def test_cpu_statement_is_not_the_accurate_modes(oracle):
    """Guard against a vacuous check: the fused sums change bits (on most cases of config_C2_1M), so the two flags are two statements."""
    c = K.config_dense("C2_1M")
    got = _variant(oracle, c, c["fi0"], c["knowns_a"], oracle.V_SYM | oracle.V_FMA)
    sym = _variant(oracle, c, c["fi0"], c["knowns_a"], oracle.V_SYM)
    differ = (_bits(got) != _bits(sym)).any(axis=1)
    print("config_C2_1M: %d of %d cases differ in bits between V_SYM | V_FMA and V_SYM" % (differ.sum(), len(differ)))
    assert differ.sum() > len(differ) // 2
    assert np.allclose(got, sym, rtol=1e-6, atol=0)                      # ... and still the same fit


@pytest.mark.parametrize("dim", [2, 3])
def test_cpu_statement_on_the_sweep_goldens(oracle, dim):
    """Sweep goldens (every order, both weightings, knowns masks incl. stray bits, ragged nk), orders 0-3 in 2D and 0-2 in 3D: per order
    P.assert_parity against the reference's fi, and no further from the extended-precision solution than twice the oracle's distance
    plus 1e-12 (measured: at most 0.59 of that bound)."""
    got, ora, truth, d = CT.sweep_statement(oracle, dim)
    CT.check_sweep(got, ora, truth, d, dim, "contracted (CPU statement)")
