"""Utilities of the wlsqm package.

    wlsqm.utils.lapackdrivers  # batched dense solves (LU / Bunch-Kaufman on the GPU) and small matrix helpers

Like the reference, ``wlsqm`` itself does not re-export this subpackage: ``import wlsqm.utils.lapackdrivers``.
"""
