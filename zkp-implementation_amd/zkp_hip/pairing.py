"""Pairing-product checks on the GPU over the C ABI (zkp_pairing_checker_* in include/zkp_hip.h): many independent checks
prod_j e(P[c][j], Q_j) == 1 over k fixed G2 points per launch, one verdict byte per check.  Points are (.., 12) uint64 Montgomery
limbs as everywhere in zkp_hip; the value a check can return is E = (the canonical pairing product)^3, 12 x 6 limbs in
``zkp_hip.pairing``'s order.
"""
import ctypes as C

import numpy as np

import sys
import types

from . import ZKP_E_ARG, ZkpError, _Handle, _chk, _dev_ptr, _np, _ptr, _stream_ptr, lib
from . import pairing as _host_pairing  # the package's function zkp_hip.pairing(p, q): still the attribute while this module loads


class _PairingModule(types.ModuleType):
    """Importing this module rebinds the package attribute `pairing` from the function to the module; the module stays callable
    as that function, so zkp_hip.pairing(p_xy, q_xy) means the same before and after the import."""

    def __call__(self, *args, **kwargs):
        return _host_pairing(*args, **kwargs)


sys.modules[__name__].__class__ = _PairingModule

# operation numbers of zkp_selftest_fq12_dev
FQ12_MUL, FQ12_SQR, FQ12_MUL_LINE, FQ12_INVERSE, FQ12_FROB1, FQ12_FROB2, FQ12_FROB3, FQ12_CYCLO_SQR, FQ12_FINAL_EXP = range(9)


class PairingChecker(_Handle):
    """zkp_pairing_checker: g2_xy (k, 24) fixed G2 points, k in 1 .. 8 (g2_is_inf: k flags marking identity slots), for at most
    max_checks checks per call.  Lives on the current slot."""
    _destroy = "zkp_pairing_checker_destroy"

    def __init__(self, g2_xy, max_checks, g2_is_inf=None):
        g2 = _np(g2_xy, np.uint64)
        if g2.size % 24 or not g2.size:
            raise ZkpError(ZKP_E_ARG, "g2_xy is (k, 24) limbs")
        g2 = g2.reshape(-1, 24)
        self.k, self.max_checks = g2.shape[0], int(max_checks)
        inf = _np(g2_is_inf, np.uint8, (self.k,)) if g2_is_inf is not None else None
        self._h = C.c_void_p()
        _chk(lib().zkp_pairing_checker_create(_ptr(g2), _ptr(inf), self.k, self.max_checks, C.byref(self._h)))

    def check_batch(self, p_xy, p_is_inf=None, validate=True, values=False):
        """p_xy (n_checks, k, 12) host limbs, p_is_inf (n_checks, k) or None -> ok (n_checks,) uint8, and with values=True also
        E (n_checks, 12, 6).  Blocks."""
        p = _np(p_xy, np.uint64).reshape(-1, self.k, 12)
        n = p.shape[0]
        inf = _np(p_is_inf, np.uint8, (n, self.k)) if p_is_inf is not None else None
        ok = np.zeros(n, dtype=np.uint8)
        out = np.zeros((n, 12, 6), dtype=np.uint64) if values else None
        _chk(lib().zkp_pairing_check_batch(self._h, _ptr(p), _ptr(inf), n, int(bool(validate)), _ptr(ok), _ptr(out)))
        return (ok, out) if values else ok

    def check_batch_dev(self, p_tensor, n_checks, ok_tensor=None, p_inf_tensor=None, validate=True, out_tensor=None, stream=None):
        """The same with everything resident on the checker's device: p_tensor n_checks x k x 12 limbs, ok_tensor n_checks bytes,
        out_tensor n_checks x 72 limbs (either may be None, not both).  validate defaults to True as in check_batch (it synchronises);
        with validate=False nothing is synchronised."""
        n, pts = int(n_checks), int(n_checks) * self.k
        _chk(lib().zkp_pairing_check_batch_dev(self._h, _dev_ptr(p_tensor, 96 * pts), _dev_ptr(p_inf_tensor, pts) if p_inf_tensor is not None else None,
                                               n, int(bool(validate)), _dev_ptr(ok_tensor, n) if ok_tensor is not None else None,
                                               _dev_ptr(out_tensor, 576 * n) if out_tensor is not None else None, _stream_ptr(stream)))

    def miller_dev(self, p_tensor, n_checks, out_tensor, p_inf_tensor=None, stream=None):
        """zkp_selftest_miller_dev: the Miller value before the final exponentiation, n_checks x 72 limbs into out_tensor"""
        n, pts = int(n_checks), int(n_checks) * self.k
        _chk(lib().zkp_selftest_miller_dev(self._h, _dev_ptr(p_tensor, 96 * pts), _dev_ptr(p_inf_tensor, pts) if p_inf_tensor is not None else None, n,
                                           _dev_ptr(out_tensor, 576 * n), _stream_ptr(stream)))


def selftest_fq12_dev(op, a_tensor, b_tensor, n, out_tensor, stream=None):
    """zkp_selftest_fq12_dev: one lane per case, n x 72 limbs in a (and b, for the two-operand operations) and out"""
    _chk(lib().zkp_selftest_fq12_dev(int(op), _dev_ptr(a_tensor, 576 * n), _dev_ptr(b_tensor, 576 * n) if b_tensor is not None else None, int(n),
                                     _dev_ptr(out_tensor, 576 * n), _stream_ptr(stream)))


def final_exp_counts():
    """zkp_selftest_final_exp_counts -> (host pairing checks ended in the x-chain, in the plain power) since the library was loaded"""
    out = np.zeros(2, dtype=np.uint64)
    _chk(lib().zkp_selftest_final_exp_counts(_ptr(out)))
    return int(out[0]), int(out[1])
