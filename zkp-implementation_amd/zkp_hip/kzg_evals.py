"""Evaluation-form KZG over the C ABI (zkp_kzg_eval_opener_* in include/zkp_hip.h): commitments and openings of a batch of polynomials
given by their values on the roots of unity, with no transform.  ``KzgScheme.commit_evals_batch`` / ``open_evals_batch`` keep one
opener per shape; this module is the handle itself.  Field elements are (n, 4) uint64 Montgomery limbs as everywhere in zkp_hip.
"""
import ctypes as C

import numpy as np

from . import ZKP_KZG_ORDER_BITREV, ZKP_KZG_ORDER_NATURAL, _Handle, _chk, _dev_ptr, _np, _ptr, _stream_ptr, lib


class KzgEvalOpener(_Handle):
    """zkp_kzg_eval_opener: commitments and openings of up to max_polys polynomials per call, each given by its n = 2^log_n values
    on the roots of unity (position i: the value at w^i, or at w^bitrev(i) with bitrev=True), with no transform.  lagrange_bases is
    G1Bases.lagrange(log_n) of the SRS, borrowed (kept alive here).  Row p of every result is what kzg_commit / kzg_open return for
    the coefficients of row p's interpolant."""
    _destroy = "zkp_kzg_eval_opener_destroy"

    def __init__(self, lagrange_bases, log_n, max_polys=1, bitrev=False):
        self.log_n, self.n, self.max_polys, self.bitrev = log_n, 1 << log_n, int(max_polys), bool(bitrev)
        self._lagrange = lagrange_bases
        self._h = C.c_void_p()
        _chk(lib().zkp_kzg_eval_opener_create(lagrange_bases._h, log_n, ZKP_KZG_ORDER_BITREV if bitrev else ZKP_KZG_ORDER_NATURAL,
                                              self.max_polys, C.byref(self._h)))

    def _rows(self, evals):
        evals = _np(evals, np.uint64)
        if evals.ndim != 3 or evals.shape[1:] != (self.n, 4):
            raise ValueError("a (P, n, 4) array of evaluations")
        return evals

    def commit_batch(self, evals):
        """evals (P, n, 4) -> ((P, 12) commitments, (P,) flags)"""
        evals = self._rows(evals)
        polys = evals.shape[0]
        xy = np.zeros((polys, 12), dtype=np.uint64)
        inf = np.zeros(polys, dtype=np.uint8)
        _chk(lib().zkp_kzg_commit_evals_batch(self._h, _ptr(evals), polys, _ptr(xy), _ptr(inf)))
        return xy, inf

    def commit_batch_dev(self, evals_tensor, n_polys, stream=None):
        """The same with the rows resident on the opener's device; blocks like commit_batch."""
        xy = np.zeros((n_polys, 12), dtype=np.uint64)
        inf = np.zeros(n_polys, dtype=np.uint8)
        _chk(lib().zkp_kzg_commit_evals_batch_dev(self._h, _dev_ptr(evals_tensor, 32 * self.n * n_polys), n_polys, _stream_ptr(stream),
                                                  _ptr(xy), _ptr(inf)))
        return xy, inf

    def open_batch(self, evals, zs):
        """evals (P, n, 4), zs (P, 4) -> (((P, 12) proofs, (P,) flags), (P, 4) values y_p = f_p(z_p))"""
        evals = self._rows(evals)
        polys = evals.shape[0]
        zs = _np(zs, np.uint64, (polys, 4))
        xy = np.zeros((polys, 12), dtype=np.uint64)
        inf = np.zeros(polys, dtype=np.uint8)
        y = np.zeros((polys, 4), dtype=np.uint64)
        _chk(lib().zkp_kzg_open_evals_batch(self._h, _ptr(evals), polys, _ptr(zs), _ptr(xy), _ptr(inf), _ptr(y)))
        return (xy, inf), y

    def open_batch_dev(self, evals_tensor, n_polys, z_tensor, stream=None):
        """The same with the rows and the points z resident on the opener's device; blocks like open_batch."""
        xy = np.zeros((n_polys, 12), dtype=np.uint64)
        inf = np.zeros(n_polys, dtype=np.uint8)
        y = np.zeros((n_polys, 4), dtype=np.uint64)
        _chk(lib().zkp_kzg_open_evals_batch_dev(self._h, _dev_ptr(evals_tensor, 32 * self.n * n_polys), n_polys, _dev_ptr(z_tensor, 32 * n_polys),
                                                _stream_ptr(stream), _ptr(xy), _ptr(inf), _ptr(y)))
        return (xy, inf), y

    def field_dev(self, evals_tensor, n_polys, z_tensor, out_y_tensor, out_quotient_tensor, stream=None):
        """zkp_kzg_open_evals_field_dev: the field half alone -> y (n_polys x 4) and the quotients' values (n_polys x n x 4, natural
        order whatever the opener's) in the two tensors.  Nothing is allocated, nothing synchronised."""
        _chk(lib().zkp_kzg_open_evals_field_dev(self._h, _dev_ptr(evals_tensor, 32 * self.n * n_polys), n_polys, _dev_ptr(z_tensor, 32 * n_polys),
                                                _dev_ptr(out_y_tensor, 32 * n_polys), _dev_ptr(out_quotient_tensor, 32 * self.n * n_polys),
                                                _stream_ptr(stream)))
