"""Batched verification of point openings over the C ABI (zkp_kzg_point_verifier_* in include/zkp_hip.h): any number of openings
f(z) = y of any number of commitments behind one pairing check.  ``KzgScheme.verify_points`` keeps one verifier and draws the
weights; this module is the handle itself.  Field elements are (n, 4) uint64 Montgomery limbs as everywhere in zkp_hip.
"""
import ctypes as C

import numpy as np

from . import (ZKP_E_ARG, ZkpError, _G1_STATUS_WORD, _Handle, _bytes48, _chk, _dev_ptr, _np, _points, _ptr, _stream_ptr, fr_from_bytes_dev,
               g1_decompress_dev, lib)

NO_BAD_OPENING = C.c_size_t(-1).value  # SIZE_MAX: what zkp_kzg_verify_points_find_bad gives for an accepted batch


class KzgPointVerifier(_Handle):
    """zkp_kzg_point_verifier: any number of point openings (kzg_open, KzgOpener.open_all, KzgEvalOpener.open_batch), of any number of
    commitments, behind one pairing check.  g2s_xy = [s]_2; the verifier needs no SRS and lives on the current slot.  The weights are
    the caller's randomness: see include/zkp_hip.h."""
    _destroy = "zkp_kzg_point_verifier_destroy"

    def __init__(self, g2s_xy, max_openings, max_commits):
        self.max_openings, self.max_commits = int(max_openings), int(max_commits)
        self._h = C.c_void_p()
        g2 = _np(g2s_xy, np.uint64).reshape(24)
        _chk(lib().zkp_kzg_point_verifier_create(_ptr(g2), self.max_openings, self.max_commits, C.byref(self._h)))

    @staticmethod
    def _index(commit_index):
        if commit_index is None:
            return None
        ci = _np(commit_index, np.uint32)
        if ci.ndim != 1:
            raise ZkpError(ZKP_E_ARG, "commit_index is a vector, or None for opening i of commitment i")
        return ci

    def _host_args(self, commitments, commit_index, zs, ys, proofs, weights):
        ci = self._index(commit_index)
        (cxy, cinf), (pxy, pinf) = _points(commitments), _points(proofs)
        count = pxy.shape[0]
        if ci is not None and ci.shape[0] != count:
            raise ZkpError(ZKP_E_ARG, "one proof per opening")
        z, y, wt = _np(zs, np.uint64, (count, 4)), _np(ys, np.uint64, (count, 4)), _np(weights, np.uint64, (count, 4))
        return (cxy, cinf, pxy, pinf, ci, z, y, wt), (self._h, _ptr(cxy), _ptr(cinf), cxy.shape[0], count, _ptr(ci), _ptr(z), _ptr(y), _ptr(pxy),
                                                      _ptr(pinf), _ptr(wt))

    def _dev_args(self, commits_tensor, n_commits, commit_index, n_openings, z_tensor, y_tensor, proofs_tensor, weights_tensor, commits_inf_tensor,
                  proofs_inf_tensor, stream):
        ci = self._index(commit_index)
        if ci is not None and ci.shape[0] != n_openings:
            raise ZkpError(ZKP_E_ARG, "one index per opening")
        cinf = _dev_ptr(commits_inf_tensor, n_commits) if commits_inf_tensor is not None else None
        pinf = _dev_ptr(proofs_inf_tensor, n_openings) if proofs_inf_tensor is not None else None
        return ci, (self._h, _dev_ptr(commits_tensor, 96 * n_commits), cinf, n_commits, n_openings, _ptr(ci), _dev_ptr(z_tensor, 32 * n_openings),
                    _dev_ptr(y_tensor, 32 * n_openings), _dev_ptr(proofs_tensor, 96 * n_openings), pinf, _dev_ptr(weights_tensor, 32 * n_openings),
                    _stream_ptr(stream))

    def verify(self, commitments, zs, ys, proofs, weights, commit_index=None):
        """commitments / proofs: (xy, is_inf) or xy alone; zs, ys, weights (n_openings, 4); commit_index None: opening i belongs to
        commitment i -> accepted"""
        keep, args = self._host_args(commitments, commit_index, zs, ys, proofs, weights)
        acc = C.c_int(0)
        _chk(lib().zkp_kzg_verify_points(*args, C.byref(acc)))
        return bool(acc.value)

    def verify_dev(self, commits_tensor, n_commits, n_openings, z_tensor, y_tensor, proofs_tensor, weights_tensor, commit_index=None,
                   commits_inf_tensor=None, proofs_inf_tensor=None, stream=None):
        """The same with everything but the index vector (host) resident on the verifier's device; blocks like verify."""
        keep, args = self._dev_args(commits_tensor, n_commits, commit_index, n_openings, z_tensor, y_tensor, proofs_tensor, weights_tensor,
                                    commits_inf_tensor, proofs_inf_tensor, stream)
        acc = C.c_int(0)
        _chk(lib().zkp_kzg_verify_points_dev(*args, C.byref(acc)))
        return bool(acc.value)

    def find_bad(self, commitments, zs, ys, proofs, weights, commit_index=None):
        """zkp_kzg_verify_points_find_bad -> None when the batch is accepted, else the lowest index whose opening fails"""
        keep, args = self._host_args(commitments, commit_index, zs, ys, proofs, weights)
        acc, bad = C.c_int(0), C.c_size_t(0)
        _chk(lib().zkp_kzg_verify_points_find_bad(*args, C.byref(acc), C.byref(bad)))
        return None if acc.value else int(bad.value)

    def find_bad_dev(self, commits_tensor, n_commits, n_openings, z_tensor, y_tensor, proofs_tensor, weights_tensor, commit_index=None,
                     commits_inf_tensor=None, proofs_inf_tensor=None, stream=None):
        """find_bad with everything but the index vector resident on the verifier's device"""
        keep, args = self._dev_args(commits_tensor, n_commits, commit_index, n_openings, z_tensor, y_tensor, proofs_tensor, weights_tensor,
                                    commits_inf_tensor, proofs_inf_tensor, stream)
        acc, bad = C.c_int(0), C.c_size_t(0)
        _chk(lib().zkp_kzg_verify_points_find_bad_dev(*args, C.byref(acc), C.byref(bad)))
        return None if acc.value else int(bad.value)

    def verify_each(self, commitments, zs, ys, proofs, commit_index=None):
        """zkp_kzg_verify_points_each: a verdict per opening, no weights -> (ok (n_openings,) uint8, n_bad).  ok[i] = 1 iff opening i
        alone verifies.  Blocks."""
        ci = self._index(commit_index)
        (cxy, cinf), (pxy, pinf) = _points(commitments), _points(proofs)
        count = pxy.shape[0]
        if ci is not None and ci.shape[0] != count:
            raise ZkpError(ZKP_E_ARG, "one proof per opening")
        z, y = _np(zs, np.uint64, (count, 4)), _np(ys, np.uint64, (count, 4))
        ok, bad = np.zeros(count, dtype=np.uint8), C.c_size_t(0)
        _chk(lib().zkp_kzg_verify_points_each(self._h, _ptr(cxy), _ptr(cinf), cxy.shape[0], count, _ptr(ci), _ptr(z), _ptr(y), _ptr(pxy), _ptr(pinf),
                                              _ptr(ok), C.byref(bad)))
        return ok, int(bad.value)

    def verify_each_dev(self, commits_tensor, n_commits, n_openings, z_tensor, y_tensor, proofs_tensor, ok_tensor, commit_index=None,
                        commits_inf_tensor=None, proofs_inf_tensor=None, stream=None):
        """The same with everything but the index vector (host) resident on the verifier's device: ok_tensor receives n_openings
        bytes -> n_bad.  Blocks."""
        ci = self._index(commit_index)
        if ci is not None and ci.shape[0] != n_openings:
            raise ZkpError(ZKP_E_ARG, "one index per opening")
        cinf = _dev_ptr(commits_inf_tensor, n_commits) if commits_inf_tensor is not None else None
        pinf = _dev_ptr(proofs_inf_tensor, n_openings) if proofs_inf_tensor is not None else None
        bad = C.c_size_t(0)
        _chk(lib().zkp_kzg_verify_points_each_dev(self._h, _dev_ptr(commits_tensor, 96 * n_commits), cinf, n_commits, n_openings, _ptr(ci),
                                                  _dev_ptr(z_tensor, 32 * n_openings), _dev_ptr(y_tensor, 32 * n_openings),
                                                  _dev_ptr(proofs_tensor, 96 * n_openings), pinf, _dev_ptr(ok_tensor, n_openings), C.byref(bad),
                                                  _stream_ptr(stream)))
        return int(bad.value)

    def verify_bytes(self, commitments48, zs32, ys32, proofs48, weights, commit_index=None, big_endian=True):
        """The wire form: commitments48 (n_commits x 48) and proofs48 (n_openings x 48) compressed points, zs32 and ys32 n_openings x 32
        bytes of canonical scalars (big-endian unless told otherwise), weights (n_openings, 4) limbs as in verify -> accepted.
        Everything is decoded on the device; the points without the subgroup test, which zkp_kzg_verify_points_dev runs on every
        point anyway.  A point or scalar that does not decode raises ZkpError(ZKP_E_ARG) naming the array, the index and the status
        word."""
        import torch
        cb, pb = _bytes48(commitments48), _bytes48(proofs48)
        count = pb.shape[0]
        if count == 0:
            return True
        pts = []
        for name, b in (("commitments", cb), ("proofs", pb)):
            n = b.shape[0]
            xy = torch.empty(max(n, 1) * 12, dtype=torch.int64, device="cuda")
            inf = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")
            rep = g1_decompress_dev(torch.from_numpy(b).cuda(), n, xy, inf, check_subgroup=False) if n else {"bad": 0}
            if rep["bad"]:
                raise ZkpError(ZKP_E_ARG, f"{name}[{rep['first_bad']}] does not decode ({_G1_STATUS_WORD[rep['first_status']]})")
            pts.append((xy, inf, n))
        scalars = []
        for name, data in (("zs32", zs32), ("ys32", ys32)):
            sb = _np(np.frombuffer(data, dtype=np.uint8).copy() if isinstance(data, (bytes, bytearray, memoryview)) else data, np.uint8, (count, 32))
            out = torch.empty(count * 4, dtype=torch.int64, device="cuda")
            bad, first = fr_from_bytes_dev(torch.from_numpy(sb).cuda(), count, out, big_endian=big_endian)
            if bad:
                raise ZkpError(ZKP_E_ARG, f"{name}[{first}] does not decode (canonical)")
            scalars.append(out)
        wt = torch.from_numpy(_np(weights, np.uint64, (count, 4)).view(np.int64)).cuda()
        (cxy, cinf, n_commits), (pxy, pinf, _) = pts
        return self.verify_dev(cxy, n_commits, count, scalars[0], scalars[1], pxy, wt, commit_index=commit_index, commits_inf_tensor=cinf,
                               proofs_inf_tensor=pinf)

    def aggregate_dev(self, n_commits, n_openings, z_tensor, y_tensor, weights_tensor, out_commit_weights_tensor, out_rz_tensor, out_r_tensor,
                      out_neg_sum_tensor, commit_index=None, stream=None):
        """zkp_kzg_points_aggregate_dev: the field half alone -> the n_commits sums of the weights, r_i z_i, r_i and -sum r_i y_i in the
        four tensors.  Nothing is synchronised."""
        ci = self._index(commit_index)
        if ci is not None and ci.shape[0] != n_openings:
            raise ZkpError(ZKP_E_ARG, "one index per opening")
        _chk(lib().zkp_kzg_points_aggregate_dev(self._h, n_commits, n_openings, _ptr(ci), _dev_ptr(z_tensor, 32 * n_openings),
                                                _dev_ptr(y_tensor, 32 * n_openings), _dev_ptr(weights_tensor, 32 * n_openings),
                                                _dev_ptr(out_commit_weights_tensor, 32 * n_commits), _dev_ptr(out_rz_tensor, 32 * n_openings),
                                                _dev_ptr(out_r_tensor, 32 * n_openings), _dev_ptr(out_neg_sum_tensor, 32), _stream_ptr(stream)))

    def verify_evals_dev(self, eval_opener, evals_tensor, n_polys, z_tensor, commits_tensor, proofs_tensor, weights_tensor, commits_inf_tensor=None,
                         proofs_inf_tensor=None, stream=None):
        """zkp_kzg_verify_evals_batch_dev: the blob form.  Row p of evals_tensor (the rows of eval_opener, a KzgEvalOpener of the same
        slot, in its order) opened at z_p against commitment p and proof p; the values are formed on the device -> accepted"""
        cinf = _dev_ptr(commits_inf_tensor, n_polys) if commits_inf_tensor is not None else None
        pinf = _dev_ptr(proofs_inf_tensor, n_polys) if proofs_inf_tensor is not None else None
        acc = C.c_int(0)
        _chk(lib().zkp_kzg_verify_evals_batch_dev(self._h, eval_opener._h, _dev_ptr(evals_tensor, 32 * eval_opener.n * n_polys), n_polys,
                                                  _dev_ptr(z_tensor, 32 * n_polys), _dev_ptr(commits_tensor, 96 * n_polys), cinf,
                                                  _dev_ptr(proofs_tensor, 96 * n_polys), pinf, _dev_ptr(weights_tensor, 32 * n_polys),
                                                  _stream_ptr(stream), C.byref(acc)))
        return bool(acc.value)
