"""Nova folding (nova/src) over the C ABI: the NIFS prover, its openings and its verifier, and the relaxed-R1CS check.

Same names as the reference: R1CS (r1cs/mod.rs:9-16) is ``NovaR1CS``, FInstance / FWitness (r1cs/mod.rs:19-36),
NIFS::{prover, prove, verify} (nifs/nifs_prover.rs, nifs/nifs_verifier.rs) are ``nifs_prover`` / ``nifs_prove`` / ``nifs_verify``,
Transcript (transcript.rs) is ``NovaTranscript``.  Field elements are (n, 4) uint64 Montgomery limbs as everywhere in zkp_hip; a
commitment is ``(xy (12,) uint64, is_inf)``.  Witness vectors are numpy arrays (the host-pointer entries) or contiguous CUDA tensors
of int64 (the ``*_dev`` entries, used in place).
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import G1Bases, KzgScheme, ZkpError, ZKP_E_ARG, _Handle, _chk, _dev_ptr, _np, _ptr, _stream_ptr, kzg_commit, lib

_R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
FR_ONE = np.array([(((1 << 256) % _R) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)  # Fr::one()

# *accepted of zkp_nova_nifs_verify, with the reference's messages (nifs_verifier.rs:22-91)
VERIFY_RESULTS = {1: "accepted", -1: "Verify: Error in computing random r", -2: "Verify: Error in computing random opening point",
                  0: "Verify: Folding wrong at W", -3: "Verify: Folding wrong at E"}


class _Csr(C.Structure):  # zkp_csr in include/zkp_hip.h
    _fields_ = [("row_ptr", C.c_void_p), ("cols", C.c_void_p), ("vals", C.c_void_p)]


class _Instance(C.Structure):  # zkp_nova_instance
    _fields_ = [("com_e_xy", C.c_uint64 * 12), ("com_e_is_inf", C.c_uint8), ("u", C.c_uint64 * 4), ("com_w_xy", C.c_uint64 * 12),
                ("com_w_is_inf", C.c_uint8), ("x", C.c_void_p)]


class _Proof(C.Structure):  # zkp_nova_proof
    _fields_ = [("r", C.c_uint64 * 4), ("opening_point", C.c_uint64 * 4), ("open_e_xy", C.c_uint64 * 12), ("open_e_is_inf", C.c_uint8),
                ("eval_e", C.c_uint64 * 4), ("open_w_xy", C.c_uint64 * 12), ("open_w_is_inf", C.c_uint8), ("eval_w", C.c_uint64 * 4)]


def _arr(a):
    return np.ctypeslib.as_array(a).copy()


def _is_tensor(a):
    return hasattr(a, "is_cuda") and a.is_cuda


# ----------------------------------------------------------------------------- matrices
def csr_from_dense(matrix, ncols):
    """The reference's dense ragged rows (utils.rs:14-22) -> (row_ptr u64, cols u32, vals (nnz, 4) u64).

    ``matrix`` is a list of rows; row i is a sequence of Fr limbs ((k, 4) array or k arrays of 4), possibly shorter than z.  Zero
    entries are dropped (they add nothing to the dense sum), and so are entries at columns >= ncols: matrix_vector_product only
    walks min(len(row), len(z)) columns (utils.rs:17)."""
    row_ptr, cols, vals = [0], [], []
    for row in matrix:
        row = _np(row, np.uint64, (-1, 4)) if len(row) else np.zeros((0, 4), dtype=np.uint64)
        nz = np.nonzero(row.any(axis=1))[0]
        nz = nz[nz < ncols]
        cols.extend(int(j) for j in nz)
        vals.append(row[nz])
        row_ptr.append(len(cols))
    return (np.array(row_ptr, dtype=np.uint64), np.array(cols, dtype=np.uint32),
            np.concatenate(vals).reshape(-1, 4) if vals else np.zeros((0, 4), dtype=np.uint64))


def csr_from_triplets(rows, row_idx, cols, vals):
    """(row, column, value) entries in any order -> CSR.  Duplicates are kept (the kernels add them up, as a dense sum would) and
    explicit zeros are kept; entries of a row stay in their given order."""
    row_idx = np.asarray(row_idx, dtype=np.int64)
    order = np.argsort(row_idx, kind="stable")
    counts = np.bincount(row_idx, minlength=rows)[:rows] if len(row_idx) else np.zeros(rows, dtype=np.int64)
    row_ptr = np.zeros(rows + 1, dtype=np.uint64)
    row_ptr[1:] = np.cumsum(counts)
    return row_ptr, np.asarray(cols, dtype=np.uint32)[order], _np(vals, np.uint64, (-1, 4))[order]


class NovaR1CS(_Handle):
    """R1CS (r1cs/mod.rs:9-16) resident on the SRS's device as CSR (zkp_nova_r1cs_create)."""
    _destroy = "zkp_nova_r1cs_destroy"

    def __init__(self, srs, rows, num_vars, num_io, a, b, c):
        """a, b, c: (row_ptr, cols, vals) CSR triples."""
        self.srs = _bases(srs) if srs is not None else None
        self.rows, self.num_vars, self.num_io = int(rows), int(num_vars), int(num_io)
        keep, mats = [], []
        for m in (a, b, c):
            rp = _np(m[0], np.uint64)
            cl = _np(m[1], np.uint32) if m[1] is not None else None
            vl = _np(m[2], np.uint64, (-1, 4)) if m[2] is not None else None
            keep += [rp, cl, vl]
            ptr = lambda a: a.ctypes.data if a is not None and a.size else None
            mats.append(_Csr(rp.ctypes.data, ptr(cl), ptr(vl)))
        self._h = C.c_void_p()
        _chk(lib().zkp_nova_r1cs_create(self.srs._h if self.srs is not None else None, self.rows, self.num_vars, self.num_io, C.byref(mats[0]), C.byref(mats[1]),
                                        C.byref(mats[2]), C.byref(self._h)))

    @classmethod
    def from_dense(cls, srs, matrix_a, matrix_b, matrix_c, num_vars, num_io):
        """The reference's own form: three lists of dense ragged rows (equal row counts)."""
        if not (len(matrix_a) == len(matrix_b) == len(matrix_c)):
            raise ZkpError(ZKP_E_ARG, "A, B and C must have the same number of rows")
        ncols = num_vars + num_io + 1
        return cls(srs, len(matrix_a), num_vars, num_io, *(csr_from_dense(m, ncols) for m in (matrix_a, matrix_b, matrix_c)))

    def cross_term_dev(self, w1, x1, u1, w2, x2, u2, t_out, stream=None):
        """NIFS::compute_t (nifs/mod.rs:34-59) into the CUDA tensor t_out (rows x 4 int64)."""
        x1, x2 = _np(x1, np.uint64, (-1, 4)), _np(x2, np.uint64, (-1, 4))
        u1, u2 = _np(u1, np.uint64, (4,)), _np(u2, np.uint64, (4,))
        _chk(lib().zkp_nova_cross_term_dev(self._h, _dev_ptr(w1, 32 * self.num_vars), _ptr(x1), _ptr(u1), _dev_ptr(w2, 32 * self.num_vars),
                                           _ptr(x2), _ptr(u2), _dev_ptr(t_out, 32 * self.rows), _stream_ptr(stream)))
        return t_out

    def fold_witness_dev(self, r, e1, w1, e2, w2, t, e_out, w_out, stream=None):
        """NIFS::fold_witness (nifs/mod.rs:64-82); e_out / w_out may be e1 / w1."""
        r = _np(r, np.uint64, (4,))
        eb, wb = 32 * self.rows, 32 * self.num_vars
        _chk(lib().zkp_nova_fold_witness_dev(self._h, _ptr(r), _dev_ptr(e1, eb), _dev_ptr(w1, wb), _dev_ptr(e2, eb), _dev_ptr(w2, wb),
                                             _dev_ptr(t, eb), _dev_ptr(e_out, eb), _dev_ptr(w_out, wb), _stream_ptr(stream)))

    def relaxed_residual(self, w, x, u, e, stream=None):
        """Number of rows with (A z)_i (B z)_i != u (C z)_i + E_i (r1cs/mod.rs:111-118); w, e: CUDA tensors or host arrays."""
        w, e = _to_device(w), _to_device(e)
        x, u = _np(x, np.uint64, (-1, 4)), _np(u, np.uint64, (4,))
        bad = C.c_uint64(0)
        _chk(lib().zkp_nova_relaxed_residual_dev(self._h, _dev_ptr(w, 32 * self.num_vars), _ptr(x), _ptr(u), _dev_ptr(e, 32 * self.rows),
                                                 _stream_ptr(stream), C.byref(bad)))
        return int(bad.value)


def _bases(srs):
    if isinstance(srs, G1Bases):
        return srs
    if isinstance(srs, KzgScheme):
        return srs.srs.bases
    return srs.bases  # zkp_hip.Srs


def _to_device(a):
    if _is_tensor(a):
        return a
    import torch
    return torch.from_numpy(_np(a, np.uint64, (-1, 4)).view(np.int64)).cuda()


# ----------------------------------------------------------------------------- instances, witnesses, transcript
@dataclass
class FInstance:
    """r1cs/mod.rs:19-26: com_e, com_w = (xy, is_inf); u (4,); x (num_io, 4)."""
    com_e: tuple
    u: np.ndarray
    com_w: tuple
    x: np.ndarray

    def _c(self):
        s = _Instance()
        s.com_e_xy[:] = [int(v) for v in _np(self.com_e[0], np.uint64).reshape(12)]
        s.com_e_is_inf = int(self.com_e[1])
        s.u[:] = [int(v) for v in _np(self.u, np.uint64).reshape(4)]
        s.com_w_xy[:] = [int(v) for v in _np(self.com_w[0], np.uint64).reshape(12)]
        s.com_w_is_inf = int(self.com_w[1])
        x = _np(self.x, np.uint64, (-1, 4)).copy()
        s.x = x.ctypes.data if x.size else None
        return s, x

    @staticmethod
    def _from_c(s, x):
        return FInstance((_arr(s.com_e_xy), int(s.com_e_is_inf)), _arr(s.u), (_arr(s.com_w_xy), int(s.com_w_is_inf)), x)


@dataclass
class FWitness:
    """r1cs/mod.rs:29-36: e (rows, 4), w (num_vars, 4) -- numpy arrays or CUDA tensors."""
    e: object
    w: object

    @classmethod
    def new(cls, w, rows):  # FWitness::new, r1cs/mod.rs:39-47: E = 0
        if _is_tensor(w):
            import torch
            return cls(torch.zeros(rows * 4, dtype=torch.int64, device=w.device), w)
        return cls(np.zeros((rows, 4), dtype=np.uint64), _np(w, np.uint64, (-1, 4)))

    def commit(self, scheme, x):  # r1cs/mod.rs:58-70: commit_vector on E and W, u = 1
        host = lambda a: a.cpu().numpy().view(np.uint64).reshape(-1, 4) if _is_tensor(a) else a
        b = _bases(scheme)
        return FInstance(kzg_commit(b, host(self.e)), FR_ONE.copy(), kzg_commit(b, host(self.w)), _np(x, np.uint64, (-1, 4)))


@dataclass
class NifsProof:
    """NIFSProof, nifs/mod.rs:19-25 (each opening = (point, evaluation))."""
    r: np.ndarray
    opening_point: np.ndarray
    opening_e: tuple
    opening_w: tuple

    def _c(self):
        s = _Proof()
        s.r[:] = [int(v) for v in self.r]
        s.opening_point[:] = [int(v) for v in self.opening_point]
        for name, (pt, ev) in (("e", self.opening_e), ("w", self.opening_w)):
            getattr(s, f"open_{name}_xy")[:] = [int(v) for v in _np(pt[0], np.uint64).reshape(12)]
            setattr(s, f"open_{name}_is_inf", int(pt[1]))
            getattr(s, f"eval_{name}")[:] = [int(v) for v in _np(ev, np.uint64).reshape(4)]
        return s

    @staticmethod
    def _from_c(s):
        return NifsProof(_arr(s.r), _arr(s.opening_point), ((_arr(s.open_e_xy), int(s.open_e_is_inf)), _arr(s.eval_e)),
                         ((_arr(s.open_w_xy), int(s.open_w_is_inf)), _arr(s.eval_w)))


class NovaTranscript(_Handle):
    """Transcript<Sha256> (nova/src/transcript.rs)."""
    _destroy = "zkp_nova_transcript_destroy"

    def __init__(self):
        self._h = C.c_void_p()
        _chk(lib().zkp_nova_transcript_create(C.byref(self._h)))

    def feed(self, commitment):  # transcript.rs:69-78
        xy, inf = commitment
        _chk(lib().zkp_nova_transcript_feed(self._h, _ptr(_np(xy, np.uint64).reshape(12)), int(inf)))

    def feed_scalar_num(self, s):  # transcript.rs:80-88
        _chk(lib().zkp_nova_transcript_feed_scalar(self._h, _ptr(_np(s, np.uint64, (4,)))))

    feed_scalar = feed_scalar_num

    def generate_challenges(self, n):  # transcript.rs:95-114
        out = np.zeros((n, 4), dtype=np.uint64)
        _chk(lib().zkp_nova_transcript_challenges(self._h, n, _ptr(out)))
        return out

    challenges = generate_challenges


# ----------------------------------------------------------------------------- NIFS
def nifs_prover(r1cs, fw1, fw2, fi1, fi2, transcript, inplace=False, stream=None):
    """NIFS::prover (nifs_prover.rs:11-47) -> (FWitness, FInstance, com_t, r).  CUDA-tensor witnesses go through the `_dev` entry;
    with inplace=True the folded witness overwrites fw1's buffers (the running instance of an IVC chain)."""
    c1, x1 = fi1._c()
    c2, x2 = fi2._c()
    xo = np.zeros((r1cs.num_io, 4), dtype=np.uint64)
    co = _Instance()
    co.x = xo.ctypes.data if xo.size else None
    ct_xy, ct_inf, r = np.zeros(12, dtype=np.uint64), C.c_uint8(0), np.zeros(4, dtype=np.uint64)
    eb, wb = 32 * r1cs.rows, 32 * r1cs.num_vars
    if _is_tensor(fw1.e):
        e_out, w_out = (fw1.e, fw1.w) if inplace else (fw1.e.clone(), fw1.w.clone())
        _chk(lib().zkp_nova_nifs_prover_dev(r1cs._h, _dev_ptr(fw1.e, eb), _dev_ptr(fw1.w, wb), _dev_ptr(fw2.e, eb), _dev_ptr(fw2.w, wb),
                                            C.byref(c1), C.byref(c2), transcript._h, _dev_ptr(e_out, eb), _dev_ptr(w_out, wb),
                                            _stream_ptr(stream), C.byref(co), _ptr(ct_xy), C.byref(ct_inf), _ptr(r)))
    else:
        e1, w1 = _np(fw1.e, np.uint64, (-1, 4)), _np(fw1.w, np.uint64, (-1, 4))
        e2, w2 = _np(fw2.e, np.uint64, (-1, 4)), _np(fw2.w, np.uint64, (-1, 4))
        if e1.shape[0] != r1cs.rows or e2.shape[0] != r1cs.rows or w1.shape[0] != r1cs.num_vars or w2.shape[0] != r1cs.num_vars:
            raise ZkpError(ZKP_E_ARG, "witness sizes do not match the R1CS")
        e_out, w_out = (e1, w1) if inplace else (np.empty_like(e1), np.empty_like(w1))  # e1 / w1 are views of fw1's arrays when possible
        _chk(lib().zkp_nova_nifs_prover(r1cs._h, _ptr(e1), _ptr(w1), _ptr(e2), _ptr(w2), C.byref(c1), C.byref(c2), transcript._h,
                                        _ptr(e_out), _ptr(w_out), C.byref(co), _ptr(ct_xy), C.byref(ct_inf), _ptr(r)))
    return FWitness(e_out, w_out), FInstance._from_c(co, xo), (ct_xy, int(ct_inf.value)), r


def nifs_prove(r1cs, r, fw, fi, transcript, stream=None):
    """NIFS::prove (nifs_prover.rs:49-70): openings of E and W at the transcript's point, computed on the device."""
    c, _x = fi._c()
    out = _Proof()
    rr = _np(r, np.uint64, (4,))
    if _is_tensor(fw.e):
        _chk(lib().zkp_nova_nifs_prove_dev(r1cs._h, _ptr(rr), _dev_ptr(fw.e, 32 * r1cs.rows), _dev_ptr(fw.w, 32 * r1cs.num_vars),
                                           C.byref(c), transcript._h, _stream_ptr(stream), C.byref(out)))
    else:
        e, w = _np(fw.e, np.uint64, (-1, 4)), _np(fw.w, np.uint64, (-1, 4))
        if e.shape[0] != r1cs.rows or w.shape[0] != r1cs.num_vars:
            raise ZkpError(ZKP_E_ARG, "witness sizes do not match the R1CS")
        _chk(lib().zkp_nova_nifs_prove(r1cs._h, _ptr(rr), _ptr(e), _ptr(w), C.byref(c), transcript._h, C.byref(out)))
    return NifsProof._from_c(out)


def nifs_verify(g2s_xy, proof, fi1, fi2, fi3, com_t, transcript):
    """NIFS::verify (nifs_verifier.rs:22-91): 1 accepted, otherwise the rejection code of VERIFY_RESULTS."""
    p = proof._c()
    (c1, _x1), (c2, _x2), (c3, _x3) = fi1._c(), fi2._c(), fi3._c()
    g2s = _np(g2s_xy, np.uint64).reshape(24)
    ct = _np(com_t[0], np.uint64).reshape(12)
    acc = C.c_int(0)
    _chk(lib().zkp_nova_nifs_verify(_ptr(g2s), C.byref(p), C.byref(c1), C.byref(c2), C.byref(c3), _ptr(ct), int(com_t[1]), transcript._h,
                                    C.byref(acc)))
    return acc.value


def is_r1cs_satisfied(r1cs, fi, fw, scheme):
    """r1cs/mod.rs:94-127: the relaxed equation on the device (zkp_nova_relaxed_residual_dev) and both commitments."""
    if r1cs.num_io != len(_np(fi.x, np.uint64, (-1, 4))):
        return False
    if r1cs.relaxed_residual(fw.w, fi.x, fi.u, fw.e) != 0:
        return False
    again = FWitness(fw.e, fw.w).commit(scheme, fi.x)
    same = lambda a, b: a[1] == b[1] and (a[1] or np.array_equal(_np(a[0], np.uint64).reshape(12), _np(b[0], np.uint64).reshape(12)))
    return same(again.com_e, fi.com_e) and same(again.com_w, fi.com_w)
