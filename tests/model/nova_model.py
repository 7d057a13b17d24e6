"""Big-int restatement of the reference's Nova folding (nova/src): compute_t, fold_witness, fold_instance, is_r1cs_satisfied, the
Nova transcript, and the reference's x^3 + x + 5 test R1CS (gen_test_values, nifs/nifs_verifier.rs:98-144).

Field elements are canonical python ints mod R.  Commitments are kept as DISCRETE LOGS: with an SRS [s^i]G whose secret s is known,
commit_vector(v) = v(s) G, so a commitment is the int v(s) mod R and point equality is equality of these ints ("compared in the
exponent through the trapdoor").  ``point(d)`` turns one into the affine point when the transcript needs its bytes.
"""
import hashlib

import numpy as np

import bigmodel as M

R = M.R


# ----------------------------------------------------------------------------- utils.rs / nifs/mod.rs
def matrix_vector_product(matrix, z):  # utils.rs:14-22: dense ragged rows, an entry beyond z is ignored
    return [sum(row[j] * z[j] for j in range(min(len(row), len(z)))) % R for row in matrix]


def csr_matvec(csr, z):
    """The same product over CSR (row_ptr, cols, vals as ints): duplicates add up."""
    rp, cols, vals = csr
    return [sum(vals[e] * z[cols[e]] for e in range(rp[i], rp[i + 1])) % R for i in range(len(rp) - 1)]


def z_vector(w, x, u):  # nifs_prover.rs:22-28
    return list(w) + list(x) + [u]


def compute_t_from(az1, bz1, cz1, az2, bz2, cz2, u1, u2):  # nifs/mod.rs:48-56
    return [(a1 * b2 + a2 * b1 - u1 * c2 - u2 * c1) % R for a1, b1, c1, a2, b2, c2 in zip(az1, bz1, cz1, az2, bz2, cz2)]


def compute_t(r1cs, u1, u2, z1, z2):  # nifs/mod.rs:34-59
    mv = matrix_vector_product
    return compute_t_from(mv(r1cs["a"], z1), mv(r1cs["b"], z1), mv(r1cs["c"], z1), mv(r1cs["a"], z2), mv(r1cs["b"], z2),
                          mv(r1cs["c"], z2), u1, u2)


def compute_t_csr(mats, u1, u2, z1, z2):
    a, b, c = mats
    return compute_t_from(csr_matvec(a, z1), csr_matvec(b, z1), csr_matvec(c, z1), csr_matvec(a, z2), csr_matvec(b, z2),
                          csr_matvec(c, z2), u1, u2)


def fold_witness(r, fw1, fw2, t):  # nifs/mod.rs:64-82
    e = [(e1 + r * tt + r * r * e2) % R for e1, tt, e2 in zip(fw1["e"], t, fw2["e"])]
    w = [(a + b * r) % R for a, b in zip(fw1["w"], fw2["w"])]
    return {"e": e, "w": w}


def fold_instance(r, fi1, fi2, com_t):  # nifs/mod.rs:88-106, commitments as discrete logs
    return {"com_e": (fi1["com_e"] + r * com_t + r * r * fi2["com_e"]) % R, "u": (fi1["u"] + r * fi2["u"]) % R,
            "com_w": (fi1["com_w"] + r * fi2["com_w"]) % R, "x": [(a + b * r) % R for a, b in zip(fi1["x"], fi2["x"])]}


def commit_vector(v, s):  # kzg/src/scheme.rs:63-67 in the exponent
    return M.poly_eval(list(v), s, R)


def is_r1cs_satisfied(r1cs, fi, fw, s):  # r1cs/mod.rs:94-127
    if r1cs["num_vars"] != len(fw["w"]) or r1cs["num_io"] != len(fi["x"]):
        return False
    z = z_vector(fw["w"], fi["x"], fi["u"])
    az, bz, cz = (matrix_vector_product(r1cs[k], z) for k in "abc")
    eq = all(a * b % R == (fi["u"] * c + e) % R for a, b, c, e in zip(az, bz, cz, fw["e"]))
    return eq and fi["com_w"] == commit_vector(fw["w"], s) and fi["com_e"] == commit_vector(fw["e"], s)


def residual_rows(r1cs, w, x, u, e):
    z = z_vector(w, x, u)
    az, bz, cz = (matrix_vector_product(r1cs[k], z) for k in "abc")
    return sum(1 for a, b, c, ee in zip(az, bz, cz, e) if a * b % R != (u * c + ee) % R)


# ----------------------------------------------------------------------------- transcript.rs
def point(d):
    """discrete log -> affine point (bigmodel form; None = identity)."""
    return M.g1_mul(M.G1, d)


def g1_bytes(pt):  # serialize_uncompressed(G1Affine), as PLONK's ChallengeGenerator feeds it
    if pt is None:
        return bytes([0x40]) + bytes(95)
    return pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big")


class Transcript:
    """Transcript<Sha256>, nova/src/transcript.rs:69-114.  challenges() returns canonical field values."""

    def __init__(self):
        self.data, self.generated = None, False

    def _absorb(self, b):
        self.data = hashlib.sha256((self.data or b"") + b).digest()
        self.generated = False

    def feed(self, pt):
        self._absorb(g1_bytes(pt))

    def feed_scalar_num(self, v):  # serialize_uncompressed(Fr): canonical, 32 bytes little-endian
        self._absorb((v % R).to_bytes(32, "little"))

    def generate_challenges(self, n):
        if self.generated or self.data is None:
            raise RuntimeError("I'm hungry! Feed me something first")
        self.generated = True
        rng = M.StdRng(int.from_bytes(self.data[:8], "little"))
        return [M.fr_from_mont(rng.rand_field(R, 4)) for _ in range(n)]


# ----------------------------------------------------------------------------- NIFS with a known SRS secret
def kzg_open(v, z, s):
    """open_vector at z: (quotient commitment as a discrete log, evaluation)."""
    c = M.poly_trim(list(v))
    if not c:
        return 0, 0
    q = M.poly_div_linear(c, z, R)
    return M.poly_eval(q, s, R), M.poly_eval(c, z, R)


def instance(fw, x, s):  # FWitness::commit, r1cs/mod.rs:58-70
    return {"com_e": commit_vector(fw["e"], s), "u": 1, "com_w": commit_vector(fw["w"], s), "x": list(x)}


def prover(r1cs, fw1, fw2, fi1, fi2, s, tr):  # nifs_prover.rs:11-47
    z1, z2 = z_vector(fw1["w"], fi1["x"], fi1["u"]), z_vector(fw2["w"], fi2["x"], fi2["u"])
    t = compute_t(r1cs, fi1["u"], fi2["u"], z1, z2)
    com_t = commit_vector(t, s)
    tr.feed_scalar_num(fi1["u"])
    tr.feed_scalar_num(fi2["u"])
    tr.feed(point(com_t))
    r, = tr.generate_challenges(1)
    return fold_witness(r, fw1, fw2, t), fold_instance(r, fi1, fi2, com_t), com_t, r, t


def prove(r, fw, fi, s, tr):  # nifs_prover.rs:49-70
    tr.feed(point(fi["com_e"]))
    tr.feed(point(fi["com_w"]))
    z, = tr.generate_challenges(1)
    return {"r": r, "opening_point": z, "opening_e": kzg_open(fw["e"], z, s), "opening_w": kzg_open(fw["w"], z, s)}


# ----------------------------------------------------------------------------- nifs_verifier.rs:98-144
REF_A = [[1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [1, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 5]]
REF_B = [[1, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 1]]
REF_C = [[0, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 1, 0]]


def gen_test_values(inputs):
    """(r1cs, witnesses, x) of the reference's x^3 + x + 5 = y example."""
    r1cs = {"a": REF_A, "b": REF_B, "c": REF_C, "num_io": 1, "num_vars": 4}
    w = [[i, i * i, i ** 3, i ** 3 + i] for i in inputs]
    x = [[i ** 3 + i + 5] for i in inputs]
    return r1cs, w, x


# ----------------------------------------------------------------------------- ABI forms
def fr_limbs(vals):
    """canonical ints -> (n, 4) uint64 Montgomery limbs."""
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        m = M.fr_to_mont(v % R)
        for k in range(4):
            out[i, k] = (m >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return out


def fr_ints(limbs):
    """(n, 4) uint64 Montgomery limbs -> canonical ints."""
    a = np.asarray(limbs, dtype=np.uint64).reshape(-1, 4)
    return [M.fr_from_mont(sum(int(a[i, k]) << (64 * k) for k in range(4))) for i in range(a.shape[0])]


def g1_abi(pt):
    """affine point (bigmodel) -> ((12,) uint64 Montgomery limbs, is_inf)."""
    xy = np.zeros(12, dtype=np.uint64)
    if pt is None:
        return xy, 1
    for j, v in enumerate(pt):
        m = M.fq_to_mont(v)
        for k in range(6):
            xy[6 * j + k] = (m >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return xy, 0
