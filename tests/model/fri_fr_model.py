"""Independent big-int + hashlib model of the FRI commitment path over the BLS12-381 scalar field Fr (TEST INFRASTRUCTURE ONLY).

fri/src is generic over F: PrimeField; this is its Fr instance, on canonical Python integers:
  * hasher.rs:14-36            hash / hash_slice: SHA-256 over Display strings, digest as a little-endian integer mod r
  * merkle_tree.rs:42-135      levels (odd last node hashed alone) and authentication paths
  * fiat_shamir/transcript.rs  SHA-256(prev || index_le64 || Display), seed = first 8 digest bytes, StdRng, F::rand
  * prover.rs:141-168          generate_proof, flattened to the layout of zkp_fri_prove_fr (include/zkp_hip.h)
Field arithmetic, the layer evaluation, the fold and StdRng come from bigmodel.py's field-parametric pieces."""
import hashlib
import struct

import bigmodel as M

R = M.R
GENERATOR = M.FR_GENERATOR  # ark-bls12-381 Fr GENERATOR


def display(x, zero_as_0=False):
    """ark-ff 0.4 Display: the canonical integer in decimal, zero prints as the empty string."""
    return (str(x) if x else ("0" if zero_as_0 else "")).encode()


def hash_slice(vals, zero_as_0=False):
    h = hashlib.sha256(b"".join(display(v, zero_as_0) for v in vals)).digest()
    return int.from_bytes(h, "little") % R


def merkle_levels(leaves, zero_as_0=False):
    n = len(leaves)
    depth = (n - 1).bit_length() if n > 1 else 0
    levels = [[hash_slice([v], zero_as_0) for v in leaves]]
    for _ in range(depth):
        prev = levels[-1]
        levels.append([hash_slice(prev[i:i + 2], zero_as_0) for i in range(0, len(prev), 2)])
    return levels


def merkle_path(levels, index):
    path, cur = [], index
    for i in range(len(levels) - 1):
        path.append(levels[i][cur ^ 1])
        cur //= 2
    return path


def merkle_node_count(n):
    return sum(len(l) for l in merkle_levels([0] * n)) if n else 0


class FriTranscript:
    def __init__(self, zero_as_0=False):
        self.data, self.index, self.z0 = b"", 0, zero_as_0
        self.digest(0)

    def digest(self, canon):
        self.data = hashlib.sha256(self.data + struct.pack("<Q", self.index) + display(canon, self.z0)).digest()
        self.index += 1

    def rng(self):
        return M.StdRng(int.from_bytes(self.data[:8], "little"))

    def challenge(self):
        """F::rand: the sampled integer is the Montgomery residue; returns the canonical value"""
        return M.fr_from_mont(self.rng().rand_field(R, 4))

    def challenge_list_usize(self, n):
        r = self.rng()
        return [M.fr_from_mont(r.rand_field(R, 4)) & (2 ** 64 - 1) for _ in range(n)]


def layer_eval(coeffs, coset, size):
    """FriLayer::from_poly: Horner at every point for small layers, the coset NTT (same values) for larger ones."""
    if len(coeffs) * size <= 4096:
        return M.fri_layer_eval(coeffs, coset, size, mod=R)
    return M.coset_ntt(list(coeffs) + [0] * (size - len(coeffs)), coset, mod=R)


def fri_prove(coeffs, blowup, nq, zero_as_0=False):
    """generate_proof over Fr on canonical integers; returns a dict."""
    poly = M.poly_trim(list(coeffs))
    dom = 1
    while dom < len(poly) * blowup:
        dom <<= 1
    layers_n = dom.bit_length() - 1
    t, coset, size = FriTranscript(zero_as_0), GENERATOR, dom
    layers = []
    for _ in range(layers_n):
        evals = layer_eval(poly, coset, size)
        levels = merkle_levels(evals, zero_as_0)
        t.digest(levels[-1][0])
        layers.append((evals, levels, size))
        poly = M.fri_fold(poly, t.challenge(), mod=R)
        coset, size = coset * coset % R, size // 2
    const = poly[0] if poly else 0
    t.digest(const)
    queries = []
    for ch in ([c % dom for c in t.challenge_list_usize(nq)] if layers else []):
        rec = []
        for evals, levels, size in layers:
            idx = ch % size
            sym = (idx + size // 2) % size
            rec.append((idx, evals[idx], evals[sym], merkle_path(levels, idx), merkle_path(levels, sym)))
        queries.append(rec)
    return {"domain_size": dom, "coset": GENERATOR, "number_of_queries": nq, "roots": [l[1][-1][0] for l in layers],
            "const": const, "queries": queries}


def limbs(x):
    """canonical integer -> 4 little-endian u64 words of its Montgomery form (arkworks memory form)"""
    return M.to_limbs(M.fr_to_mont(x), 4)


def fri_flatten(proof):
    out = [proof["domain_size"], len(proof["roots"]), proof["number_of_queries"]] + limbs(proof["coset"])
    for r in proof["roots"]:
        out += limbs(r)
    out += limbs(proof["const"])
    for rec in proof["queries"]:
        for idx, ev, sv, path, spath in rec:
            out += [idx] + limbs(ev) + limbs(sv)
            for x in path + spath:
                out += limbs(x)
    return out


def to_mem(vals):
    """canonical integers -> (n, 4) memory-form rows (as lists)"""
    return [limbs(v) for v in vals]


def from_mem(rows):
    return [M.fr_from_mont(M.from_limbs([int(w) for w in r])) for r in rows]
