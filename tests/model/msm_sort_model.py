"""Host model of the MSM's digit recoding and counting sort (csrc/msm.hpp: msm_digits* .. msm_order; csrc/msm_host.inc: launch_sort),
stage by stage, as zkp_selftest_msm_sort_dev hands the stage outputs back.  Plain Python and numpy; the scalars are Python ints.

  reference_digits(geom, scalars, base_is_inf)   the digits the recoding must produce, bit for bit (it is deterministic)
  check_sort_outputs(geom, digits, outputs)      the contract of every later stage, the digits being the input truth
  reference_outputs(geom, digits)                ONE valid set of outputs (the CPU test corrupts it to show that the checker bites)

`geom` is the geometry dict of zkp_hip.selftest_msm_sort_dev: c, nwin, nb, nslice, shared, glv, lo_bits, nhi, run_limit, piece, over_cap,
desc_cap, n (entries per sort window), ns (scalars of the range), off (nslice + 1 bit offsets).  Every array is uint32 and window-major:
digits (W, n), entries (W, n, 2), pstart (W, nhi + 1), ghist (W, 256), start (W, nb + 2), sorted (W, n), perm (W, nb), over (W, 2),
over_b (W, over_cap), over_off (W, over_cap + 1), desc (W, desc_cap, 4).  The hook fills the outputs with 0xFF bytes before the sort runs,
so a word no kernel owns must still read 0xFFFFFFFF.

Several stages place their items with atomics (msm_partscatter inside a partition, msm_binsort inside a bucket, msm_rank inside a size
class): those orders are unspecified, and the checker compares them as sets, never position by position."""
import numpy as np

LAMBDA = 0xAC45A4010001A40200000000FFFFFFFF  # the endomorphism's eigenvalue (csrc/glv.hpp; tests/test_glv_cpu.py derives it)
FILL = 0xFFFFFFFF
OUTPUTS = ("entries", "pstart", "ghist", "start", "sorted", "perm", "over", "over_b", "over_off", "desc")


class SortContractError(AssertionError):
    def __init__(self, window, stage, index, what):
        super().__init__(f"window {window}, stage {stage}, index {index}: {what}")
        self.window, self.stage, self.index = window, stage, index


# ---------------------------------------------------------------------------------------------------------------- digits
def recode(k, off):
    """The signed digits of the integer k over the slices [off[s], off[s + 1]) with the carry rule of msm_recode: a slice value (plus
    the carry in) above 2^(width - 1) becomes that value minus 2^width and carries one into the next slice."""
    digits, carry = [], 0
    for s in range(len(off) - 1):
        width = off[s + 1] - off[s]
        u = ((k >> off[s]) & ((1 << width) - 1)) + carry
        if u > 1 << (width - 1):
            digits.append(u - (1 << width))
            carry = 1
        else:
            digits.append(u)
            carry = 0
    return digits, carry


def check_recoding(k, off, digits, carry):
    """The model's own check: the digits say k exactly, no carry leaves the top slice, every |d| <= 2^(width - 1)."""
    assert carry == 0, f"carry out of the top slice of {k:#x}"
    assert sum(d << off[s] for s, d in enumerate(digits)) == k, f"digits of {k:#x} do not sum to it"
    for s, d in enumerate(digits):
        assert abs(d) <= 1 << (off[s + 1] - off[s] - 1), f"digit {s} of {k:#x} out of range"


def encode(d):
    return (abs(d) << 1) | (1 if d < 0 else 0)


def reference_digits(geom, scalars_canonical, base_is_inf=None):
    """scalars_canonical: one list of ns canonical integers per MSM of the batch; base_is_inf: ns flags or None.  -> (W, n) uint32,
    laid out [group][slice][scalar]: group = the MSM, or with glv geometry 2m for k mod lambda and 2m + 1 for k div lambda."""
    off, ns, nslice = list(geom["off"]), geom["ns"], geom["nslice"]
    assert len(off) == nslice + 1
    groups = []
    for sc in scalars_canonical:
        assert len(sc) == ns
        if geom["glv"]:
            groups.append([k % LAMBDA for k in sc])
            groups.append([k // LAMBDA for k in sc])
        else:
            groups.append(list(sc))
    out = np.zeros((len(groups), nslice, ns), dtype=np.uint32)
    for gi, vals in enumerate(groups):
        for i, k in enumerate(vals):
            digits, carry = recode(k, off)
            check_recoding(k, off, digits, carry)
            if base_is_inf is not None and base_is_inf[i]:
                continue  # an infinity base contributes nothing: every digit 0 = skip
            out[gi, :, i] = [encode(d) for d in digits]
    assert out.size == geom["nwin"] * geom["n"], "geometry: nwin x n is not groups x slices x scalars"
    return out.reshape(geom["nwin"], geom["n"])


R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def edge_scalars(off, glv=False):
    """The scalars every case carries next to its random ones, built from the slice offsets of the geometry under test: 0, 1, r - 1,
    every slice all ones (the carry runs through every window), every slice 2^(width - 1) (the largest positive digit: bucket nb), every
    slice 2^(width - 1) + 1 (the first negative one), and those two values -- and 2^(width - 1) - 1, which the carry lifts to bucket
    nb -- behind a lowest slice of all ones, i.e. with a carry coming in.  Top bits are cleared until the value is below r.  glv: the
    patterns are laid into both halves, k = k1 + lambda k2 with k1 < lambda."""
    nslice = len(off) - 1
    width = [off[s + 1] - off[s] for s in range(nslice)]

    def lay(val_of_slice):
        return sum(val_of_slice(s) << off[s] for s in range(nslice))

    pats = [lay(lambda s: (1 << width[s]) - 1), lay(lambda s: 1 << (width[s] - 1)), lay(lambda s: (1 << (width[s] - 1)) + 1)]
    for rest in (0, 1, -1):
        pats.append(lay(lambda s: (1 << width[s]) - 1 if s == 0 else (1 << (width[s] - 1)) + rest))

    def below(v, bound):
        while v >= bound:
            v &= (1 << (v.bit_length() - 1)) - 1
        return v

    if glv:
        out = []
        for v in pats:
            k1, k2 = below(v, LAMBDA), below(v, LAMBDA)
            while k1 + LAMBDA * k2 >= R:
                k2 >>= 1
            out += [k1 + LAMBDA * k2, k1, LAMBDA * k2]
    else:
        out = [below(v, R) for v in pats]
    return [0, 1, R - 1] + out


def plant_c8_buckets(geom, scalars, edge, skip=()):
    """Scalars for per-window c = 8 whose window 0 has buckets 1..4 of exactly 255, run_limit, run_limit + 1 and 3 piece + 1 entries:
    the low byte of every scalar is set (1..4 as often as that, then 5..120 in turn: positive digits only).  The indices in `skip`
    (bases flagged infinity, which leave no digit) are passed over, and the last len(edge) scalars become those edge scalars whose lowest
    digit keeps out of buckets 1..4, then random ones again."""
    sizes = [255, geom["run_limit"], geom["run_limit"] + 1, 3 * geom["piece"] + 1]
    keep = [k for k in edge if abs(recode(k, geom["off"])[0][0]) not in (1, 2, 3, 4)]
    body = len(scalars) - len(edge)
    low = iter([b + 1 for b, k in enumerate(sizes) for _ in range(k)])
    out = []
    for i in range(body):
        byte = 77 if i in skip else next(low, 5 + i % 116)
        out.append((scalars[i] & ~0xFF) | byte)
    assert next(low, None) is None, "too few scalars for the planted buckets"
    out += keep
    out += [(k & ~0xFF) | 77 for k in scalars[len(out):]]
    assert len(out) == len(scalars) and all(k < R for k in out)
    return out


def model_geometry(count, ns, c=None, slice_off=None, glv=False, lo_bits=None):
    """The geometry plan_msm (csrc/msm_plan.hpp) gives a single-range pass, for the CPU tests of this model (the GPU tests take theirs from
    the hook).  slice_off None: per-window buckets of c bits; otherwise the shared bucket set of bases expanded with those offsets."""
    shared = slice_off is not None
    if shared:
        off = list(slice_off)
        c = max(off[s + 1] - off[s] for s in range(len(off) - 1))
    else:
        off = [s * c for s in range(-(-256 // c) + 1)]
    nslice = len(off) - 1
    nwin = (2 if glv else 1) * count if shared else nslice * count
    n = nslice * ns if shared else ns
    nb = 1 << (c - 1)
    if lo_bits is None:
        lo_bits = min(10 if c >= 21 else 9 if c >= 20 else 8, c - 1)
    piece = max(32, n // nb)
    run_limit = max(128, 4 * (n // nb))
    return {"c": c, "nwin": nwin, "nb": nb, "nslice": nslice, "shared": int(shared), "glv": int(glv), "lo_bits": lo_bits, "nhi": nb >> lo_bits,
            "run_limit": run_limit, "piece": piece, "over_cap": min(n // 128 + 1, nb), "desc_cap": n // piece + n // run_limit + 2,
            "n": n, "ns": ns, "off": off}


def balanced_slice_offsets(cover, window_bits):
    """msm_slice_offsets (csrc/msm_plan.hpp) with balancing from any overshoot: ceil(cover / window_bits) slices of floor / ceil bits."""
    planes = -(-cover // window_bits)
    base, rem = divmod(cover, planes)
    off = [0]
    for k in range(planes):
        off.append(off[-1] + base + (1 if k < rem else 0))
    return off


# ---------------------------------------------------------------------------------------------------------------- the sort
def _first(mask):
    return int(np.flatnonzero(mask)[0])


def _window_truth(geom, w, dw):
    """What the digits of one window determine: bucket sizes, partition sizes, both prefixes, the size classes."""
    nb, nhi, lo_bits = geom["nb"], geom["nhi"], geom["lo_bits"]
    b = (dw >> 1).astype(np.int64)
    if (b > nb).any():
        raise SortContractError(w, "digits", _first(b > nb), "bucket id above nb")
    nz = b[b != 0]
    counts = np.bincount(nz, minlength=nb + 1)[1:]
    pcount = np.bincount((nz - 1) >> lo_bits, minlength=nhi)
    t = {"b": b, "counts": counts, "total": int(nz.size), "pcount": pcount}
    t["pstart"] = np.concatenate(([0], np.cumsum(pcount)))
    t["start"] = np.concatenate(([0, 0], np.cumsum(counts)))  # start[0] = 0, start[b] = entries of buckets below b, start[nb + 1] = total
    t["cls"] = np.minimum(counts, 255)
    t["ghist"] = np.bincount(255 - t["cls"], minlength=256)
    return t


def _expect_equal(w, stage, got, want):
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    if got.shape != want.shape:
        raise SortContractError(w, stage, 0, f"shape {got.shape}, expected {want.shape}")
    if (got != want).any():
        i = _first((got != want).reshape(-1))
        raise SortContractError(w, stage, i, f"is {int(got.reshape(-1)[i])}, expected {int(want.reshape(-1)[i])}")


def _expect_untouched(w, stage, arr, first):
    flat = np.asarray(arr).reshape(-1)
    if (flat != FILL).any():
        i = _first(flat != FILL)
        raise SortContractError(w, stage, first + i, f"word past the kernel's own slots was written ({int(flat[i]):#x})")


def _expect_distinct(w, stage, idx):
    order = np.argsort(idx, kind="stable")
    s = idx[order]
    dup = s[1:] == s[:-1]
    if dup.any():
        i = _first(dup)
        raise SortContractError(w, stage, int(order[i + 1]), f"index {int(s[i])} appears twice (also at {int(order[i])})")


def _pieces_of(geom, sizes):
    return np.where(sizes > geom["run_limit"], (sizes + geom["piece"] - 1) // geom["piece"], 0)


def check_sort_outputs(geom, digits, outputs):
    """Raises SortContractError (window, stage, first offending index) unless `outputs` is a valid result of the sort of `digits`."""
    W, n, nb, nhi, lo_bits = geom["nwin"], geom["n"], geom["nb"], geom["nhi"], geom["lo_bits"]
    run_limit, piece, over_cap, desc_cap = geom["run_limit"], geom["piece"], geom["over_cap"], geom["desc_cap"]
    lo_mask = (1 << lo_bits) - 1
    shapes = {"entries": (W, n, 2), "pstart": (W, nhi + 1), "ghist": (W, 256), "start": (W, nb + 2), "sorted": (W, n), "perm": (W, nb),
              "over": (W, 2), "over_b": (W, over_cap), "over_off": (W, over_cap + 1), "desc": (W, desc_cap, 4)}
    o = {k: np.asarray(outputs[k]).view(np.uint32).reshape(shapes[k]) for k in OUTPUTS}
    digits = np.asarray(digits).view(np.uint32).reshape(W, n)
    for w in range(W):
        dw = digits[w].astype(np.int64)
        t = _window_truth(geom, w, dw)
        counts, total, cls = t["counts"], t["total"], t["cls"]

        # ---- first pass: partition sizes and the entries of every partition (order inside a partition unspecified)
        _expect_equal(w, "pstart", o["pstart"][w], t["pstart"])
        ent = o["entries"][w].astype(np.int64)
        x, y = ent[:total, 0], ent[:total, 1]
        idx, sign = x & 0x7FFFFFFF, x >> 31
        if (idx >= n).any():
            raise SortContractError(w, "entries", _first(idx >= n), "index outside the window")
        d_at = dw[idx]
        hi_of_pos = np.repeat(np.arange(nhi), t["pcount"])
        bad = (d_at >> 1) == 0
        if bad.any():
            raise SortContractError(w, "entries", _first(bad), f"index {int(idx[_first(bad)])} has a zero digit")
        bad = ((d_at >> 1) - 1) >> lo_bits != hi_of_pos
        if bad.any():
            i = _first(bad)
            raise SortContractError(w, "entries", i, f"bucket {int(d_at[i] >> 1)} filed in partition {int(hi_of_pos[i])}")
        bad = y != (((d_at >> 1) - 1) & lo_mask)
        if bad.any():
            raise SortContractError(w, "entries", _first(bad), ".y is not the low bits of the bucket of its index")
        bad = sign != (d_at & 1)
        if bad.any():
            raise SortContractError(w, "entries", _first(bad), "sign bit differs from the digit's")
        _expect_distinct(w, "entries", idx)
        _expect_untouched(w, "entries", o["entries"][w][total:], total)

        # ---- second pass: bucket starts and the sorted indices (order inside a bucket unspecified)
        _expect_equal(w, "start", o["start"][w], t["start"])
        s = o["sorted"][w].astype(np.int64)
        idx = s[:total] & 0x7FFFFFFF
        if (idx >= n).any():
            raise SortContractError(w, "sorted", _first(idx >= n), "index outside the window")
        bucket_of_pos = np.repeat(np.arange(1, nb + 1), counts)
        bad = dw[idx] != ((bucket_of_pos << 1) | (s[:total] >> 31))
        if bad.any():
            i = _first(bad)
            raise SortContractError(w, "sorted", i, f"position of bucket {int(bucket_of_pos[i])} holds {int(s[i]):#x}, whose digit is "
                                                    f"{int(dw[idx[i]]):#x}")
        _expect_distinct(w, "sorted", idx)
        _expect_untouched(w, "sorted", o["sorted"][w][total:], total)

        # ---- size histogram and the ranking (order inside a size class unspecified)
        _expect_equal(w, "ghist", o["ghist"][w], t["ghist"])
        perm = o["perm"][w].astype(np.int64)
        bad = (perm < 1) | (perm > nb)
        if bad.any():
            raise SortContractError(w, "perm", _first(bad), f"{int(perm[_first(bad)])} is no bucket id")
        seen = np.bincount(perm, minlength=nb + 1)[1:]
        if (seen != 1).any():
            bkt = _first(seen != 1) + 1
            raise SortContractError(w, "perm", bkt, f"bucket {bkt} appears {int(seen[bkt - 1])} times")
        pc = cls[perm - 1]
        if (pc[1:] > pc[:-1]).any():
            i = _first(pc[1:] > pc[:-1]) + 1
            raise SortContractError(w, "perm", i, f"rank {i} (bucket {int(perm[i])}, size class {int(pc[i])}) follows a smaller class {int(pc[i - 1])}")

        # ---- oversized buckets and their pieces.  The caps are a condition on the reference, not something measured
        n_over = int((cls > min(run_limit, 254)).sum())
        sizes_all_pieces = int(_pieces_of(geom, counts).sum())
        if n_over > over_cap:
            raise SortContractError(w, "plan", n_over, f"{n_over} candidates exceed over_cap {over_cap}")
        if sizes_all_pieces > desc_cap:
            raise SortContractError(w, "plan", sizes_all_pieces, f"{sizes_all_pieces} pieces exceed desc_cap {desc_cap}")
        if int(o["over"][w][0]) != n_over:
            raise SortContractError(w, "over", 0, f"n_over is {int(o['over'][w][0])}, expected {n_over}")
        over_b = o["over_b"][w].astype(np.int64)
        _expect_equal(w, "over_b", over_b[:n_over], perm[:n_over])
        _expect_untouched(w, "over_b", o["over_b"][w][n_over:], n_over)
        cand_sizes = counts[over_b[:n_over] - 1]
        cand_pieces = _pieces_of(geom, cand_sizes)
        off = np.concatenate(([0], np.cumsum(cand_pieces)))
        _expect_equal(w, "over_off", o["over_off"][w][:n_over + 1], off)
        _expect_untouched(w, "over_off", o["over_off"][w][n_over + 1:], n_over + 1)
        n_pieces = int(off[-1])
        if int(o["over"][w][1]) != n_pieces:
            raise SortContractError(w, "over", 1, f"piece total is {int(o['over'][w][1])}, expected {n_pieces}")
        desc = o["desc"][w].astype(np.int64)
        db = np.repeat(over_b[:n_over], cand_pieces)
        dp = np.arange(n_pieces) - np.repeat(off[:-1], cand_pieces)
        first = t["start"][db] + dp * piece
        want = np.stack([db, dp, first, np.minimum(first + piece, t["start"][db + 1])], axis=1).reshape(-1, 4)
        _expect_equal(w, "desc", desc[:n_pieces], want)
        _expect_untouched(w, "desc", o["desc"][w][n_pieces:], n_pieces)
        # the tiling as a property of its own, from the descriptors alone: no piece longer than `piece`, the pieces of a bucket above
        # run_limit cover [start[b], start[b + 1]) exactly once, no other bucket has a piece
        d = desc[:n_pieces]
        if n_pieces:
            ln = d[:, 3] - d[:, 2]
            bad = (ln <= 0) | (ln > piece)
            if bad.any():
                raise SortContractError(w, "desc tiling", _first(bad), f"piece of {int(ln[_first(bad)])} entries (piece = {piece})")
            bad = (d[:, 0] < 1) | (d[:, 0] > nb)
            if bad.any():
                raise SortContractError(w, "desc tiling", _first(bad), "piece of no bucket")
            bad = counts[d[:, 0] - 1] <= run_limit
            if bad.any():
                i = _first(bad)
                raise SortContractError(w, "desc tiling", i, f"bucket {int(d[i, 0])} of {int(counts[d[i, 0] - 1])} entries (run_limit {run_limit}) has a piece")
        covered = np.zeros(total + 1, dtype=np.int64)
        if n_pieces:
            np.add.at(covered, d[:, 2], 1)
            np.add.at(covered, d[:, 3], -1)
        covered = np.cumsum(covered)[:total]
        must = np.repeat(counts > run_limit, counts).astype(np.int64)
        if (covered != must).any():
            i = _first(covered != must)
            raise SortContractError(w, "desc tiling", i, f"sorted position {i} (bucket {int(bucket_of_pos[i])}) is covered by {int(covered[i])} "
                                                         f"pieces, expected {int(must[i])}")
        if n_pieces:  # a piece stays inside its own bucket
            bad = (d[:, 2] < t["start"][d[:, 0]]) | (d[:, 3] > t["start"][d[:, 0] + 1])
            if bad.any():
                raise SortContractError(w, "desc tiling", _first(bad), "piece leaves its bucket's run")


def reference_outputs(geom, digits):
    """One valid set of outputs: every unspecified order resolved by index (stable sorts), every unowned word 0xFFFFFFFF."""
    W, n, nb, nhi, lo_bits = geom["nwin"], geom["n"], geom["nb"], geom["nhi"], geom["lo_bits"]
    over_cap, desc_cap, piece = geom["over_cap"], geom["desc_cap"], geom["piece"]
    digits = np.asarray(digits).view(np.uint32).reshape(W, n)
    o = {"entries": np.full((W, n, 2), FILL, np.uint32), "pstart": np.zeros((W, nhi + 1), np.uint32), "ghist": np.zeros((W, 256), np.uint32),
         "start": np.zeros((W, nb + 2), np.uint32), "sorted": np.full((W, n), FILL, np.uint32), "perm": np.zeros((W, nb), np.uint32),
         "over": np.zeros((W, 2), np.uint32), "over_b": np.full((W, over_cap), FILL, np.uint32),
         "over_off": np.full((W, over_cap + 1), FILL, np.uint32), "desc": np.full((W, desc_cap, 4), FILL, np.uint32)}
    for w in range(W):
        dw = digits[w].astype(np.int64)
        t = _window_truth(geom, w, dw)
        counts, total, cls = t["counts"], t["total"], t["cls"]
        idx = np.flatnonzero(dw)
        bkt = dw[idx] >> 1
        word = idx | ((dw[idx] & 1) << 31)
        by_part = np.argsort((bkt - 1) >> lo_bits, kind="stable")
        o["entries"][w, :total, 0] = word[by_part]
        o["entries"][w, :total, 1] = (bkt[by_part] - 1) & ((1 << lo_bits) - 1)
        o["pstart"][w], o["start"][w], o["ghist"][w] = t["pstart"], t["start"], t["ghist"]
        o["sorted"][w, :total] = word[np.argsort(bkt, kind="stable")]
        perm = np.argsort(-cls, kind="stable") + 1
        o["perm"][w] = perm
        n_over = int((cls > min(geom["run_limit"], 254)).sum())
        assert n_over <= over_cap
        ob = perm[:n_over]
        pieces = _pieces_of(geom, counts[ob - 1])
        off = np.concatenate(([0], np.cumsum(pieces)))
        n_pieces = int(off[-1])
        assert n_pieces <= desc_cap
        o["over"][w] = (n_over, n_pieces)
        o["over_b"][w, :n_over] = ob
        o["over_off"][w, :n_over + 1] = off
        db = np.repeat(ob, pieces)
        dp = np.arange(n_pieces) - np.repeat(off[:-1], pieces)
        first = t["start"][db] + dp * piece
        o["desc"][w, :n_pieces] = np.stack([db, dp, first, np.minimum(first + piece, t["start"][db + 1])], axis=1).reshape(-1, 4)
    return o
