"""Big-integer mirror of the batched point-opening verification's field half (csrc/kzg_points_plan.hpp, kzg_points.hpp,
kzg_points_host.inc): the four outputs of zkp_kzg_points_aggregate_dev, summed in the order the kernels sum them (a tree of 256 leaves
per workgroup, the workgroups' sums in strides of 256 and a tree again; the weights of a commitment chunk by chunk).  Every sum is
exact in Fr, so the order changes no bit; the walk is kept so that a reordering bug in the model itself would show against the plain
sums of tests/test_kzg_points_model_cpu.py.  Also the verdict of the batched equation in scalars, for an SRS of known secret."""
from kzg_cells_model import R, sort_with_chunks

THREADS = 256  # KZG_CELLS_THREADS
SIZE_MAX = (1 << 64) - 1


def tree_sum(leaves):
    """The sum of THREADS leaves, pairs left to right, level by level"""
    assert len(leaves) == THREADS
    level = list(leaves)
    while len(level) > 1:
        level = [(level[2 * k] + level[2 * k + 1]) % R for k in range(len(level) // 2)]
    return level[0]


def neg_sum(zs_unused, ys, weights):
    """-sum r_i y_i as the scalars and the finishing kernel form it"""
    count = len(weights)
    blocks = (count + THREADS - 1) // THREADS
    partial = []
    for b in range(blocks):
        leaves = [weights[i] % R * ys[i] % R if i < count else 0 for i in range(b * THREADS, (b + 1) * THREADS)]
        partial.append(tree_sum(leaves))
    leaves = [sum(partial[t::THREADS]) % R for t in range(THREADS)]
    return (-tree_sum(leaves)) % R


def commit_weights(n_commits, commit_index, weights, chunk_log=0):
    """The sums of the weights per commitment: the identity index is a copy, any other is sorted, chunked and summed twice"""
    if commit_index is None:
        assert n_commits == len(weights)
        return [w % R for w in weights]
    order, chunk_start, _, seg = sort_with_chunks(commit_index, n_commits, chunk_log, False)
    cpartial = [sum(weights[i] % R for i in order[chunk_start[q]:chunk_start[q + 1]]) % R for q in range(len(chunk_start) - 1)]
    return [sum(cpartial[seg[m]:seg[m + 1]]) % R for m in range(n_commits)]


def aggregate(n_commits, commit_index, zs, ys, weights, chunk_log=0):
    """-> (the n_commits sums of the weights, [r_i z_i], [r_i], -sum r_i y_i), every value canonical whatever the inputs' size"""
    return (commit_weights(n_commits, commit_index, weights, chunk_log), [w * z % R for w, z in zip(weights, zs)], [w % R for w in weights],
            neg_sum(zs, ys, weights))


def table_words(openings, commits, cchunks):
    """32-bit words of the packed table of one call with an index"""
    return openings + (cchunks + 1) + (commits + 1)


def accepts(s, commit_scalars, proof_scalars, n_commits, commit_index, zs, ys, weights, chunk_log=0):
    """The batched equation with integers standing in for points ([a]G is a; commitment m is f_m(s), proof i is q_i):
         sum_m cw_m C_m + sum_i (r_i z_i) W_i - (sum_i r_i y_i) G  ==  s sum_i r_i W_i
    which is  sum_i r_i (f_m(i)(s) - y_i + z_i q_i) == s sum_i r_i q_i."""
    cw, rz, r, neg = aggregate(n_commits, commit_index, zs, ys, weights, chunk_log)
    right = (sum(c * x for c, x in zip(cw, commit_scalars)) + sum(a * q for a, q in zip(rz, proof_scalars)) + neg) % R
    left = sum(a * q for a, q in zip(r, proof_scalars)) % R
    return right == left * s % R


def find_bad(s, commit_scalars, proof_scalars, n_commits, commit_index, zs, ys, weights):
    """The bisection of zkp_kzg_verify_points_find_bad -> (SIZE_MAX or the lowest failing index, pairing checks spent)"""
    index = list(range(len(weights))) if commit_index is None else list(commit_index)

    def check(lo, hi):
        sl = slice(lo, hi)
        return accepts(s, commit_scalars, proof_scalars[sl], n_commits, index[sl], zs[sl], ys[sl], weights[sl])

    checks = 1
    if check(0, len(weights)):
        return SIZE_MAX, checks
    lo, hi = 0, len(weights)
    while hi - lo > 1:
        mid = lo + (hi - lo + 1) // 2
        checks += 1
        if check(lo, mid):
            lo = mid
        else:
            hi = mid
    return lo, checks
