"""Big-integer mirror of the batched cell verification's field half (csrc/kzg_cells_plan.hpp, kzg_cells.hpp, kzg_cells_host.inc): the
grouping of a batch by coset and by commitment with its chunks, the vector A, and the three outputs of zkp_kzg_cells_aggregate_dev.
The index arithmetic is the plan header's, written independently.  tests/test_kzg_cells_model_cpu.py ties the identity the
construction rests on to g1_coset_model.interpolant."""
from g1_coset_model import R, interpolant, root, transform  # noqa: F401


def sort_with_chunks(keys, count, chunk_log, compact):
    """Stable counting sort of the cell ids by key with every segment cut into chunks of at most 2^chunk_log cells ->
    (order, chunk_start, used keys (or None), seg: the first chunk of every (used) key, and the chunk count at the end)"""
    per = 1 << chunk_log
    members = [[] for _ in range(count)]
    for i, k in enumerate(keys):
        members[k].append(i)
    order, chunk_start, used, seg = [], [], [], []
    for k in range(count):
        if compact and not members[k]:
            continue
        used.append(k)
        seg.append(len(chunk_start))
        for off in range(0, len(members[k]), per):
            chunk_start.append(len(order) + off)
        order += members[k]
    seg.append(len(chunk_start))
    chunk_start.append(len(order))
    return order, chunk_start, (used if compact else None), seg


def table_words(cells, commits, used, chunks, cchunks):
    """32-bit words of the packed table of one call"""
    return cells + (chunks + 1) + used + (used + 1) + cells + cells + (cchunks + 1) + (commits + 1)


def max_chunks(cells, segments, chunk_log):
    return min(cells, min(segments, cells) + (cells >> chunk_log))


def vector_a(log_n, log_l, coset_index, evals, weights, chunk_log=0):
    """A[k + j r] = sum over the cells i of coset k of rho_i e_i[j], summed chunk by chunk as the two kernels do (the result does not
    depend on chunk_log; the walk does)"""
    n, l = 1 << log_n, 1 << log_l
    r = n // l
    order, chunk_start, used, seg = sort_with_chunks(coset_index, r, chunk_log, True)
    partial = [[sum(weights[i] * evals[i][j] for i in order[chunk_start[q]:chunk_start[q + 1]]) % R for j in range(l)]
               for q in range(len(chunk_start) - 1)]
    a = [0] * n
    for u, k in enumerate(used):
        for j in range(l):
            a[k + j * r] = sum(partial[q][j] for q in range(seg[u], seg[u + 1])) % R
    return a


def aggregate(log_n, log_l, n_commits, commit_index, coset_index, evals, weights, chunk_log=0):
    """-> (the l coefficients of sum rho_i I_i, the n_commits sums of the weights, the scalars rho_i c_i), c_i = (w^l)^(k_i)"""
    n, l = 1 << log_n, 1 << log_l
    r = n // l
    coeffs = transform(vector_a(log_n, log_l, coset_index, evals, weights, chunk_log), inverse=True)
    interp = [c * r % R for c in coeffs[:l]]
    order, chunk_start, _, seg = sort_with_chunks(commit_index, n_commits, chunk_log, False)
    cpartial = [sum(weights[i] for i in order[chunk_start[q]:chunk_start[q + 1]]) % R for q in range(len(chunk_start) - 1)]
    commit_weights = [sum(cpartial[seg[m]:seg[m + 1]]) % R for m in range(n_commits)]
    rho = pow(root(log_n), l, R)
    return interp, commit_weights, [w * pow(rho, k, R) % R for w, k in zip(weights, coset_index)]


def interpolant_sum(log_n, log_l, coset_index, evals, weights):
    """sum rho_i I_i by the definition: every cell's interpolant on its coset (g1_coset_model.interpolant), weighted and added"""
    n, l = 1 << log_n, 1 << log_l
    out = [0] * l
    for k, e, w in zip(coset_index, evals, weights):
        for j, c in enumerate(interpolant(e, n, l, k)):
            out[j] = (out[j] + w * c) % R
    return out
