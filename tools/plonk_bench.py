"""PLONK prover timings on one GPU.

    plonk_bench.py [log_n] [expand|auto]       the bench.py workload (five rounds, generate_proof) at another size
    plonk_bench.py --from-gates [log_n ...]    Circuit::compile on the device against the host-column route, default sizes 16 20

--from-gates, per size, in one process, every route warmed up first, median of five (host clock around calls that end in a
device synchronise):
  a  the route bench.py uses: twelve evaluation columns ready on the host -> upload, ntt_fr_dev(batch=12, inverse), download,
     PlonkProver(...)                                                   (the host loop that builds the columns is NOT in the figure)
  b  PlonkProver.from_gates from a packed gate table
  c  the first prove() of a prover from each route
  d  set_witness + prove on a live prover against a new prover + its first prove, for a second witness
and the shader clock of the run (zkp.probe_mad_rate).  One JSON line."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "zkp-implementation_amd"))
import numpy as np
import torch
import bench, zkp_hip as zkp

R = bench.R_MOD


def chain_circuit(n, seed, start, consts=None):
    """The chain of bench.py::bench_plonk (mul / add / mul / constant, gate i's output wired to gate i+1's left input, public inputs on
    all three kinds) as gates.  consts: the constants of the constant gates of an earlier call -- the same circuit with another
    witness, whose public input at those gates is then whatever makes the gate hold (the constant is a selector, pi is not)."""
    rnd = np.random.default_rng(seed)
    rb = [int(x) for x in rnd.integers(1, 2 ** 62, n)]
    circ, used, a = zkp.PlonkCircuit(), [], start
    for i in range(n):
        kind, pi = i % 4, (7 * i + 1 if i % 8 in (0, 1, 3) else 0)
        a_pos = (2, i - 1) if i else (0, 0)
        c_pos = (0, i + 1) if i < n - 1 else (2, i)
        if kind == 3:
            k = (a - pi) % R if consts is None else consts[len(used)]
            used.append(k)
            circ.add_constant_gate(a_pos + (a,), (1, i, rb[i]), c_pos + (a,), pi=(a - k) % R, constant=k)
        elif kind == 1:
            c = (a + rb[i] - pi) % R
            circ.add_addition_gate(a_pos + (a,), (1, i, rb[i]), c_pos + (c,), pi=pi)
            a = c
        else:
            c = (a * rb[i] - pi) % R
            circ.add_multiplication_gate(a_pos + (a,), (1, i, rb[i]), c_pos + (c,), pi=pi)
            a = c
    return circ, used


def columns_of(table, log_n):
    """The twelve evaluation columns route (a) starts from, (12, n, 4) in CIRCUIT_POLYS order: the nine assignment columns are the
    table's own, the permutation columns are the chain's."""
    pos, sel, vals = table
    n = 1 << log_n
    assert pos.shape[0] == n
    w = pow(pow(7, (R - 1) >> 32, R), 1 << (32 - log_n), R)
    roots = [1] * n
    for i in range(1, n):
        roots[i] = roots[i - 1] * w % R
    s1 = [(roots[i - 1] * 3) % R if i else roots[0] for i in range(n)]
    s2 = [roots[i] * 2 % R for i in range(n)]
    s3 = [roots[i + 1] if i < n - 1 else roots[i] * 3 % R for i in range(n)]
    sig = zkp._fr_mont_rows(s1 + s2 + s3).reshape(3, n, 4)
    return np.ascontiguousarray(np.concatenate([sel.transpose(1, 0, 2), vals.transpose(1, 0, 2), sig]))


def med(fn, reps=5):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


def from_gates_bench(log_n, device):
    n = 1 << log_n
    f = lambda v: bench.fr_mont([v])[0]
    circ_a, consts = chain_circuit(n, 0xC16C, 5)
    circ_b, _ = chain_circuit(n, 0xB0B, 11, consts)
    tab_a, tab_b = circ_a.gate_table(), circ_b.gate_table()
    assert np.array_equal(tab_a[0], tab_b[0]) and np.array_equal(tab_a[1][:, :5], tab_b[1][:, :5])
    cols_a, cols_b = columns_of(tab_a, log_n), columns_of(tab_b, log_n)
    pi_a, pi_b = np.ascontiguousarray(tab_a[1][:, 5]), np.ascontiguousarray(tab_b[1][:, 5])
    srs = zkp.Srs.new_from_secret(f(0x5EC12E7), n)
    srs.bases.precompute(0)
    bl = bench.fr_mont(list(range(3, 12)))
    print(f"2^{log_n}: inputs ready", file=sys.stderr, flush=True)

    def route_a(cols):
        stack = torch.from_numpy(cols.view(np.int64)).to(device)
        zkp.ntt_fr_dev(stack.reshape(-1), log_n, batch=12, inverse=True)
        host = stack.cpu().numpy().view(np.uint64).reshape(12, n, 4)
        return zkp.PlonkProver(srs.bases, log_n, {k: host[i] for i, k in enumerate(zkp.CIRCUIT_POLYS)}, f(2), f(3))

    def route_b(tab):
        return zkp.PlonkProver.from_gates(srs.bases, *tab)

    cur = [None]

    def swap(pr):  # the provers of the timed loops: one alive at a time
        if cur[0] is not None:
            cur[0].close()
        cur[0] = pr
        return pr

    # warm-up of each route (plans, code objects) and the check that the routes agree; pb stays: it is the prover that is rebound
    pa, pb = route_a(cols_a), route_b(tab_a)
    proof, other = pa.prove(bl), pb.prove(bl)
    assert np.array_equal(proof["u"], other["u"]) and all(np.array_equal(proof["commits"][k][0], other["commits"][k][0]) for k in proof["commits"])
    pa.close()
    res = {"log_n": log_n}
    res["a_upload_ntt_download_create_ms"] = med(lambda: swap(route_a(cols_a)))
    res["b_create_from_gates_ms"] = med(lambda: swap(route_b(tab_a)))

    def first_prove(route, arg):
        ts = []
        for _ in range(5):
            pr = swap(route(arg))
            t0 = time.perf_counter()
            pr.prove(bl)
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ts), 3)

    res["c_first_prove_route_a_ms"] = first_prove(route_a, cols_a)
    res["c_first_prove_route_b_ms"] = first_prove(route_b, tab_a)
    res["later_prove_ms"] = med(lambda: pb.prove(bl))
    pb.set_witness(tab_b[2], pi_b)
    second = pb.prove(bl)
    flip, turn = [(tab_a[2], pi_a), (tab_b[2], pi_b)], [0]

    def rebind():
        vals, pi = flip[turn[0] % 2]
        turn[0] += 1
        pb.set_witness(vals, pi)
        pb.prove(bl)

    res["d_set_witness_and_prove_ms"] = med(rebind)
    res["d_new_prover_route_a_and_first_prove_ms"] = med(lambda: swap(route_a(cols_b)).prove(bl))
    res["d_new_prover_route_b_and_first_prove_ms"] = med(lambda: swap(route_b(tab_b)).prove(bl))
    assert np.array_equal(cur[0].prove(bl)["u"], second["u"]), "set_witness and a fresh prover disagree"
    swap(None)
    pb.close()
    return res


def main():
    zkp.init()
    device = torch.device("cuda", 0)
    if "--from-gates" in sys.argv:
        sizes = [int(a) for a in sys.argv[1:] if a.isdigit()] or [16, 20]
        out = {"sizes": [], "clock": {}}
        for log_n in sizes:
            out["sizes"].append(from_gates_bench(log_n, device))
        rate, mhz, ms = zkp.probe_mad_rate(20)
        out["clock"] = {"shader_mhz": round(mhz, 1), "lane_mads_per_s": rate}
        print(json.dumps(out))
        return
    print(bench.bench_plonk(zkp, torch, device, int(sys.argv[1]) if len(sys.argv) > 1 else 16,
                            expand=("auto" if sys.argv[2] == "auto" else int(sys.argv[2])) if len(sys.argv) > 2 else 0))


if __name__ == "__main__":
    main()
