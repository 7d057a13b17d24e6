// The plan of the sharded Fr transform (csrc/ntt_shard_plan.hpp), checked with g++ alone (tests/test_ntt_shard_plan_cpu.py):
//   A  the operations of every slot equal the ones recorded from shard_job before the plan existed (tests/golden/ntt_shard_plans.txt,
//      whose header describes the format and how it was made)
//   B  the ordering protocol over all slots' plans of a call: equal phase counts, every event recorded at most once, every wait behind
//      its record, every pair of conflicting accesses from different queues connected by queue order and record -> wait edges, and every
//      access to a slot's exchange buffers before the end of that slot's launch stream
//   C  the plan computes the transform: its operations interpreted over F_65537 against a naive DFT of the whole vector
// usage: ntt_shard_plan <golden file>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>

#include "ntt_shard_plan.hpp"

using namespace zkp;

static int g_failures = 0;
static void failure(const std::string& what) {
    if (++g_failures <= 20) std::printf("FAIL %s\n", what.c_str());
}

struct Call {
    unsigned slots, log_n, chunks;
    bool host;
    int lin, lout, inverse;
    bool coset;
    std::string name() const {
        std::ostringstream s;
        s << "case " << slots << " " << log_n << " " << chunks << " " << (host ? "host" : "dev") << " " << lin << " " << lout << " " << inverse << " " << (coset ? 1 : 0);
        return s.str();
    }
};
static bool plans_of(const Call& c, ShardGeom* G, std::vector<ShardPlan>* plans) {
    if (!shard_geometry(c.log_n, c.slots, c.chunks, G).empty()) return false;
    plans->clear();
    for (size_t g = 0; g < c.slots; g++) plans->push_back(plan_shard(*G, c.log_n, c.inverse, c.lin, c.lout, c.host, c.coset, g));
    return true;
}
static const int kPairs[5][2] = {{SH_NATURAL, SH_K1SLAB}, {SH_NATURAL, SH_NATURAL}, {SH_COLUMNS, SH_K1SLAB}, {SH_K1SLAB, SH_NATURAL}, {SH_K1SLAB, SH_COLUMNS}};

// ---------------------------------------------------------------------------------------------------- A
static std::string render(const ShardPlan& plan, uint32_t slot, unsigned log_n, int inverse) {
    std::ostringstream o;
    auto buf = [&](const ShardRef& r) {
        std::ostringstream s;
        if (r.slot != slot) s << r.slot << ":";
        s << "XAB"[r.buf] << "+" << r.off;
        return s.str();
    };
    auto remap = [](const NttRemap& r) {
        std::ostringstream s;
        if (!r.on) return std::string("[0]");
        s << "[1 " << r.lo_bits << " " << r.mid_bits << " " << r.mid_stride << " " << r.hi_stride << " " << r.batch_stride << "]";
        return s.str();
    };
    size_t first = 0;
    for (size_t p = 0; p < plan.phase_end.size(); first = plan.phase_end[p++])
        for (size_t i = first; i < plan.phase_end[p]; i++) {
            const ShardOp& op = plan.ops[i];
            if (op.label && (i == first || plan.ops[i - 1].label != op.label)) o << p << " L scope " << op.label << "\n";  // one scope per maximal run
            o << p << " " << "LC"[op.stream] << " ";
            switch (op.kind) {
            case SH_WAIT:
            case SH_RECORD:
                o << (op.kind == SH_WAIT ? "wait " : "record ");
                if (op.ev_slot != slot) o << op.ev_slot << ":";
                o << op.ev;
                break;
            case SH_PEER: o << "copy " << buf(op.dst) << " " << buf(op.src) << " " << op.dst.count; break;
            case SH_PERMUTE:
                o << "permute " << buf(op.src) << " " << buf(op.dst) << " bits";
                for (int d = 0; d < 4; d++) o << " " << op.perm.bits[d];
                o << " in";
                for (int d = 0; d < 4; d++) o << " " << op.perm.in_stride[d];
                o << " out";
                for (int d = 0; d < 4; d++) o << " " << op.perm.out_stride[d];
                break;
            case SH_AXIS0:
                o << "axis0 " << buf(op.src) << " " << buf(op.dst) << " " << op.len_log << " " << op.batch << " " << inverse << " " << op.tw_log_n << " " << op.tw_first;
                break;
            case SH_ROWS:
                o << "rows " << buf(op.src) << " " << buf(op.dst) << " " << op.len_log << " " << op.batch << " " << inverse << " in" << remap(op.in_remap) << " out"
                  << remap(op.out_remap) << " " << op.tw_log_n << " " << op.tw_first;
                break;
            case SH_COSET: o << "coset " << buf(op.dst) << " " << op.dst.count << " " << op.tw_first << " " << log_n << " " << inverse; break;
            }
            o << "\n";
            if (op.label && (i + 1 == plan.phase_end[p] || plan.ops[i + 1].label != op.label)) o << p << " L end\n";
        }
    return o.str();
}
static uint64_t fnv1a(const std::string& s) {
    uint64_t h = 1469598103934665603ull;
    for (unsigned char c : s) h = (h ^ c) * 1099511628211ull;
    return h;
}
static void first_difference(const std::string& where, const std::string& want, const std::string& got) {
    std::istringstream a(want), b(got);
    std::string la, lb;
    for (int n = 1;; n++) {
        const bool ha = (bool)std::getline(a, la), hb = (bool)std::getline(b, lb);
        if (!ha && !hb) return;
        if (!ha || !hb || la != lb) {
            std::ostringstream s;
            s << where << " line " << n << ": recorded '" << (ha ? la : "<none>") << "', plan '" << (hb ? lb : "<none>") << "'";
            return failure(s.str());
        }
    }
}

static void check_protocol(const Call& c, const ShardGeom& G, const std::vector<ShardPlan>& plans);

static int check_recorded(const char* path, int* protocol_calls) {
    std::ifstream f(path);
    if (!f) return failure(std::string("cannot open ") + path), 0;
    std::string line;
    int cases = 0, declared = -1;
    Call c{};
    ShardGeom G;
    std::vector<ShardPlan> plans;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream s(line);
        std::string word, form;
        s >> word;
        if (word == "end") {
            std::string rest;
            s >> rest;
            declared = std::atoi(rest.c_str() + std::strlen("cases="));
        } else if (word == "case") {
            int coset = 0;
            s >> c.slots >> c.log_n >> c.chunks >> form >> c.lin >> c.lout >> c.inverse >> coset;
            c.host = form == "host";
            c.coset = coset != 0;
            cases++;
            if (!plans_of(c, &G, &plans)) failure(c.name() + ": geometry refused");
            else check_protocol(c, G, plans), ++*protocol_calls;
        } else if (word == "slot") {
            uint32_t slot = 0;
            size_t lines = 0;
            std::string hash, want;
            s >> slot >> lines >> hash;
            if (slot >= plans.size()) { failure(c.name() + ": slot out of range"); continue; }
            const std::string got = render(plans[slot], slot, c.log_n, c.inverse);
            const size_t got_lines = (size_t)std::count(got.begin(), got.end(), '\n');
            const std::string where = c.name() + " slot " + std::to_string(slot);
            if (hash.empty()) {
                for (size_t i = 0; i < lines && std::getline(f, line); i++) want += line + "\n";
                if (want != got) first_difference(where, want, got);
            } else {
                char h[32];
                std::snprintf(h, sizeof h, "%016llx", (unsigned long long)fnv1a(got));
                if (got_lines != lines) failure(where + ": " + std::to_string(got_lines) + " lines, recorded " + std::to_string(lines));
                else if (hash != h) failure(where + ": hash " + h + ", recorded " + hash);
            }
        } else {
            failure("golden file: stray line '" + line + "'");
        }
    }
    if (declared != cases) failure("golden file: " + std::to_string(cases) + " cases, its last line declares " + std::to_string(declared));
    return cases;
}

// ---------------------------------------------------------------------------------------------------- B
// A violation of rule 4 or 5 that the recorded protocol itself has would be listed here, as "<case name>|<first op>|<second op>",
// and reported at the top of the change that found it.  None is known.
static const char* const kKnownViolations[] = {nullptr};
static bool known_violation(const std::string& v) {
    for (const char* const* k = kKnownViolations; *k; k++)
        if (v == *k) return true;
    return false;
}

struct Access {
    uint64_t off, count;
    bool write;
    uint32_t queue, pos;  // queue = 2 * slot + stream, pos = 1-based index of the operation in its queue
    uint32_t slot, op;    // who: for the message
};
static void check_protocol(const Call& c, const ShardGeom& G, const std::vector<ShardPlan>& plans) {
    const size_t W = plans.size(), Q = 2 * W, nev = shard_event_count(G);
    const std::string name = c.name();
    for (size_t g = 1; g < W; g++)  // rule 1
        if (plans[g].phase_end.size() != plans[0].phase_end.size()) return failure(name + ": slot " + std::to_string(g) + " has another number of phases than slot 0");
    // clock[q][r]: how many operations of queue r happen before the next operation of queue q.  The operations are visited phase by
    // phase, slot by slot: a topological order of queue order and record -> wait edges once rule 3 holds.
    std::vector<std::vector<uint32_t>> clock(Q, std::vector<uint32_t>(Q, 0));
    std::vector<std::vector<uint32_t>> recorded(W * nev);  // the clock of the recording queue at the record; empty: not recorded yet
    std::vector<size_t> recorded_phase(W * nev, 0);
    std::vector<uint32_t> issued(Q, 0);
    std::vector<std::vector<Access>> touched(W * 3);
    auto describe = [&](uint32_t slot, uint32_t op) {
        std::istringstream all(render(plans[slot], slot, c.log_n, c.inverse));
        std::string l, hit;
        // (the rendering has one line per operation plus the scope lines: count the operation lines)
        for (uint32_t k = 0; std::getline(all, l);)
            if (l.find(" scope ") == std::string::npos && l.find(" end") == std::string::npos && k++ == op) hit = l;
        return "slot " + std::to_string(slot) + " '" + hit + "'";
    };
    for (size_t p = 0; p < plans[0].phase_end.size(); p++)
        for (uint32_t g = 0; g < W; g++) {
            const ShardPlan& plan = plans[g];
            for (size_t i = p ? plan.phase_end[p - 1] : 0; i < plan.phase_end[p]; i++) {
                const ShardOp& op = plan.ops[i];
                const uint32_t q = 2 * g + op.stream;
                const uint32_t pos = ++issued[q];
                std::vector<uint32_t>& now = clock[q];
                if (op.kind == SH_RECORD) {
                    if (op.ev_slot != g || op.ev >= nev) return failure(name + ": " + describe(g, (uint32_t)i) + " records an event that is not this slot's");
                    std::vector<uint32_t>& r = recorded[g * nev + op.ev];
                    if (!r.empty()) return failure(name + ": " + describe(g, (uint32_t)i) + " records an event twice");  // rule 2
                    r = now;
                    r[q] = pos;
                    recorded_phase[g * nev + op.ev] = p;
                } else if (op.kind == SH_WAIT) {
                    // rule 3: recorded in an earlier phase, or by this slot earlier in this phase -- which is what this visiting order has seen
                    if (op.ev_slot >= W || op.ev >= nev || recorded[op.ev_slot * nev + op.ev].empty())
                        return failure(name + ": " + describe(g, (uint32_t)i) + " waits for an event that has not been recorded");
                    if (op.ev_slot != g && recorded_phase[op.ev_slot * nev + op.ev] == p)  // (a lower slot's record of THIS phase has been visited too)
                        return failure(name + ": " + describe(g, (uint32_t)i) + " waits for an event that another slot records in the same phase");
                    const std::vector<uint32_t>& r = recorded[op.ev_slot * nev + op.ev];
                    for (size_t k = 0; k < Q; k++) now[k] = std::max(now[k], r[k]);
                } else {
                    const ShardRef* refs[2] = {op.kind == SH_COSET ? nullptr : &op.src, &op.dst};
                    for (int side = 0; side < 2; side++) {
                        if (!refs[side]) continue;
                        const ShardRef& r = *refs[side];
                        if (r.slot >= W || r.buf > SH_B || r.off + r.count > G.slab) return failure(name + ": " + describe(g, (uint32_t)i) + " leaves its buffer");
                        const Access a{r.off, r.count, side == 1 || op.kind == SH_COSET, q, pos, g, (uint32_t)i};
                        std::vector<Access>& list = touched[r.slot * 3 + r.buf];
                        for (const Access& b : list)  // rule 4
                            if (b.queue != q && (a.write || b.write) && a.off < b.off + b.count && b.off < a.off + a.count && now[b.queue] < b.pos) {
                                const std::string v = name + "|" + describe(b.slot, b.op) + "|" + describe(g, (uint32_t)i);
                                if (!known_violation(v)) failure("unordered accesses: " + v);
                            }
                        list.push_back(a);
                    }
                }
                now[q] = pos;
            }
        }
    for (uint32_t g = 0; g < W; g++)  // rule 5
        for (int b = SH_A; b <= SH_B; b++)
            for (const Access& a : touched[g * 3 + (size_t)b])
                if (clock[2 * g + SH_LAUNCH][a.queue] < a.pos) {
                    const std::string v = name + "|" + describe(a.slot, a.op) + "|end of slot " + std::to_string(g) + "'s launch stream";
                    if (!known_violation(v)) failure("an exchange buffer is still in use at the end of the call: " + v);
                }
}

// ---------------------------------------------------------------------------------------------------- C
static const uint32_t P = 65537;  // 2-adicity 16, 3 generates the multiplicative group
static uint32_t mul(uint32_t a, uint32_t b) { return (uint32_t)((uint64_t)a * b % P); }
static uint32_t power(uint32_t a, uint64_t e) {
    uint32_t r = 1;
    for (; e; e >>= 1, a = mul(a, a))
        if (e & 1) r = mul(r, a);
    return r;
}
static uint32_t root(unsigned log_n, int inverse) {  // omega_{2^log_n}^(+-1)
    const uint32_t w = power(3, 65536u >> log_n);
    return inverse ? power(w, P - 2) : w;
}
// out[k] = c * sum_j in[j] w^(jk)
static void naive_dft(const std::vector<uint32_t>& in, std::vector<uint32_t>& out, uint32_t w, uint32_t c) {
    const size_t n = in.size();
    std::vector<uint32_t> pw(n);
    pw[0] = 1;
    for (size_t i = 1; i < n; i++) pw[i] = mul(pw[i - 1], w);
    out.assign(n, 0);
    for (size_t k = 0; k < n; k++) {
        uint64_t acc = 0;
        for (size_t j = 0; j < n; j++) acc += (uint64_t)in[j] * pw[(j * k) & (n - 1)] % P;
        out[k] = mul((uint32_t)(acc % P), c);
    }
}
// where element i of the whole vector lives: (slot, offset in the slab) -- the layouts of ntt_sharded.inc's header comment
static std::pair<size_t, size_t> place(const ShardGeom& G, int layout, uint64_t i) {
    if (layout == SH_NATURAL) return {i / G.slab, i % G.slab};
    if (layout == SH_K1SLAB) {  // slab g [j][k2] = X[(g r1 + j) + N1 k2]
        const uint64_t k1 = i % G.n1, k2 = i / G.n1;
        return {k1 / G.r1, (k1 % G.r1) * G.n2 + k2};
    }
    // COLUMNS: slab g [q][n1][c] = x[n1 N2 + g r2 + q cw + c]
    const uint64_t n1 = i / G.n2, n2 = i % G.n2, g = n2 / G.r2, q = (n2 % G.r2) / G.cw, cc = n2 % G.cw;
    return {g, (q * G.n1 + n1) * G.cw + cc};
}
struct Reference {
    std::vector<uint32_t> x, y[2];  // the input and its forward / inverse transform
};
static const Reference& reference(unsigned log_n) {
    static std::map<unsigned, Reference> cache;
    auto it = cache.find(log_n);
    if (it != cache.end()) return it->second;
    Reference& r = cache[log_n];
    const size_t n = (size_t)1 << log_n;
    r.x.resize(n);
    uint64_t s = 0x9E3779B97F4A7C15ull + log_n;
    for (size_t i = 0; i < n; i++) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        r.x[i] = (uint32_t)((s >> 33) % P);
    }
    for (int inv = 0; inv < 2; inv++) naive_dft(r.x, r.y[inv], root(log_n, inv), inv ? power((uint32_t)(n % P), P - 2) : 1);
    return r;
}
static void check_transform(const Call& c) {
    ShardGeom G;
    std::vector<ShardPlan> plans;
    const std::string name = c.name();
    if (!plans_of(c, &G, &plans)) return failure(name + ": geometry refused");
    const Reference& ref = reference(c.log_n);
    const size_t W = c.slots, n = (size_t)1 << c.log_n;
    std::vector<std::vector<uint32_t>> mem(W * 3, std::vector<uint32_t>(G.slab, 0xdead));  // (nothing may depend on what A and B held)
    for (size_t i = 0; i < n; i++) {
        const auto at = place(G, c.lin, i);
        mem[at.first * 3 + SH_SLAB][at.second] = ref.x[i];
    }
    auto at = [&](const ShardRef& r) -> uint32_t* { return mem[r.slot * 3 + r.buf].data() + r.off; };
    // phase by phase, slot by slot: one of the orders that check B allows
    for (size_t p = 0; p < plans[0].phase_end.size(); p++)
        for (size_t g = 0; g < W; g++)
            for (size_t i = p ? plans[g].phase_end[p - 1] : 0; i < plans[g].phase_end[p]; i++) {
                const ShardOp& op = plans[g].ops[i];
                if (op.kind == SH_WAIT || op.kind == SH_RECORD) continue;
                if (op.kind == SH_COSET) return failure(name + ": a coset scale in a device-form plan");
                const uint32_t* src = at(op.src);
                uint32_t* dst = at(op.dst);
                const size_t len = (size_t)1 << op.len_log;
                const uint32_t w = root(op.len_log, c.inverse), scale = c.inverse ? power((uint32_t)(len % P), P - 2) : 1;
                std::vector<uint32_t> in(len), out;
                if (op.kind == SH_PEER) {
                    std::memmove(dst, src, sizeof(uint32_t) * op.dst.count);
                } else if (op.kind == SH_PERMUTE) {
                    uint64_t total = 1;
                    for (int d = 0; d < 4; d++) total <<= op.perm.bits[d];
                    for (uint64_t e = 0; e < total; e++) {
                        const PermuteIndex x = permute_index(op.perm, e);
                        dst[x.dst] = src[x.src];
                    }
                } else if (op.kind == SH_AXIS0) {  // matrix [len][batch], natural order in and out, output (k, b) times omega_N^(+-(col0 + b) k)
                    for (uint64_t b = 0; b < op.batch; b++) {
                        for (size_t j = 0; j < len; j++) in[j] = src[j * op.batch + b];
                        naive_dft(in, out, w, scale);
                        for (size_t k = 0; k < len; k++) dst[k * op.batch + b] = op.tw_log_n ? mul(out[k], power(root(op.tw_log_n, c.inverse), (op.tw_first + b) * k)) : out[k];
                    }
                } else {  // SH_ROWS: element e of transform b at ntt_phys(remap, b, len, e), output k times omega_N^(+-(row0 + b) k)
                    std::vector<std::vector<uint32_t>> outs(op.batch);
                    for (uint64_t b = 0; b < op.batch; b++) {
                        for (size_t j = 0; j < len; j++) in[j] = src[ntt_phys(op.in_remap, b, len, j)];
                        naive_dft(in, outs[b], w, scale);
                    }
                    for (uint64_t b = 0; b < op.batch; b++)
                        for (size_t k = 0; k < len; k++)
                            dst[ntt_phys(op.out_remap, b, len, k)] = op.tw_log_n ? mul(outs[b][k], power(root(op.tw_log_n, c.inverse), (op.tw_first + b) * k)) : outs[b][k];
                }
            }
    size_t wrong = 0;
    for (size_t i = 0; i < n; i++) {
        const auto o = place(G, c.lout, i);
        if (mem[o.first * 3 + SH_SLAB][o.second] != ref.y[c.inverse][i]) wrong++;
    }
    if (wrong) failure(name + ": " + std::to_string(wrong) + " of " + std::to_string(n) + " elements differ from the naive DFT");
}

static unsigned smallest_log_n(unsigned slots) {
    ShardGeom G;
    unsigned log_n = 0;
    while (!shard_geometry(log_n, slots, 0, &G).empty()) log_n++;
    return log_n;
}

int main(int argc, char** argv) {
    if (argc < 2) return std::printf("usage: ntt_shard_plan <golden file>\n"), 2;
    int protocol_calls = 0, transforms = 0;
    const int cases = check_recorded(argv[1], &protocol_calls);
    // B beyond the recorded cases: the slot counts that no GPU test reaches
    for (unsigned slots : {16u, 32u, 64u})
        for (unsigned log_n : {smallest_log_n(slots), 26u})
            for (unsigned chunks : {0u, 1u, 2u, 8u})
                for (int form = 0; form < 7; form++)
                    for (int inv = 0; inv < 2; inv++) {
                        const bool host = form >= 5;
                        if (host && chunks) continue;
                        const Call c{slots, log_n, chunks, host, host ? SH_NATURAL : kPairs[form][0], host ? SH_NATURAL : kPairs[form][1], inv, form == 6};
                        ShardGeom G;
                        std::vector<ShardPlan> plans;
                        if (!plans_of(c, &G, &plans)) continue;  // this chunk count is not valid here
                        check_protocol(c, G, plans);
                        protocol_calls++;
                    }
    // C
    struct Size { unsigned slots, log_n, chunks; };
    std::vector<Size> sizes;
    for (unsigned slots : {1u, 2u, 4u, 8u, 16u})
        for (unsigned extra = 0; extra < (slots == 16 ? 1u : 2u); extra++)
            for (unsigned chunks : {1u, 0u}) sizes.push_back(Size{slots, smallest_log_n(slots) + extra, chunks});
    sizes.push_back(Size{2, 12, 8});
    for (const Size& s : sizes)
        for (const auto& pr : kPairs)
            for (int inv = 0; inv < 2; inv++) {
                check_transform(Call{s.slots, s.log_n, s.chunks, false, pr[0], pr[1], inv, false});
                transforms++;
            }
    std::printf("ntt shard plan: %d recorded cases, %d calls through the protocol rules, %d transforms interpreted, %d failures\n", cases, protocol_calls, transforms,
                g_failures);
    return g_failures ? 1 : 0;
}
