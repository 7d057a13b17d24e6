// fri.hpp -- the device side of the FRI commitment path (fri/src is generic over F: PrimeField).  First the Goldilocks
// hashing: SHA-256 Merkle trees over the decimal strings of the evaluations (fri/src/hasher.rs:14-36,
// fri/src/merkle_tree.rs:42-63).  Then what both fields share, as templates over a field policy F (FriGl below, FriFr in
// fri_fr.hpp): the transcript step, the fold, the one-workgroup tail of small layers and the gather of query decommitments
// (fri/src/prover.rs:34-134, merkle_tree.rs:84-107).
//
// hash(x)       = SHA-256(Display(x))                 -> F::from_le_bytes_mod_order(digest)
// hash_slice(v) = SHA-256(Display(v0) || Display(v1))   (no separator)
// Display = decimal of the canonical integer, leading zeros trimmed: at most 20 digits per element, so a leaf (<= 20
// bytes) and a pair (<= 40 bytes) always fit ONE 64-byte SHA-256 block.  One lane per hash; the variable-length message is
// assembled in a 68-byte LDS slot per lane (byte stores at data-dependent offsets stay out of scratch memory), then the
// 64 rounds run in registers (~2500 VALU instructions per hash, no memory traffic: the kernel is ALU-bound).
// A workgroup of 256 lanes covers 1024 adjacent nodes and climbs up to 10 levels above them (2 inside each lane, 8 through
// LDS), so a tree of 2^21 leaves takes three launches instead of twenty-two.
#pragma once
#include "ff.hpp"

namespace zkp {

constexpr int MERKLE_BLOCK = 256;      // lanes per workgroup
constexpr int MERKLE_MAX_LEVELS = 11;  // leaf hashes + 2 in-lane levels + 8 LDS levels
constexpr int SHA_SLOT = 68;           // bytes of LDS per lane (64 + 4: consecutive slots start on different banks)

__device__ __constant__ const uint32_t SHA256_K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
    0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
    0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
    0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
    0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

ZKP_DEV uint32_t rotr32(uint32_t x, int n) { return __builtin_amdgcn_alignbit(x, x, n); }
// gfx950's three-input boolean: one instruction for the xor of the three rotations, for Ch and for Maj
ZKP_DEV uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
ZKP_DEV uint32_t sha_ch(uint32_t e, uint32_t f, uint32_t g) { return __builtin_amdgcn_bitop3_b32(e, f, g, 0xca); }   // e ? f : g
ZKP_DEV uint32_t sha_maj(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xe8); }

// st = compress(st, block w[0..15] of big-endian words)
ZKP_DEV void sha256_compress(uint32_t st[8], uint32_t w[16]) {
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
    for (int i = 0; i < 64; i++) {
        if (i >= 16) {
            const uint32_t w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
            const uint32_t s0 = xor3(rotr32(w15, 7), rotr32(w15, 18), w15 >> 3);
            const uint32_t s1 = xor3(rotr32(w2, 17), rotr32(w2, 19), w2 >> 10);
            w[i & 15] = w[i & 15] + s0 + w[(i - 7) & 15] + s1;
        }
        const uint32_t t1 = h + xor3(rotr32(e, 6), rotr32(e, 11), rotr32(e, 25)) + sha_ch(e, f, g) + SHA256_K[i] + w[i & 15];
        const uint32_t t2 = xor3(rotr32(a, 2), rotr32(a, 13), rotr32(a, 22)) + sha_maj(a, b, c);
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// decimal digits of x, most significant first, leading zeros trimmed (zero -> nothing, or "0" when zero_as_0);
// returns the number of bytes written
ZKP_DEV int gl_write_decimal(uint64_t x, uint8_t* dst, bool zero_as_0) {
    const uint32_t hi = (uint32_t)(x / 10000000000ull);  // < 1.85e9
    const uint64_t lo = x - (uint64_t)hi * 10000000000ull;  // < 1e10
    uint32_t part[4] = {hi / 100000u, hi % 100000u, (uint32_t)(lo / 100000u), (uint32_t)(lo % 100000u)};
    uint8_t d[20];
#pragma unroll
    for (int p = 0; p < 4; p++) {
        uint32_t v = part[p];
#pragma unroll
        for (int k = 4; k >= 0; k--) {
            d[5 * p + k] = (uint8_t)(v % 10u);
            v /= 10u;
        }
    }
    int nz = 0;
    bool lead = true;
#pragma unroll
    for (int i = 0; i < 20; i++) {
        lead = lead && d[i] == 0;
        nz += lead ? 1 : 0;
    }
    if (nz == 20 && zero_as_0) nz = 19;
#pragma unroll
    for (int i = 0; i < 20; i++)
        if (i >= nz) dst[i - nz] = (uint8_t)('0' + d[i]);
    return 20 - nz;
}

// F::from_le_bytes_mod_order of the digest: sum of the four little-endian 64-bit limbs l_k 2^(64k), with
// 2^64 = EPS, 2^128 = -2^32, 2^192 = 1 (mod p).  Returns the canonical value.
ZKP_DEV Gl sha_digest_to_gl(const uint32_t dg[8]) {
    uint64_t l[4];
#pragma unroll
    for (int k = 0; k < 4; k++)
        l[k] = (uint64_t)__builtin_bswap32(dg[2 * k]) | (uint64_t)__builtin_bswap32(dg[2 * k + 1]) << 32;
    Gl acc{l[0] >= Gl::MOD ? l[0] - Gl::MOD : l[0]};
    acc = acc + Gl{l[1]} * Gl{Gl::EPS};            // operator* accepts any 64-bit operand
    acc = acc - Gl{l[2]} * Gl{1ull << 32};
    acc = acc + Gl{l[3] >= Gl::MOD ? l[3] - Gl::MOD : l[3]};
    return acc;
}

// hash of one or two canonical elements; `slot` is this lane's LDS scratch
ZKP_DEV Gl gl_hash_elems(uint64_t a, uint64_t b, bool two, uint8_t* slot, bool zero_as_0) {
    uint32_t* sw = reinterpret_cast<uint32_t*>(slot);
#pragma unroll
    for (int i = 0; i < 16; i++) sw[i] = 0;
    int len = gl_write_decimal(a, slot, zero_as_0);
    if (two) len += gl_write_decimal(b, slot + len, zero_as_0);
    slot[len] = 0x80;
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = __builtin_bswap32(sw[i]);
    w[15] = (uint32_t)len * 8;  // message bits (< 2^32), big-endian length field
    uint32_t dg[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    sha256_compress(dg, w);
    return sha_digest_to_gl(dg);
}

ZKP_DEV uint64_t gl_canonical_from_mont(uint64_t m) { return (Gl{m} * Gl{0xfffffffe00000001ull}).v; }  // * 2^-64
ZKP_DEV uint64_t gl_mont_from_canonical(uint64_t c) { return (Gl{c} * Gl{Gl::EPS}).v; }               // * 2^64

struct MerkleLaunch {
    const uint64_t* in;   // leaves (leaf_mode) or the nodes of the level below out[0]
    uint64_t n_in;
    int leaf_mode;        // 1: out[0][i] = hash(in[i]); 0: `in` is a node level, out[0] is the level above it
    int levels;           // levels written by this launch (<= 1 + ipl_log + 8 in leaf mode, one fewer otherwise)
    int ipl_log;          // log2 of the inputs per lane: 2 for large levels (throughput), 0 for small ones (shortest chain)
    int zero_as_0;
    uint64_t* out[MERKLE_MAX_LEVELS];
};

// Workgroup b owns input nodes [span b, span (b + 1)), span = 256 << ipl_log.  Every lane first walks its own subtree of
// 2^ipl_log inputs serially (for 4 inputs: 4 leaf hashes, 2 parents, 1 grandparent: full lanes, no barrier), then the 256
// lane results climb up to 8 more levels through LDS.  Level s above the input starts at (span b) >> s.  A tree is a chain of
// depth + 1 dependent hashes (~5 us each): large levels take 4 inputs per lane, small ones 1 so that the chain stays short.
__global__ __launch_bounds__(MERKLE_BLOCK) void merkle_levels_kernel(MerkleLaunch p) {
    __shared__ uint64_t cur[MERKLE_BLOCK];
    __shared__ uint32_t slots32[MERKLE_BLOCK * SHA_SLOT / 4];
    const int tid = threadIdx.x;
    const uint32_t ipl = 1u << p.ipl_log, span_max = (uint32_t)MERKLE_BLOCK << p.ipl_log;
    const uint64_t base = (uint64_t)blockIdx.x * span_max;
    uint8_t* slot = reinterpret_cast<uint8_t*>(slots32) + tid * SHA_SLOT;
    const bool z0 = p.zero_as_0 != 0;
    const uint32_t span = (uint32_t)(p.n_in - base < span_max ? p.n_in - base : span_max);
    const uint32_t mine = span > ipl * tid ? (span - ipl * tid < ipl ? span - ipl * tid : ipl) : 0u;  // valid inputs of this lane
    int lvl = 0;  // next entry of p.out
    uint64_t v[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < mine; k++) v[k] = gl_canonical_from_mont(p.in[base + ipl * tid + k]);
    if (p.leaf_mode) {
        for (uint32_t k = 0; k < mine; k++) {
            v[k] = gl_hash_elems(v[k], 0, false, slot, z0).v;
            p.out[0][base + ipl * tid + k] = gl_mont_from_canonical(v[k]);
        }
        lvl = 1;
    }
    uint32_t have = mine;  // nodes this lane holds at the current level
    int s = 1;             // level distance from the input level
    for (; s <= p.ipl_log && lvl < p.levels; s++, lvl++) {
        const uint32_t next = (have + 1) / 2;
        for (uint32_t j = 0; j < next; j++) {
            const bool two = 2 * j + 1 < have;
            v[j] = gl_hash_elems(v[2 * j], two ? v[2 * j + 1] : 0, two, slot, z0).v;
            p.out[lvl][(base >> s) + (uint64_t)tid * (ipl >> s) + j] = gl_mont_from_canonical(v[j]);
        }
        have = next;
    }
    if (lvl >= p.levels) return;  // uniform: depends on the launch parameters only
    uint32_t count = (span + ipl - 1) / ipl;  // lane results in this workgroup
    if (tid < (int)count) cur[tid] = v[0];
    __syncthreads();
    for (; lvl < p.levels; s++, lvl++) {
        const uint32_t next = (count + 1) / 2;
        uint64_t h = 0;
        if (tid < (int)next) {
            const bool two = 2 * tid + 1 < (int)count;
            h = gl_hash_elems(cur[2 * tid], two ? cur[2 * tid + 1] : 0, two, slot, z0).v;
            p.out[lvl][(base >> s) + tid] = gl_mont_from_canonical(h);
        }
        __syncthreads();
        if (tid < (int)next) cur[tid] = h;
        __syncthreads();
        count = next;
    }
}

struct FriTranscriptState {
    uint32_t data[8];  // digest so far, big-endian words
    uint64_t index;    // messages digested
};

// SHA-256 over the `len` message bytes already in `slot` (zero beyond them, room for the padding), one compression per block
ZKP_DEV void sha256_slot(uint8_t* slot, int len, uint32_t st[8]) {
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(slot);
    slot[len] = 0x80;
    const int blocks = (len + 9 + 63) >> 6;
    st[0] = 0x6a09e667; st[1] = 0xbb67ae85; st[2] = 0x3c6ef372; st[3] = 0xa54ff53a;
    st[4] = 0x510e527f; st[5] = 0x9b05688c; st[6] = 0x1f83d9ab; st[7] = 0x5be0cd19;
    for (int b = 0; b < blocks; b++) {
        uint32_t w[16];
#pragma unroll
        for (int i = 0; i < 16; i++) w[i] = __builtin_bswap32(sw[16 * b + i]);
        if (b == blocks - 1) w[15] = (uint32_t)len * 8;  // message bits (< 2^32), big-endian length field
        sha256_compress(st, w);
    }
}

ZKP_DEV uint32_t rotl32(uint32_t x, int n) { return __builtin_amdgcn_alignbit(x, x, 32 - n); }
#define ZKP_CHACHA_QR(a, b, c, d)                                                                                         \
    a += b; d ^= a; d = rotl32(d, 16); c += d; b ^= c; b = rotl32(b, 12); a += b; d ^= a; d = rotl32(d, 8); c += d; b ^= c; \
    b = rotl32(b, 7);
// rand_chacha's ChaCha12 block `counter` under `key` (stream id 0): the 16 output words
ZKP_DEV void chacha12_block(const uint32_t key[8], uint64_t counter, uint32_t out[16]) {
    const uint32_t in[16] = {0x61707865, 0x3320646e, 0x79622d32, 0x6b206574, key[0], key[1], key[2], key[3], key[4], key[5], key[6],
                             key[7], (uint32_t)counter, (uint32_t)(counter >> 32), 0, 0};
    uint32_t x[16];
    for (int i = 0; i < 16; i++) x[i] = in[i];
    for (int r = 0; r < 6; r++) {
        ZKP_CHACHA_QR(x[0], x[4], x[8], x[12]) ZKP_CHACHA_QR(x[1], x[5], x[9], x[13])
        ZKP_CHACHA_QR(x[2], x[6], x[10], x[14]) ZKP_CHACHA_QR(x[3], x[7], x[11], x[15])
        ZKP_CHACHA_QR(x[0], x[5], x[10], x[15]) ZKP_CHACHA_QR(x[1], x[6], x[11], x[12])
        ZKP_CHACHA_QR(x[2], x[7], x[8], x[13]) ZKP_CHACHA_QR(x[3], x[4], x[9], x[14])
    }
    for (int i = 0; i < 16; i++) out[i] = x[i] + in[i];
}
#undef ZKP_CHACHA_QR

// The Goldilocks side of the field parameter F of everything below (FriFr in fri_fr.hpp is the other).  F::E is the element
// as the kernels hold it and as it lies in memory (a Montgomery residue).  A SCALAR -- coset, root of unity, stride, folding
// challenge -- reaches a kernel in the form that E's operator* wants for its second factor so that the product stays in memory
// form: the canonical value here (plain modular product), the Montgomery residue over Fr.
struct FriGl {
    typedef Gl E;
    static constexpr int SLOT = SHA_SLOT;     // bytes of LDS per hashing lane
    static constexpr int TAIL_LOG = 11;       // the tail kernel holds layers of up to 2^TAIL_LOG points ...
    static constexpr int TAIL_THREADS = 1024; // ... in one workgroup of this many threads: one parent / folded coefficient each
    static constexpr int PREP_CHUNK = 8;      // fri_fold_prep_kernel<FriGl>: elements per thread,
    static constexpr int PREP_THREADS = 256;  // threads per workgroup,
    static constexpr int PREP_STEP = 1;       // and the distance between two elements of one thread (consecutive)
    static ZKP_DEV E canonical(const E& mont) { return Gl{gl_canonical_from_mont(mont.v)}; }
    static ZKP_DEV E mont(const E& canon) { return Gl{gl_mont_from_canonical(canon.v)}; }
    static ZKP_DEV int write_decimal(const E& canon, uint8_t* dst, bool z0) { return gl_write_decimal(canon.v, dst, z0); }
    // hash (one element) or hash_slice (two) of canonical values, canonical result; b is ignored unless `two`
    static ZKP_DEV E hash_elems(const E& a, const E& b, bool two, uint8_t* slot, bool z0) { return gl_hash_elems(a.v, b.v, two, slot, z0); }
    // F::rand from one ChaCha block: next_u64 is two consecutive words, rejected while >= p; the accepted integer IS the
    // Montgomery residue of the challenge.  false: all eight candidates of the block were rejected
    static ZKP_DEV bool challenge_from_block(const uint32_t x[16], E& scalar) {
        for (int i = 0; i < 16; i += 2) {
            const uint64_t v = (uint64_t)x[i] | (uint64_t)x[i + 1] << 32;
            if (v < Gl::MOD) {
                scalar = Gl{gl_canonical_from_mont(v)};
                return true;
            }
        }
        return false;
    }
};

// One lane: Transcript::digest(root) (transcript.rs:64-72) followed by generate_a_challenge (86-89); returns the challenge
// as a scalar and updates data / index.  `buf` = 128 bytes of LDS scratch: 40 + Display(root) + 9 bytes of padding fit two blocks.
template <class F>
ZKP_DEV typename F::E fri_transcript_challenge(uint32_t data[8], uint64_t& index, const typename F::E& root_canonical, uint8_t* buf,
                                               bool z0) {
    uint32_t* bw = reinterpret_cast<uint32_t*>(buf);
    for (int i = 0; i < 32; i++) bw[i] = 0;
    for (int i = 0; i < 8; i++) bw[i] = __builtin_bswap32(data[i]);        // previous digest, byte order of the digest
    for (int i = 0; i < 8; i++) buf[32 + i] = (uint8_t)(index >> (8 * i));  // index.to_le_bytes()
    const int len = 40 + F::write_decimal(root_canonical, buf + 40, z0);
    uint32_t st[8];
    sha256_slot(buf, len, st);
    for (int i = 0; i < 8; i++) data[i] = st[i];
    index++;
    // seed = first 8 digest bytes, little-endian (transcript.rs:80-83); rand_core seed_from_u64: PCG32
    uint64_t state = (uint64_t)__builtin_bswap32(st[0]) | (uint64_t)__builtin_bswap32(st[1]) << 32;
    uint32_t key[8];
    for (int i = 0; i < 8; i++) {
        state = state * 6364136223846793005ull + 11634580027462260723ull;
        const uint32_t xs = (uint32_t)(((state >> 18) ^ state) >> 27), rot = (uint32_t)(state >> 59);
        key[i] = (xs >> rot) | (xs << ((32 - rot) & 31));
    }
    for (uint64_t counter = 0;; counter++) {
        uint32_t x[16];
        chacha12_block(key, counter, x);
        typename F::E r;
        if (F::challenge_from_block(x, r)) return r;
    }
}

// One layer's transcript step for the large layers (one lane): digest the root, draw the folding challenge into *r_out (a
// scalar), copy the root next to the other small outputs (one D2H for all of them).  The host never waits for a root before it
// enqueues the next layer.
template <class F>
__global__ void fri_transcript_kernel(FriTranscriptState* state, const typename F::E* root_mont, typename F::E* r_out,
                                      typename F::E* root_out, int zero_as_0) {
    typedef typename F::E E;
    __shared__ uint32_t buf[32];
    const E root = E::load(root_mont);
    root.store(root_out);
    uint32_t data[8];
    for (int i = 0; i < 8; i++) data[i] = state->data[i];
    uint64_t index = state->index;
    const E r = fri_transcript_challenge<F>(data, index, F::canonical(root), reinterpret_cast<uint8_t*>(buf), zero_as_0 != 0);
    r.store(r_out);
    for (int i = 0; i < 8; i++) state->data[i] = data[i];
    state->index = index;
}

// fold_polynomial (prover.rs:34-42) with the challenge (a scalar) read from device memory: out[j] = c[2j] + r c[2j+1]
template <class F>
__global__ __launch_bounds__(256) void fri_fold_kernel(const typename F::E* __restrict__ c, uint64_t d,
                                                       const typename F::E* __restrict__ r, typename F::E* __restrict__ out) {
    typedef typename F::E E;
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (2 * j >= d) return;
    E v = E::load(c + 2 * j);
    if (2 * j + 1 < d) v = v + E::load(r) * E::load(c + 2 * j + 1);
    v.store(out + j);
}

// fold_polynomial fused with the preparation of the NEXT layer's transform input: next_poly[j] = c[2j] + r c[2j+1]
// (j < ceil(d / 2)) and next_ev[j] = next_poly[j] coset^j, zero-padded to next_dom (FriLayer::from_poly evaluates on
// coset <omega>: scaling coefficient j by coset^j turns it into a plain NTT).  r == nullptr: no fold, `c` is scaled as it is
// (the first layer).  A workgroup covers F::PREP_THREADS x F::PREP_CHUNK consecutive j; every thread computes one power of
// the coset and then steps by `stride` = coset^F::PREP_STEP.  The thread mapping is the field's own: here 8
// consecutive j per thread, over Fr (fri_fr.hpp) 16 interleaved ones so that neighbouring lanes touch neighbouring elements.
template <class F>
__global__ void fri_fold_prep_kernel(const typename F::E* __restrict__ c, uint64_t d, const typename F::E* __restrict__ r,
                                     typename F::E coset, typename F::E stride, uint64_t next_dom,
                                     typename F::E* __restrict__ next_poly, typename F::E* __restrict__ next_ev);
template <>
__global__ __launch_bounds__(FriGl::PREP_THREADS) void fri_fold_prep_kernel<FriGl>(const Gl* __restrict__ c, uint64_t d,
                                                                                   const Gl* __restrict__ r_ptr, Gl coset, Gl stride,
                                                                                   uint64_t next_dom, Gl* __restrict__ next_poly,
                                                                                   Gl* __restrict__ next_ev) {
    const uint64_t j0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * FriGl::PREP_CHUNK;
    if (j0 >= next_dom) return;
    const bool fold = r_ptr != nullptr;
    const uint64_t nl = fold ? (d + 1) / 2 : d;
    const Gl r{fold ? r_ptr->v : 0};
    Gl pw = pow_u64(coset, j0);
    for (uint64_t j = j0; j < j0 + FriGl::PREP_CHUNK && j < next_dom; j++) {
        uint64_t e = 0;
        if (j < nl) {
            Gl v;
            if (fold) {
                v = c[2 * j];
                if (2 * j + 1 < d) v = v + r * c[2 * j + 1];
            } else {
                v = c[j];
            }
            if (next_poly) next_poly[j] = v;
            e = (v * pw).v;
        }
        next_ev[j].v = e;
        pw = pw * stride;
    }
}

// The small layers in ONE workgroup: coset NTT, Merkle tree, transcript step and fold of every layer with at most
// 2^F::TAIL_LOG points, all in LDS, so that a layer costs its chain of log2(size) + 1 dependent hashes and no launches.
// Dynamic LDS (no static LDS: the kernel raises its dynamic limit to the full 160 KB): coef[MAX] | ev[MAX] (evaluations, then
// the Merkle levels in place) | tw[MAX / 2] | 128-byte transcript buffer | broadcast element | one SHA slot per thread.
// Goldilocks: 2^11 points, 1024 threads, 40 KiB + 68 KiB of slots.  Fr: 2^10 points, 256 threads, 80 KiB + 49 KiB of slots
// (at 2^11 points the three arrays alone take 160 KiB, and with 512 threads the slots would not fit next to 2^10 points).
template <class F>
struct FriTailParams {
    typedef typename F::E E;
    const E* poly;              // coefficients entering the first tail layer (memory form)
    uint32_t len;               // how many (<= size)
    uint32_t log_size;          // first tail layer has 2^log_size points; the tail runs log_size layers (sizes 2^log_size .. 2)
    E coset;                    // coset of the first tail layer (scalar)
    E coset_stride;             // coset^F::TAIL_THREADS (scalar)
    E omega;                    // root of unity of order 2^log_size (scalar)
    FriTranscriptState* state;  // transcript digest so far and message counter (device memory, updated in place)
    int zero_as_0;
    E* evals[F::TAIL_LOG];
    E* nodes[F::TAIL_LOG];
    E* roots;                   // [log_size] layer roots
    E* r_out;                   // [log_size] folding challenges (scalars)
    E* cst_out;                 // the final constant
};
template <class F>
constexpr size_t fri_tail_bcast_bytes() { return (sizeof(typename F::E) + 15) / 16 * 16; }
template <class F>
constexpr size_t fri_tail_lds() {
    return sizeof(typename F::E) * ((size_t)5 << (F::TAIL_LOG - 1)) + 128 + fri_tail_bcast_bytes<F>() + (size_t)F::TAIL_THREADS * F::SLOT;
}
template <class F>
__global__ __launch_bounds__(F::TAIL_THREADS) void fri_tail_kernel(FriTailParams<F> p) {
    typedef typename F::E E;
    constexpr uint32_t MAX = 1u << F::TAIL_LOG, THREADS = F::TAIL_THREADS;
    constexpr int PER_THREAD = MAX / 2 / THREADS;  // parents / folded coefficients per thread
    static_assert(PER_THREAD >= 1 && PER_THREAD * THREADS * 2 == MAX, "the threads share the parents of the largest layer evenly");
    extern __shared__ uint4 zkp_smem[];
    E* coef = reinterpret_cast<E*>(zkp_smem);  // folded coefficients (memory form)
    E* ev = coef + MAX;                        // evaluations, then the current Merkle level (canonical hashes)
    E* tw = ev + MAX;                          // omega^k, k < 2^(log_size - 1)
    uint8_t* tbuf = reinterpret_cast<uint8_t*>(tw + MAX / 2);
    E* bcast = reinterpret_cast<E*>(tbuf + 128);
    const uint32_t tid = threadIdx.x;
    uint8_t* slot = tbuf + 128 + fri_tail_bcast_bytes<F>() + tid * F::SLOT;
    const bool z0 = p.zero_as_0 != 0;
    uint32_t len = p.len;
    for (uint32_t i = tid; i < len; i += THREADS) coef[i] = E::load(p.poly + i);
    uint32_t data[8];
    for (int i = 0; i < 8; i++) data[i] = p.state->data[i];
    uint64_t index = p.state->index;
    E coset = p.coset, stride = p.coset_stride;
    // the twiddles of every stage of every tail layer are strided reads of this table: layer j uses omega^(2^j k) = tw[k << j]
    for (uint32_t k = tid; k < (1u << (p.log_size - 1)); k += THREADS) tw[k] = pow_u64(p.omega, (uint64_t)k);
    __syncthreads();
    for (uint32_t j = 0; j < p.log_size; j++) {
        const uint32_t ls = p.log_size - j, size = 1u << ls;
        // FriLayer::from_poly (fri_layer.rs:40-46): ev[k] = sum_i c_i (coset w^k)^i = NTT of c_i coset^i, DIT on a bit-reversed
        // load; thread t scales i = t, t + THREADS, ...
        E pw = pow_u64(coset, (uint64_t)tid);
        for (uint32_t i = tid; i < size; i += THREADS) {
            ev[__brev(i) >> (32 - ls)] = i < len ? coef[i] * pw : E::zero();
            pw = pw * stride;
        }
        __syncthreads();
        for (uint32_t s = 0; s < ls; s++) {
            const uint32_t half = 1u << s;
            for (uint32_t b = tid; b < size / 2; b += THREADS) {  // distinct pairs: no hazard inside a stage
                const uint32_t pos = b & (half - 1), i0 = ((b >> s) << (s + 1)) | pos;
                const E u = ev[i0], v = ev[i0 + half] * tw[((uint32_t)pos << (ls - 1 - s)) << j];
                ev[i0] = u + v;
                ev[i0 + half] = u - v;
            }
            __syncthreads();
        }
        // MerkleTree::new (merkle_tree.rs:42-63); ev[] turns into the current level (canonical hashes), in place
        E* nodes = p.nodes[j];
        for (uint32_t i = tid; i < size; i += THREADS) {
            const E e = ev[i];
            e.store(p.evals[j] + i);
            const E h = F::hash_elems(F::canonical(e), e, false, slot, z0);
            ev[i] = h;
            F::mont(h).store(nodes + i);
        }
        __syncthreads();
        uint32_t off = size;
        for (uint32_t count = size; count > 1; count >>= 1) {  // read - barrier - write, up to PER_THREAD parents per thread
            const uint32_t next = count >> 1;
            E h[PER_THREAD];
#pragma unroll
            for (int k = 0; k < PER_THREAD; k++) {
                const uint32_t i = tid + k * THREADS;
                if (i < next) h[k] = F::hash_elems(ev[2 * i], ev[2 * i + 1], true, slot, z0);
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < PER_THREAD; k++) {
                const uint32_t i = tid + k * THREADS;
                if (i < next) {
                    ev[i] = h[k];
                    F::mont(h[k]).store(nodes + off + i);
                }
            }
            __syncthreads();
            off += next;
        }
        // transcript: digest the root, draw the folding challenge (prover.rs:58-66)
        if (tid == 0) {
            const E root = ev[0];
            F::mont(root).store(p.roots + j);
            const E r = fri_transcript_challenge<F>(data, index, root, tbuf, z0);
            r.store(p.r_out + j);
            *bcast = r;
        }
        __syncthreads();
        const E r = *bcast;
        // fold_polynomial (prover.rs:34-42): read - barrier - write
        const uint32_t nl = (len + 1) / 2;
        E v[PER_THREAD];
#pragma unroll
        for (int k = 0; k < PER_THREAD; k++) {
            const uint32_t i = tid + k * THREADS;
            if (i < nl) {
                v[k] = coef[2 * i];
                if (2 * i + 1 < len) v[k] = v[k] + r * coef[2 * i + 1];
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER_THREAD; k++) {
            const uint32_t i = tid + k * THREADS;
            if (i < nl) coef[i] = v[k];
        }
        __syncthreads();
        len = nl;
        coset = coset * coset;
        stride = stride * stride;
    }
    if (tid == 0) {
        coef[0].store(p.cst_out);
        for (int i = 0; i < 8; i++) p.state->data[i] = data[i];
        p.state->index = index;
    }
}

template <class E>
struct FriLayerRef {
    const E* evals;
    const E* nodes;  // all Merkle levels, concatenated
    uint64_t size;   // domain size of the layer (a power of two)
};
// One workgroup per (query, layer): index (1 word), then eval, sym_eval, path[depth], sym_path[depth] (sizeof(E) / 8 words
// each; prover.rs:100-121).  rec_off[q * layers + l] = word offset of the record inside `out`.
template <class E>
__global__ __launch_bounds__(64) void fri_gather_kernel(const FriLayerRef<E>* layers, uint32_t n_layers, const uint64_t* challenges,
                                                        const uint64_t* rec_off, uint64_t* out) {
    constexpr int W = sizeof(E) / 8;
    const uint32_t q = blockIdx.x, l = blockIdx.y;
    const FriLayerRef<E> L = layers[l];
    const uint64_t idx = challenges[q] % L.size, sym = (idx + L.size / 2) % L.size;
    uint32_t depth = 0;
    while ((1ull << depth) < L.size) depth++;
    uint64_t* rec = out + rec_off[(uint64_t)q * n_layers + l];
    if (threadIdx.x == 0) rec[0] = idx;
    for (uint32_t t = threadIdx.x; t < 2 + 2 * depth; t += 64) {
        const E* src;
        if (t == 0) src = L.evals + idx;
        else if (t == 1) src = L.evals + sym;
        else {
            const uint32_t i = (t - 2) % depth;
            const uint64_t leaf = (t - 2) < depth ? idx : sym;
            const uint64_t off = 2 * L.size - 2 * (L.size >> i);  // start of level i for a power-of-two tree
            src = L.nodes + off + ((leaf >> i) ^ 1);
        }
        const uint64_t* s = reinterpret_cast<const uint64_t*>(src);
        uint64_t* dst = rec + 1 + W * (uint64_t)t;  // 8-byte aligned only: word copies
        for (int k = 0; k < W; k++) dst[k] = s[k];
    }
}

}  // namespace zkp
