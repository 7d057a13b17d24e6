// fri_fr.hpp -- the FRI commitment path over the BLS12-381 scalar field Fr (fri/src is generic over F: PrimeField; fri.hpp
// is its Goldilocks instance).  Same objects, larger messages:
//
// Display(x) of a canonical Fr value is up to 77 decimal digits, so a leaf message is <= 77 bytes (1 SHA-256 block up to
// 55 bytes, 2 above) and a parent message <= 154 bytes (1 block up to 55, 2 up to 119, 3 above).  Lanes of one wave hash
// different block counts; the message is assembled in a 196-byte LDS slot per lane (3 blocks + 4 bytes: consecutive slots
// start on different banks) and the compression function of fri.hpp runs once per block.
//
// The decimal conversion: gfx950 has no 64-bit integer divide, so the 255-bit value (8 x u32) is split into nine base-10^9
// chunks by schoolbook division with a 62-bit dividend (rem 2^32 + limb, rem < 10^9) and a multiply-high by a constant; limbs
// known to be zero at a given chunk are skipped at compile time (44 limb divisions instead of 72).  Each chunk gives 9 digits
// through 32-bit divisions by 10 (multiply-high as well).
//
// Digest -> Fr: F::from_le_bytes_mod_order (hasher.rs:14-36) of the 256-bit little-endian digest; r ~ 0.45 2^256, so two
// conditional subtractions reduce it.  Nodes are stored in memory form (4 x u64 Montgomery residues, as zkp_ntt_fr).
#pragma once
#include "ff.hpp"
#include "fri.hpp"

namespace zkp {

constexpr int FR_MERKLE_BLOCK = 256;     // lanes per workgroup
constexpr int FR_MERKLE_MAX_LEVELS = 9;  // leaf hashes + 8 LDS levels
constexpr int FR_SHA_SLOT = 196;         // bytes of LDS per lane: 3 blocks + 4
constexpr int FR_DEC_CHUNKS = 9;         // base-10^9 chunks: 81 digits >= the 77 of r - 1

// q = floor(x / 10^9) for x < 2^62: multiply-high by M = ceil(2^92 / 10^9), shift 28 (exact: M 10^9 - 2^92 < 2^30 and
// x 2^30 < 2^92)
ZKP_DEV uint32_t div_1e9(uint64_t x) { return (uint32_t)(__umul64hi(x, 0x44b82fa09b5a52ccull) >> 28); }

// decimal digits of the canonical value x (ark-ff Display: leading zeros trimmed, zero -> nothing, or "0" when zero_as_0);
// returns the number of bytes written
ZKP_DEV int fr_write_decimal(const Fr& x, uint8_t* dst, bool zero_as_0) {
    uint32_t t[8], chunk[FR_DEC_CHUNKS];
#pragma unroll
    for (int i = 0; i < 8; i++) t[i] = x.l[i];
#pragma unroll
    for (int c = 0; c < FR_DEC_CHUNKS; c++) {
        // before this division the value is < 2^255 / 10^(9c) < 2^(255 - floor(29.897 c)): limbs at or above that bit are zero
        const int bits = 255 - (c * 29897) / 1000;
        uint32_t rem = 0;
#pragma unroll
        for (int i = 7; i >= 0; i--) {
            if (32 * i >= bits) continue;  // compile-time after unrolling
            const uint64_t cur = (uint64_t)rem << 32 | t[i];
            const uint32_t q = div_1e9(cur);
            rem = (uint32_t)cur - q * 1000000000u;
            t[i] = q;
        }
        chunk[c] = rem;
    }
    int len = 0;
#pragma unroll
    for (int c = 0; c < FR_DEC_CHUNKS; c++) {
        const uint32_t v = chunk[c];
        const int nd = 1 + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) +
                       (v >= 10000000u) + (v >= 100000000u);
        if (v) len = 9 * c + nd;
    }
    if (len == 0 && zero_as_0) len = 1;
    const int nz = 9 * FR_DEC_CHUNKS - len;
#pragma unroll
    for (int c = 0; c < FR_DEC_CHUNKS; c++) {
        uint32_t v = chunk[c];
#pragma unroll
        for (int j = 8; j >= 0; j--) {
            const uint32_t q = v / 10u;
            const int pos = (FR_DEC_CHUNKS - 1 - c) * 9 + j;  // position in the 81-digit zero-padded string
            if (pos >= nz) dst[pos - nz] = (uint8_t)('0' + (v - 10u * q));
            v = q;
        }
    }
    return len;
}

// F::from_le_bytes_mod_order of the digest (state words, big-endian bytes): canonical value
ZKP_DEV Fr fr_from_digest(const uint32_t st[8]) {
    Fr x;
#pragma unroll
    for (int k = 0; k < 8; k++) x.l[k] = __builtin_bswap32(st[k]);
#pragma unroll
    for (int s = 0; s < 2; s++) {  // x < 2^256 < 3 r
        uint32_t t[8];
        const uint32_t br = sub_limbs<8>(t, x.l, FrParams::MOD);
#pragma unroll
        for (int k = 0; k < 8; k++) x.l[k] = br ? x.l[k] : t[k];
    }
    return x;
}

ZKP_DEV Fr fr_canonical_from_mont(const Fr& m) { return from_mont(m); }
ZKP_DEV Fr fr_mont_from_canonical(const Fr& c) { return c * Fr::r2(); }

// SHA-256 over the `len` message bytes already in `slot` (zero beyond them, room for the padding): 1 to 3 blocks
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

// hash (one element) or hash_slice (two, no separator) of canonical values; canonical result.  `slot` = this lane's LDS
ZKP_DEV Fr fr_hash_elems(const Fr& a, const Fr& b, bool two, uint8_t* slot, bool zero_as_0) {
    uint32_t* sw = reinterpret_cast<uint32_t*>(slot);
#pragma unroll
    for (int i = 0; i < 48; i++) sw[i] = 0;
    int len = 0;
    for (int e = 0; e < (two ? 2 : 1); e++) len += fr_write_decimal(e ? b : a, slot + len, zero_as_0);  // one copy of the code
    uint32_t st[8];
    sha256_slot(slot, len, st);
    return fr_from_digest(st);
}

struct FrMerkleLaunch {
    const Fr* in;   // leaves (leaf_mode) or the nodes of the level below out[0] (memory form)
    uint64_t n_in;
    int leaf_mode;  // 1: out[0][i] = hash(in[i]); 0: `in` is a node level, out[0] is the level above it
    int levels;     // levels written by this launch (<= 9 in leaf mode, <= 8 otherwise)
    int zero_as_0;
    Fr* out[FR_MERKLE_MAX_LEVELS];
};

// MerkleTree::new (merkle_tree.rs:42-63), several levels per launch.  Workgroup b owns inputs [256 b, 256 (b + 1)): one per
// lane (an Fr hash holds ~3x the registers of a Goldilocks one; the in-lane subtree of fri.hpp would index register arrays
// dynamically), then the lane results climb up to 8 levels through LDS.  Level s above the input starts at (256 b) >> s.
__global__ __launch_bounds__(FR_MERKLE_BLOCK) void fri_fr_merkle_levels_kernel(FrMerkleLaunch p) {
    __shared__ Fr cur[FR_MERKLE_BLOCK];
    __shared__ uint32_t slots32[FR_MERKLE_BLOCK * FR_SHA_SLOT / 4];
    const int tid = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * FR_MERKLE_BLOCK;
    uint8_t* slot = reinterpret_cast<uint8_t*>(slots32) + tid * FR_SHA_SLOT;
    const bool z0 = p.zero_as_0 != 0;
    const uint32_t count0 = (uint32_t)(p.n_in - base < (uint64_t)FR_MERKLE_BLOCK ? p.n_in - base : FR_MERKLE_BLOCK);
    int lvl = 0;
    Fr v = Fr::zero();
    if (tid < (int)count0) {
        v = fr_canonical_from_mont(Fr::load(p.in + base + tid));
        if (p.leaf_mode) {
            v = fr_hash_elems(v, v, false, slot, z0);
            fr_mont_from_canonical(v).store(p.out[0] + base + tid);
        }
    }
    if (p.leaf_mode) lvl = 1;
    if (lvl >= p.levels) return;  // uniform: depends on the launch parameters only
    if (tid < (int)count0) cur[tid] = v;
    __syncthreads();
    uint32_t count = count0;
    for (int s = 1; lvl < p.levels; s++, lvl++) {
        const uint32_t next = (count + 1) / 2;
        Fr h = Fr::zero();
        if (tid < (int)next) {
            const bool two = 2 * tid + 1 < (int)count;
            h = fr_hash_elems(cur[2 * tid], two ? cur[2 * tid + 1] : cur[2 * tid], two, slot, z0);
            fr_mont_from_canonical(h).store(p.out[lvl] + (base >> s) + tid);
        }
        __syncthreads();
        if (tid < (int)next) cur[tid] = h;
        __syncthreads();
        count = next;
    }
}

// One lane: Transcript::digest(root) (transcript.rs:64-72) followed by generate_a_challenge (86-89) over Fr.  data / index
// are updated; the challenge is returned in memory form (ark-ff UniformRand: 4 x next_u64, top bit masked, rejected while
// >= r; the accepted integer IS the Montgomery residue).  `buf` = 128 bytes of LDS: 40 + 77 + 9 <= 128, two blocks.
ZKP_DEV Fr fri_fr_transcript_challenge(uint32_t data[8], uint64_t& index, const Fr& root_canonical, uint8_t* buf, bool z0) {
    uint32_t* bw = reinterpret_cast<uint32_t*>(buf);
    for (int i = 0; i < 32; i++) bw[i] = 0;
    for (int i = 0; i < 8; i++) bw[i] = __builtin_bswap32(data[i]);        // previous digest, byte order of the digest
    for (int i = 0; i < 8; i++) buf[32 + i] = (uint8_t)(index >> (8 * i));  // index.to_le_bytes()
    const int len = 40 + fr_write_decimal(root_canonical, buf + 40, z0);
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
    for (uint64_t counter = 0;; counter++) {  // ChaCha12 blocks of 16 words = two 8-word candidates each
        uint32_t in[16] = {0x61707865, 0x3320646e, 0x79622d32, 0x6b206574, key[0], key[1], key[2], key[3], key[4], key[5], key[6],
                           key[7], (uint32_t)counter, (uint32_t)(counter >> 32), 0, 0};
        uint32_t x[16];
        for (int i = 0; i < 16; i++) x[i] = in[i];
        for (int r = 0; r < 6; r++) {
            ZKP_CHACHA_QR(x[0], x[4], x[8], x[12]) ZKP_CHACHA_QR(x[1], x[5], x[9], x[13])
            ZKP_CHACHA_QR(x[2], x[6], x[10], x[14]) ZKP_CHACHA_QR(x[3], x[7], x[11], x[15])
            ZKP_CHACHA_QR(x[0], x[5], x[10], x[15]) ZKP_CHACHA_QR(x[1], x[6], x[11], x[12])
            ZKP_CHACHA_QR(x[2], x[7], x[8], x[13]) ZKP_CHACHA_QR(x[3], x[4], x[9], x[14])
        }
        for (int h = 0; h < 2; h++) {
            Fr v;
            for (int i = 0; i < 8; i++) v.l[i] = x[8 * h + i] + in[8 * h + i];
            v.l[7] &= 0x7fffffffu;  // 255-bit modulus
            uint32_t t[8];
            if (sub_limbs<8>(t, v.l, FrParams::MOD)) return v;  // borrow: v < r
        }
    }
}

// One layer's transcript step (one lane): digest the root, draw the folding challenge into *r_out (memory form), copy the
// root next to the other small outputs.  Nothing on the host waits for a root before the next layer is enqueued.
__global__ void fri_fr_transcript_kernel(FriTranscriptState* state, const Fr* root_mont, Fr* r_out, Fr* root_out, int zero_as_0) {
    __shared__ uint32_t buf[32];
    const Fr root = Fr::load(root_mont);
    root.store(root_out);
    uint32_t data[8];
    for (int i = 0; i < 8; i++) data[i] = state->data[i];
    uint64_t index = state->index;
    const Fr r = fri_fr_transcript_challenge(data, index, fr_canonical_from_mont(root), reinterpret_cast<uint8_t*>(buf),
                                             zero_as_0 != 0);
    r.store(r_out);
    for (int i = 0; i < 8; i++) state->data[i] = data[i];
    state->index = index;
}

// fold_polynomial (prover.rs:34-42) with the challenge (memory form) read from device memory: out[j] = c[2j] + r c[2j+1]
__global__ __launch_bounds__(256) void fri_fr_fold_kernel(const Fr* __restrict__ c, uint64_t d, const Fr* __restrict__ r_mont,
                                                          Fr* __restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (2 * j >= d) return;
    Fr v = Fr::load(c + 2 * j);
    if (2 * j + 1 < d) v = v + Fr::load(r_mont) * Fr::load(c + 2 * j + 1);
    v.store(out + j);
}

// fold_polynomial fused with the preparation of the NEXT layer's transform input: next_poly[j] = c[2j] + r c[2j+1]
// (j < ceil(d / 2)) and next_ev[j] = next_poly[j] coset^j, zero-padded to next_dom (FriLayer::from_poly evaluates on
// coset <omega>: scaling coefficient j by coset^j turns it into a plain NTT).  r_mont == nullptr: no fold, `c` is scaled
// as it is (the first layer).  A workgroup covers FR_PREP_CHUNK x 256 consecutive j, interleaved (lane t: base + 256 k + t,
// so that neighbouring lanes touch neighbouring elements): one power per lane, then steps by coset^256 (`stride`).
constexpr int FR_PREP_CHUNK = 16;
constexpr int FR_PREP_THREADS = 256;
__global__ __launch_bounds__(FR_PREP_THREADS) void fri_fr_fold_prep_kernel(const Fr* __restrict__ c, uint64_t d,
                                                                           const Fr* __restrict__ r_mont, Fr coset, Fr stride,
                                                                           uint64_t next_dom, Fr* __restrict__ next_poly,
                                                                           Fr* __restrict__ next_ev) {
    const uint64_t j0 = (uint64_t)blockIdx.x * FR_PREP_THREADS * FR_PREP_CHUNK + threadIdx.x;
    if (j0 >= next_dom) return;
    const bool fold = r_mont != nullptr;
    const uint64_t nl = fold ? (d + 1) / 2 : d;
    const Fr r = fold ? Fr::load(r_mont) : Fr::zero();
    Fr pw = pow_u64(coset, j0);
    for (int k = 0; k < FR_PREP_CHUNK; k++) {
        const uint64_t j = j0 + (uint64_t)k * FR_PREP_THREADS;
        if (j >= next_dom) break;
        Fr e = Fr::zero();
        if (j < nl) {
            Fr v;
            if (fold) {
                v = Fr::load(c + 2 * j);
                if (2 * j + 1 < d) v = v + r * Fr::load(c + 2 * j + 1);
            } else {
                v = Fr::load(c + j);
            }
            if (next_poly) v.store(next_poly + j);
            e = v * pw;
        }
        e.store(next_ev + j);
        pw = pw * stride;
    }
}

// The small layers in ONE workgroup (fri_tail_kernel's design over Fr): coset NTT, Merkle tree, transcript step and fold of
// every layer with <= FR_TAIL_MAX points, all in LDS, so that a layer costs its chain of log2(size) + 1 dependent hashes and
// no launches.  LDS at 2^FR_TAIL_LOG points: coefficients 32 KiB + evaluations (then the Merkle levels in place) 32 KiB +
// twiddles 16 KiB + 160 B transcript buffer / broadcast + 256 SHA slots of 196 B (49 KiB) = 129 KiB of the 160 KiB.  At 2048
// points the three arrays alone take 160 KiB, and with 512 threads the slots would not fit next to 1024 points either.
constexpr int FR_TAIL_LOG = 10;          // capacity of the kernel's LDS layout
constexpr int FR_TAIL_DEFAULT_LOG = 9;   // threshold the driver uses (2^20 proofs at 2^8 / 2^9 / 2^10 within 1 %)
constexpr int FR_TAIL_MAX = 1 << FR_TAIL_LOG;
constexpr int FR_TAIL_THREADS = 256;
constexpr int FR_TAIL_PER_THREAD = FR_TAIL_MAX / 2 / FR_TAIL_THREADS;  // parents / folded coefficients per thread (2)
constexpr size_t FR_TAIL_LDS = sizeof(Fr) * (2 * FR_TAIL_MAX + FR_TAIL_MAX / 2) + 160 + (size_t)FR_TAIL_THREADS * FR_SHA_SLOT;
struct FriFrTailParams {
    const Fr* poly;             // coefficients entering the first tail layer (memory form)
    uint32_t len;               // how many (<= size)
    uint32_t log_size;          // first tail layer has 2^log_size points; the tail runs log_size layers (sizes 2^log_size .. 2)
    Fr coset;                   // coset of the first tail layer (memory form)
    Fr coset_stride;            // coset^FR_TAIL_THREADS
    Fr omega;                   // root of unity of order 2^log_size (memory form)
    FriTranscriptState* state;  // transcript digest so far and message counter (device memory, updated in place)
    int zero_as_0;
    Fr* evals[FR_TAIL_LOG];
    Fr* nodes[FR_TAIL_LOG];
    Fr* roots;                  // [log_size] layer roots
    Fr* r_out;                  // [log_size] folding challenges
    Fr* cst_out;                // the final constant
};
__global__ __launch_bounds__(FR_TAIL_THREADS) void fri_fr_tail_kernel(FriFrTailParams p) {
    extern __shared__ uint4 zkp_smem[];
    Fr* coef = reinterpret_cast<Fr*>(zkp_smem);  // folded coefficients (memory form)
    Fr* ev = coef + FR_TAIL_MAX;                  // evaluations, then the current Merkle level (canonical hashes)
    Fr* tw = ev + FR_TAIL_MAX;                    // omega^k, k < 2^(log_size - 1)
    uint8_t* tbuf = reinterpret_cast<uint8_t*>(tw + FR_TAIL_MAX / 2);
    Fr* bcast = reinterpret_cast<Fr*>(tbuf + 128);
    const int tid = threadIdx.x;
    uint8_t* slot = tbuf + 160 + tid * FR_SHA_SLOT;
    const bool z0 = p.zero_as_0 != 0;
    uint32_t len = p.len;
    for (uint32_t i = tid; i < len; i += FR_TAIL_THREADS) coef[i] = Fr::load(p.poly + i);
    uint32_t data[8];
    for (int i = 0; i < 8; i++) data[i] = p.state->data[i];
    uint64_t index = p.state->index;
    Fr coset = p.coset, stride = p.coset_stride;
    // layer j uses omega^(2^j k) = tw[k << j]
    for (uint32_t k = tid; k < (1u << (p.log_size - 1)); k += FR_TAIL_THREADS) tw[k] = pow_u64(p.omega, (uint64_t)k);
    __syncthreads();
    for (uint32_t j = 0; j < p.log_size; j++) {
        const uint32_t ls = p.log_size - j, size = 1u << ls;
        // FriLayer::from_poly: ev = NTT of c_i coset^i, DIT on a bit-reversed load; thread t scales i = t, t + 256, ...
        Fr pw = pow_u64(coset, (uint64_t)tid);
        for (uint32_t i = tid; i < size; i += FR_TAIL_THREADS) {
            ev[__brev(i) >> (32 - ls)] = i < len ? coef[i] * pw : Fr::zero();
            pw = pw * stride;
        }
        __syncthreads();
        for (uint32_t s = 0; s < ls; s++) {
            const uint32_t half = 1u << s;
            for (uint32_t b = tid; b < size / 2; b += FR_TAIL_THREADS) {  // distinct pairs: no hazard inside a stage
                const uint32_t pos = b & (half - 1), i0 = ((b >> s) << (s + 1)) | pos;
                const Fr u = ev[i0], v = ev[i0 + half] * tw[((uint32_t)pos << (ls - 1 - s)) << j];
                ev[i0] = u + v;
                ev[i0 + half] = u - v;
            }
            __syncthreads();
        }
        // MerkleTree::new; ev[] turns into the current level (canonical hashes), in place
        Fr* nodes = p.nodes[j];
        for (uint32_t i = tid; i < size; i += FR_TAIL_THREADS) {
            const Fr e = ev[i];
            e.store(p.evals[j] + i);
            const Fr h = fr_hash_elems(fr_canonical_from_mont(e), e, false, slot, z0);
            ev[i] = h;
            fr_mont_from_canonical(h).store(nodes + i);
        }
        __syncthreads();
        uint32_t off = size;
        for (uint32_t count = size; count > 1; count >>= 1) {  // read - barrier - write, up to 2 parents per thread
            const uint32_t next = count >> 1;
            Fr h[FR_TAIL_PER_THREAD];
#pragma unroll
            for (int k = 0; k < FR_TAIL_PER_THREAD; k++) {
                const uint32_t i = tid + k * FR_TAIL_THREADS;
                if (i < next) h[k] = fr_hash_elems(ev[2 * i], ev[2 * i + 1], true, slot, z0);
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < FR_TAIL_PER_THREAD; k++) {
                const uint32_t i = tid + k * FR_TAIL_THREADS;
                if (i < next) {
                    ev[i] = h[k];
                    fr_mont_from_canonical(h[k]).store(nodes + off + i);
                }
            }
            __syncthreads();
            off += next;
        }
        // transcript: digest the root, draw the folding challenge (prover.rs:58-66)
        if (tid == 0) {
            const Fr root = ev[0];
            fr_mont_from_canonical(root).store(p.roots + j);
            const Fr r = fri_fr_transcript_challenge(data, index, root, tbuf, z0);
            r.store(p.r_out + j);
            *bcast = r;
        }
        __syncthreads();
        const Fr r = *bcast;
        // fold_polynomial (prover.rs:34-42): read - barrier - write
        const uint32_t nl = (len + 1) / 2;
        Fr v[FR_TAIL_PER_THREAD];
#pragma unroll
        for (int k = 0; k < FR_TAIL_PER_THREAD; k++) {
            const uint32_t i = tid + k * FR_TAIL_THREADS;
            if (i < nl) {
                v[k] = coef[2 * i];
                if (2 * i + 1 < len) v[k] = v[k] + r * coef[2 * i + 1];
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < FR_TAIL_PER_THREAD; k++) {
            const uint32_t i = tid + k * FR_TAIL_THREADS;
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

struct FriFrLayerRef {
    const Fr* evals;
    const Fr* nodes;  // all Merkle levels, concatenated
    uint64_t size;    // domain size of the layer (a power of two)
};
// One workgroup per (query, layer): index (1 word), eval, sym_eval, path[depth], sym_path[depth] (4 words each;
// prover.rs:100-121).  rec_off[q * layers + l] = word offset of the record inside `out`.
__global__ __launch_bounds__(64) void fri_fr_gather_kernel(const FriFrLayerRef* layers, uint32_t n_layers, const uint64_t* challenges,
                                                           const uint64_t* rec_off, uint64_t* out) {
    const uint32_t q = blockIdx.x, l = blockIdx.y;
    const FriFrLayerRef L = layers[l];
    const uint64_t idx = challenges[q] % L.size, sym = (idx + L.size / 2) % L.size;
    uint32_t depth = 0;
    while ((1ull << depth) < L.size) depth++;
    uint64_t* rec = out + rec_off[(uint64_t)q * n_layers + l];
    if (threadIdx.x == 0) rec[0] = idx;
    for (uint32_t t = threadIdx.x; t < 2 + 2 * depth; t += 64) {
        const Fr* src;
        if (t == 0) src = L.evals + idx;
        else if (t == 1) src = L.evals + sym;
        else {
            const uint32_t i = (t - 2) % depth;
            const uint64_t leaf = (t - 2) < depth ? idx : sym;
            const uint64_t off = 2 * L.size - 2 * (L.size >> i);  // start of level i for a power-of-two tree
            src = L.nodes + off + ((leaf >> i) ^ 1);
        }
        const uint64_t* s = reinterpret_cast<const uint64_t*>(src);
        uint64_t* dst = rec + 1 + 4 * (uint64_t)t;  // 8-byte aligned only: word copies
        for (int k = 0; k < 4; k++) dst[k] = s[k];
    }
}

}  // namespace zkp
