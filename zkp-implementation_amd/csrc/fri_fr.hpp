// fri_fr.hpp -- what the FRI commitment path needs of the BLS12-381 scalar field Fr: Display, digest reduction, sampling,
// and the two kernels whose shape is Fr's own (Merkle levels, fold + coset scaling).  Everything else is fri.hpp's templates
// over the policy FriFr at the end of this file.  Same objects as over Goldilocks, larger messages:
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

// The Fr side of the field parameter of fri.hpp's templates (FriGl is the other): scalars are Montgomery residues, the
// element's own form, so they multiply like any element.
struct FriFr {
    typedef Fr E;
    static constexpr int SLOT = FR_SHA_SLOT;
    static constexpr int TAIL_LOG = 10;       // capacity of the tail kernel's LDS layout; the driver's default threshold is 2^9
    static constexpr int TAIL_THREADS = 256;  // two parents / folded coefficients per thread at 2^10 points
    static constexpr int PREP_CHUNK = 16;     // fri_fold_prep_kernel<FriFr>: elements per thread,
    static constexpr int PREP_THREADS = 256;  // threads per workgroup,
    static constexpr int PREP_STEP = 256;     // and the distance between two elements of one thread (interleaved)
    static ZKP_DEV E canonical(const E& mont) { return fr_canonical_from_mont(mont); }
    static ZKP_DEV E mont(const E& canon) { return fr_mont_from_canonical(canon); }
    static ZKP_DEV int write_decimal(const E& canon, uint8_t* dst, bool z0) { return fr_write_decimal(canon, dst, z0); }
    static ZKP_DEV E hash_elems(const E& a, const E& b, bool two, uint8_t* slot, bool z0) { return fr_hash_elems(a, b, two, slot, z0); }
    // ark-ff UniformRand from one ChaCha block: 4 x next_u64 = 8 words per candidate, top bit masked (255-bit modulus),
    // rejected while >= r; the accepted integer IS the Montgomery residue.  false: both candidates of the block were rejected
    static ZKP_DEV bool challenge_from_block(const uint32_t x[16], E& scalar) {
        for (int h = 0; h < 2; h++) {
            Fr v;
            for (int i = 0; i < 8; i++) v.l[i] = x[8 * h + i];
            v.l[7] &= 0x7fffffffu;
            uint32_t t[8];
            if (sub_limbs<8>(t, v.l, FrParams::MOD)) {  // borrow: v < r
                scalar = v;
                return true;
            }
        }
        return false;
    }
};

// fri_fold_prep_kernel (fri.hpp) in the Fr mapping: lane t of a workgroup takes base + 256 k + t, k < 16, so that
// neighbouring lanes touch neighbouring 32-byte elements; one power per lane, then steps by `stride` = coset^256.
template <>
__global__ __launch_bounds__(FriFr::PREP_THREADS) void fri_fold_prep_kernel<FriFr>(const Fr* __restrict__ c, uint64_t d,
                                                                                   const Fr* __restrict__ r_mont, Fr coset, Fr stride,
                                                                                   uint64_t next_dom, Fr* __restrict__ next_poly,
                                                                                   Fr* __restrict__ next_ev) {
    const uint64_t j0 = (uint64_t)blockIdx.x * FriFr::PREP_THREADS * FriFr::PREP_CHUNK + threadIdx.x;
    if (j0 >= next_dom) return;
    const bool fold = r_mont != nullptr;
    const uint64_t nl = fold ? (d + 1) / 2 : d;
    const Fr r = fold ? Fr::load(r_mont) : Fr::zero();
    Fr pw = pow_u64(coset, j0);
    for (int k = 0; k < FriFr::PREP_CHUNK; k++) {
        const uint64_t j = j0 + (uint64_t)k * FriFr::PREP_STEP;
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

}  // namespace zkp
