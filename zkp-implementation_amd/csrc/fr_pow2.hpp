// fr_pow2.hpp -- the table x^(2^b), b < FR_POW2_BITS, of one Fr element x as a kernel argument: v x^k for an index k < 2^23 is v times
// the entries at the set bits of k (no squarings on the device).  The recoverer and the cell verifier keep one of the root of their
// transforms of r (fr_pow2_table in kzg_handle.inc fills it).
#pragma once
#include "ff.hpp"
#include "fr29.hpp"

namespace zkp {

constexpr unsigned FR_POW2_BITS = 23;  // the openers' range: an index is below r <= 2^23

struct FrPow2 {
    Fr p[FR_POW2_BITS];
};

__device__ __forceinline__ Fr fr_pow2_mul(const Fr& x, const FrPow2& t, uint32_t k) {
    Fr v = x;
#pragma unroll 1
    for (unsigned b = 0; b < FR_POW2_BITS && (k >> b) != 0; b++)
        if ((k >> b) & 1) v = v * t.p[b];
    return v;
}

}  // namespace zkp
