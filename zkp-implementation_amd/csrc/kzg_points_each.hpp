// kzg_points_each.hpp -- the kernel of zkp_kzg_verify_points_each*: the G1 half of one pairing-product check PER OPENING (driver:
// pairing_host.inc; the checks themselves: pairing.hpp).  Opening i alone verifies iff
//     e(C_m(i) + [z_i]W_i - [y_i]G, G_2) * e(-W_i, [s]_2) == 1,
// so one lane per opening forms the left point L_i = C_m(i) + [z_i]W_i - [y_i]G and writes the pair (L_i, -W_i) where the pairing
// checker over (G_2, [s]_2) reads its points.  No value visits the host on the way.
//
// The two scalar multiplications are the lane routine of g1_ntt.hpp (g1_28_mul_glv: endomorphism split, one joint double-and-add over
// a table kept in memory); the generator is one more base, in a slot of the lane's own.  The three-term sum uses the complete
// additions of g1_28.hpp on operands in the forms the point transform's butterfly gives them (a product stored and reloaded, a
// negated Y as 8p - Y), and the affine coordinates come from one division-step inversion per lane, as in g1_ntt_store_kernel.
// Workspace, plane-major with `cap` points per plane (chunk q of point e at [q * cap + e]): ws_w the proofs, ws_g the generator
// once per lane, ws_t the lane's table entry and, between the steps, its intermediate points -- 3 x 256 bytes per opening.
// Points are expected validated (canonical, on the curve, in G1); garbage gives garbage, and no index or trip count depends on it.
#pragma once
#include "g1_ntt.hpp"

namespace zkp {

// 96-byte ABI point -> affine on 28-bit limbs (as g1_ntt_load_kernel<true>: eight modular doublings, then the bits re-sliced)
ZKP_DEV A28 points_each_from_abi(const uint4* p) {
    G1Affine a = G1Affine::load(p);
#pragma unroll 1
    for (int k = 0; k < 8; k++) {
        a.x = dbl(a.x);
        a.y = dbl(a.y);
    }
    A28 q;
    q.x = fq28_from_sat(a.x);
    q.y = fq28_from_sat(a.y);
    return q;
}

// commit_index: device copy of the call's index, or null (opening i belongs to commitment i).  out_xy: n x 2 x 96 bytes, out_inf: n x 2.
__global__ __launch_bounds__(G1_NTT_THREADS) void points_each_kernel(const uint4* __restrict__ commits, const uint8_t* __restrict__ commits_inf,
                                                                     const uint32_t* __restrict__ commit_index, const uint4* __restrict__ proofs,
                                                                     const uint8_t* __restrict__ proofs_inf, const Fr* __restrict__ z,
                                                                     const Fr* __restrict__ y, const uint4* __restrict__ gen, uint64_t n,
                                                                     uint4* ws_w, uint4* ws_g, uint4* ws_t, uint64_t cap,
                                                                     uint4* __restrict__ out_xy, uint8_t* __restrict__ out_inf) {
    const uint64_t i = (uint64_t)blockIdx.x * G1_NTT_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint64_t m = commit_index ? commit_index[i] : i;
    const bool w_inf = proofs_inf && proofs_inf[i];
    const bool c_inf = commits_inf && commits_inf[m];
    const Fr kz = from_mont(z[i]), ky = from_mont(y[i]);

    // -W_i: the ABI point with its y negated (canonical in, canonical out)
    {
        G1Affine w = G1Affine::load(proofs + 6 * i);
        w.y = neg(w.y);
        if (w_inf) {
            w.x = Fq::zero();
            w.y = Fq::zero();
        }
        w.store(out_xy + 6 * (2 * i + 1));
        out_inf[2 * i + 1] = w_inf ? 1 : 0;
    }

    // [z_i]W_i, left in ws_w[i]
    X28 zw = X28::infinity();
    if (!w_inf && !kz.is_zero()) {
        X28::from_affine(points_each_from_abi(proofs + 6 * i)).store_s(ws_w + i, cap);
        zw = g1_28_mul_glv(kz.l, ws_w + i, cap, ws_t + i, cap);
    }
    zw.store_s(ws_w + i, cap);
    // -[y_i]G, left in ws_g[i]
    X28 yg = X28::infinity();
    if (!ky.is_zero()) {
        X28::from_affine(points_each_from_abi(gen)).store_s(ws_g + i, cap);
        yg = g1_28_mul_glv(ky.l, ws_g + i, cap, ws_t + i, cap);
        yg.y = normalise(sub8(Fq28::zero(), yg.y));
    }
    yg.store_s(ws_g + i, cap);
    // C_m(i), through ws_t[i]
    X28 acc = X28::infinity();
    if (!c_inf) acc = X28::from_affine(points_each_from_abi(commits + 6 * m));
    acc.store_s(ws_t + i, cap);

    acc = X28::load_s(ws_t + i, cap);
    g1_28_add(acc, X28::load_s(ws_w + i, cap));
    g1_28_add(acc, X28::load_s(ws_g + i, cap));

    // to affine: one inversion per lane (0 -> 0)
    const bool inf = acc.is_inf();
    const Fq28 zi3 = fq28_inverse_gcd(acc.zzz);
    const Fq28 zi = zi3 * acc.zz;  // ZZ / ZZZ = 1 / Z
    const Fq28 lx = acc.x * (zi * zi), ly = acc.y * zi3;
    G1Affine r;
    r.x = fq28_to_abi(lx);
    r.y = fq28_to_abi(ly);
    if (inf) {
        r.x = Fq::zero();
        r.y = Fq::zero();
    }
    r.store(out_xy + 6 * (2 * i));
    out_inf[2 * i] = inf ? 1 : 0;
}

}  // namespace zkp
