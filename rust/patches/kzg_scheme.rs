// SOURCE-ONLY (not compiled here, see ../README.md): the replacement for kzg/src/scheme.rs:22-47 and 84-96.
// Everything else in scheme.rs (commit, commit_vector, open, open_vector, commit_para, verify, batch_verify) is unchanged: they
// all funnel into evaluate_in_s.  verify_cells at the end is an addition: the batched counterpart of batch_verify for the cells of
// zkp_kzg_open_cosets (data-availability sampling), one pairing check for any number of cells.
use ark_ec::AffineRepr;
use ark_ff::{BigInt, Fp};
use ark_poly::Polynomial;
use zkp_hip_sys as sys;

use crate::srs::Srs;
use crate::types::{G1Point, G2Point, Poly};
use ark_bls12_381::Fr;
use rand::Rng;

/// The SRS `Vec<G1Affine>` resident in HBM, uploaded ONCE (the reference clones the vector on every commit, srs.rs:78-80).
/// With `zkp_init_devices` and more than one device the upload shards the points over the GPUs by contiguous chunk and every
/// later MSM runs on all of them (include/zkp_hip.h, "Device slots").
pub struct GpuBases {
    ptr: *mut sys::zkp_bases,
}
unsafe impl Send for GpuBases {} // handles are immutable after creation and may be shared across threads (zkp_hip.h)
unsafe impl Sync for GpuBases {}

impl GpuBases {
    pub fn upload(points: &[G1Point]) -> Self {
        // G1Affine { x, y, infinity } is repr(Rust): repack, never transmute
        let mut xy = Vec::with_capacity(points.len() * 12);
        let mut inf = Vec::with_capacity(points.len());
        for p in points {
            xy.extend_from_slice(&p.x.0 .0); // Montgomery residue limbs, as in memory
            xy.extend_from_slice(&p.y.0 .0);
            inf.push(p.infinity as u8);
        }
        let mut ptr = core::ptr::null_mut();
        let rc = unsafe { sys::zkp_g1_bases_create(xy.as_ptr(), inf.as_ptr(), points.len(), &mut ptr) };
        assert_eq!(rc, sys::ZKP_OK, "{}", sys::last_error());
        // the SRS is fixed for the life of the scheme: pay the one-off expansion (shared bucket set, ~1.4x faster commits)
        let rc = unsafe { sys::zkp_g1_bases_precompute(ptr, 0) };
        assert_eq!(rc, sys::ZKP_OK, "{}", sys::last_error());
        Self { ptr }
    }
    pub fn len(&self) -> usize {
        unsafe { sys::zkp_g1_bases_len(self.ptr) }
    }
    /// Every point on the curve and in G1 (zkp_g1_bases_validate): for an SRS that did not come from typed, checked arkworks values.
    pub fn validate(&self) -> sys::zkp_g1_validation {
        let mut rep: sys::zkp_g1_validation = unsafe { core::mem::zeroed() };
        let rc = unsafe { sys::zkp_g1_bases_validate(self.ptr, core::ptr::null_mut(), &mut rep) };
        assert_eq!(rc, sys::ZKP_OK, "{}", sys::last_error());
        rep
    }
}
impl Drop for GpuBases {
    fn drop(&mut self) {
        unsafe { sys::zkp_g1_bases_destroy(self.ptr) }
    }
}

pub struct KzgScheme(pub(crate) Srs, pub(crate) GpuBases);

impl KzgScheme {
    /// scheme.rs:34
    pub fn new(srs: Srs) -> Self {
        let bases = GpuBases::upload(&srs.g1_points());
        Self(srs, bases)
    }

    /// `new` for an SRS read from outside (a file, a ceremony transcript): the report of the GPU validity check comes back with the
    /// scheme, `bad == 0` means every point is a G1 point.  A bad point is the caller's decision, not a panic: the report names the
    /// first one.  (Whether the points are the powers of one secret is zkp_srs_check, which needs [s]_2 and random scalars.)
    pub fn new_checked(srs: Srs) -> (Self, sys::zkp_g1_validation) {
        let scheme = Self::new(srs);
        let report = scheme.1.validate();
        (scheme, report)
    }

    /// scheme.rs:84-96 -- the one seam: sum_i c_i [s^i]G_1 as ONE Pippenger MSM on the GPU(s) instead of n double-and-add
    /// scalar multiplications and 2n inversions.
    pub(crate) fn evaluate_in_s(&self, polynomial: &Poly) -> G1Point {
        assert!(self.1.len() > polynomial.degree()); // unchanged (scheme.rs:86)
        let c = &polynomial.coeffs; // &[Fr]: BigInt<4> Montgomery residues, contiguous
        let (mut xy, mut inf) = ([0u64; 12], 0u8);
        let rc = unsafe { sys::zkp_msm_g1(self.1.ptr, c.as_ptr() as *const u64, c.len(), xy.as_mut_ptr(), &mut inf) };
        assert_eq!(rc, sys::ZKP_OK, "{}", sys::last_error());
        if inf != 0 {
            return G1Point::zero(); // empty polynomial -> identity (scheme.rs:94)
        }
        let limb = |o: usize| BigInt::<6>([xy[o], xy[o + 1], xy[o + 2], xy[o + 3], xy[o + 4], xy[o + 5]]);
        // the limbs ARE the Montgomery residues: construct the field elements without another conversion
        G1Point::new_unchecked(Fp::new_unchecked(limb(0)), Fp::new_unchecked(limb(6)))
    }
}

/// One cell of zkp_kzg_open_cosets: the l values of `commitments[commit]` on coset `coset` of the domain of 2^log_n, and its proof.
pub struct Cell {
    pub commit: u32,
    pub coset: u32,
    pub evals: Vec<Fr>,
    pub proof: G1Point,
}

fn g1_limbs(points: impl Iterator<Item = G1Point>) -> (Vec<u64>, Vec<u8>) {
    let (mut xy, mut inf) = (Vec::new(), Vec::new());
    for p in points {
        xy.extend_from_slice(&p.x.0 .0);
        xy.extend_from_slice(&p.y.0 .0);
        inf.push(p.infinity as u8);
    }
    (xy, inf)
}

impl KzgScheme {
    /// All `cells` in ONE pairing check (include/zkp_hip.h, "batched cell verification"): `g2_sl` = [s^l]_2, l = 2^log_l.  The
    /// weights are drawn here as batch_verify draws its r_primes (scheme.rs:215-245: `Fr::from(rng.gen::<u128>())`); every
    /// commitment and proof is validated on the device before it is used.  A long-lived caller keeps the verifier instead of
    /// making one per call.
    pub fn verify_cells(&self, g2_sl: &G2Point, commitments: &[G1Point], cells: &[Cell], log_n: u32, log_l: u32) -> bool {
        let l = 1usize << log_l;
        let mut g2 = [0u64; 24];
        for (i, c) in [g2_sl.x.c0, g2_sl.x.c1, g2_sl.y.c0, g2_sl.y.c1].iter().enumerate() {
            g2[6 * i..6 * i + 6].copy_from_slice(&c.0 .0);
        }
        let mut v = core::ptr::null_mut();
        let rc = unsafe {
            sys::zkp_kzg_cell_verifier_create(self.1.ptr, g2.as_ptr(), log_n, log_l, cells.len().max(1), commitments.len().max(1), &mut v)
        };
        assert_eq!(rc, sys::ZKP_OK, "{}", sys::last_error());
        let (commits_xy, commits_inf) = g1_limbs(commitments.iter().copied());
        let (proofs_xy, proofs_inf) = g1_limbs(cells.iter().map(|c| c.proof));
        let commit_index: Vec<u32> = cells.iter().map(|c| c.commit).collect();
        let coset_index: Vec<u32> = cells.iter().map(|c| c.coset).collect();
        let mut evals: Vec<Fr> = Vec::with_capacity(cells.len() * l);
        for c in cells {
            assert_eq!(c.evals.len(), l);
            evals.extend_from_slice(&c.evals);
        }
        let mut rng = rand::thread_rng();
        let weights: Vec<Fr> = cells.iter().map(|_| Fr::from(rng.gen::<u128>())).collect();
        let mut accepted = 0i32;
        let rc = unsafe {
            sys::zkp_kzg_verify_cells(v, commits_xy.as_ptr(), commits_inf.as_ptr(), commitments.len(), cells.len(), commit_index.as_ptr(),
                                      coset_index.as_ptr(), evals.as_ptr() as *const u64, proofs_xy.as_ptr(), proofs_inf.as_ptr(),
                                      weights.as_ptr() as *const u64, &mut accepted)
        };
        unsafe { sys::zkp_kzg_cell_verifier_destroy(v) };
        // a point outside G1 is ZKP_E_ARG: for a verifier that is a rejection, any other failure is the caller's to see
        if rc == sys::ZKP_E_ARG {
            return false;
        }
        assert_eq!(rc, sys::ZKP_OK, "{}", sys::last_error());
        accepted != 0
    }

    /// The cells of a whole block: the coset openings of every polynomial of `polys` (rows of equal length, zero-padded by the
    /// caller) in ONE call of zkp_kzg_open_cosets_batch -- every dependent step of the opener runs once for all of them.  Returns,
    /// per polynomial, its n / l proofs and its n evaluations in natural order (the values of coset k are evals[k + j r]).  A
    /// long-lived producer keeps the opener instead of making one per call.
    pub fn open_cosets_batch(&self, polys: &[Vec<Fr>], log_n: u32, log_l: u32) -> Vec<(Vec<G1Point>, Vec<Fr>)> {
        let (n, r) = (1usize << log_n, 1usize << (log_n - log_l));
        if polys.is_empty() {
            return Vec::new();
        }
        let len = polys[0].len();
        assert!(polys.iter().all(|p| p.len() == len));
        let coeffs: Vec<Fr> = polys.iter().flatten().copied().collect();
        let mut o = core::ptr::null_mut();
        let rc = unsafe { sys::zkp_kzg_opener_create_cosets_batch(self.1.ptr, log_n, log_l, polys.len(), &mut o) };
        assert_eq!(rc, sys::ZKP_OK, "{}", sys::last_error());
        let mut xy = vec![0u64; polys.len() * r * 12];
        let mut inf = vec![0u8; polys.len() * r];
        let mut evals = vec![Fr::from(0u64); polys.len() * n];
        let rc = unsafe {
            sys::zkp_kzg_open_cosets_batch(o, coeffs.as_ptr() as *const u64, polys.len(), len, len, xy.as_mut_ptr(), inf.as_mut_ptr(),
                                           evals.as_mut_ptr() as *mut u64)
        };
        unsafe { sys::zkp_kzg_opener_destroy(o) };
        assert_eq!(rc, sys::ZKP_OK, "{}", sys::last_error());
        let limb = |o: usize| BigInt::<6>([xy[o], xy[o + 1], xy[o + 2], xy[o + 3], xy[o + 4], xy[o + 5]]);
        (0..polys.len())
            .map(|p| {
                let proofs = (p * r..(p + 1) * r)
                    .map(|i| if inf[i] != 0 { G1Point::zero() } else { G1Point::new_unchecked(Fp::new_unchecked(limb(12 * i)), Fp::new_unchecked(limb(12 * i + 6))) })
                    .collect();
                (proofs, evals[p * n..(p + 1) * n].to_vec())
            })
            .collect()
    }

    /// The blobs of a whole block from the cells a node holds: every row of `cells` (r cells of l values each, as they travel on
    /// the wire; the cells whose `present` byte is 0 are not read) misses the same cosets, so ONE call of
    /// zkp_kzg_recover_cosets_batch builds the vanishing polynomial once and recovers all rows behind it.  Returns, per row, its
    /// `len` coefficients, all its r cells (the missing ones filled in) and whether the present cells were those of a polynomial
    /// of `len` coefficients.  A long-lived node keeps the recoverer instead of making one per call.
    pub fn recover_cosets_batch(&self, cells: &[Vec<Fr>], present: &[u8], len: usize, log_n: u32, log_l: u32) -> Vec<(Vec<Fr>, Vec<Fr>, bool)> {
        let (n, r) = (1usize << log_n, 1usize << (log_n - log_l));
        if cells.is_empty() {
            return Vec::new();
        }
        assert!(present.len() == r && cells.iter().all(|c| c.len() == n));
        let evals: Vec<Fr> = cells.iter().flatten().copied().collect();
        let mut rc_handle = core::ptr::null_mut();
        let rc = unsafe { sys::zkp_kzg_recoverer_create_batch(log_n, log_l, cells.len(), &mut rc_handle) };
        assert_eq!(rc, sys::ZKP_OK, "{}", sys::last_error());
        let mut coeffs = vec![Fr::from(0u64); cells.len() * len];
        let mut filled = vec![Fr::from(0u64); cells.len() * n];
        let mut consistent = vec![0u8; cells.len()];
        let rc = unsafe {
            sys::zkp_kzg_recover_cosets_batch(rc_handle, evals.as_ptr() as *const u64, cells.len(), present.as_ptr(), len, sys::ZKP_KZG_LAYOUT_CELLS,
                                              coeffs.as_mut_ptr() as *mut u64, filled.as_mut_ptr() as *mut u64, consistent.as_mut_ptr())
        };
        unsafe { sys::zkp_kzg_recoverer_destroy(rc_handle) };
        assert_eq!(rc, sys::ZKP_OK, "{}", sys::last_error());
        (0..cells.len())
            .map(|p| (coeffs[p * len..(p + 1) * len].to_vec(), filled[p * n..(p + 1) * n].to_vec(), consistent[p] != 0))
            .collect()
    }
}
