// Replacement for the body of `Circuit::compile` (plonk/src/circuit.rs:166-245) and the owner of the prover it yields.
// SOURCE-ONLY, not compiled here (see rust/README.md).  Instead of padding the gate list, collecting twelve vectors and
// interpolating them on the host, the gates go to the device as they are: zkp_plonk_prover_create_from_gates pads, builds the
// twelve columns, interpolates and keeps everything resident.  A `GpuPlonkProver` then proves any number of witnesses of the
// same circuit (`set_witness`), where the reference compiles and uploads again.
use ark_bls12_381::Fr;
use zkp_hip_sys::*;

pub struct GpuPlonkProver {
    ptr: *mut zkp_plonk_prover,
    gates: usize,
}

fn limbs(x: &Fr) -> [u64; 4] {
    x.0 .0 // the Montgomery residue, arkworks 0.4 memory form (rust/README.md, "Layouts relied upon")
}

fn wire(p: &Position) -> [u32; 2] {
    match p {
        Position::Pos(col, row) => [*col as u32, *row as u32],
        Position::Dummy => unreachable!("dummy gates are never sent: the device pads"),
    }
}

impl Circuit {
    /// `compile(self)`, device form: Err carries zkp_last_error() ("Invalid position ...", a short SRS, fewer than two gates).
    pub fn compile_gpu(&self, srs: &GpuBases) -> Result<GpuPlonkProver, String> {
        let real: Vec<usize> = (0..self.gates.len()).filter(|&i| !self.gates[i].is_dummy_gate()).collect();
        let (mut pos, mut sel, mut vals) = (Vec::new(), Vec::new(), Vec::new());
        for &i in &real {
            let g = &self.gates[i];
            for w in [g.get_a_wire(), g.get_b_wire(), g.get_c_wire()] {
                pos.extend_from_slice(&wire(w));
            }
            for q in [&g.q_m, &g.q_l, &g.q_r, &g.q_o, &g.q_c, &g.pi] {
                sel.extend_from_slice(&limbs(q)); // pi as stored: Gate::new_* already negated it (gate.rs:53)
            }
            for col in 0..3 {
                vals.extend_from_slice(&limbs(&self.vals[col][i]));
            }
        }
        let table = zkp_plonk_gates { gates: real.len(), pos: pos.as_ptr(), sel: sel.as_ptr(), vals: vals.as_ptr() };
        let mut ptr = core::ptr::null_mut();
        match unsafe { zkp_plonk_prover_create_from_gates(srs.ptr, &table, &mut ptr) } {
            ZKP_OK => Ok(GpuPlonkProver { ptr, gates: real.len() }),
            _ => Err(last_error()),
        }
    }
}

impl GpuPlonkProver {
    /// Another witness for the same gates: `vals[col][i]` as in Circuit::vals, `pi` as stored in the gates (None: unchanged).
    /// The next proof starts at round 1; an unsatisfying witness is reported by round 3 / zkp_plonk_prove as before.
    pub fn set_witness(&mut self, vals: &[Vec<Fr>; 3], pi: Option<&[Fr]>) -> Result<(), String> {
        let flat: Vec<u64> = (0..self.gates).flat_map(|i| (0..3).flat_map(move |c| limbs(&vals[c][i]))).collect();
        let pi_flat: Option<Vec<u64>> = pi.map(|p| p.iter().flat_map(limbs).collect());
        let pi_ptr = pi_flat.as_ref().map_or(core::ptr::null(), |v| v.as_ptr());
        match unsafe { zkp_plonk_prover_set_witness(self.ptr, flat.as_ptr(), pi_ptr, self.gates) } {
            ZKP_OK => Ok(()),
            _ => Err(last_error()),
        }
    }
}

impl Drop for GpuPlonkProver {
    fn drop(&mut self) {
        unsafe { zkp_plonk_prover_destroy(self.ptr) }
    }
}
