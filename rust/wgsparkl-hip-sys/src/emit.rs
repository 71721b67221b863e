//! FFI declarations for include/wgsparkl_hip_emit.h, the run-time particle extension of the C ABI — SOURCE ONLY, like lib.rs:
//! tests/test_emit_abi.py holds this file to the extension header (the struct's repr(C) layout, the constant, the parameter kinds).
//! A `wgs_data` may reserve particle slots at creation (`wgs_data_create_reserved`) and fill them later: batches the caller hands over
//! (`wgs_add_particles`, blocking) or up to `WGS_MAX_EMITTERS` emitters the library fires inside `wgs_step`. The new particles get the
//! caller's indices behind the residents; the next substep rebuilds the block table. Host state of the handle: no device memory, not
//! part of a checkpoint. Detect `wgs_add_particles` by symbol lookup on older libraries of ABI version 7.
use super::{wgs_collider, wgs_data, wgs_particle, wgs_pipeline, wgs_sim_params, wgs_status, DIM};

pub const WGS_MAX_EMITTERS: usize = 8;

/// The integer mixer of the jitter (`wgs_lowbias32` of the header, restated).
pub const fn wgs_lowbias32(mut x: u32) -> u32 {
    x ^= x >> 16;
    x = x.wrapping_mul(0x7feb352d);
    x ^= x >> 15;
    x = x.wrapping_mul(0x846ca68b);
    x ^= x >> 16;
    x
}

/// One emitter: an axis-aligned lattice box of prod(count) particles, emitted again every `period` substeps. 240 bytes in 3D, 176 in 2D.
#[repr(C)]
#[derive(Copy, Clone)]
pub struct wgs_emitter {
    pub proto: wgs_particle, // everything but the position is copied; dynamics.velocity is the emission velocity
    pub model: u8,           // WGS_MODEL_*, read only while the data carries a per-particle table
    pub lo: [f32; DIM],
    pub count: [u32; DIM],
    pub spacing: f32,
    pub jitter: f32, // in [0, 0.5], a fraction of `spacing`
    pub seed: u32,
    pub start_substep: u32,
    pub period: u32,  // >= 1
    pub batches: u32, // 0 = no limit
}

extern "C" {
    /// `wgs_data_create` with room for max(num_particles, particle_capacity) particles; num_particles == 0 is allowed.
    pub fn wgs_data_create_reserved(
        pipeline: *mut wgs_pipeline, params: *const wgs_sim_params, particles: *const wgs_particle, num_particles: usize,
        colliders: *const wgs_collider, num_colliders: usize, cell_width: f32, grid_capacity: u32, particle_capacity: u32,
        out: *mut *mut wgs_data,
    ) -> wgs_status;
    pub fn wgs_get_particle_capacity(d: *mut wgs_data, out: *mut u32) -> wgs_status;
    /// `models`: `k` bytes or null. Blocking. A refusal changes nothing.
    pub fn wgs_add_particles(d: *mut wgs_data, particles: *const wgs_particle, models: *const u8, k: usize) -> wgs_status;
    /// `emitters`: `n` entries (null with n == 0: every emitter is removed). Replaces the set and zeroes the counters.
    pub fn wgs_set_emitters(d: *mut wgs_data, emitters: *const wgs_emitter, n: u32) -> wgs_status;
    /// `out`: room for `WGS_MAX_EMITTERS` entries; `n` receives the count last set.
    pub fn wgs_get_emitters(d: *mut wgs_data, out: *mut wgs_emitter, n: *mut u32) -> wgs_status;
    /// particles emitted and batches skipped for lack of room, per emitter slot (`WGS_MAX_EMITTERS` entries each)
    pub fn wgs_get_emitter_counts(d: *mut wgs_data, emitted: *mut u64, skipped_batches: *mut u64) -> wgs_status;
}
