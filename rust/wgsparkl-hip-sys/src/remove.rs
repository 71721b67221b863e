//! FFI declarations for include/wgsparkl_hip_remove.h, the particle-removal extension of the C ABI — SOURCE ONLY, like lib.rs:
//! tests/test_remove_abi.py holds this file to the extension header (the struct's repr(C) layout, the constants, the parameter kinds).
//! Particles leave a `wgs_data` by a mask of the caller's (`wgs_remove_particles`, `wgs_remove_particles_device`), by regions evaluated
//! on the device now (`wgs_remove_particles_in`) or by up to `WGS_MAX_SINKS` sinks the library evaluates inside `wgs_step`, in one pass
//! in front of the substeps their schedule names, ahead of the emitters. The survivors keep their relative order and are renumbered
//! densely; the next substep rebuilds the block table. Every removal reads the new particle count back: the explicit calls block, a
//! due sink makes `wgs_step` wait for the stream. Host state of the handle: no device memory, not part of a checkpoint. Detect
//! `wgs_remove_particles` by symbol lookup on older libraries of ABI version 7.
use super::{wgs_data, wgs_pipeline, wgs_status};

pub const WGS_MAX_SINKS: usize = 8;
pub const WGS_SINK_INSIDE: u32 = 0;
pub const WGS_SINK_OUTSIDE: u32 = 1;

/// One region, the side of it that is removed, and (read by `wgs_set_sinks` only) the schedule. 40 bytes in both dimensions; the third
/// components are ignored in 2D.
#[repr(C)]
#[derive(Copy, Clone)]
pub struct wgs_sink {
    pub region: u32, // WGS_REGION_BOX or WGS_REGION_BALL (forces.rs)
    pub side: u32,   // WGS_SINK_INSIDE or WGS_SINK_OUTSIDE
    pub center: [f32; 3],
    pub half: [f32; 3], // BOX: half extents; BALL: half[0] is the radius
    pub start_substep: u32,
    pub period: u32, // >= 1
}

extern "C" {
    /// `remove`: num_particles bytes, nonzero = remove. `kept_from`: null, or room for the OLD num_particles. Blocking.
    pub fn wgs_remove_particles(d: *mut wgs_data, remove: *const u8, kept_from: *mut u32, num_removed: *mut u32) -> wgs_status;
    /// the same with `remove_device` and `kept_from_device` (or null) in device memory, on the data's stream. Blocking.
    pub fn wgs_remove_particles_device(d: *mut wgs_data, remove_device: *const u8, kept_from_device: *mut u32, num_removed: *mut u32) -> wgs_status;
    /// the regions' membership evaluated on the device, once, now; the schedule fields are ignored
    pub fn wgs_remove_particles_in(d: *mut wgs_data, regions: *const wgs_sink, n: u32, kept_from: *mut u32, num_removed: *mut u32) -> wgs_status;
    /// `sinks`: `n` entries (null with n == 0: every sink is removed). Replaces the set and zeroes the counters.
    pub fn wgs_set_sinks(d: *mut wgs_data, sinks: *const wgs_sink, n: u32) -> wgs_status;
    /// `out`: room for `WGS_MAX_SINKS` entries; `n` receives the count last set.
    pub fn wgs_get_sinks(d: *mut wgs_data, out: *mut wgs_sink, n: *mut u32) -> wgs_status;
    /// particles removed per sink slot (`WGS_MAX_SINKS` entries)
    pub fn wgs_get_sink_counts(d: *mut wgs_data, removed: *mut u64) -> wgs_status;
    /// test hook: the keep-scan alone on caller arrays
    pub fn wgs_debug_compact_map(pipeline: *mut wgs_pipeline, remove: *const u8, n: u32, new_index: *mut u32, kept: *mut u32) -> wgs_status;
}
