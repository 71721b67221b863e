//! FFI declarations for include/wgsparkl_hip_forces.h, the force-field extension of the C ABI — SOURCE ONLY, like lib.rs:
//! tests/test_force_abi.py holds this file to the extension header (the struct's repr(C) layout, the constants, the parameter kinds).
//! Up to `WGS_MAX_FORCE_FIELDS` rules on the grid nodes' velocities per `wgs_data`, applied in array order behind the grid update
//! and in front of the domain walls and the fused G2P. Host state of the handle: no device memory, not part of a checkpoint.
//! Detect `wgs_set_force_fields` by symbol lookup on older libraries of ABI version 7.
use super::{wgs_data, wgs_status};

/// `wgs_force_field::kind`
pub const WGS_FORCE_NONE: u32 = 0;
pub const WGS_FORCE_UNIFORM: u32 = 1; // v += dt * vec
pub const WGS_FORCE_RADIAL: u32 = 2; // toward `center` (strength > 0 attracts), falloff w_p(|r|^2 + softening^2)
pub const WGS_FORCE_VORTEX: u32 = 3; // about the axis `vec` through `center` (2D: +z)
pub const WGS_FORCE_DRAG: u32 = 4; // backward Euler relaxation toward the velocity `vec` at the rate `strength`
/// `wgs_force_field::region`
pub const WGS_REGION_ALL: u32 = 0;
pub const WGS_REGION_BOX: u32 = 1; // |x_k - region_center_k| <= region_half_k
pub const WGS_REGION_BALL: u32 = 2; // |x - region_center|^2 <= region_half[0]^2
pub const WGS_MAX_FORCE_FIELDS: usize = 8;

/// One force field: the same 68 bytes in both dimensions; the third components are ignored by the 2D library.
#[repr(C)]
#[derive(Copy, Clone)]
pub struct wgs_force_field {
    pub kind: u32,    // WGS_FORCE_*
    pub falloff: u32, // p of w_p(q): 1, 1/sqrt(q), 1/q, 1/(q sqrt(q))
    pub region: u32,  // WGS_REGION_*
    pub strength: f32,
    pub softening: f32,
    pub center: [f32; 3],
    pub vec: [f32; 3],
    pub region_center: [f32; 3],
    pub region_half: [f32; 3],
}

extern "C" {
    /// `fields`: `n` entries (null with n == 0: every field is removed); entries of kind `WGS_FORCE_NONE` are kept and skipped.
    /// A refusal changes nothing. Stream-ordered; single-domain data.
    pub fn wgs_set_force_fields(d: *mut wgs_data, fields: *const wgs_force_field, n: u32) -> wgs_status;
    /// `out`: room for `WGS_MAX_FORCE_FIELDS` entries; `n` receives the count last set.
    pub fn wgs_get_force_fields(d: *mut wgs_data, out: *mut wgs_force_field, n: *mut u32) -> wgs_status;
}
