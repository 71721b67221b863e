/* wgsparkl_hip_plasticity.h — the plasticity extension of the C ABI of include/wgsparkl_hip.h: the plasticity rule of a wgs_data and
 * the snow rule. Included by wgsparkl_hip.h (inside its extern "C" block, behind the declarations it needs); include that file, not
 * this one. Added at WGS_ABI_VERSION 7 without touching a struct, an enum value or a signature of wgsparkl_hip.h: a binding that must
 * run against older libraries of version 7 detects wgs_set_plasticity_model by symbol lookup. The mirrors: wgsparkl_amd/_ffi.py
 * (plasticity_prototypes), the second extern block of rust/wgsparkl-hip-sys/src/lib.rs, include/wgsparkl_hip.hpp; tests/test_snow_truth.py
 * holds them to this file with the means of tests/abi.py. */
#ifndef WGSPARKL_HIP_PLASTICITY_H
#define WGSPARKL_HIP_PLASTICITY_H

/* Snow plasticity. NEW: the reference's only plastic material is Drucker-Prager sand. WGS_PLASTICITY_SNOW is the singular-value clamp
 * with hardening of Stomakhin et al. 2013, on the corotated stress. One rule per wgs_data (default WGS_PLASTICITY_DRUCKER_PRAGER): it
 * says which projection the plastic particle update applies and how the six slots of a particle's wgs_drucker_prager are read.
 * A particle is a snow particle under the gate that sends it into the Drucker-Prager projection otherwise: phase == 0 (from the start,
 * or broken in this substep) and plasticity.lambda != 0. Its slots then mean
 *     h0 = theta_c  critical compression      h1 = theta_s  critical stretch      h2 = xi  hardening coefficient
 *     h3 = the cap on the hardening exponent  lambda = the switch alone (non-zero: on)     mu = unused
 * (the struct is not touched: WGS_MODEL_FLUID reinterprets wgs_elastic_coefficients the same way). Per snow particle and substep, all
 * in fp32, with s_k the signed singular values of the trial matrix F + (G dt) F (U, V proper rotations, the sign on the smallest),
 * Jp = wgs_plastic_state.plastic_deformation_gradient_det and lambda, mu = the particle's own wgs_elastic_coefficients:
 *     s^_k = min(max(s_k, 1 - theta_c), 1 + theta_s)
 *     Jp'  = Jp * prod |s_k| / prod s^_k
 *     F_E  = U diag(s^) V^T                          stored in def_grad
 *     hf   = exp(min(xi * (1 - Jp'), h3))
 *     tau  = the corotated stress of F_E with lambda * hf, mu * hf
 * lambda, mu are stored unchanged (hf is never stored); plastic_hardening and log_vol_gain are written back bit for bit. hf is taken
 * of the UPDATED Jp on purpose: whoever reads the stored state recomputes the very coefficients the step applied. A particle that
 * does not pass the gate is advanced exactly as without the switch. An inverted or vanished singular value comes back to
 * 1 - theta_c; Jp' >= 0 always, and 0 where a singular value vanished.
 * Preconditions on the parameters, the caller's: 0 <= theta_c < 1, theta_s >= 0, xi and h3 finite (the Python mirror models.Snow
 * checks them). They enter arithmetic only: no value makes a kernel read or write outside its arrays.
 * What follows the rule: wgs_read_particle_fields[_device] evaluate the stress of a snow particle with lambda * hf, mu * hf, hf of the
 * stored Jp (wgs_particle_field.model stays WGS_MODEL_COROTATED); WGS_SUM_ELASTIC takes Psi with the same coefficients
 * (max_wave_speed keeps the stored ones). The state digest, wgs_read_particles and wgs_set_plastic_state are unchanged, so
 * wgs_read_particles (+ plastic state) -> wgs_data_create -> wgs_set_plastic_state -> wgs_set_plasticity_model(WGS_PLASTICITY_SNOW)
 * restarts a run bit for bit.
 * Stream-ordered like the other setters: the substeps and read-outs enqueued after the call use it; no device memory, no launch.
 * WGS_PLASTICITY_DRUCKER_PRAGER, or WGS_PLASTICITY_SNOW on data whose step carries no plastic state, launches exactly what was
 * launched before. Errors (nothing is changed): an unknown kind, NULL data / NULL out -> WGS_ERR_INVALID_ARGUMENT; sharded data
 * (wgs_data_create_sharded: the arrivals' kernel has no snow variant) -> WGS_ERR_UNSUPPORTED from the setter, like wgs_set_domain_walls
 * (the getter answers WGS_PLASTICITY_DRUCKER_PRAGER there); WGS_PLASTICITY_SNOW while the data's model is not WGS_MODEL_COROTATED or
 * a table of per-particle models is set -> WGS_ERR_UNSUPPORTED; and while WGS_PLASTICITY_SNOW is set,
 * wgs_set_constitutive_model(any other model) -> WGS_ERR_UNSUPPORTED. */
enum { WGS_PLASTICITY_DRUCKER_PRAGER = 0, WGS_PLASTICITY_SNOW = 1 };
wgs_status wgs_set_plasticity_model(wgs_data *data, int32_t kind);
wgs_status wgs_get_plasticity_model(wgs_data *data, int32_t *out);

#endif /* WGSPARKL_HIP_PLASTICITY_H */
