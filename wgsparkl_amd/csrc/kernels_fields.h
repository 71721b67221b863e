// kernels_fields.h — device code of the Lagrangian field output (include/wgsparkl_hip.h "Lagrangian field output"): the
// Kirchhoff stress, its two invariants, the volume ratio and the stretches of every particle's STORED state, evaluated with the
// step's own functions (device_math.h svd / kirchoff_corotated / kirchoff_neo_hookean / fluid_update, the calls of
// g2p_body.inc's constitutive block) and written in the caller's order. Read-only: nothing here writes simulation state, and
// Dev is what every other kernel gets. The entry points that launch it are in capi_fields.inc. The kernel is a template on the
// dimension for the reason kernels_probe.h gives: it is emitted where capi_fields.inc, the last part of capi.hip, first launches
// it, behind every kernel that existed.
#pragma once

namespace {

constexpr int FIELD_WORDS = DD + 3 + D + 1;   // words of a wgs_particle_field: stress, mean_stress, von_mises, volume_ratio, stretch, model
constexpr int FIELD_THREADS = 256;
// A record leaves as FIELD_UNITS vectors of FIELD_VEC words: four float4 in 3D (one aligned 64-byte piece), five float2 in 2D
// (a 40-byte record is only 8-byte aligned).
constexpr int FIELD_VEC = D == 3 ? 4 : 2;
constexpr int FIELD_UNITS = FIELD_WORDS / FIELD_VEC;
static_assert(FIELD_UNITS * FIELD_VEC == FIELD_WORDS, "a record is a whole number of vectors");
// LDS stride of a record in words. 3D: 16 + 4 of padding — the 64 lanes' ds_write_b128 at 80-byte steps start on 8 different
// banks of 32 and cover all of them evenly (at 64-byte steps they would share two). 2D: 10 words do that as they are.
constexpr int FIELD_STRIDE = D == 3 ? FIELD_WORDS + 4 : FIELD_WORDS;

template <int N> struct FieldVec;
template <> struct FieldVec<4> {
    using type = float4;
    static __device__ float4 make(const float *w) { return make_float4(w[0], w[1], w[2], w[3]); }
};
template <> struct FieldVec<2> {
    using type = float2;
    static __device__ float2 make(const float *w) { return make_float2(w[0], w[1]); }
};

// One record from one slot. `rec` is the record's words in the order of the struct.
// SNOW (data with plastic state under WGS_PLASTICITY_SNOW, corotated): a snow particle — the step's gate on the STORED state, phase == 0
// and plasticity.lambda != 0 — takes lambda hf, mu hf with hf of its stored Jp (device_math.h snow_hardening): the coefficients the
// step that stored the state applied. Every other particle is evaluated as without the switch, by the same instructions.
template <int DIM, bool SNOW = false> __device__ inline void particle_field(const Dev &d, int side, const float *in, uint32_t j, float *rec) {
    Unpacked u;
    unpack_slot<DIM>(in, d.npad, j, SNOW, false, 0u, u);
    fix_uniform<DIM>(d, u);
    if constexpr (SNOW) {
        if (u.phase[0] == 0.f && u.dp[4] != 0.f) {
            const float hf = snow_hardening(u.dp, u.st[0]);
            u.lam = u.lam * hf;
            u.mu = u.mu * hf;
        }
    }
    // (the particle's own model where the data carries a table: layout.h Dev::pmodel)
    const int model = d.pmodel[side] ? (int)d.pmodel[side][j] : d.model;
    float tau[DD], s[D], J;
    if (model == WGS_MODEL_FLUID) {
        // F holds diag(J, 1[, 1]) (layout.h). A zero gradient leaves J as it is and the viscous part out: tau = -Jc p I.
        float zero[DD];
#pragma unroll
        for (int k = 0; k < DD; k++) zero[k] = 0.f;
        J = u.F[0];
        fluid_update<DIM>(u.lam, u.mu, d.fluid_gamma, zero, 0.f, J, tau);
        const float iso = DIM == 3 ? cbrtf(J) : sqrtf(J);   // what k_prep_instances draws
#pragma unroll
        for (int k = 0; k < D; k++) s[k] = iso;
    } else {
        Svd<DIM> sv;
        svd<DIM>(u.F, sv);
        if (model == WGS_MODEL_NEO_HOOKEAN) kirchoff_neo_hookean<DIM>(u.lam, u.mu, u.F, tau);
        else kirchoff_corotated<DIM>(u.lam, u.mu, u.F, sv, tau);
        J = mat_det<DIM>(u.F);
#pragma unroll
        for (int k = 0; k < D; k++) s[k] = sv.s[k];
    }
    // the invariants are functions of the record's own stress, in one order: the diagonal summed k = 0 .. D-1, the deviator squared
    // and summed in storage order. The deviator is scaled by the power of two of its largest entry first (exact): a stress of 1e20,
    // which an inverted element under a large lambda does carry, has no fp32 square.
    float tr = tau[0];
#pragma unroll
    for (int k = 1; k < D; k++) tr = tr + tau[k * D + k];
    const float mean = tr / (float)D;
    float dev[DD], big = 0.f;
#pragma unroll
    for (int c = 0; c < D; c++)
#pragma unroll
        for (int r = 0; r < D; r++) {
            dev[c * D + r] = c == r ? tau[c * D + r] - mean : tau[c * D + r];
            big = fmaxf(big, fabsf(dev[c * D + r]));
        }
    int e = 0;
    if (big - big == 0.f) frexpf(big, &e);   // (finite; 0 gives e = 0. A NaN or an infinity goes through unscaled and stays one)
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < DD; k++) {
        const float x = ldexpf(dev[k], -e);
        q = q + x * x;
    }
#pragma unroll
    for (int k = 0; k < DD; k++) rec[k] = tau[k];
    rec[DD] = mean;
    rec[DD + 1] = ldexpf(sqrtf(1.5f * q), e);
    rec[DD + 2] = J;
#pragma unroll
    for (int k = 0; k < D; k++) rec[DD + 3 + k] = s[k];
    rec[DD + 3 + D] = __uint_as_float((uint32_t)model);
}

// One particle per lane, blocks of FIELD_THREADS slots in a grid-stride loop. The records are scattered by particle id, so a lane
// that stored its own record word by word would touch 16 cache lines per store instruction: a workgroup's records go through LDS
// instead and FIELD_UNITS consecutive lanes write one record as vectors — in 3D four lanes fill one aligned 64-byte piece.
// `out` must be aligned to a vector (16 bytes in 3D, 8 in 2D: capi_fields.inc checks). No atomics; a record depends on its
// particle only.
// (the body is included textually — fields_body.inc, with SNOW in scope — so that the snow kernel of capi_plasticity.inc compiles the
// very text of this one and this one stays the code it was)
template <int DIM> __global__ __launch_bounds__(FIELD_THREADS) void k_particle_fields(Dev d, int side, float *out) {
    constexpr bool SNOW = false;
#include "fields_body.inc"
}

}  // namespace
