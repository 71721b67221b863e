// diag_pass2_body.inc — the body of k_diag_pass2 (kernels_diag.h) and of k_diag_pass2_snow (capi_plasticity.inc), included textually.
// Expects in scope: d, side, acc, the template parameter ENERGY and the constant SNOW.
    __shared__ unsigned long long s_fixed[DIAG_PARTICLE_SUMS];
    if (threadIdx.x < DIAG_PARTICLE_SUMS) s_fixed[threadIdx.x] = 0ull;
    __syncthreads();
    const float *in = d.buf[side];
    const uint32_t npad = d.npad, n = num_slots(d);
    const double h2q = 0.25 * (double)d.h * (double)d.h;
    const double grav[3] = {(double)d.sp->gravity[0], (double)d.sp->gravity[1], D == 3 ? (double)d.sp->gravity[D - 1] : 0.0};
    double scale[DG_PARTICLE_GROUPS];
    for (int k = 0; k < DG_PARTICLE_GROUPS; k++) scale[k] = acc->scale[k];
    unsigned long long fixed[DIAG_PARTICLE_SUMS];   // (two's complement: the wrap-around sum of the bit patterns is the signed sum)
    for (int s = 0; s < DIAG_PARTICLE_SUMS; s++) fixed[s] = 0ull;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < n; j += gridDim.x * 256u) {
        if (ldpid<D>(in, npad, j) == PID_DEAD) continue;
        Unpacked u;
        unpack_slot<D>(in, npad, j, SNOW, false, 0u, u);
        fix_uniform<D>(d, u);
        if (!diag_finite(u)) continue;
        if constexpr (SNOW) diag_snow_harden(u);
        double t[DIAG_PARTICLE_SUMS];
        diag_particle_terms<ENERGY>(u, h2q, grav, d.pmodel[side] ? (int)d.pmodel[side][j] : d.model, (double)d.fluid_gamma, t);
#pragma unroll
        for (int s = 0; s < DIAG_PARTICLE_SUMS; s++) fixed[s] += (unsigned long long)__double2ll_rn(t[s] * scale[diag_group_of(s)]);
    }
    const bool leader = (threadIdx.x & 63u) == 0u;
    for (int s = 0; s < DIAG_PARTICLE_SUMS; s++) {
        const unsigned long long v = diag_wave_add(fixed[s]);
        if (leader && v) atomicAdd(&s_fixed[s], v);
    }
    __syncthreads();
    if (threadIdx.x < DIAG_PARTICLE_SUMS && s_fixed[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long *>(&acc->fixed[threadIdx.x]), s_fixed[threadIdx.x]);
