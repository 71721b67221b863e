// diag_pass1_body.inc — the body of k_diag_pass1 (kernels_diag.h) and of k_diag_pass1_snow (capi_plasticity.inc), included textually.
// Expects in scope: d, side, plastic, phase_by_pid, acc, the template parameters PART / ENERGY / DIGEST and the constant SNOW.
    __shared__ unsigned long long s_add[DA_NADD], s_tmax[DG_PARTICLE_GROUPS];
    __shared__ uint32_t s_umax[DM_NMAX], s_umin[DN_NMIN];
    if (threadIdx.x < DA_NADD) s_add[threadIdx.x] = 0ull;
    if (threadIdx.x < DG_PARTICLE_GROUPS) s_tmax[threadIdx.x] = 0ull;
    if (threadIdx.x < DM_NMAX) s_umax[threadIdx.x] = 0u;
    if (threadIdx.x < DN_NMIN) s_umin[threadIdx.x] = 0xffffffffu;
    __syncthreads();
    const float *in = d.buf[side];
    const uint32_t npad = d.npad, n = num_slots(d);
    const double h2q = 0.25 * (double)d.h * (double)d.h;
    const double grav[3] = {(double)d.sp->gravity[0], (double)d.sp->gravity[1], D == 3 ? (double)d.sp->gravity[D - 1] : 0.0};
    unsigned long long add[DA_NADD] = {0ull, 0ull, 0ull, 0ull}, tmax[DG_PARTICLE_GROUPS];
    uint32_t umax[DM_NMAX], umin[DN_NMIN];
    for (int k = 0; k < DG_PARTICLE_GROUPS; k++) tmax[k] = 0ull;
    for (int k = 0; k < DM_NMAX; k++) umax[k] = 0u;
    for (int k = 0; k < DN_NMIN; k++) umin[k] = 0xffffffffu;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < n; j += gridDim.x * 256u) {
        const uint32_t pid = ldpid<D>(in, npad, j);
        if (pid == PID_DEAD) continue;
        Unpacked u;
        unpack_slot<D>(in, npad, j, SNOW ? true : DIGEST && plastic, false, 0u, u);
        fix_uniform<D>(d, u);
        add[DA_COUNT]++;
        if constexpr (DIGEST) {
            float st[3] = {1.f, 1.f, 0.f}, ph[2] = {0.f, 0.f};
            if (plastic) {
                for (int k = 0; k < 3; k++) st[k] = u.st[k];
                ph[0] = u.phase[0]; ph[1] = u.phase[1];
            } else if (phase_by_pid) {
                ph[0] = phase_by_pid[(size_t)pid * 2]; ph[1] = phase_by_pid[(size_t)pid * 2 + 1];
            }
            const unsigned long long h = diag_hash(pid, u, st, ph);
            add[DA_DIGEST0] += h;
            add[DA_DIGEST1] += diag_mix(h + DIAG_SECOND);
        }
        if constexpr (PART) {
            if (!diag_finite(u)) { add[DA_NONFINITE]++; continue; }
            double t[DIAG_PARTICLE_SUMS];
            // (Psi of the particle's OWN model where the data carries a table: layout.h Dev::pmodel)
            if constexpr (SNOW) {
                Unpacked uh = u;
                diag_snow_harden(uh);
                diag_particle_terms<ENERGY>(uh, h2q, grav, d.model, (double)d.fluid_gamma, t);
            } else
            diag_particle_terms<ENERGY>(u, h2q, grav, d.pmodel[side] ? (int)d.pmodel[side][j] : d.model, (double)d.fluid_gamma, t);
#pragma unroll
            for (int s = 0; s < DIAG_PARTICLE_SUMS; s++) {
                const unsigned long long b = diag_abs_bits(t[s]);
                tmax[diag_group_of(s)] = b > tmax[diag_group_of(s)] ? b : tmax[diag_group_of(s)];
            }
            double vv = 0.0, aa = 0.0;
            float vinf = 0.f;
            for (int k = 0; k < D; k++) {
                const uint32_t o = diag_ord(u.x[k]);
                umax[DM_AABB + k] = max(umax[DM_AABB + k], o);
                umin[DN_AABB + k] = min(umin[DN_AABB + k], o);
                vv += (double)u.v[k] * (double)u.v[k];
                vinf = fmaxf(vinf, fabsf(u.v[k]));
            }
            for (int k = 0; k < DD; k++) aa += (double)u.C[k] * (double)u.C[k];
            const uint32_t det = diag_ord((float)diag_det(u.F));
            umax[DM_DET] = max(umax[DM_DET], det);
            umin[DN_DET] = min(umin[DN_DET], det);
            // (non-negative fp32 values: their bit patterns are ordered as they are)
            umax[DM_SPEED] = max(umax[DM_SPEED], __float_as_uint((float)sqrt(vv)));
            umax[DM_AFFINE] = max(umax[DM_AFFINE], __float_as_uint((float)sqrt(aa)));
            umax[DM_VINF] = max(umax[DM_VINF], __float_as_uint(vinf));
            const double w2 = u.mass > 0.f ? ((double)u.lam + 2.0 * (double)u.mu) * (double)u.vol / (double)u.mass : 0.0;
            if (w2 > 0.0) umax[DM_WAVE] = max(umax[DM_WAVE], __float_as_uint((float)sqrt(w2)));
        }
    }
    const bool leader = (threadIdx.x & 63u) == 0u;
    for (int k = 0; k < DA_NADD; k++) {
        const unsigned long long v = diag_wave_add(add[k]);
        if (leader && v) atomicAdd(&s_add[k], v);
    }
    if constexpr (PART) {
        for (int k = 0; k < DG_PARTICLE_GROUPS; k++) {
            const unsigned long long v = diag_wave_max(tmax[k]);
            if (leader) atomicMax(&s_tmax[k], v);
        }
        for (int k = 0; k < DM_NMAX; k++) {
            const uint32_t v = diag_wave_max(umax[k]);
            if (leader) atomicMax(&s_umax[k], v);
        }
        for (int k = 0; k < DN_NMIN; k++) {
            const uint32_t v = diag_wave_min(umin[k]);
            if (leader) atomicMin(&s_umin[k], v);
        }
    }
    __syncthreads();
    if (threadIdx.x < DA_NADD && s_add[threadIdx.x]) atomicAdd(&acc->add[threadIdx.x], s_add[threadIdx.x]);
    if constexpr (PART) {
        if (threadIdx.x < DG_PARTICLE_GROUPS && s_tmax[threadIdx.x]) atomicMax(&acc->tmax[threadIdx.x], s_tmax[threadIdx.x]);
        if (threadIdx.x < DM_NMAX) atomicMax(&acc->umax[threadIdx.x], s_umax[threadIdx.x]);
        if (threadIdx.x < DN_NMIN) atomicMin(&acc->umin[threadIdx.x], s_umin[threadIdx.x]);
    }
