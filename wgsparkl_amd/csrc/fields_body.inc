// fields_body.inc — the body of k_particle_fields (kernels_fields.h) and of k_particle_fields_snow (capi_plasticity.inc), included
// textually. Expects in scope: d, side, out, the template parameter DIM and the constant SNOW.
    using V = typename FieldVec<FIELD_VEC>::type;
    __shared__ __attribute__((aligned(16))) float s_rec[FIELD_THREADS * FIELD_STRIDE];
    __shared__ uint32_t s_pid[FIELD_THREADS];
    const float *in = d.buf[side];
    const uint32_t n = d.n;
    for (uint32_t base = blockIdx.x * FIELD_THREADS; base < n; base += gridDim.x * FIELD_THREADS) {   // (uniform over the workgroup)
        const uint32_t j = base + threadIdx.x;
        if (j < n) {
            float rec[FIELD_WORDS];
            particle_field<DIM, SNOW>(d, side, in, j, rec);
            V *row = reinterpret_cast<V *>(s_rec + threadIdx.x * FIELD_STRIDE);
#pragma unroll
            for (int k = 0; k < FIELD_UNITS; k++) row[k] = FieldVec<FIELD_VEC>::make(rec + FIELD_VEC * k);
            s_pid[threadIdx.x] = ldpid<DIM>(in, d.npad, j);
        }
        __syncthreads();
        const uint32_t units = min((uint32_t)FIELD_THREADS, n - base) * FIELD_UNITS;
        for (uint32_t t = threadIdx.x; t < units; t += FIELD_THREADS) {
            const uint32_t r = t / FIELD_UNITS, k = t - r * FIELD_UNITS;
            const uint32_t pid = s_pid[r];
            if (pid < n)   // (single-domain data: a permutation of [0, n); nothing is ever written past the caller's n records)
                reinterpret_cast<V *>(out + (size_t)pid * FIELD_WORDS)[k] = reinterpret_cast<const V *>(s_rec + r * FIELD_STRIDE)[k];
        }
        __syncthreads();
    }
