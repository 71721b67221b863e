// kernels_diag.h — device-side diagnostics (include/wgsparkl_hip.h "Device-side diagnostics"): reproducible sums, bounds and a
// state digest, reduced on the device. NEW: the reference reduces nothing on the device.
//
// Included by capi.hip AFTER every other kernel header and after the entry points of the step (it uses unpack_slot + fix_uniform
// of kernels_readback.h, and the kernels of the step keep their place in the code object: DESIGN.md 9.7). Ends in diag_enqueue,
// the launch sequence of one diagnostics call; its two entry points are in capi_debug.inc.
//
// Shape: a streaming pass over the particle quads of the current buffer (16-byte-per-lane loads, one SGPR base: layout.h ldq),
// grid-stride, 256 threads; each lane keeps its partial results in registers, a wave combines them by a __shfl_xor ladder, the four
// waves of a workgroup through LDS integer atomics, the workgroups by ONE set of 64-bit integer atomics each. Nothing is a
// floating-point addition, so none of these orders matters:
//   pass 1  counts, bounds (integer max / min of ordered bit patterns), digest (sums modulo 2^64), and the largest |term| of every sum;
//   scales  one thread: exponent of every sum from the largest |term| and the count (the formula is in the header);
//   pass 2  the same terms again, rint(term * 2^-exponent) accumulated as int64;
//   finish  one thread: the accumulators -> wgs_diagnostics.
#pragma once

namespace {

// groups of sums that share one exponent (the components of a vector sum do)
enum { DG_MASS = 0, DG_MOMENTUM, DG_ANGULAR, DG_MASS_MOMENT, DG_KINETIC, DG_KINETIC_AFFINE, DG_ELASTIC, DG_GRAVITY,
       DG_GRID_MASS, DG_GRID_MOMENTUM, DG_GRID_ANGULAR, DG_COUNT };
constexpr int DG_PARTICLE_GROUPS = DG_GRID_MASS;
constexpr int DIAG_PARTICLE_SUMS = WGS_SUM_GRID_MASS;                  // sums [0, 14) come from particles
constexpr int DIAG_GRID_SUMS = WGS_NUM_SUMS - WGS_SUM_GRID_MASS;       // 7
__host__ __device__ constexpr int diag_group_of(int s) {
    return s < WGS_SUM_MOMENTUM ? DG_MASS : s < WGS_SUM_ANGULAR ? DG_MOMENTUM : s < WGS_SUM_MASS_MOMENT ? DG_ANGULAR :
           s < WGS_SUM_KINETIC ? DG_MASS_MOMENT : s == WGS_SUM_KINETIC ? DG_KINETIC : s == WGS_SUM_KINETIC_AFFINE ? DG_KINETIC_AFFINE :
           s == WGS_SUM_ELASTIC ? DG_ELASTIC : s == WGS_SUM_GRAVITY_POTENTIAL ? DG_GRAVITY : s == WGS_SUM_GRID_MASS ? DG_GRID_MASS :
           s < WGS_SUM_GRID_ANGULAR ? DG_GRID_MOMENTUM : DG_GRID_ANGULAR;
}

enum { DA_COUNT = 0, DA_NONFINITE, DA_DIGEST0, DA_DIGEST1, DA_NADD };
enum { DM_AABB = 0 /* +0..2 */, DM_SPEED = 3, DM_AFFINE, DM_DET, DM_WAVE, DM_VINF, DM_NMAX };
enum { DN_AABB = 0 /* +0..2 */, DN_DET = 3, DN_NMIN };

struct DiagAcc {                          // device accumulators of one diagnostics call
    unsigned long long add[DA_NADD];      // sums modulo 2^64
    unsigned long long tmax[DG_COUNT];    // bit pattern of the largest |term| (fp64, non-negative: ordered like the integers)
    long long fixed[WGS_NUM_SUMS];
    uint32_t umax[DM_NMAX], umin[DN_NMIN];  // ordered bit patterns of fp32 values (diag_ord)
    int32_t exponent[DG_COUNT];
    uint32_t grid_nodes;
    double scale[DG_COUNT];               // 2^-exponent
};

// fp32 -> uint32 with the order of the reals (negative values below positive ones); diag_unord is its inverse
__device__ inline uint32_t diag_ord(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float diag_unord(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

__device__ inline unsigned long long diag_mix(unsigned long long z) {   // splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
constexpr unsigned long long DIAG_GOLDEN = 0x9e3779b97f4a7c15ull, DIAG_SECOND = 0xd1b54a32d192ed03ull;

// the per-particle hash of the header: id, then the words of x, v, F, A, plastic state, phase in pairs
__device__ inline unsigned long long diag_hash(uint32_t pid, const Unpacked &u, const float *st, const float *phase) {
    constexpr int NW = 2 * D + 2 * DD + 5;
    uint32_t w[NW + 1];
    int n = 0;
    for (int k = 0; k < D; k++) w[n++] = __float_as_uint(u.x[k]);
    for (int k = 0; k < D; k++) w[n++] = __float_as_uint(u.v[k]);
    for (int k = 0; k < DD; k++) w[n++] = __float_as_uint(u.F[k]);
    for (int k = 0; k < DD; k++) w[n++] = __float_as_uint(u.C[k]);
    for (int k = 0; k < 3; k++) w[n++] = __float_as_uint(st[k]);
    for (int k = 0; k < 2; k++) w[n++] = __float_as_uint(phase[k]);
    w[NW] = 0u;
    unsigned long long h = diag_mix((unsigned long long)pid + DIAG_GOLDEN);
#pragma unroll
    for (int k = 0; k < NW; k += 2) h = diag_mix(h + DIAG_GOLDEN + ((unsigned long long)w[k] | ((unsigned long long)w[k + 1] << 32)));
    return h;
}

// eigenvalues of the symmetric matrix E (row r, column c at e[r][c]) in fp64: closed form in 2D, cyclic Jacobi in 3D — a fixed number of
// sweeps (quadratic convergence: five leave nothing above round-off for a 3 x 3 matrix), the same instructions for every particle
__device__ inline void diag_sym_eigenvalues(double e[D][D], double *ev) {
    if constexpr (D == 2) {
        const double mean = 0.5 * (e[0][0] + e[1][1]), half = 0.5 * (e[0][0] - e[1][1]);
        const double r = sqrt(half * half + e[0][1] * e[0][1]);
        ev[0] = mean + r;
        ev[1] = mean - r;
    } else {
        for (int sweep = 0; sweep < 5; sweep++)
#pragma unroll
            for (int pq = 0; pq < 3; pq++) {
                const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2, r = 3 - p - q;
                const double apq = e[p][q];
                if (apq == 0.0) continue;
                const double theta = (e[q][q] - e[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                e[p][p] -= t * apq;
                e[q][q] += t * apq;
                e[p][q] = e[q][p] = 0.0;
                const double arp = e[r][p], arq = e[r][q];
                e[r][p] = e[p][r] = c * arp - s * arq;
                e[r][q] = e[q][r] = s * arp + c * arq;
            }
        for (int k = 0; k < D; k++) ev[k] = e[k][k];
    }
}

// Psi(F) of the header in fp64, through G = F - I (exact for an fp32 F) and E = G + G^T + G^T G
__device__ inline double diag_psi(int model, double lambda, double mu, double gamma, const float *F) {
    double g[D][D], e[D][D];   // [row][column]; F is column-major
    for (int c = 0; c < D; c++)
        for (int r = 0; r < D; r++) g[r][c] = (double)F[c * D + r] - (r == c ? 1.0 : 0.0);
    for (int r = 0; r < D; r++)
        for (int c = 0; c < D; c++) {
            double gtg = 0.0;
            for (int k = 0; k < D; k++) gtg += g[k][r] * g[k][c];
            e[r][c] = (g[r][c] + g[c][r]) + gtg;
        }
    // det F - 1 from the invariants of G: tr G + (second invariant) + det G
    double tr = 0.0, i2 = 0.0, detg;
    for (int k = 0; k < D; k++) tr += g[k][k];
    if constexpr (D == 2) {
        detg = g[0][0] * g[1][1] - g[0][1] * g[1][0];
    } else {
        i2 = (g[0][0] * g[1][1] - g[0][1] * g[1][0]) + (g[0][0] * g[2][2] - g[0][2] * g[2][0]) + (g[1][1] * g[2][2] - g[1][2] * g[2][1]);
        detg = g[0][0] * (g[1][1] * g[2][2] - g[1][2] * g[2][1]) - g[0][1] * (g[1][0] * g[2][2] - g[1][2] * g[2][0]) +
               g[0][2] * (g[1][0] * g[2][1] - g[1][1] * g[2][0]);
    }
    const double jm1 = (tr + i2) + detg;
    if (model == WGS_MODEL_FLUID) {
        // (lambda / gamma) (Jc^(1-gamma) / (gamma-1) + Jc - gamma / (gamma-1)), as ((Jc^(1-gamma) - 1) / (gamma-1) + (Jc - 1)): both terms are
        // O(J - 1) with opposite signs near the rest state, and each is formed from ln Jc = log1p(J - 1) without rounding 1 + (J - 1) first
        const bool clamped = !(1.0 + jm1 >= 1.0e-10);
        const double lnj = clamped ? log(1.0e-10) : log1p(jm1);
        const double jcm1 = clamped ? 1.0e-10 - 1.0 : jm1;
        return (lambda / gamma) * (expm1((1.0 - gamma) * lnj) / (gamma - 1.0) + jcm1);
    }
    if (model == WGS_MODEL_NEO_HOOKEAN) {
        double tre = 0.0;
        for (int k = 0; k < D; k++) tre += e[k][k];
        const double lnj = (1.0 + jm1 >= 1.0e-10) ? log1p(jm1) : log(1.0e-10);
        return (0.5 * mu * tre - mu * lnj) + 0.5 * lambda * lnj * lnj;
    }
    double ev[D];
    diag_sym_eigenvalues(e, ev);
    int kmin = 0;
    for (int k = 1; k < D; k++)
        if (ev[k] < ev[kmin]) kmin = k;
    const bool flipped = 1.0 + jm1 < 0.0;   // det F < 0: the smallest singular value carries the sign
    double dev = 0.0;
    for (int k = 0; k < D; k++) {
        const double s = sqrt(fmax(1.0 + ev[k], 0.0));
        const double sm1 = (flipped && k == kmin) ? -(s + 1.0) : ev[k] / (s + 1.0);
        dev += sm1 * sm1;
    }
    return mu * dev + 0.5 * lambda * jm1 * jm1;
}

__device__ inline bool diag_finite(const Unpacked &u) {
    bool ok = isfinite(u.mass) && isfinite(u.vol) && isfinite(u.lam) && isfinite(u.mu);
    for (int k = 0; k < D; k++) ok = ok && isfinite(u.x[k]) && isfinite(u.v[k]);
    for (int k = 0; k < DD; k++) ok = ok && isfinite(u.F[k]) && isfinite(u.C[k]);
    return ok;
}

// the terms of the particle sums (header), in fp64
template <bool ENERGY> __device__ inline void diag_particle_terms(const Unpacked &u, double h2q, const double *grav, int model, double gamma, double *t) {
    const double m = u.mass;
    double x[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < D; k++) { x[k] = u.x[k]; v[k] = u.v[k]; }
    t[WGS_SUM_MASS] = m;
    double vv = 0.0, gx = 0.0, aa = 0.0;
    for (int k = 0; k < 3; k++) {
        t[WGS_SUM_MOMENTUM + k] = m * v[k];
        t[WGS_SUM_MASS_MOMENT + k] = m * x[k];
        vv += v[k] * v[k];
        gx += grav[k] * x[k];
    }
    for (int k = 0; k < DD; k++) aa += (double)u.C[k] * (double)u.C[k];
    const float *A = u.C;   // column-major: row r, column c at A[c * D + r]
    if constexpr (D == 3) {
        t[WGS_SUM_ANGULAR + 0] = m * (x[1] * v[2] - x[2] * v[1]) + h2q * ((double)A[m9(5)] - (double)A[m9(7)]);
        t[WGS_SUM_ANGULAR + 1] = m * (x[2] * v[0] - x[0] * v[2]) + h2q * ((double)A[m9(6)] - (double)A[2]);
        t[WGS_SUM_ANGULAR + 2] = m * (x[0] * v[1] - x[1] * v[0]) + h2q * ((double)A[1] - (double)A[3]);
    } else {
        t[WGS_SUM_ANGULAR + 0] = m * (x[0] * v[1] - x[1] * v[0]) + h2q * ((double)A[1] - (double)A[2]);
        t[WGS_SUM_ANGULAR + 1] = 0.0;
        t[WGS_SUM_ANGULAR + 2] = 0.0;
    }
    t[WGS_SUM_KINETIC] = 0.5 * m * vv;
    t[WGS_SUM_KINETIC_AFFINE] = m != 0.0 ? 0.5 * h2q * aa / m : 0.0;
    t[WGS_SUM_GRAVITY_POTENTIAL] = -(m * gx);
    t[WGS_SUM_ELASTIC] = 0.0;
    if constexpr (ENERGY) t[WGS_SUM_ELASTIC] = (double)u.vol * diag_psi(model, (double)u.lam, (double)u.mu, gamma, u.F);
}

__device__ inline double diag_det(const float *F) {
    if constexpr (D == 2) {
        return (double)F[0] * F[3] - (double)F[2] * F[1];
    } else {
        const double a = F[0], b = F[m9(3)], c = F[m9(6)], d = F[1], e = F[m9(4)], f = F[m9(7)], g = F[2], h = F[m9(5)], i = F[m9(8)];
        return a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    }
}

template <typename T> __device__ inline T diag_wave_max(T v) {
    for (int o = 32; o > 0; o >>= 1) { const T w = __shfl_xor(v, o); v = w > v ? w : v; }
    return v;
}
template <typename T> __device__ inline T diag_wave_min(T v) {
    for (int o = 32; o > 0; o >>= 1) { const T w = __shfl_xor(v, o); v = w < v ? w : v; }
    return v;
}
__device__ inline unsigned long long diag_wave_add(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline unsigned long long diag_abs_bits(double t) { return (unsigned long long)__double_as_longlong(fabs(t)); }

// Pass 1 over the particles. PART: counts of non-finite particles, bounds, the largest |term| of every particle sum (ENERGY: of
// WGS_SUM_ELASTIC too); DIGEST: the two digest sums. `phase_by_pid`: the caller's input phase of data whose step carries no plastic
// state (null on sharded data of that kind).
// SNOW (the bodies below; data with plastic state under WGS_PLASTICITY_SNOW, kernels in capi_plasticity.inc): WGS_SUM_ELASTIC takes Psi
// of a snow particle — phase == 0 and plasticity.lambda != 0 in the stored state — with lambda hf, mu hf, hf of its stored Jp
// (device_math.h snow_hardening): the coefficients of the stress the step applied. Nothing else differs; the digest hashes the stored
// coefficients.
__device__ inline void diag_snow_harden(Unpacked &u) {
    if (u.phase[0] == 0.f && u.dp[4] != 0.f) {
        const float hf = snow_hardening(u.dp, u.st[0]);
        u.lam = u.lam * hf;
        u.mu = u.mu * hf;
    }
}

// (the bodies of the two passes are included textually — diag_pass1_body.inc / diag_pass2_body.inc, with SNOW in scope — so that the snow
// kernels of capi_plasticity.inc compile the very text of these and these stay the code they were)
template <bool PART, bool ENERGY, bool DIGEST>
__global__ __launch_bounds__(256) void k_diag_pass1(Dev d, int side, bool plastic, const float *phase_by_pid, DiagAcc *acc) {
    constexpr bool SNOW = false;
#include "diag_pass1_body.inc"
}

// Pass 2 over the particles: rint(term * 2^-exponent) as int64, summed
template <bool ENERGY> __global__ __launch_bounds__(256) void k_diag_pass2(Dev d, int side, DiagAcc *acc) {
    constexpr bool SNOW = false;
#include "diag_pass2_body.inc"
}

// The grid sums walk the active list like k_export_grid: node t of the list is node t & 63 of block active[t >> 6]. PASS 1: the largest
// |term| of the three sums; PASS 2: the fixed-point sums. Nodes with a non-finite value are left out.
__device__ inline bool diag_node_terms(const Dev &d, uint32_t t, double *out) {
    constexpr int BW = Dim<D>::BW, BS = Dim<D>::BSHIFT;
    const uint32_t b = d.active[t >> 6], ln = t & 63u;
    int bc[3] = {0, 0, 0};
    unpack_key<D>(d.block_key[b], bc);
    const int l[3] = {(int)(ln & (BW - 1)), (int)((ln >> BS) & (BW - 1)), D == 3 ? (int)(ln >> (2 * BS)) : 0};
    const float4 nd = d.nodes[(size_t)b * NPB + ln];
    const float mass = D == 3 ? nd.w : nd.z;
    double x[3] = {0.0, 0.0, 0.0}, v[3] = {(double)nd.x, (double)nd.y, D == 3 ? (double)nd.z : 0.0};
    for (int k = 0; k < D; k++) x[k] = (double)(bc[k] * BW + l[k]) * (double)d.h;
    if (!(isfinite(mass) && isfinite(nd.x) && isfinite(nd.y) && (D == 2 || isfinite(nd.z)))) return false;
    const double m = mass;
    out[0] = m;
    for (int k = 0; k < 3; k++) out[1 + k] = m * v[k];
    if constexpr (D == 3) {
        out[4] = m * (x[1] * v[2] - x[2] * v[1]);
        out[5] = m * (x[2] * v[0] - x[0] * v[2]);
        out[6] = m * (x[0] * v[1] - x[1] * v[0]);
    } else {
        out[4] = m * (x[0] * v[1] - x[1] * v[0]);
        out[5] = out[6] = 0.0;
    }
    return true;
}

template <int PASS> __global__ __launch_bounds__(256) void k_diag_grid(Dev d, DiagAcc *acc) {
    __shared__ unsigned long long s_v[DIAG_GRID_SUMS];
    if (threadIdx.x < DIAG_GRID_SUMS) s_v[threadIdx.x] = 0ull;
    __syncthreads();
    const uint32_t nblocks = min(d.counters[CTR_NBLOCKS], d.cap), total = nblocks * (uint32_t)NPB;
    unsigned long long v[DIAG_GRID_SUMS];
    double scale[DIAG_GRID_SUMS];
    for (int s = 0; s < DIAG_GRID_SUMS; s++) {
        v[s] = 0ull;
        scale[s] = PASS == 2 ? acc->scale[diag_group_of(WGS_SUM_GRID_MASS + s)] : 0.0;
    }
    for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < total; t += gridDim.x * 256u) {
        double term[DIAG_GRID_SUMS];
        if (!diag_node_terms(d, t, term)) continue;
#pragma unroll
        for (int s = 0; s < DIAG_GRID_SUMS; s++) {
            if constexpr (PASS == 1) { const unsigned long long b = diag_abs_bits(term[s]); v[s] = b > v[s] ? b : v[s]; }
            else v[s] += (unsigned long long)__double2ll_rn(term[s] * scale[s]);
        }
    }
    const bool leader = (threadIdx.x & 63u) == 0u;
    for (int s = 0; s < DIAG_GRID_SUMS; s++) {
        if constexpr (PASS == 1) { const unsigned long long w = diag_wave_max(v[s]); if (leader) atomicMax(&s_v[s], w); }
        else { const unsigned long long w = diag_wave_add(v[s]); if (leader && w) atomicAdd(&s_v[s], w); }
    }
    __syncthreads();
    if (threadIdx.x < DIAG_GRID_SUMS && s_v[threadIdx.x]) {
        if constexpr (PASS == 1) atomicMax(&acc->tmax[diag_group_of(WGS_SUM_GRID_MASS + (int)threadIdx.x)], s_v[threadIdx.x]);
        else atomicAdd(reinterpret_cast<unsigned long long *>(&acc->fixed[WGS_SUM_GRID_MASS + threadIdx.x]), s_v[threadIdx.x]);
    }
    if (PASS == 1 && blockIdx.x == 0 && threadIdx.x == 0) acc->grid_nodes = total;
}

template <int DIM> __global__ void k_diag_init(DiagAcc *acc) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int k = 0; k < DA_NADD; k++) acc->add[k] = 0ull;
    for (int k = 0; k < DG_COUNT; k++) { acc->tmax[k] = 0ull; acc->exponent[k] = 0; acc->scale[k] = 0.0; }
    for (int k = 0; k < WGS_NUM_SUMS; k++) acc->fixed[k] = 0ll;
    for (int k = 0; k < DM_NMAX; k++) acc->umax[k] = 0u;
    for (int k = 0; k < DN_NMIN; k++) acc->umin[k] = 0xffffffffu;
    acc->grid_nodes = 0u;
}

// (the small kernels are templates like the others: instantiations are emitted behind every kernel of the step, plain kernels in front of the
// instantiated ones — and placement moves a kernel's time: DESIGN.md 9.7)
// exponent = b + nbits(N) - 62, clamped (header); one thread per group
template <int DIM> __global__ void k_diag_scales(DiagAcc *acc) {
    const int k = (int)threadIdx.x;
    if (k >= DG_COUNT || blockIdx.x != 0) return;
    const unsigned long long count = k < DG_PARTICLE_GROUPS ? acc->add[DA_COUNT] : (unsigned long long)acc->grid_nodes;
    const int nbits = count ? 64 - __clzll((long long)count) : 0;
    int b = -200;
    if (acc->tmax[k]) (void)frexp(__longlong_as_double((long long)acc->tmax[k]), &b);
    const int e = max(-1000, min(1000, b + nbits - 62));
    acc->exponent[k] = e;
    acc->scale[k] = ldexp(1.0, -e);
}

template <int DIM> __global__ void k_diag_finish(Dev d, DiagAcc *acc, uint32_t what, wgs_diagnostics *out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    wgs_diagnostics r;
    memset(&r, 0, sizeof(r));
    r.num_particles = acc->add[DA_COUNT];
    r.num_nonfinite = acc->add[DA_NONFINITE];
    r.digest[0] = acc->add[DA_DIGEST0];   // (zero unless asked for)
    r.digest[1] = acc->add[DA_DIGEST1];
    r.what = what;
    r.model = d.pmodel[0] ? (uint32_t)WGS_MODEL_PER_PARTICLE : (uint32_t)d.model;
    for (int s = 0; s < WGS_NUM_SUMS; s++) {
        const bool asked = s < WGS_SUM_GRID_MASS ? ((what & WGS_DIAG_PARTICLES) && (s != WGS_SUM_ELASTIC || (what & WGS_DIAG_ENERGY))) : (what & WGS_DIAG_GRID) != 0u;
        if (!asked) continue;
        r.sum[s].fixed = acc->fixed[s];
        r.sum[s].exponent = acc->exponent[diag_group_of(s)];
        r.sum[s].value = ldexp((double)acc->fixed[s], acc->exponent[diag_group_of(s)]);
    }
    if (what & WGS_DIAG_PARTICLES) {
        const bool any = r.num_particles > r.num_nonfinite;
        const float inf = __uint_as_float(0x7f800000u);
        for (int k = 0; k < D; k++) {
            r.aabb_min[k] = any ? diag_unord(acc->umin[DN_AABB + k]) : inf;
            r.aabb_max[k] = any ? diag_unord(acc->umax[DM_AABB + k]) : -inf;
        }
        r.min_det_f = any ? diag_unord(acc->umin[DN_DET]) : inf;
        r.max_det_f = any ? diag_unord(acc->umax[DM_DET]) : -inf;
        r.max_speed = __uint_as_float(acc->umax[DM_SPEED]);
        r.max_affine_norm = __uint_as_float(acc->umax[DM_AFFINE]);
        r.max_wave_speed = __uint_as_float(acc->umax[DM_WAVE]);
        r.cfl = (__uint_as_float(acc->umax[DM_VINF]) * d.sp->dt) / d.h;
    }
    *out = r;
}

// the two passes over the particles under WGS_PLASTICITY_SNOW with WGS_DIAG_ENERGY (capi_plasticity.inc: kernels behind every other)
void launch_diag_pass1_snow(wgs_data *d, bool digest, dim3 blocks, DiagAcc *acc);
void launch_diag_pass2_snow(wgs_data *d, dim3 blocks, DiagAcc *acc);

// the launches of one diagnostics call, in stream order; `out` is device memory
wgs_status diag_enqueue(wgs_data *d, uint32_t what, wgs_diagnostics *out) {
    if (what == 0u || (what & ~(uint32_t)(WGS_DIAG_PARTICLES | WGS_DIAG_ENERGY | WGS_DIAG_GRID | WGS_DIAG_DIGEST)))
        return fail(WGS_ERR_INVALID_ARGUMENT, "what: an OR of WGS_DIAG_*");
    if (what & WGS_DIAG_ENERGY) what |= WGS_DIAG_PARTICLES;
    if (!d->diag_acc) WGS_TRY(dev_alloc(d, &d->diag_acc, 1));
    DiagAcc *acc = d->diag_acc;
    if (d->dev.sharded) catch_up_counters(d);   // (the particle counters of a slab live on the device, in the set of the substep's parity)
    const bool part = what & WGS_DIAG_PARTICLES, energy = what & WGS_DIAG_ENERGY, digest = what & WGS_DIAG_DIGEST, grid = what & WGS_DIAG_GRID;
    const dim3 blocks(grid_for(d, 4)), threads(256);
    const float *phase = (d->plastic || d->dev.sharded) ? nullptr : d->static_phase;
    hipLaunchKernelGGL(k_diag_init<D>, dim3(1), dim3(64), 0, d->stream, acc);
#define DIAG_PASS1(P, E, G) hipLaunchKernelGGL((k_diag_pass1<P, E, G>), blocks, threads, 0, d->stream, d->dev, d->side, d->plastic, phase, acc)
    // (the hardened coefficients enter WGS_SUM_ELASTIC alone: every other request launches what it always did)
    const bool snow = energy && d->plastic && d->plasticity == WGS_PLASTICITY_SNOW;
    if (snow) launch_diag_pass1_snow(d, digest, blocks, acc);
    else if (part && energy && digest) DIAG_PASS1(true, true, true);
    else if (part && energy) DIAG_PASS1(true, true, false);
    else if (part && digest) DIAG_PASS1(true, false, true);
    else if (part) DIAG_PASS1(true, false, false);
    else if (digest) DIAG_PASS1(false, false, true);
    else DIAG_PASS1(false, false, false);   // (the counts)
#undef DIAG_PASS1
    if (grid) hipLaunchKernelGGL(k_diag_grid<1>, blocks, threads, 0, d->stream, d->dev, acc);
    if (part || grid) hipLaunchKernelGGL(k_diag_scales<D>, dim3(1), dim3(64), 0, d->stream, acc);
    if (part) {
        if (snow) launch_diag_pass2_snow(d, blocks, acc);
        else if (energy) hipLaunchKernelGGL(k_diag_pass2<true>, blocks, threads, 0, d->stream, d->dev, d->side, acc);
        else hipLaunchKernelGGL(k_diag_pass2<false>, blocks, threads, 0, d->stream, d->dev, d->side, acc);
    }
    if (grid) hipLaunchKernelGGL(k_diag_grid<2>, blocks, threads, 0, d->stream, d->dev, acc);
    hipLaunchKernelGGL(k_diag_finish<D>, dim3(1), dim3(64), 0, d->stream, d->dev, acc, what, out);
    HIP_TRY(hipGetLastError());
    return WGS_OK;
}

}  // namespace
