// devmath_probe.hip — test-only entry points into the shipped device math (wgsparkl_amd/csrc/device_math.h): the fp32
// SVD, the two Kirchhoff stresses and the Drucker-Prager projection, one lane per matrix, so that tests can compare them
// with fp64 truth at hard deformations. Compiled by tests/test_gpu_devmath.py with the flags of csrc/build.sh (the rounding
// is the shipped rounding) and -DWGS_DIM=2 or 3. Every entry point returns 0, or the first failing hipError_t.
#include "device_math.h"

namespace {

constexpr int D = WGS_DIM;
constexpr int DD = D * D;
constexpr int WAVE = 64;   // one workgroup = one wave: the tests place matrices into waves by their index

__global__ void k_svd(const float *F, float *U, float *S, float *V, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = i < n;
    float f[DD];
    for (int k = 0; k < DD; k++) f[k] = on ? F[(size_t)i * DD + k] : 0.f;
    wgs::Svd<D> sv;
    wgs::svd<D>(f, sv);   // (every lane of the wave runs it: the sweep exit is a vote of the whole wave)
    if (!on) return;
    for (int k = 0; k < DD; k++) {
        U[(size_t)i * DD + k] = sv.u[k];
        V[(size_t)i * DD + k] = sv.v[k];
    }
    for (int k = 0; k < D; k++) S[(size_t)i * D + k] = sv.s[k];
}

// model 0: corotated (fed by wgs::svd, like the G2P), 1: neo-Hookean
__global__ void k_stress(int model, const float *lam, const float *mu, const float *F, float *tau, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = i < n;
    float f[DD], t[DD];
    for (int k = 0; k < DD; k++) f[k] = on ? F[(size_t)i * DD + k] : 0.f;
    const float l = on ? lam[i] : 0.f, m = on ? mu[i] : 0.f;
    if (model == 1) {
        wgs::kirchoff_neo_hookean<D>(l, m, f, t);
    } else {
        wgs::Svd<D> sv;
        wgs::svd<D>(f, sv);
        wgs::kirchoff_corotated<D>(l, m, f, sv, t);
    }
    if (!on) return;
    for (int k = 0; k < DD; k++) tau[(size_t)i * DD + k] = t[k];
}

__global__ void k_dp(const float *dp, const float *state, const float *F, int *changed, float *state_out, float *F_out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = i < n;
    float p[6], st[3], f[DD];
    for (int k = 0; k < 6; k++) p[k] = on ? dp[(size_t)i * 6 + k] : 0.f;
    for (int k = 0; k < 3; k++) st[k] = on ? state[(size_t)i * 3 + k] : 0.f;
    for (int k = 0; k < DD; k++) f[k] = on ? F[(size_t)i * DD + k] : 0.f;
    wgs::Svd<D> sv;
    wgs::svd<D>(f, sv);
    const bool c = wgs::drucker_prager_project<D>(p, st, f, sv);
    if (!on) return;
    changed[i] = c ? 1 : 0;
    for (int k = 0; k < 3; k++) state_out[(size_t)i * 3 + k] = st[k];
    for (int k = 0; k < DD; k++) F_out[(size_t)i * DD + k] = f[k];
}

struct Bufs {
    void *p[8] = {};
    int k = 0;
    ~Bufs() {
        for (int j = 0; j < k; j++) (void)hipFree(p[j]);
    }
    template <class T> hipError_t alloc(T **out, size_t count) {
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, count * sizeof(T) + 16);
        if (e != hipSuccess) return e;
        p[k++] = q;
        *out = static_cast<T *>(q);
        return hipSuccess;
    }
};

#define PROBE_TRY(x)                       \
    do {                                   \
        hipError_t e_ = (x);               \
        if (e_ != hipSuccess) return (int)e_; \
    } while (0)

inline unsigned grid_of(int n) { return (unsigned)((n + WAVE - 1) / WAVE); }

template <class T> int upload(Bufs &b, T **dst, const T *src, size_t count) {
    PROBE_TRY(b.alloc(dst, count));
    PROBE_TRY(hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

inline int finish() {
    PROBE_TRY(hipGetLastError());
    PROBE_TRY(hipDeviceSynchronize());
    return 0;
}

}  // namespace

extern "C" int probe_dim() { return D; }

extern "C" int probe_svd(const float *F, int n, float *U, float *S, float *V) {
    if (n <= 0) return 0;
    Bufs b;
    float *dF, *dU, *dS, *dV;
    int r;
    if ((r = upload(b, &dF, F, (size_t)n * DD))) return r;
    PROBE_TRY(b.alloc(&dU, (size_t)n * DD));
    PROBE_TRY(b.alloc(&dS, (size_t)n * D));
    PROBE_TRY(b.alloc(&dV, (size_t)n * DD));
    hipLaunchKernelGGL(k_svd, dim3(grid_of(n)), dim3(WAVE), 0, 0, dF, dU, dS, dV, n);
    if ((r = finish())) return r;
    PROBE_TRY(hipMemcpy(U, dU, (size_t)n * DD * sizeof(float), hipMemcpyDeviceToHost));
    PROBE_TRY(hipMemcpy(S, dS, (size_t)n * D * sizeof(float), hipMemcpyDeviceToHost));
    PROBE_TRY(hipMemcpy(V, dV, (size_t)n * DD * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int probe_stress(int model, const float *lam, const float *mu, const float *F, int n, float *tau) {
    if (n <= 0) return 0;
    Bufs b;
    float *dl, *dm, *dF, *dt;
    int r;
    if ((r = upload(b, &dl, lam, (size_t)n))) return r;
    if ((r = upload(b, &dm, mu, (size_t)n))) return r;
    if ((r = upload(b, &dF, F, (size_t)n * DD))) return r;
    PROBE_TRY(b.alloc(&dt, (size_t)n * DD));
    hipLaunchKernelGGL(k_stress, dim3(grid_of(n)), dim3(WAVE), 0, 0, model, dl, dm, dF, dt, n);
    if ((r = finish())) return r;
    PROBE_TRY(hipMemcpy(tau, dt, (size_t)n * DD * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int probe_dp(const float *dp, const float *state, const float *F, int n, int *changed, float *state_out, float *F_out) {
    if (n <= 0) return 0;
    Bufs b;
    float *ddp, *dst, *dF, *dso, *dFo;
    int *dc;
    int r;
    if ((r = upload(b, &ddp, dp, (size_t)n * 6))) return r;
    if ((r = upload(b, &dst, state, (size_t)n * 3))) return r;
    if ((r = upload(b, &dF, F, (size_t)n * DD))) return r;
    PROBE_TRY(b.alloc(&dc, (size_t)n));
    PROBE_TRY(b.alloc(&dso, (size_t)n * 3));
    PROBE_TRY(b.alloc(&dFo, (size_t)n * DD));
    hipLaunchKernelGGL(k_dp, dim3(grid_of(n)), dim3(WAVE), 0, 0, ddp, dst, dF, dc, dso, dFo, n);
    if ((r = finish())) return r;
    PROBE_TRY(hipMemcpy(changed, dc, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    PROBE_TRY(hipMemcpy(state_out, dso, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    PROBE_TRY(hipMemcpy(F_out, dFo, (size_t)n * DD * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}
