// vaa_patch_jitter.hip — colorjitter (K0c): a per-image photometric draw on the BASE patch and its adjoint.
//
// The reference carries a `colorjitter=` flag through TMA.py into apply_random_patch_batch and never acts on it, so
// there is no arithmetic to mirror: include/vaa.h defines it. Per image b with factors (beta, kappa, sigma), p the base patch [3,ph,pw],
// N = ph*pw and gray(y) = 0.299 y_R + 0.587 y_G + 0.114 y_B:
//     y1 = clamp(beta*p, 0, 1)                                   brightness
//     m  = sum over the texels of gray(y1) / N                   one scalar per image
//     y2 = clamp(kappa*y1 + (1-kappa)*m, 0, 1)                   contrast
//     y3 = clamp(sigma*y2 + (1-sigma)*gray(y2), 0, 1)            saturation (gray per texel)
// Every product + sum above is ONE explicit FMA on the rounded (1-kappa)*m / (1-sigma)*gray term, so factors (1, 1, 1) return p bit for bit.
// The adjoint is the exact derivative with torch.clamp's gate (the gradient passes where 0 <= pre-clamp <= 1); the gates are recomputed from the
// patch and the factors, nothing of the forward is kept.
//
// One workgroup per image. The two sums over a whole patch (m; the adjoint's sum of the gated contrast-stage gradients) are accumulated in fp64
// in a fixed order — thread t adds texels t, t + 1024, ... in sequence, a butterfly adds the lanes of a wave, the waves are added in order — so
// the same arguments give the same bits. The stage is latency, not bandwidth (a 3x100x100 patch is 120 KB and stays in L2): the texels are
// re-read per phase instead of being staged. The sum over the images is the fixed-order fp64 reduce of vaa_patch_grad.hip over per-image partials.
#include "vaa_common.h"

namespace vaa {

constexpr int kJitThreads = 1024;
constexpr int kJitWaves = kJitThreads / 64;

struct JitterArgs {
    const float* patch;    // [3,ph,pw] base patch
    const float* factors;  // [B,3] = {beta, kappa, sigma}
    const int32_t* pdesc;  // [B,4] = {ph, pw, offset, 0}
    const float* gpacked;  // bwd: d L / d packed
    float* out;            // fwd: packed; bwd: per-image base-patch gradients [B][3*ph*pw]
    unsigned* err_word;    // the library's device-failure word (a descriptor of another size is reported there)
    int B, ph, pw;
};

__device__ __forceinline__ float gray3(const float* y) { return __builtin_fmaf(0.114f, y[2], __builtin_fmaf(0.587f, y[1], 0.299f * y[0])); }
__device__ __forceinline__ float clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }  // torch.clamp: a NaN stays a NaN
__device__ __forceinline__ bool gate01(float x) { return x >= 0.0f && x <= 1.0f; }

struct Factors {
    float beta, kappa, sigma, omk, oms;  // omk = 1 - kappa, oms = 1 - sigma (fp32)
};

__device__ __forceinline__ Factors load_factors(const float* f) {
    Factors k;
    k.beta = f[0]; k.kappa = f[1]; k.sigma = f[2];
    k.omk = 1.0f - k.kappa;
    k.oms = 1.0f - k.sigma;
    return k;
}

// The pre-clamp values of the three stages of one texel (the forward's outputs are their clamps, the adjoint's gates their range tests).
struct Stages {
    float pre1[3], pre2[3], pre3[3];
};

__device__ __forceinline__ void brightness(const JitterArgs& a, int N, int t, const Factors& k, float* pre1, float* y1) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        pre1[c] = k.beta * a.patch[(size_t)c * N + t];
        y1[c] = clamp01(pre1[c]);
    }
}

__device__ __forceinline__ void stages(const JitterArgs& a, int N, int t, const Factors& k, float km, Stages& s, float* y3) {
    float y1[3], y2[3];
    brightness(a, N, t, k, s.pre1, y1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        s.pre2[c] = __builtin_fmaf(k.kappa, y1[c], km);  // km = (1-kappa)*m
        y2[c] = clamp01(s.pre2[c]);
    }
    const float sg = k.oms * gray3(y2);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        s.pre3[c] = __builtin_fmaf(k.sigma, y2[c], sg);
        y3[c] = clamp01(s.pre3[c]);
    }
}

// m of image b's factors: mean over the texels of gray(clamp(beta*p))
__device__ __forceinline__ float mean_gray(const JitterArgs& a, int N, const Factors& k, double* sl) {
    double acc = 0.0;
    for (int t = threadIdx.x; t < N; t += kJitThreads) {
        float pre1[3], y1[3];
        brightness(a, N, t, k, pre1, y1);
        acc += (double)gray3(y1);
    }
    return (float)(block_sum<kJitWaves>(acc, sl) / (double)N);
}

// image b's descriptor must state the base patch's own size (workgroup-uniform); anything else is reported and the image left alone
__device__ __forceinline__ bool desc_ok(const JitterArgs& a, int b) {
    const bool ok = a.pdesc[4 * b] == a.ph && a.pdesc[4 * b + 1] == a.pw && a.pdesc[4 * b + 2] >= 0;
    if (!ok && threadIdx.x == 0 && a.err_word)
        __hip_atomic_store(a.err_word, VAA_ASYNC_JITTER_PDESC, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return ok;
}

// grid = B: workgroup b writes image b's jittered patch [3,ph,pw] at packed + pdesc[b].offset
__global__ __launch_bounds__(kJitThreads) void patch_jitter_fwd_kernel(JitterArgs a) {
    __shared__ double sl[kJitWaves];
    const int b = blockIdx.x, N = a.ph * a.pw;
    if (!desc_ok(a, b)) return;
    const Factors k = load_factors(a.factors + 3 * b);
    const float km = k.omk * mean_gray(a, N, k, sl);
    float* dst = a.out + a.pdesc[4 * b + 2];
    for (int t = threadIdx.x; t < N; t += kJitThreads) {
        Stages s;
        float y3[3];
        stages(a, N, t, k, km, s, y3);
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[(size_t)c * N + t] = y3[c];
    }
}

// The gated gradient in front of the contrast stage's clamp (G2' of vaa.h) of one texel, from the upstream gradient g3 of its three channels:
// saturation stage backwards (its clamp's gate, then sigma*G + (1-sigma)*w_c * sum over the channels), then the contrast stage's gate.
__device__ __forceinline__ void contrast_grad(const Factors& k, const Stages& s, const float* g3, float* g2) {
    float g3g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) g3g[c] = gate01(s.pre3[c]) ? g3[c] : 0.0f;
    const float sum3 = (g3g[0] + g3g[1]) + g3g[2];
    const float wc[3] = {0.299f, 0.587f, 0.114f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float g = __builtin_fmaf(k.sigma, g3g[c], (k.oms * wc[c]) * sum3);
        g2[c] = gate01(s.pre2[c]) ? g : 0.0f;
    }
}

// grid = B: workgroup b writes adjoint_b(gpacked_b) [3,ph,pw] at out + b*3*ph*pw
__global__ __launch_bounds__(kJitThreads) void patch_jitter_bwd_kernel(JitterArgs a) {
    __shared__ double sl[kJitWaves];
    const int b = blockIdx.x, N = a.ph * a.pw;
    float* dst = a.out + (size_t)b * 3 * N;
    if (!desc_ok(a, b)) {  // the reduce reads every image's partial
        for (int e = threadIdx.x; e < 3 * N; e += kJitThreads) dst[e] = 0.0f;
        return;
    }
    const Factors k = load_factors(a.factors + 3 * b);
    const float km = k.omk * mean_gray(a, N, k, sl);
    const float* g = a.gpacked + a.pdesc[4 * b + 2];
    // the whole-patch term of the contrast stage: every texel's m depends on every texel's y1
    double acc = 0.0;
    for (int t = threadIdx.x; t < N; t += kJitThreads) {
        Stages s;
        float y3[3], g3[3], g2[3];
        stages(a, N, t, k, km, s, y3);
#pragma unroll
        for (int c = 0; c < 3; ++c) g3[c] = g[(size_t)c * N + t];
        contrast_grad(k, s, g3, g2);
        acc += (double)((g2[0] + g2[1]) + g2[2]);
    }
    const float gmean = (float)(block_sum<kJitWaves>(acc, sl) / (double)N);
    const float wc[3] = {0.299f, 0.587f, 0.114f};
    for (int t = threadIdx.x; t < N; t += kJitThreads) {
        Stages s;
        float y3[3], g3[3], g2[3];
        stages(a, N, t, k, km, s, y3);
#pragma unroll
        for (int c = 0; c < 3; ++c) g3[c] = g[(size_t)c * N + t];
        contrast_grad(k, s, g3, g2);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float g1 = __builtin_fmaf(k.kappa, g2[c], (k.omk * wc[c]) * gmean);
            dst[(size_t)c * N + t] = gate01(s.pre1[c]) ? k.beta * g1 : 0.0f;
        }
    }
}

}  // namespace vaa

extern "C" int vaa_patch_jitter_fwd(const float* patch, int ph, int pw, const float* factors, const int32_t* pdesc, int B, float* packed,
                                    void* stream) {
    using namespace vaa;
    if (B == 0) return VAA_OK;
    int rc = check_patch_stage("vaa_patch_jitter_fwd", {patch, factors, pdesc, packed}, B, ph, pw, /*frame_bound=*/true);
    if (rc != VAA_OK) return rc;
    const JitterArgs a{patch, factors, pdesc, nullptr, packed, async_error_word(), B, ph, pw};
    VAA_LAUNCH(patch_jitter_fwd_kernel, dim3(B), dim3(kJitThreads), 0, (hipStream_t)stream, a);
    return check_launch("vaa_patch_jitter_fwd");
}

extern "C" size_t vaa_patch_jitter_ws_bytes(int B, int ph, int pw) {
    return (B <= 0 || ph <= 0 || pw <= 0) ? 0 : vaa::patch_stage_ws_bytes(B, ph, pw);  // one partial per image; a single image writes gpatch itself
}

extern "C" int vaa_patch_jitter_bwd(const float* gpacked, const float* patch, int ph, int pw, const float* factors, const int32_t* pdesc, int B,
                                    float* gpatch, void* ws, size_t ws_bytes, void* stream) {
    using namespace vaa;
    hipStream_t st = (hipStream_t)stream;
    return patch_stage_bwd("vaa_patch_jitter_bwd", {gpacked, patch, factors, pdesc, gpatch}, B, ph, pw, /*frame_bound=*/true, /*empty_ok=*/true,
                           /*parts=*/B, gpatch, ws, ws_bytes, st, [&](float* out) {
        const JitterArgs a{patch, factors, pdesc, gpacked, out, async_error_word(), B, ph, pw};
        VAA_LAUNCH(patch_jitter_bwd_kernel, dim3(B), dim3(kJitThreads), 0, st, a);
    });
}
