// vaa_scene_jitter.hip — K10: scene-lighting jitter of the pasted frame (brightness, contrast, saturation, hue of K1 / K9's planar pixel values,
// bf16 [B,6,224,224], one factor row per image) and its adjoint.
//
// The photometric half of OpenVLA's `image_aug` (prismatic/vla/datasets/datasets.py:126-138), applied to the whole frame behind the crop (K9).
// include/vaa.h states the arithmetic; every a*x + c below is ONE explicit FMA on a rounded c (the library is built with -ffp-contract=off), so
// the identity factors pass every value of [0, 1] through the four stages unchanged. The two towers' planes (channels 0-2, 3-5) are two
// independent RGB images with the same factors.
//
// One image-tower is 3 planes x 50,176 bf16 = 301 KB, and each direction needs one sum over a whole plane before any element can be written
// (the contrast mean; the adjoint's sum of the gated contrast-stage gradients). A workgroup per image-tower would leave most of 256 CUs idle, so
// an image-tower is cut into kSjParts parts of kSjThreads x 8 consecutive elements and every direction is a statistics launch followed by an
// apply launch:
//   * statistics: workgroup (image-tower, part) adds its share of the three per-channel sums — 8 elements in ascending order per thread, a
//     butterfly inside a wave, the waves in order, all in fp64 (block_sum) — and writes three doubles to the workspace.
//   * apply: every workgroup folds the kSjParts partials of its image-tower in ascending order (the same bits in every workgroup), divides by N
//     and rounds once to fp32, then recomputes the stages of its own elements.
// No atomics, no workgroup waits for another, an image's partials depend on that image alone: same arguments, same bits, whatever the batch.
// A thread owns 8 consecutive elements of the three planes of its tower: one 16-byte load per plane and tensor, one 16-byte store per plane;
// consecutive lanes own consecutive runs. kSjParts x kSjThreads x 8 is exactly one plane: no tail, every element is written, nothing is
// addressed beyond [B,6,224,224]. No index depends on the factors: a device copy that differs from the validated host copy changes values only.
// The adjoint keeps nothing of the forward: it recomputes the means (one more statistics launch) and the gates from x and the factors.
#include "vaa_common.h"

#pragma clang fp contract(off)

namespace vaa {

constexpr int kSjPix = 8;                                   // elements per thread and plane (one 16-byte vector)
constexpr int kSjWaves = 7;
constexpr int kSjThreads = 64 * kSjWaves;                   // 448
constexpr int kSjParts = 14;                                // workgroups per image-tower
constexpr int kSjMaxB = 0x7fffffff / (2 * kSjParts);        // the grid is B * 2 * kSjParts workgroups
static_assert(kSjParts * kSjThreads * kSjPix == VAA_NPIX, "the parts tile one plane exactly");

struct SceneArgs {
    const uint16_t* x;      // [B,6,224,224]
    const uint16_t* gout;   // adjoint: d L / d out
    uint16_t* out;          // forward: out; adjoint: gx
    const float* factors;   // dev [B,12] {delta, kappa, sigma, R[3][3] row-major}
    double* msum;           // [B*2][kSjParts][3] partial sums of y1
    double* gsum;           // [B*2][kSjParts][3] partial sums of G2' (adjoint)
    Norm6 nrm;
    float istd[6];
    int B;
};

struct SceneF {
    float delta, kappa, sigma, omk, oms;  // omk = 1 - kappa, oms = 1 - sigma (fp32)
    float R[3][3];
};

__device__ __forceinline__ SceneF load_scene(const float* f) {
    const float4 a = *reinterpret_cast<const float4*>(f), b = *reinterpret_cast<const float4*>(f + 4), c = *reinterpret_cast<const float4*>(f + 8);
    SceneF k;
    k.delta = a.x; k.kappa = a.y; k.sigma = a.z;
    k.omk = 1.0f - k.kappa;
    k.oms = 1.0f - k.sigma;
    k.R[0][0] = a.w; k.R[0][1] = b.x; k.R[0][2] = b.y;
    k.R[1][0] = b.z; k.R[1][1] = b.w; k.R[1][2] = c.x;
    k.R[2][0] = c.y; k.R[2][1] = c.z; k.R[2][2] = c.w;
    return k;
}

__device__ __forceinline__ float sj_clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }  // torch.clamp: a NaN stays a NaN
__device__ __forceinline__ bool sj_gate01(float x) { return x >= 0.0f && x <= 1.0f; }                     // false for a NaN
__device__ __forceinline__ float sj_gray(const float* y) { return __builtin_fmaf(0.114f, y[2], __builtin_fmaf(0.587f, y[1], 0.299f * y[0])); }

// where a workgroup stands: image-tower `it` = 2*b + tower, part, and the offset of this thread's run inside a plane
struct ScenePos {
    int it, b, tw, part;
    size_t base;  // element offset of the run in the tower's first plane
};

__device__ __forceinline__ ScenePos scene_pos() {
    ScenePos p;
    p.it = (int)(blockIdx.x / kSjParts);
    p.part = (int)(blockIdx.x - (unsigned)p.it * kSjParts);
    p.b = p.it >> 1;
    p.tw = p.it & 1;
    p.base = ((size_t)p.b * 6 + 3 * (size_t)p.tw) * VAA_NPIX + ((size_t)p.part * kSjThreads + threadIdx.x) * kSjPix;
    return p;
}

// the three planes' runs of one tensor, widened to fp32: v[c][i]
__device__ __forceinline__ void load_run(const uint16_t* t, size_t base, float (*v)[kSjPix]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint4 d = *reinterpret_cast<const uint4*>(t + base + (size_t)c * VAA_NPIX);
        const uint32_t w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[c][2 * i] = __uint_as_float(w[i] << 16);
            v[c][2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
        }
    }
}

__device__ __forceinline__ void store_run(uint16_t* t, size_t base, const float (*v)[kSjPix]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        uint32_t q[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = f32_to_bf16_bits(v[c][2 * i]) | (f32_to_bf16_bits(v[c][2 * i + 1]) << 16);
        *reinterpret_cast<uint4*>(t + base + (size_t)c * VAA_NPIX) = make_uint4(q[0], q[1], q[2], q[3]);
    }
}

// brightness stage of one element: pre1 = (x*std + mean) + delta
__device__ __forceinline__ float scene_pre1(float x, float mean, float stdv, float delta) { return __builtin_fmaf(x, stdv, mean) + delta; }

// The pre-clamp values of the four stages of one pixel of one tower (the forward's output is the last one's clamp, the adjoint's gates their
// range tests). km[c] = (1 - kappa)*m_c.
struct SceneStages {
    float pre1[3], pre2[3], pre3[3], pre4[3];
};

__device__ __forceinline__ void scene_stages(const float* x, const float* mean, const float* stdv, const SceneF& k, const float* km, SceneStages& s) {
    float y2[3], y3[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        s.pre1[c] = scene_pre1(x[c], mean[c], stdv[c], k.delta);
        s.pre2[c] = __builtin_fmaf(k.kappa, sj_clamp01(s.pre1[c]), km[c]);
        y2[c] = sj_clamp01(s.pre2[c]);
    }
    const float sg = k.oms * sj_gray(y2);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        s.pre3[c] = __builtin_fmaf(k.sigma, y2[c], sg);
        y3[c] = sj_clamp01(s.pre3[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) s.pre4[c] = __builtin_fmaf(k.R[c][2], y3[2], __builtin_fmaf(k.R[c][1], y3[1], k.R[c][0] * y3[0]));
}

// The gated gradient in front of the contrast stage's clamp (G2' of vaa.h) of one pixel from the upstream gradient g of its three channels:
// normalisation, hue stage (its gate, the transposed matrix), saturation stage (its gate, sigma*G + (1-sigma)*w_c * sum), the contrast gate.
__device__ __forceinline__ void scene_contrast_grad(const SceneF& k, const SceneStages& s, const float* g, const float* istd, float* g2) {
    float g4[3], g3[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) g4[c] = sj_gate01(s.pre4[c]) ? g[c] * istd[c] : 0.0f;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float t = __builtin_fmaf(k.R[2][d], g4[2], __builtin_fmaf(k.R[1][d], g4[1], k.R[0][d] * g4[0]));
        g3[d] = sj_gate01(s.pre3[d]) ? t : 0.0f;
    }
    const float sum3 = (g3[0] + g3[1]) + g3[2];
    const float wc[3] = {0.299f, 0.587f, 0.114f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t = __builtin_fmaf(k.sigma, g3[c], (k.oms * wc[c]) * sum3);
        g2[c] = sj_gate01(s.pre2[c]) ? t : 0.0f;
    }
}

// the kSjParts partials of image-tower `it` in ascending order, divided by N, rounded once: the same bits in every workgroup that folds them
__device__ __forceinline__ void fold_parts(const double* parts, int it, float* m) {
    const double* p = parts + (size_t)it * kSjParts * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < kSjParts; ++q) t += p[3 * q + c];
        m[c] = (float)(t / (double)VAA_NPIX);
    }
}

// grid = B*2*kSjParts: workgroup (it, part) writes msum[it][part][c] = its share of sum over the pixels of y1_c
__global__ __launch_bounds__(kSjThreads) void scene_mean_kernel(const SceneArgs a) {
    __shared__ double sl[kSjWaves];
    const ScenePos p = scene_pos();
    const float delta = a.factors[12 * (size_t)p.b];
    float x[3][kSjPix];
    load_run(a.x, p.base, x);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float mean = a.nrm.mean[3 * p.tw + c], stdv = a.nrm.stdv[3 * p.tw + c];
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < kSjPix; ++i) acc += (double)sj_clamp01(scene_pre1(x[c][i], mean, stdv, delta));
        const double t = block_sum<kSjWaves>(acc, sl);
        if (threadIdx.x == 0) a.msum[((size_t)p.it * kSjParts + p.part) * 3 + c] = t;
    }
}

__global__ __launch_bounds__(kSjThreads) void scene_jitter_fwd_kernel(const SceneArgs a) {
    const ScenePos p = scene_pos();
    const SceneF k = load_scene(a.factors + 12 * (size_t)p.b);
    float mean[3], stdv[3], km[3];
    fold_parts(a.msum, p.it, km);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mean[c] = a.nrm.mean[3 * p.tw + c];
        stdv[c] = a.nrm.stdv[3 * p.tw + c];
        km[c] = k.omk * km[c];
    }
    float x[3][kSjPix];
    load_run(a.x, p.base, x);
#pragma unroll
    for (int i = 0; i < kSjPix; ++i) {
        const float xi[3] = {x[0][i], x[1][i], x[2][i]};
        SceneStages s;
        scene_stages(xi, mean, stdv, k, km, s);
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c][i] = (sj_clamp01(s.pre4[c]) - mean[c]) / stdv[c];
    }
    store_run(a.out, p.base, x);
}

// grid = B*2*kSjParts: workgroup (it, part) writes gsum[it][part][c] = its share of sum over the pixels of G2'_c
__global__ __launch_bounds__(kSjThreads) void scene_gsum_kernel(const SceneArgs a) {
    __shared__ double sl[kSjWaves];
    const ScenePos p = scene_pos();
    const SceneF k = load_scene(a.factors + 12 * (size_t)p.b);
    float mean[3], stdv[3], istd[3], km[3];
    fold_parts(a.msum, p.it, km);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mean[c] = a.nrm.mean[3 * p.tw + c];
        stdv[c] = a.nrm.stdv[3 * p.tw + c];
        istd[c] = a.istd[3 * p.tw + c];
        km[c] = k.omk * km[c];
    }
    float x[3][kSjPix], g[3][kSjPix];
    load_run(a.x, p.base, x);
    load_run(a.gout, p.base, g);
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < kSjPix; ++i) {
        const float xi[3] = {x[0][i], x[1][i], x[2][i]}, gi[3] = {g[0][i], g[1][i], g[2][i]};
        SceneStages s;
        float g2[3];
        scene_stages(xi, mean, stdv, k, km, s);
        scene_contrast_grad(k, s, gi, istd, g2);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += (double)g2[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double t = block_sum<kSjWaves>(acc[c], sl);
        if (threadIdx.x == 0) a.gsum[((size_t)p.it * kSjParts + p.part) * 3 + c] = t;
    }
}

__global__ __launch_bounds__(kSjThreads) void scene_jitter_bwd_kernel(const SceneArgs a) {
    const ScenePos p = scene_pos();
    const SceneF k = load_scene(a.factors + 12 * (size_t)p.b);
    float mean[3], stdv[3], istd[3], km[3], kg[3];
    fold_parts(a.msum, p.it, km);
    fold_parts(a.gsum, p.it, kg);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mean[c] = a.nrm.mean[3 * p.tw + c];
        stdv[c] = a.nrm.stdv[3 * p.tw + c];
        istd[c] = a.istd[3 * p.tw + c];
        km[c] = k.omk * km[c];
        kg[c] = k.omk * kg[c];  // the whole-image term of the contrast mean: every pixel's m_c depends on every pixel's y1_c
    }
    float x[3][kSjPix], g[3][kSjPix];
    load_run(a.x, p.base, x);
    load_run(a.gout, p.base, g);
#pragma unroll
    for (int i = 0; i < kSjPix; ++i) {
        const float xi[3] = {x[0][i], x[1][i], x[2][i]}, gi[3] = {g[0][i], g[1][i], g[2][i]};
        SceneStages s;
        float g2[3];
        scene_stages(xi, mean, stdv, k, km, s);
        scene_contrast_grad(k, s, gi, istd, g2);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float g1 = __builtin_fmaf(k.kappa, g2[c], kg[c]);
            x[c][i] = sj_gate01(s.pre1[c]) ? g1 * stdv[c] : 0.0f;
        }
    }
    store_run(a.out, p.base, x);
}

static int check_scene_call(const char* who, const void* t0, const void* t1, const float* factors_host, const float* factors_dev, const float* mean6,
                            const float* std6, int B, const void* t_out, const void* ws, size_t ws_bytes) {
    const int rc = check_stage_call(who, B, kSjMaxB, "", {t0, t1, t_out, factors_dev}, {factors_host, mean6, std6}, "factors_dev");
    if (rc != VAA_OK || B == 0) return rc;
    for (int q = 0; q < 6; ++q)
        if (!(isfinite(mean6[q]) && isfinite(std6[q]) && std6[q] > 0.0f)) {
            set_error("%s: channel %d has mean = %g, std = %g: need finite values and std > 0", who, q, (double)mean6[q], (double)std6[q]);
            return VAA_E_INVALID;
        }
    for (int b = 0; b < B; ++b) {
        const float* f = factors_host + 12 * (size_t)b;
        for (int q = 0; q < 12; ++q)
            if (!isfinite(f[q])) {
                set_error("%s: factor %d of image %d is not finite", who, q, b);
                return VAA_E_INVALID;
            }
        if (f[1] < 0.0f || f[2] < 0.0f) {
            set_error("%s: image %d has kappa = %g, sigma = %g: need kappa >= 0 and sigma >= 0", who, b, (double)f[1], (double)f[2]);
            return VAA_E_INVALID;
        }
    }
    const size_t need = vaa_scene_jitter_ws_bytes(B);
    if (!ws || ws_bytes < need || ((uintptr_t)ws & 7u)) {
        set_error("%s: workspace %zu B < required %zu B (or missing, or not 8-byte aligned)", who, ws ? ws_bytes : (size_t)0, need);
        return VAA_E_WORKSPACE;
    }
    return VAA_OK;
}

static SceneArgs scene_args(const uint16_t* x, const uint16_t* gout, uint16_t* out, const float* factors_dev, const float* mean6, const float* std6, int B,
                            void* ws) {
    SceneArgs a;
    a.x = x; a.gout = gout; a.out = out; a.factors = factors_dev; a.B = B;
    a.msum = (double*)ws;
    a.gsum = a.msum + (size_t)B * 2 * kSjParts * 3;
    for (int q = 0; q < 6; ++q) {
        a.nrm.mean[q] = mean6[q];
        a.nrm.stdv[q] = std6[q];
    }
    inv_std6(std6, a.istd);
    return a;
}

}  // namespace vaa

extern "C" size_t vaa_scene_jitter_ws_bytes(int B) {
    if (B <= 0 || B > vaa::kSjMaxB) return 0;
    return (size_t)B * 2 * vaa::kSjParts * 3 * sizeof(double) * 2;  // the partials of the means, then those of the adjoint's sums
}

extern "C" int vaa_scene_jitter_fwd(const uint16_t* x_bf16, const float* factors_host, const float* factors_dev, const float* mean6, const float* std6,
                                    int B, uint16_t* out_bf16, void* ws, size_t ws_bytes, void* stream) {
    using namespace vaa;
    const char* who = "vaa_scene_jitter_fwd";
    int rc = check_scene_call(who, x_bf16, x_bf16, factors_host, factors_dev, mean6, std6, B, out_bf16, ws, ws_bytes);
    if (rc != VAA_OK || B == 0) return rc;
    const SceneArgs a = scene_args(x_bf16, nullptr, out_bf16, factors_dev, mean6, std6, B, ws);
    const dim3 grid((unsigned)(B * 2 * kSjParts));
    VAA_LAUNCH(scene_mean_kernel, grid, dim3(kSjThreads), 0, (hipStream_t)stream, a);
    rc = check_launch("vaa_scene_jitter_fwd(mean)");
    if (rc != VAA_OK) return rc;
    VAA_LAUNCH(scene_jitter_fwd_kernel, grid, dim3(kSjThreads), 0, (hipStream_t)stream, a);
    return check_launch(who);
}

extern "C" int vaa_scene_jitter_bwd(const uint16_t* gout_bf16, const uint16_t* x_bf16, const float* factors_host, const float* factors_dev,
                                    const float* mean6, const float* std6, int B, uint16_t* gx_bf16, void* ws, size_t ws_bytes, void* stream) {
    using namespace vaa;
    const char* who = "vaa_scene_jitter_bwd";
    int rc = check_scene_call(who, gout_bf16, x_bf16, factors_host, factors_dev, mean6, std6, B, gx_bf16, ws, ws_bytes);
    if (rc != VAA_OK || B == 0) return rc;
    const SceneArgs a = scene_args(x_bf16, gout_bf16, gx_bf16, factors_dev, mean6, std6, B, ws);
    const dim3 grid((unsigned)(B * 2 * kSjParts));
    VAA_LAUNCH(scene_mean_kernel, grid, dim3(kSjThreads), 0, (hipStream_t)stream, a);
    rc = check_launch("vaa_scene_jitter_bwd(mean)");
    if (rc != VAA_OK) return rc;
    VAA_LAUNCH(scene_gsum_kernel, grid, dim3(kSjThreads), 0, (hipStream_t)stream, a);
    rc = check_launch("vaa_scene_jitter_bwd(sum)");
    if (rc != VAA_OK) return rc;
    VAA_LAUNCH(scene_jitter_bwd_kernel, grid, dim3(kSjThreads), 0, (hipStream_t)stream, a);
    return check_launch(who);
}
