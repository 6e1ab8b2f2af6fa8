// vaa_patch_reg.hip — K6: the smoothness (total variation) and printability (non-printability score) terms of the patch, values + gradient in
// ONE launch.
//
// The reference has no such term (Thys et al.'s adversarial-patch code and Sharif et al.'s NPS are where they come from), so there is no
// arithmetic to mirror: include/vaa.h defines it. With p the patch [3,ph,pw], N = ph*pw, N3 = 3*N, q the palette [K,3] and eps = 1e-6:
//     TV(p)  = ( sum of |p[c,i,j+1] - p[c,i,j]| + sum of |p[c,i+1,j] - p[c,i,j]| ) / N3
//     d_k(t) = sqrt( sum_c (p[c,t] - q[k,c])^2 + eps ),   NPS(p) = ( sum_t min_k d_k(t) ) / N3
// and the gradient of w_tv*TV + w_nps*NPS, which needs a texel's four neighbours and the palette only — no cross-texel reduction.
//
// One thread per texel (its three channels), 256 texels per workgroup, the palette (at most 768 B) staged in LDS once per workgroup and read
// from there by every lane at the same address (a broadcast): a 3x50x50 patch is 10 workgroups, 3x100x100 is 40, instead of one workgroup
// looping 64 colours over every texel. The two values leave the launch as per-workgroup fp64 partial sums in a fixed order (thread order, the
// butterfly of a wave, the waves in order: block_sum); the host side folds them on demand. No atomics, nothing handed over between workgroups.
#include "vaa_common.h"

namespace vaa {

constexpr int kRegThreads = 256;
constexpr int kRegWaves = kRegThreads / 64;
constexpr int kRegMaxColours = 64;

struct RegArgs {
    const float* patch;    // [3,ph,pw]
    const float* palette;  // [K,3] or NULL (K = 0)
    float* grad;           // [3,ph,pw] or NULL (values only)
    double* part;          // [blocks][2] = {sum of the right / down |differences| of the block's texels, sum of their min distances}
    int ph, pw, K, accumulate;
    float c_tv, c_nps;     // w_tv / N3, w_nps / N3 (rounded from double on the host)
};

__device__ __forceinline__ float sgn(float d) { return (float)((d > 0.0f) - (d < 0.0f)); }  // torch.abs's rule: sgn(0) = 0 (and sgn(NaN) = 0)

__global__ __launch_bounds__(kRegThreads) void patch_reg_kernel(RegArgs a) {
    __shared__ float pal[kRegMaxColours * 3];
    __shared__ double sl[kRegWaves];
    const int N = a.ph * a.pw;
    const int t = blockIdx.x * kRegThreads + threadIdx.x;
    const bool nps = a.palette != nullptr && a.K > 0;
    if (nps) {
        if ((int)threadIdx.x < 3 * a.K) pal[threadIdx.x] = a.palette[threadIdx.x];
        __syncthreads();
    }
    double tv_acc = 0.0, nps_acc = 0.0;
    if (t < N) {
        const int i = t / a.pw, j = t - i * a.pw;
        const bool has_r = j + 1 < a.pw, has_d = i + 1 < a.ph, has_l = j > 0, has_u = i > 0;
        const bool tv_grad = a.grad != nullptr && a.c_tv != 0.0f;
        float p[3], s[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* pc = a.patch + (size_t)c * N;
            p[c] = pc[t];
            // the differences this texel owns: towards its right and its lower neighbour
            const float dr = has_r ? pc[t + 1] - p[c] : 0.0f;
            const float dd = has_d ? pc[t + a.pw] - p[c] : 0.0f;
            tv_acc += (double)fabsf(dr);
            tv_acc += (double)fabsf(dd);
            if (tv_grad) {
                const float dl = has_l ? p[c] - pc[t - 1] : 0.0f;
                const float du = has_u ? p[c] - pc[t - a.pw] : 0.0f;
                s[c] = ((sgn(dl) - sgn(dr)) + sgn(du)) - sgn(dd);  // small integers: exact
            }
        }
        float e[3] = {0.0f, 0.0f, 0.0f}, best = 0.0f;
        if (nps) {
            for (int k = 0; k < a.K; ++k) {
                const float e0 = p[0] - pal[3 * k], e1 = p[1] - pal[3 * k + 1], e2 = p[2] - pal[3 * k + 2];
                const float d = sqrtf(__builtin_fmaf(e2, e2, __builtin_fmaf(e1, e1, e0 * e0)) + 1e-6f);
                // the lowest index attaining the minimum; a NaN distance is taken and, once taken, kept (no comparison drops it)
                if (k == 0 || d < best || d != d) {
                    best = d;
                    e[0] = e0; e[1] = e1; e[2] = e2;
                }
            }
            nps_acc = (double)best;
        }
        if (a.grad != nullptr) {
            const bool nps_grad = nps && a.c_nps != 0.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float r;
                if (tv_grad && nps_grad) r = __builtin_fmaf(a.c_tv, s[c], a.c_nps * (e[c] / best));
                else if (nps_grad) r = a.c_nps * (e[c] / best);
                else r = a.c_tv * s[c];
                float* g = a.grad + (size_t)c * N + t;
                *g = a.accumulate ? *g + r : r;
            }
        }
    }
    const double tv_sum = block_sum<kRegWaves>(tv_acc, sl);
    const double nps_sum = block_sum<kRegWaves>(nps_acc, sl);
    if (threadIdx.x == 0) {
        a.part[2 * blockIdx.x] = tv_sum;
        a.part[2 * blockIdx.x + 1] = nps_sum;
    }
}

}  // namespace vaa

extern "C" size_t vaa_patch_reg_parts(int ph, int pw) {
    if (ph <= 0 || pw <= 0) return 0;
    return ((size_t)ph * pw + vaa::kRegThreads - 1) / vaa::kRegThreads;
}

extern "C" int vaa_patch_reg(const float* patch, int ph, int pw, const float* palette, int K, float w_tv, float w_nps, float* grad, int accumulate,
                             double* part, void* stream) {
    using namespace vaa;
    if (!patch || !part) {
        set_error("vaa_patch_reg: null pointer argument");
        return VAA_E_INVALID;
    }
    if (!isfinite(w_tv) || !isfinite(w_nps)) {
        set_error("vaa_patch_reg: the weights must be finite (w_tv=%g w_nps=%g)", (double)w_tv, (double)w_nps);
        return VAA_E_INVALID;
    }
    if (K < 0 || K > kRegMaxColours) {
        set_error("vaa_patch_reg: a palette holds 1..%d colours, got K=%d", kRegMaxColours, K);
        return VAA_E_INVALID;
    }
    if (w_nps != 0.0f && (K < 1 || !palette)) {
        set_error("vaa_patch_reg: w_nps=%g needs a palette of at least one colour (K=%d)", (double)w_nps, K);
        return VAA_E_INVALID;
    }
    int rc = check_patch_size("vaa_patch_reg", 1, ph, pw);
    if (rc != VAA_OK) return rc;
    const double n3 = 3.0 * ph * pw;
    RegArgs a;
    a.patch = patch; a.palette = K > 0 ? palette : nullptr; a.grad = grad; a.part = part;
    a.ph = ph; a.pw = pw; a.K = K; a.accumulate = accumulate;
    a.c_tv = (float)((double)w_tv / n3);
    a.c_nps = (float)((double)w_nps / n3);
    VAA_LAUNCH(patch_reg_kernel, dim3((unsigned)vaa_patch_reg_parts(ph, pw)), dim3(kRegThreads), 0, (hipStream_t)stream, a);
    return check_launch("vaa_patch_reg");
}
