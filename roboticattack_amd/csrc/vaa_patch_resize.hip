// vaa_patch_resize.hip — resize_patch=True (BASELINE config 5): the per-image rescaling of the BASE patch and its adjoint.
//
// Replaces `patch = transforms.Resize((height, width))(patch)` of RandomPatchTransform.apply_random_patch_batch
// (appply_random_transform.py:113-116, semantics of SURVEY.md Appendix A-D2: every image scales the base patch) and its
// autograd backward. torchvision's Resize on a tensor is torch's antialiased bilinear interpolation
// (F.interpolate(mode='bilinear', antialias=True, align_corners=False)); the arithmetic below follows torch's CPU kernel
// (ATen UpSampleKernel.cpp: _compute_indices_min_size_weights_aa, horizontal pass then vertical pass, each output
// src[0]*w[0] followed by fma(src[j], w[j], acc)) operation for operation, so the forward is BIT-EXACT against it
// (tests/test_oracle_golden.py pins the C restatement, tests/test_gpu_kernels.py this kernel).
//
// One launch resizes the base patch for the whole batch into a packed buffer (image b: [3,h_b,w_b] at pdesc[b].offset);
// one launch + the fixed-order reduce of vaa_patch_grad.hip produce the adjoint. Launch counts do not depend on B.
// The horizontal intermediate is recomputed per output element instead of being staged (a 139x139 plane is 25 taps per
// element): the values are the same fp32 numbers torch stores in its temporary, so the result is unchanged.
//
// Each kernel's arithmetic is written ONCE, over a weight source that answers "first tap, tap count, weight j" for an output index: TableTaps
// reads the per-image tables in LDS, DirectTaps evaluates make_taps / tap_weight. The tables hold tap_weight's own fp32 values: same bits.
#include "vaa_common.h"

namespace vaa {

struct Axis {
    float scale, support, invscale;
    int max_interp, in_size;
};

__device__ __forceinline__ Axis make_axis(int in_size, int out_size) {
    Axis ax;
    ax.in_size = in_size;
    ax.scale = (float)in_size / (float)out_size;  // area_pixel_compute_scale (align_corners=False, no scale_factor)
    ax.support = (ax.scale >= 1.0f) ? ax.scale : 1.0f;
    ax.invscale = (ax.scale >= 1.0f) ? (float)(1.0 / (double)ax.scale) : 1.0f;
    ax.max_interp = (int)ceilf(ax.support) * 2 + 1;
    return ax;
}

struct Taps {
    int lo, n;
    float center, total;
};

__device__ __forceinline__ float raw_weight(const Axis& ax, const Taps& t, int j) {  // HelperInterpLinear::aa_filter
    float x = (float)(((double)((float)(j + t.lo) - t.center) + 0.5) * (double)ax.invscale);
    x = fabsf(x);
    return (x < 1.0f) ? (float)(1.0 - (double)x) : 0.0f;
}

__device__ __forceinline__ Taps make_taps(const Axis& ax, int i) {
    Taps t;
    t.center = (float)((double)ax.scale * ((double)i + 0.5));
    long lo = (long)((double)(t.center - ax.support) + 0.5);
    lo = lo < 0 ? 0 : lo;
    long hi = (long)((double)(t.center + ax.support) + 0.5);
    hi = hi > ax.in_size ? ax.in_size : hi;
    long n = hi - lo;
    n = n < 0 ? 0 : (n > ax.max_interp ? ax.max_interp : n);
    t.lo = (int)lo;
    t.n = (int)n;
    t.total = 0.0f;
    for (int j = 0; j < t.n; ++j) t.total += raw_weight(ax, t, j);
    return t;
}

__device__ __forceinline__ float tap_weight(const Axis& ax, const Taps& t, int j) {
    const float w = raw_weight(ax, t, j);
    return (t.total != 0.0f) ? w / t.total : w;
}

struct ResizeArgs {
    const float* in;       // fwd: [3,ph,pw] base patch; bwd: d L / d packed
    const int32_t* pdesc;  // [B,4] = {h, w, offset, 0}
    float* out;            // fwd: packed; bwd: per-image base-patch gradients [B][3*ph*pw]
    int B, ph, pw;
};

constexpr int kTapMax = 8;
constexpr int kResizeWgs = 8192;
// images a workgroup walks in sequence: 1 while the batch is small (all images in parallel, the fixed-order reduce adds them), more once
// the grid alone fills the chip (fewer partials)
static int resize_group(int B, int ph, int pw) {
    const long wgs_per_image = 3l * (((long)ph * pw + 255) / 256);
    long g = (long)B * wgs_per_image / kResizeWgs;
    return (int)(g < 1 ? 1 : (g > 8 ? 8 : g));
}
constexpr int kMaxCand = 12;

struct TapTab {
    float w[2][VAA_IMG][kTapMax];  // [axis: 0 = y, 1 = x][output position][tap]
    short lo[2][VAA_IMG], n[2][VAA_IMG];
};

// The two weight sources. at(axis, o): the taps of output index o along axis 0 = y / 1 = x, as {lo, n, w(j)}.
struct DirectTaps {
    static constexpr bool kTabled = false;
    Axis ay, ax;
    struct Out : Taps {
        Axis a;
        __device__ __forceinline__ float w(int j) const { return tap_weight(a, *this, j); }
    };
    __device__ __forceinline__ Out at(int axis, int o) const {
        Out r;
        r.a = axis == 0 ? ay : ax;
        static_cast<Taps&>(r) = make_taps(r.a, o);
        return r;
    }
};
struct TableTaps {
    static constexpr bool kTabled = true;
    const TapTab* tab;
    struct Out {
        int lo, n;
        const float* wt;
        __device__ __forceinline__ float w(int j) const { return wt[j]; }
    };
    __device__ __forceinline__ Out at(int axis, int o) const { return {tab->lo[axis][o], tab->n[axis][o], tab->w[axis][o]}; }
};

// taps of up to kTapMax entries (down-scaling by up to 3x) of an image that fits the frame go through the tables; workgroup-uniform
__device__ __forceinline__ bool use_tables(const Axis& ay, const Axis& ax, int h, int w) {
    return ay.max_interp <= kTapMax && ax.max_interp <= kTapMax && h <= VAA_IMG && w <= VAA_IMG;
}

// Tap tables of one image in LDS: one output position per thread (h + w positions). The weights are tap_weight's own fp32 values, so
// whoever reads the table computes exactly what the direct evaluation computes.
__device__ __forceinline__ void build_tap_tables(TapTab& tab, const Axis& ay, const Axis& ax, bool vert, bool horiz, int h, int w) {
    for (int t = threadIdx.x; t < h + w; t += blockDim.x) {
        const int axis = t < h ? 0 : 1, o = t < h ? t : t - h;
        if ((axis == 0 && !vert) || (axis == 1 && !horiz)) continue;
        const Axis& aa = axis == 0 ? ay : ax;
        const Taps tp = make_taps(aa, o);
        tab.lo[axis][o] = (short)tp.lo;
        tab.n[axis][o] = (short)tp.n;
        for (int q = 0; q < tp.n; ++q) tab.w[axis][o][q] = tap_weight(aa, tp, q);
    }
}

// This workgroup's chunks of one output plane: horizontal pass (src[0]*w[0], then fma(src[j], w[j], acc)), then the vertical pass over its
// rows in the same form; an axis that keeps its size is copied, never multiplied.
template <class Src>
__device__ __forceinline__ void resize_plane(const Src& s, const float* src, float* dst, int pw, int h, int w, bool vert, bool horiz) {
    for (int e = blockIdx.z * 256 + threadIdx.x; e < h * w; e += gridDim.z * 256) {
        const int oy = e / w, ox = e - oy * w;
        typename Src::Out ty, tx;
        if (vert) ty = s.at(0, oy);
        if (horiz) tx = s.at(1, ox);
        const int r0 = vert ? ty.lo : oy, nr = vert ? ty.n : 1, x0 = horiz ? tx.lo : ox;
        float o = 0.0f;
        for (int r = 0; r < nr; ++r) {
            const float* srow = src + (size_t)(r0 + r) * pw + x0;
            float hv;
            if (horiz) {
                hv = tx.n > 0 ? srow[0] * tx.w(0) : 0.0f;
                for (int j = 1; j < tx.n; ++j) hv = __builtin_fmaf(srow[j], tx.w(j), hv);
            } else {
                hv = srow[0];
            }
            if (!vert) { o = hv; break; }
            o = (r == 0) ? hv * ty.w(0) : __builtin_fmaf(hv, ty.w(r), o);
        }
        dst[e] = o;
    }
}

// grid = (B, 3, slices): workgroup (b, c, z) computes every slices-th chunk of output plane c of image b
__global__ __launch_bounds__(256) void patch_resize_fwd_kernel(ResizeArgs a) {
    __shared__ TapTab tab;
    const int b = blockIdx.x, c = blockIdx.y;
    const int h = a.pdesc[4 * b], w = a.pdesc[4 * b + 1];
    const float* src = a.in + (size_t)c * a.ph * a.pw;
    float* dst = a.out + a.pdesc[4 * b + 2] + (size_t)c * h * w;
    const Axis ay = make_axis(a.ph, h), ax = make_axis(a.pw, w);
    const bool horiz = (w != a.pw), vert = (h != a.ph);
    if (use_tables(ay, ax, h, w)) {
        build_tap_tables(tab, ay, ax, vert, horiz, h, w);
        __syncthreads();
        resize_plane(TableTaps{&tab}, src, dst, a.pw, h, w, vert, horiz);
    } else {
        resize_plane(DirectTaps{ay, ax}, src, dst, a.pw, h, w, vert, horiz);
    }
}

// The weight of base index i under output o along `axis` (1 on an axis that keeps its size); false: o's taps do not cover i.
template <class Src>
__device__ __forceinline__ bool cover(const Src& s, bool resized, int axis, int o, int i, float& wt) {
    wt = 1.0f;
    if (!resized) return true;
    const typename Src::Out t = s.at(axis, o);
    const int d = i - t.lo;
    if (d < 0 || d >= t.n) return false;
    wt = t.w(d);
    return true;
}

// One image's share of base element (y, x): every candidate output (oy, ox) whose taps cover it, torch's grad_in += wx*wy*grad_out in (oh, ow)
// scan order. The x weights do not depend on oy: the table form (ncx <= kMaxCand) keeps them in registers and skips a candidate whose weight is
// exactly 0; the direct form evaluates them per candidate and skips only those outside the tap range. The two rules differ only for a
// non-finite g under a zero weight, and each form keeps its own.
template <class Src>
__device__ __forceinline__ float gather(const Src& s, const float* g, bool vert, bool horiz, int w, int y, int x, int oy_lo, int oy_hi, int ox_lo, int ncx) {
    float wxs[kMaxCand], wy, wx;
    if constexpr (Src::kTabled) {
#pragma unroll
        for (int q = 0; q < kMaxCand; ++q) {
            const bool in = q < ncx && cover(s, horiz, 1, ox_lo + q, x, wx);
            wxs[q] = in ? wx : 0.0f;  // a select, not a branch per candidate
        }
    }
    float acc = 0.0f;
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
        if (!cover(s, vert, 0, oy, y, wy)) continue;
        if constexpr (Src::kTabled) {
#pragma unroll
            for (int q = 0; q < kMaxCand; ++q)
                if (q < ncx && wxs[q] != 0.0f) acc += wxs[q] * wy * g[(size_t)oy * w + ox_lo + q];
        } else {
            for (int q = 0; q < ncx; ++q)
                if (cover(s, horiz, 1, ox_lo + q, x, wx)) acc += wx * wy * g[(size_t)oy * w + ox_lo + q];
        }
    }
    return acc;
}

// Adjoint, as a deterministic gather: element (y, x) of the base-patch gradient collects, image after image, every output (oy, ox)
// whose taps cover it. Candidate outputs come from the inverse of centre = scale*(o+0.5) with a +-2 margin and are tested exactly.
// grid = (image groups, 3, ceil(ph*pw / 256)): a thread owns ONE base element and walks the images of its group in order, so a batch of
// up to kResizeGroup images needs no partial buffer at all; larger batches leave one partial per group to the fixed-order reduce.
// Per image the workgroup first builds the tap tables of both axes in LDS (one output position per thread: the make_taps arithmetic —
// fp64 steps, a division per tap — is done h + w times per workgroup instead of ~20 times per element; 22 -> 9 us at config 5's
// per-rank shape) where use_tables allows; wider filters, and elements with more than kMaxCand x candidates, take the direct evaluation.
__global__ __launch_bounds__(256) void patch_resize_bwd_kernel(ResizeArgs a, int group) {
    __shared__ TapTab tab;
    const int c = blockIdx.y, e = blockIdx.z * 256 + threadIdx.x;
    const bool live = e < a.ph * a.pw;
    const int y = live ? e / a.pw : 0, x = live ? e - y * a.pw : 0;
    const int b_lo = blockIdx.x * group, b_hi = min(a.B, b_lo + group);
    float total = 0.0f;
    for (int b = b_lo; b < b_hi; ++b) {
        const int h = a.pdesc[4 * b], w = a.pdesc[4 * b + 1];
        const float* g = a.in + a.pdesc[4 * b + 2] + (size_t)c * h * w;
        const Axis ay = make_axis(a.ph, h), ax = make_axis(a.pw, w);
        const bool horiz = (w != a.pw), vert = (h != a.ph);
        const bool tabled = use_tables(ay, ax, h, w);
        if (tabled) {
            __syncthreads();  // the previous image's tables are no longer read
            build_tap_tables(tab, ay, ax, vert, horiz, h, w);
            __syncthreads();
        }
        if (!live) continue;
        int oy_lo = y, oy_hi = y, ox_lo = x, ox_hi = x;
        if (vert) {
            oy_lo = max(0, (int)floorf(((float)y - ay.support - 1.0f) / ay.scale - 0.5f) - 2);
            oy_hi = min(h - 1, (int)ceilf(((float)y + ay.support + 1.0f) / ay.scale - 0.5f) + 2);
        }
        if (horiz) {
            ox_lo = max(0, (int)floorf(((float)x - ax.support - 1.0f) / ax.scale - 0.5f) - 2);
            ox_hi = min(w - 1, (int)ceilf(((float)x + ax.support + 1.0f) / ax.scale - 0.5f) + 2);
        }
        const int ncx = ox_hi - ox_lo + 1;
        if (tabled && ncx <= kMaxCand) total += gather(TableTaps{&tab}, g, vert, horiz, w, y, x, oy_lo, oy_hi, ox_lo, ncx);
        else total += gather(DirectTaps{ay, ax}, g, vert, horiz, w, y, x, oy_lo, oy_hi, ox_lo, ncx);
    }
    if (live) a.out[((size_t)blockIdx.x * 3 + c) * a.ph * a.pw + e] = total;
}

}  // namespace vaa

extern "C" int vaa_patch_resize_fwd(const float* patch, int ph, int pw, const int32_t* pdesc, int B, float* packed, void* stream) {
    using namespace vaa;
    if (B == 0) return VAA_OK;
    int rc = check_patch_stage("vaa_patch_resize_fwd", {patch, pdesc, packed}, B, ph, pw, /*frame_bound=*/false);
    if (rc != VAA_OK) return rc;
    const ResizeArgs a{patch, pdesc, packed, B, ph, pw};
    const int slices = B * 3 >= 256 ? 4 : 32;  // few images: more workgroups per plane so the launch still spreads over the chip
    VAA_LAUNCH(patch_resize_fwd_kernel, dim3(B, 3, slices), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("vaa_patch_resize_fwd");
}

extern "C" size_t vaa_patch_resize_ws_bytes(int B, int ph, int pw) {
    if (B <= 0 || ph <= 0 || pw <= 0) return 0;
    const int group = vaa::resize_group(B, ph, pw);
    return vaa::patch_stage_ws_bytes((B + group - 1) / group, ph, pw);  // one partial per image group
}

extern "C" int vaa_patch_resize_bwd(const float* gpacked, int ph, int pw, const int32_t* pdesc, int B, float* gpatch, void* ws,
                                    size_t ws_bytes, void* stream) {
    using namespace vaa;
    hipStream_t st = (hipStream_t)stream;
    const int group = resize_group(B, ph, pw), groups = (B + group - 1) / group;
    return patch_stage_bwd("vaa_patch_resize_bwd", {gpacked, pdesc, gpatch}, B, ph, pw, /*frame_bound=*/false, /*empty_ok=*/false, groups, gpatch, ws,
                           ws_bytes, st, [&](float* out) {
        const ResizeArgs a{gpacked, pdesc, out, B, ph, pw};
        VAA_LAUNCH(patch_resize_bwd_kernel, dim3(groups, 3, (ph * pw + 255) / 256), dim3(256), 0, st, a, group);
    });
}
