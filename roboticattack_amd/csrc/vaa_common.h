// vaa_common.h — shared device helpers for the gfx950 kernels behind include/vaa.h.
//
// Numerics contract (re-verified against the reference in tests/golden):
// this translation unit is compiled with -ffp-contract=off; every fused multiply-add below is
// explicit so the warp coordinates, bilinear weights and the `canvas < -20` mask reproduce the
// reference's PyTorch-CPU path (F.affine_grid + F.grid_sample, appply_random_transform.py:93-102)
// bit for bit.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>
#include <string>

#include "../../include/vaa.h"

#define VAA_NPIX (VAA_IMG * VAA_IMG)

namespace vaa {

void set_error(const char* fmt, ...);
int check_launch(const char* what);  // the HIP runtime's last error, then async_error_poll()
unsigned* async_error_word();        // pinned, device-mapped word kernels OR failure bits into (nullptr: allocation failed)
int async_error_poll(const char* what, bool clear);
constexpr unsigned VAA_ASYNC_K3_HANDOVER_TIMEOUT = 1u;
constexpr unsigned VAA_ASYNC_JITTER_PDESC = 2u;  // vaa_patch_jitter_*: a descriptor entry whose size is not the base patch's (that image is left alone)
constexpr unsigned VAA_ASYNC_DECODE_POS = 4u;    // vaa_model_attention_decode: a row whose pos is outside [0, Tmax) (its o is zero, its cache untouched)
// vaa_patch_grad.hip: gpatch[e] = sum_p partial[p][e] (p < nparts, e < n) in a fixed order with fp64 accumulation
int launch_partial_reduce(const float* partial, float* gpatch, int n, int nparts, hipStream_t st, const char* who);

// Argument rules every patch entry point shares (host). check_patch_size: the batch / patch sizes and the frame (what vaa_patch_apply_eval,
// which has no mask mode and takes its geometry per image, checks; frame_bound = false: the sizes alone); check_patch_call adds the mask mode
// rules of K1 / K2 / K2'.
inline int check_patch_size(const char* who, int B, int h, int w, bool frame_bound = true) {
    if (B < 0 || h <= 0 || w <= 0) {
        set_error("%s: bad sizes (B=%d ph=%d pw=%d)", who, B, h, w);
        return VAA_E_INVALID;
    }
    if (frame_bound && (h > VAA_IMG || w > VAA_IMG)) {
        set_error("%s: patch %dx%d larger than the %dx%d frame", who, h, w, VAA_IMG, VAA_IMG);
        return VAA_E_UNSUPPORTED;
    }
    return VAA_OK;
}

inline int check_patch_call(const char* who, int B, int h, int w, int geometry, int mask_mode) {
    if (mask_mode != VAA_MASK_LT_M20 && mask_mode != VAA_MASK_NE_M100) {
        set_error("%s: bad mask_mode %d", who, mask_mode);
        return VAA_E_INVALID;
    }
    const int rc = check_patch_size(who, B, h, w);
    if (rc != VAA_OK) return rc;
    if (geometry && mask_mode == VAA_MASK_NE_M100) {
        // the reference pairs `canvas != -100` only with the un-warped paste (paste_patch_fix / random_paste_patch, :138-188); after a
        // warp the all-background blend -100*(nw+ne+sw+se) is not exactly -100, so the rule would depend on rounding over the whole frame
        set_error("%s: VAA_MASK_NE_M100 is defined for geometry=0 only (appply_random_transform.py:153,179)", who);
        return VAA_E_UNSUPPORTED;
    }
    return VAA_OK;
}

// The checks that open every planar frame-stage entry point (K9 / K10 / K11; host), in the order a caller observes them: the batch range (B in
// [0, max_B]; batch_note: what the stage adds behind "B=<B>", or ""), the empty batch (VAA_OK: the caller returns without a launch), a null
// pointer among `dev` or `host`, a pointer of `dev` (the tensors and the rows' device copy, named `rows_dev` in the message) that is not 16-byte
// aligned. The stage's own rules (its rows, an overlap, a workspace) follow in its own file.
inline int check_stage_call(const char* who, int B, long max_B, const char* batch_note, std::initializer_list<const void*> dev,
                            std::initializer_list<const void*> host, const char* rows_dev) {
    if (B < 0 || (long)B > max_B) {
        set_error("%s: bad batch size (B=%d%s)", who, B, batch_note);
        return VAA_E_INVALID;
    }
    if (B == 0) return VAA_OK;  // empty batch: nothing to read or write (pointers may be null)
    bool null = false, misaligned = false;
    for (const void* p : host) null |= !p;
    for (const void* p : dev) null |= !p, misaligned |= ((uintptr_t)p & 15u) != 0;
    if (null) {
        set_error("%s: null pointer argument", who);
        return VAA_E_INVALID;
    }
    if (misaligned) {
        set_error("%s: the tensors and %s must be 16-byte aligned", who, rows_dev);
        return VAA_E_INVALID;
    }
    return VAA_OK;
}

// The argument rules of the per-image patch stages (K0 resize, K0c jitter; host): a null pointer among `ptrs`, then the sizes. The stages differ
// in one rule, kept per stage (DESIGN.md lists them): K0c bounds the patch by the frame (check_patch_size), K0 only wants positive sizes.
inline int check_patch_stage(const char* who, std::initializer_list<const void*> ptrs, int B, int ph, int pw, bool frame_bound) {
    for (const void* p : ptrs)
        if (!p) {
            set_error("%s: null pointer argument", who);
            return VAA_E_INVALID;
        }
    return check_patch_size(who, B, ph, pw, frame_bound);
}

// the `parts` partial gradients [3*ph*pw] an adjoint of these stages leaves to the fixed-order reduce; one part is written to gpatch itself
inline size_t patch_stage_ws_bytes(int parts, int ph, int pw) { return parts > 1 ? (size_t)parts * 3 * ph * pw * sizeof(float) : 0; }

// What both adjoint entry points of the per-image patch stages do around their kernel (host), in the order a caller observes it: an empty batch
// zeroes gpatch (when there is one to zero) and, with empty_ok, is VAA_OK whatever else was passed (K0c; K0 goes on to the argument check, so
// B == 0 with a null gpatch is its null-pointer error); the argument check; the workspace; launch(out) with out = the workspace when
// parts > 1, else gpatch; check_launch; the fixed-order reduce of the parts.
template <typename Launch>
inline int patch_stage_bwd(const char* who, std::initializer_list<const void*> ptrs, int B, int ph, int pw, bool frame_bound, bool empty_ok, int parts,
                           float* gpatch, void* ws, size_t ws_bytes, hipStream_t st, Launch launch) {
    if (B == 0 && gpatch && ph > 0 && pw > 0)
        return hipMemsetAsync(gpatch, 0, (size_t)3 * ph * pw * sizeof(float), st) == hipSuccess ? VAA_OK
                                                                                                  : check_launch((std::string(who) + "(memset)").c_str());
    if (B == 0 && empty_ok) return VAA_OK;
    int rc = check_patch_stage(who, ptrs, B, ph, pw, frame_bound);
    if (rc != VAA_OK) return rc;
    const size_t need = patch_stage_ws_bytes(parts, ph, pw);
    if (need > 0 && (!ws || ws_bytes < need)) {
        set_error("%s: workspace %zu B < required %zu B", who, ws_bytes, need);
        return VAA_E_WORKSPACE;
    }
    launch(parts > 1 ? (float*)ws : gpatch);
    rc = check_launch(who);
    if (rc != VAA_OK || parts == 1) return rc;
    return launch_partial_reduce((const float*)ws, gpatch, 3 * ph * pw, parts, st, (std::string(who) + "(reduce)").c_str());
}

// 1/std of the six normalisation channels, rounded from double: the factor K2 / K2' apply to the incoming gradient
inline void inv_std6(const float* std6, float* istd6) {
    for (int q = 0; q < 6; ++q) istd6[q] = (float)(1.0 / (double)std6[q]);
}

// Per-dispatch timing (include/vaa.h: vaa_prof_*): while the profiler is armed every kernel of the library is dispatched through
// hipExtLaunchKernel with its own start/stop event pair, which the runtime binds to THAT dispatch's begin/end timestamps (the figures
// rocprofv3 --kernel-trace reports), so a kernel's duration inside a real step is read without bracketing markers.
bool prof_next(const char* name, hipEvent_t* start, hipEvent_t* stop);

template <typename F, typename... Args>
inline void launch_k(const char* name, F kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    hipEvent_t s, e;
    if (prof_next(name, &s, &e)) hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, st, s, e, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
}
#define VAA_LAUNCH(kernel, grid, block, lds, stream, ...) ::vaa::launch_k(#kernel, kernel, grid, block, lds, stream, __VA_ARGS__)

struct Norm6 {
    float mean[6];
    float stdv[6];
};

__device__ __forceinline__ float bf16_bits_to_f32(uint32_t h) { return __uint_as_float(h << 16); }

// torch `.to(torch.bfloat16)`: round-to-nearest-even; NaN stays NaN.
__device__ __forceinline__ uint32_t f32_to_bf16_bits(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x0040u;
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}

// Host and device share the arithmetic of the camera-pixel LUT: IEEE fp32 true divisions, RNE bf16 cast
// (host code of the library is compiled with -ffp-contract=off as well).
__host__ __device__ inline uint32_t bf16_rne(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x0040u;
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}

// value v in [0,1] of channel c -> packed {bf16 first normalisation, bf16 second normalisation} (UADA.py:56-57)
__host__ __device__ inline uint32_t norm_pack(float v, const Norm6& n, int c) {
    float o0 = (v - n.mean[c]) / n.stdv[c];
    float o1 = (v - n.mean[c + 3]) / n.stdv[c + 3];
    return bf16_rne(o0) | (bf16_rne(o1) << 16);
}

// The 3x256 table of a frame byte's normalised values, lut[c*256 + u8] = norm_pack(u8 / 255, nrm, c): built once per workgroup in LDS by all
// of its `nthreads` threads (the caller places the barrier). The one fill behind K1 (planar and tile-major) and K7: one source, same bits.
__device__ __forceinline__ void fill_norm_lut(uint32_t* lut, const Norm6& nrm, int tid, int nthreads) {
#pragma unroll
    for (int e = tid; e < 768; e += nthreads) lut[e] = norm_pack((float)(e & 255) / 255.0f, nrm, e >> 8);
}

// F.affine_grid(align_corners=False) base coordinate of pixel index i along a 224-long axis:
// torch.linspace(-1, 1, 224)[i] * 223 / 224, with linspace's two-sided evaluation (one FMA each side).
__device__ __forceinline__ float base_coord(int i) {
    const float step = 2.0f / 223.0f;
    float lin = (i < VAA_IMG / 2) ? __builtin_fmaf((float)i, step, -1.0f)
                                  : __builtin_fmaf(-(float)(VAA_IMG - 1 - i), step, 1.0f);
    return (lin * 223.0f) / 224.0f;
}

struct Samp {
    int x0, y0;            // floor of the clamped source position (north-west corner)
    float nw, ne, sw, se;  // bilinear corner weights
};

// bx/by: base coords of output column j / row i; th: row-major 2x3 affine.
// grid = base @ theta^T as torch's CPU GEMM evaluates it (product, one FMA, plain add), then
// grid_sample's unnormalise contracted into one FMA, clamp to the border, floor; (x0, y0) and the fractional parts w, n.
// (K2 stores {x0, y0, w, n} per pixel and forms the four corner weights when it scatters: the products of samp_from_frac.)
__device__ __forceinline__ void sample_pos_frac(float bx, float by, const float* th, int& x0, int& y0, float& w, float& n) {
    float gx = __builtin_fmaf(by, th[1], bx * th[0]) + th[2];
    float gy = __builtin_fmaf(by, th[4], bx * th[3]) + th[5];
    float ix = __builtin_fmaf(gx + 1.0f, 112.0f, -0.5f);
    float iy = __builtin_fmaf(gy + 1.0f, 112.0f, -0.5f);
    ix = fminf(223.0f, fmaxf(ix, 0.0f));
    iy = fminf(223.0f, fmaxf(iy, 0.0f));
    float xw = floorf(ix), yn = floorf(iy);
    w = ix - xw;
    n = iy - yn;
    x0 = (int)xw;
    y0 = (int)yn;
}

__device__ __forceinline__ Samp samp_from_frac(int x0, int y0, float w, float n) {
    Samp s;
    const float e = 1.0f - w, so = 1.0f - n;
    s.x0 = x0; s.y0 = y0;
    s.nw = so * e; s.ne = so * w; s.sw = n * e; s.se = n * w;
    return s;
}

// the sample position with its bilinear corner weights
__device__ __forceinline__ Samp sample_pos(float bx, float by, const float* th) {
    int x0, y0;
    float w, n;
    sample_pos_frac(bx, by, th, x0, y0, w, n);
    return samp_from_frac(x0, y0, w, n);
}

// The patch image b pastes: the batch's one patch [3,ph,pw], or with pdesc ([B,4] = {h_b, w_b, offset_b, 0}; resize_patch=True,
// appply_random_transform.py:113-118) its own resized patch at patch + offset_b.
__device__ __forceinline__ void patch_of(const int32_t* pdesc, int ph, int pw, const float* patch, int b, int& ph_b, int& pw_b, const float*& p_b) {
    if (pdesc) {
        ph_b = pdesc[4 * b]; pw_b = pdesc[4 * b + 1]; p_b = patch + pdesc[4 * b + 2];
    } else {
        ph_b = ph; pw_b = pw; p_b = patch;
    }
}

// canvas = -100 everywhere with the patch pasted at (px,py) (appply_random_transform.py:111,125);
// corners beyond the frame contribute 0 (grid_sample's bounds mask).
template <typename P>
__device__ __forceinline__ float canvas_at(P patch_c, int ph, int pw, int px, int py, int xx, int yy) {
    if (xx >= VAA_IMG || yy >= VAA_IMG) return 0.0f;
    int u = xx - px, v = yy - py;
    if ((unsigned)u < (unsigned)pw && (unsigned)v < (unsigned)ph) return patch_c[v * pw + u];
    return -100.0f;
}

template <typename P>
__device__ __forceinline__ float sample_canvas(P patch_c, int ph, int pw, int px, int py, const Samp& s) {
    float vnw = canvas_at(patch_c, ph, pw, px, py, s.x0, s.y0);
    float vne = canvas_at(patch_c, ph, pw, px, py, s.x0 + 1, s.y0);
    float vsw = canvas_at(patch_c, ph, pw, px, py, s.x0, s.y0 + 1);
    float vse = canvas_at(patch_c, ph, pw, px, py, s.x0 + 1, s.y0 + 1);
    return __builtin_fmaf(vse, s.se, __builtin_fmaf(vsw, s.sw, __builtin_fmaf(vne, s.ne, vnw * s.nw)));
}

__device__ __forceinline__ bool keep_rule(float cv, int mask_mode) {
    return mask_mode == VAA_MASK_LT_M20 ? !(cv < -20.0f) : (cv != -100.0f);
}

// Pixel-space view of the same affine map (used only to BOUND the footprint, never for values):
//   ix ~= a00*j + a01*i + c0,  iy ~= a10*j + a11*i + c1.
struct PixAffine {
    float a00, a01, c0, a10, a11, c1;
};

__device__ __forceinline__ PixAffine pix_affine(const float* th) {
    PixAffine p;
    p.a00 = th[0];
    p.a01 = th[1];
    p.c0 = 112.0f * (th[2] + 1.0f) - 0.5f - 111.5f * (th[0] + th[1]);
    p.a10 = th[3];
    p.a11 = th[4];
    p.c1 = 112.0f * (th[5] + 1.0f) - 0.5f - 111.5f * (th[3] + th[4]);
    return p;
}

// j-interval of row i whose (approximate, unclamped) source coordinate a*j + base lies in [lo, hi)
__device__ __forceinline__ void solve_interval(float a, float base, float lo, float hi, float& jl, float& jh) {
    if (fabsf(a) > 1e-6f) {
        float t0 = (lo - base) / a, t1 = (hi - base) / a;
        jl = fmaxf(jl, fminf(t0, t1));
        jh = fminf(jh, fmaxf(t0, t1));
    } else if (!(base >= lo - 1.0f && base < hi + 1.0f)) {
        jl = 1e30f;
        jh = -1e30f;
    }
}

// Conservative COLUMN span of output row i of an image whose ph x pw patch is pasted at (px, py): pixels [jlo, jhi] may have a source
// point with a corner on patch rows [v_lo, v_hi) (the whole patch: v_lo = 0, v_hi = ph); [0, -1] when the row is clear. theta_b: the
// image's 2x3 affine, read only when geometry != 0 (a flag and not a nullable pointer: a null test on theta + 6b does not fold away).
// INVARIANT: every role of both K1 kernels, K5 and K2 derive ownership and coverage from this one function — K1's roles split the
// frame by it, and K2 (a workgroup per band of patch rows) walks exactly the pixels K1's footprint role evaluated, so no kept pixel's
// gradient is lost.
__device__ __forceinline__ void row_span(int px, int py, int ph, int pw, int v_lo, int v_hi, int geometry, const float* theta_b, int i, int& jlo, int& jhi) {
    jlo = 0; jhi = -1;
    if (geometry) {
        float th[6];
#pragma unroll
        for (int z = 0; z < 6; ++z) th[z] = theta_b[z];
        const PixAffine pa = pix_affine(th);
        // source x must fall in [px-1, px+pw) (corner x0 or x0+1 on the patch), source y in [py+v_lo-1, py+v_hi); a side of the patch
        // that lies on the frame edge also receives every clamped out-of-frame sample (padding_mode='border'): open to infinity
        const float xlo = (px == 0) ? -1e30f : (float)(px - 1);
        const float xhi = (px + pw == VAA_IMG) ? 1e30f : (float)(px + pw);
        const float ylo = (py == 0 && v_lo == 0) ? -1e30f : (float)(py + v_lo - 1);
        const float yhi = (py + ph == VAA_IMG && v_hi == ph) ? 1e30f : (float)(py + v_hi);
        float jl = -1e30f, jh = 1e30f;
        solve_interval(pa.a00, pa.a01 * (float)i + pa.c0, xlo, xhi, jl, jh);
        solve_interval(pa.a10, pa.a11 * (float)i + pa.c1, ylo, yhi, jl, jh);
        if (jl <= jh && v_lo < v_hi) {
            jlo = (int)fmaxf(0.0f, floorf(jl) - 1.0f);
            jhi = (int)fminf((float)(VAA_IMG - 1), ceilf(jh) + 1.0f);
        }
    } else if (i >= py + v_lo && i < py + v_hi) {
        jlo = px;
        jhi = px + pw - 1;
    }
    // an interval that lies wholly beyond the frame (possible when a side is open to +-infinity) clamps to jhi < jlo with jlo > 0;
    // normalise every empty row to [0, -1] so that ALL roles see "nothing" (the background role of the planar K1 packs the count into
    // 8 bits and would otherwise skip items nobody writes)
    if (jhi < jlo) { jlo = 0; jhi = -1; }
}

// K4's per-element arithmetic (vaa_update.hip; also applied by the step epilogue when the update is fused into it: one source, same bits)
struct UpdArgs {
    float* patch;
    const float* g;
    float* m;
    float* v;
    float* stats;
    int n, mode;
    float lr, b1, b2, eps, step_size, one_m_b1, one_m_b2, l1_clip, grad_scale;
};

// The scalar part of UpdArgs (the caller sets the pointers and n): the reference optimiser's python-side doubles, narrowed to f32 exactly where
// torch narrows them. The one builder of every K4 entry point (vaa_patch_update[_seg], vaa_step_epilogue[_seg]_update): one source, same bits.
inline UpdArgs upd_args(int mode, float lr, float beta1, float beta2, float eps, int step, float l1_clip, float grad_scale) {
    UpdArgs a = {};
    a.mode = mode;
    a.lr = lr; a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.l1_clip = l1_clip; a.grad_scale = grad_scale;
    const double b1 = (double)beta1, b2 = (double)beta2;
    a.one_m_b1 = (float)(1.0 - b1);
    a.one_m_b2 = (float)(1.0 - b2);
    a.step_size = (mode == VAA_OPT_ADAMW_HF) ? (float)((double)lr * sqrt(1.0 - pow(b2, (double)step)) / (1.0 - pow(b1, (double)step))) : 0.0f;
    return a;
}

__device__ __forceinline__ float update_one(const UpdArgs& a, float g, float p, float& m, float& v) {
    if (a.mode == VAA_OPT_ADAMW_HF) {
        m = __builtin_fmaf(g, a.one_m_b1, m * a.b1);      // exp_avg.mul_(b1).add_(g, alpha=1-b1)
        v = v * a.b2 + (a.one_m_b2 * g) * g;              // exp_avg_sq.mul_(b2).addcmul_(g, g, value=1-b2)
        const float denom = sqrtf(v) + a.eps;             // v.sqrt().add_(eps)
        p = p + ((-a.step_size) * m) / denom;             // p.addcdiv_(m, denom, value=-step_size)
    } else {
        const float sg = (g > 0.0f) ? 1.0f : ((g < 0.0f) ? -1.0f : 0.0f);
        p = p - a.lr * sg;
    }
    return fminf(1.0f, fmaxf(0.0f, p));                   // patch.data.clamp(0, 1)
}

// out[e] = sum_p partial[p][e] (p < nparts, e < n) for the 64 elements of block `blk`, in a fixed two-level order (16 interleaved slices,
// then slice 0..15), fp64: the body of patch_grad_reduce_kernel, shared with the step epilogue (256 threads; sl = 16 KB of LDS).
// A thread owns four consecutive elements (16 B loads); block = 16 element-quads x 16 slices.
// Returns true in the threads that own a result element (index `oe`, value `ov`) after storing it.
__device__ __forceinline__ bool partial_reduce_block(const float* __restrict__ partial, float* __restrict__ out, int n, int nparts, int blk,
                                                     double (*sl)[16][4], int& oe, float& ov) {
    const int el = threadIdx.x & 15, s = threadIdx.x >> 4;
    const int e = (blk * 16 + el) * 4;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (e + 3 < n && (n & 3) == 0) {
#pragma unroll 8
        for (int p = s; p < nparts; p += 16) {
            const float4 v = *reinterpret_cast<const float4*>(partial + (size_t)p * n + e);
            acc[0] += (double)v.x; acc[1] += (double)v.y; acc[2] += (double)v.z; acc[3] += (double)v.w;
        }
    } else {
        for (int p = s; p < nparts; p += 16)
#pragma unroll
            for (int z = 0; z < 4; ++z)
                if (e + z < n) acc[z] += (double)partial[(size_t)p * n + e + z];
    }
#pragma unroll
    for (int z = 0; z < 4; ++z) sl[s][el][z] = acc[z];
    __syncthreads();
    if (s < 4) {  // thread (s, el) of the second level sums element z = s of quad el
        const int z = s;
        if (e + z < n) {
            double t = 0.0;
#pragma unroll
            for (int q = 0; q < 16; ++q) t += sl[q][el][z];
            out[e + z] = (float)t;
            oe = e + z;
            ov = (float)t;
            return true;
        }
    }
    return false;
}

// HF rotate_half on 8 + 8 bf16: lo = x[i .. i+7], hi = x[i+hd/2 .. i+hd/2+7], c0|c1 / s0|s1 = the 8 table entries cos/sin[t, i .. i+7].
//   ol = lo*cos - hi*sin*sgn,  oh = hi*cos + lo*sin*sgn, each rounded to bf16 once.
// The one source of the rotation's arithmetic: vaa_model_rope and vaa_model_attention_decode both call it, so their bits agree.
__device__ __forceinline__ void rope_rotate8(const uint4& lo, const uint4& hi, const float4& c0, const float4& c1, const float4& s0, const float4& s1,
                                             float sgn, uint4& ol, uint4& oh) {
    const float cs[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    const float sn[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    const uint32_t lw[4] = {lo.x, lo.y, lo.z, lo.w}, hw[4] = {hi.x, hi.y, hi.z, hi.w};
    uint32_t l4[4], h4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float x1a = __uint_as_float(lw[q] << 16), x1b = __uint_as_float(lw[q] & 0xffff0000u);
        const float x2a = __uint_as_float(hw[q] << 16), x2b = __uint_as_float(hw[q] & 0xffff0000u);
        const float sa = sn[2 * q] * sgn, sb2 = sn[2 * q + 1] * sgn;
        const float o1a = x1a * cs[2 * q] - x2a * sa, o1b = x1b * cs[2 * q + 1] - x2b * sb2;
        const float o2a = x2a * cs[2 * q] + x1a * sa, o2b = x2b * cs[2 * q + 1] + x1b * sb2;
        l4[q] = f32_to_bf16_bits(o1a) | (f32_to_bf16_bits(o1b) << 16);
        h4[q] = f32_to_bf16_bits(o2a) | (f32_to_bf16_bits(o2b) << 16);
    }
    ol = make_uint4(l4[0], l4[1], l4[2], l4[3]);
    oh = make_uint4(h4[0], h4[1], h4[2], h4[3]);
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sum of v over a workgroup of kWaves waves, the same bits in every thread: butterfly inside a wave, then the waves in order (sl: kWaves doubles
// of LDS; every thread of the workgroup must call it).
template <int kWaves>
__device__ __forceinline__ double block_sum(double v, double* sl) {
    v = wave_sum(v);
    __syncthreads();  // the previous sum's slots are no longer read
    if ((threadIdx.x & 63) == 0) sl[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) t += sl[w];
    return t;
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

}  // namespace vaa
