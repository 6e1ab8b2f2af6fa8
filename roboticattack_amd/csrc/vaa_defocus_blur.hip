// vaa_defocus_blur.hip — K11: separable 13-tap blur with edge replication of K1's planar pixel values (bf16 [B,6,224,224]), one tap row per
// image, and its adjoint. One launch per call, whatever B is.
//
// include/vaa.h states the arithmetic; every operation below is one separately rounded fp32 operation (the library is built with
// -ffp-contract=off and this file repeats it; no FMA is written here). Both passes of a direction live in one kernel: a workgroup owns a band
// of kBlurBand rows of one plane and keeps the intermediate of the first pass in LDS in fp32, so it is never rounded to bf16.
//   forward:  rows (horizontal pass, read from global as three 16-byte vectors per run of 8, the band plus a clamped 6-row halo) -> LDS
//             -> columns (vertical pass out of LDS) -> one 16-byte store per run.
//   adjoint:  the gradient's band plus a 6-row halo (rows outside the frame are zeros) -> LDS as bf16 -> the vertical pass's transpose -> LDS
//             in fp32 -> the horizontal pass's transpose -> one 16-byte store per run. A gather per source element: no atomics, no workspace.
// A thread owns runs of 8 consecutive elements, and every tap is a statically indexed register: the only run-time indices are the clamped
// rows / columns of whole 16-byte vectors, so no address depends on a tap and none leaves the plane.
// The transpose's interior is the 13 taps on a zero-padded gradient (w * 0 = +0 leaves a sum as it is: an accumulator that starts at +0 is never
// -0). Index 0 and index 223 also collect the taps the clamp folded onto them; the threads that own them recompute those elements in the
// stated order (run-time loops over the folded taps, read from the device copy of the taps).
// Band height: 32 rows is 44 x 224 x 4 B = 39 KB of LDS (adjoint: 19 KB of bf16 + 28 KB of fp32) and 1.375x reads; -DVAA_BLUR_BAND=16 builds
// the 16-row form (1.75x reads, twice the workgroups), which DESIGN.md section 4 compares.
#include "vaa_common.h"

#pragma clang fp contract(off)

#ifndef VAA_BLUR_BAND
#define VAA_BLUR_BAND 32
#endif

namespace vaa {

constexpr int kBlurBand = VAA_BLUR_BAND;                      // rows of a plane per workgroup
constexpr int kBlurHalo = 6;                                  // taps on each side
constexpr int kBlurRun = 8;                                   // elements per run (one 16-byte vector of bf16)
constexpr int kBlurRuns = VAA_IMG / kBlurRun;                 // 28 runs per row
constexpr int kBlurBands = VAA_IMG / kBlurBand;               // bands per plane
constexpr int kBlurLdsRows = kBlurBand + 2 * kBlurHalo;       // band + halo
constexpr int kBlurRowsPerThread = kBlurBand / 8;             // column pass: 8 row groups x 28 runs = 224 of the 256 threads
constexpr int kBlurThreads = 256;
constexpr int kBlurLastRun = VAA_IMG - kBlurRun;              // 216
static_assert(VAA_IMG % kBlurBand == 0 && kBlurBand % 8 == 0 && kBlurBand >= 8, "the band height divides 224 and is a multiple of 8");
static_assert(VAA_IMG % kBlurRun == 0, "a row is whole runs");
constexpr long kBlurMaxB = 0x7fffffffL / (6 * kBlurBands);   // one workgroup per (image, plane, band)

struct BlurArgs {
    const uint16_t* in;   // forward: x; adjoint: gout
    uint16_t* out;        // forward: out; adjoint: gx
    const float* taps;    // dev [B,8] {w0..w6, 0}
};

__device__ __forceinline__ void blur_unpack8(const uint4& d, float* v) {
    const uint32_t q[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = __uint_as_float(q[i] << 16);
        v[2 * i + 1] = __uint_as_float(q[i] & 0xffff0000u);
    }
}

__device__ __forceinline__ uint4 blur_pack8(const float* v) {
    uint32_t q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = f32_to_bf16_bits(v[2 * i]) | (f32_to_bf16_bits(v[2 * i + 1]) << 16);
    return make_uint4(q[0], q[1], q[2], q[3]);
}

// w[k] = w_k, k = 0..6, of image b
__device__ __forceinline__ void blur_load_taps(const float* taps, int b, float* w) {
    const float4 lo = *reinterpret_cast<const float4*>(taps + 8 * (size_t)b);
    const float4 hi = *reinterpret_cast<const float4*>(taps + 8 * (size_t)b + 4);
    w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w; w[4] = hi.x; w[5] = hi.y; w[6] = hi.z;
}

// out[p] = sum over t = -6..6 ascending of w_|t| * win[8 + p + t], from 0.0f (win: the 8 elements of the run with 8 on either side)
__device__ __forceinline__ void blur_row13(const float* w, const float* win, float* out) {
#pragma unroll
    for (int p = 0; p < kBlurRun; ++p) {
        float acc = 0.0f;
#pragma unroll
        for (int t = -kBlurHalo; t <= kBlurHalo; ++t) acc = acc + w[t < 0 ? -t : t] * win[8 + p + t];
        out[p] = acc;
    }
}

// the column pass both directions share: rows [ry, ry + kBlurRowsPerThread) of the band, 8 columns, out of `rows` LDS rows that start 6 above
// the band; LoadRow(l, v) delivers the 8 values of LDS row l. acc[o][p] = sum over t ascending of w_|t| * row(ry + o + 6 + t)[p].
template <typename LoadRow>
__device__ __forceinline__ void blur_cols(const float* w, int ry, LoadRow load_row, float (*acc)[kBlurRun]) {
#pragma unroll
    for (int o = 0; o < kBlurRowsPerThread; ++o)
#pragma unroll
        for (int p = 0; p < kBlurRun; ++p) acc[o][p] = 0.0f;
#pragma unroll
    for (int i = 0; i < kBlurRowsPerThread + 2 * kBlurHalo; ++i) {
        float v[kBlurRun];
        load_row(ry + i, v);
#pragma unroll
        for (int o = 0; o < kBlurRowsPerThread; ++o) {
            const int t = i - o - kBlurHalo;
            if (t >= -kBlurHalo && t <= kBlurHalo) {
#pragma unroll
                for (int p = 0; p < kBlurRun; ++p) acc[o][p] = acc[o][p] + w[t < 0 ? -t : t] * v[p];
            }
        }
    }
}

__global__ __launch_bounds__(kBlurThreads) void defocus_blur_fwd_kernel(const BlurArgs a) {
    __shared__ __attribute__((aligned(16))) float h[kBlurLdsRows * VAA_IMG];
    const int tid = threadIdx.x;
    const unsigned plane_id = blockIdx.x / kBlurBands;  // b*6 + c
    const int y0 = (int)(blockIdx.x - plane_id * kBlurBands) * kBlurBand;
    const int b = (int)(plane_id / 6);
    const uint16_t* src = a.in + (size_t)plane_id * VAA_NPIX;
    uint16_t* dst = a.out + (size_t)plane_id * VAA_NPIX;
    float w[7];
    blur_load_taps(a.taps, b, w);

    // rows: h[l] = the horizontal pass of image row c(y0 - 6 + l)
    for (int item = tid; item < kBlurLdsRows * kBlurRuns; item += kBlurThreads) {
        const int l = item / kBlurRuns, x0 = (item - l * kBlurRuns) * kBlurRun;
        const int y = min(max(y0 - kBlurHalo + l, 0), VAA_IMG - 1);
        const uint16_t* row = src + (size_t)y * VAA_IMG;
        float win[24], o[kBlurRun];
        blur_unpack8(*reinterpret_cast<const uint4*>(row + x0), win + 8);
        blur_unpack8(*reinterpret_cast<const uint4*>(row + max(x0 - kBlurRun, 0)), win);
        blur_unpack8(*reinterpret_cast<const uint4*>(row + min(x0 + kBlurRun, kBlurLastRun)), win + 16);
        if (x0 == 0) {  // c(x + t) = 0
#pragma unroll
            for (int k = 0; k < 8; ++k) win[k] = win[8];
        }
        if (x0 == kBlurLastRun) {  // c(x + t) = 223
#pragma unroll
            for (int k = 16; k < 24; ++k) win[k] = win[15];
        }
        blur_row13(w, win, o);
        float4* hp = reinterpret_cast<float4*>(h + l * VAA_IMG + x0);
        hp[0] = make_float4(o[0], o[1], o[2], o[3]);
        hp[1] = make_float4(o[4], o[5], o[6], o[7]);
    }
    __syncthreads();

    // columns
    for (int item = tid; item < 8 * kBlurRuns; item += kBlurThreads) {
        const int rg = item / kBlurRuns, x0 = (item - rg * kBlurRuns) * kBlurRun, ry = rg * kBlurRowsPerThread;
        float acc[kBlurRowsPerThread][kBlurRun];
        blur_cols(w, ry, [&](int l, float* v) {
            const float4* hp = reinterpret_cast<const float4*>(h + l * VAA_IMG + x0);
            const float4 lo = hp[0], hi = hp[1];
            v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
        }, acc);
#pragma unroll
        for (int o = 0; o < kBlurRowsPerThread; ++o)
            *reinterpret_cast<uint4*>(dst + (size_t)(y0 + ry + o) * VAA_IMG + x0) = blur_pack8(acc[o]);
    }
}

__global__ __launch_bounds__(kBlurThreads) void defocus_blur_bwd_kernel(const BlurArgs a) {
    __shared__ uint4 gs[kBlurLdsRows * kBlurRuns];                               // the gradient's band + halo, bf16
    __shared__ __attribute__((aligned(16))) float as[kBlurBand * VAA_IMG];       // a[r, x], fp32
    const int tid = threadIdx.x;
    const unsigned plane_id = blockIdx.x / kBlurBands;
    const int y0 = (int)(blockIdx.x - plane_id * kBlurBands) * kBlurBand;
    const int b = (int)(plane_id / 6);
    const uint16_t* src = a.in + (size_t)plane_id * VAA_NPIX;
    uint16_t* dst = a.out + (size_t)plane_id * VAA_NPIX;
    const float* wd = a.taps + 8 * (size_t)b;  // the folded taps of index 0 and 223 are read at run-time indices 0..6
    float w[7];
    blur_load_taps(a.taps, b, w);

    for (int item = tid; item < kBlurLdsRows * kBlurRuns; item += kBlurThreads) {
        const int l = item / kBlurRuns, run = item - l * kBlurRuns;
        const int y = y0 - kBlurHalo + l;
        const bool in = y >= 0 && y < VAA_IMG;
        const uint4 d = *reinterpret_cast<const uint4*>(src + (size_t)min(max(y, 0), VAA_IMG - 1) * VAA_IMG + run * kBlurRun);
        gs[item] = in ? d : make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();

    // the vertical pass's transpose: a[r, x] = sum over y ascending of w_|r - y| * g[y, x]; rows 0 and 223 with the folded taps
    for (int item = tid; item < 8 * kBlurRuns; item += kBlurThreads) {
        const int rg = item / kBlurRuns, run = item - rg * kBlurRuns, ry = rg * kBlurRowsPerThread;
        float acc[kBlurRowsPerThread][kBlurRun];
        blur_cols(w, ry, [&](int l, float* v) { blur_unpack8(gs[l * kBlurRuns + run], v); }, acc);
        const int r0 = y0 + ry;
        if (r0 == 0) {  // row 0: output row y sends t = -6..-y here
            float e[kBlurRun], v[kBlurRun];
#pragma unroll
            for (int p = 0; p < kBlurRun; ++p) e[p] = 0.0f;
#pragma nounroll
            for (int y = 0; y <= kBlurHalo; ++y) {
                blur_unpack8(gs[(y + kBlurHalo) * kBlurRuns + run], v);  // y0 = 0: LDS row y + 6
#pragma nounroll
                for (int t = -kBlurHalo; t <= -y; ++t) {
                    const float wt = wd[-t];
#pragma unroll
                    for (int p = 0; p < kBlurRun; ++p) e[p] = e[p] + wt * v[p];
                }
            }
#pragma unroll
            for (int p = 0; p < kBlurRun; ++p) acc[0][p] = e[p];
        }
        if (r0 + kBlurRowsPerThread - 1 == VAA_IMG - 1) {  // row 223: output row y sends t = 223 - y..6 here
            float e[kBlurRun], v[kBlurRun];
#pragma unroll
            for (int p = 0; p < kBlurRun; ++p) e[p] = 0.0f;
#pragma nounroll
            for (int y = VAA_IMG - 1 - kBlurHalo; y < VAA_IMG; ++y) {
                blur_unpack8(gs[(y - y0 + kBlurHalo) * kBlurRuns + run], v);
#pragma nounroll
                for (int t = VAA_IMG - 1 - y; t <= kBlurHalo; ++t) {
                    const float wt = wd[t];
#pragma unroll
                    for (int p = 0; p < kBlurRun; ++p) e[p] = e[p] + wt * v[p];
                }
            }
#pragma unroll
            for (int p = 0; p < kBlurRun; ++p) acc[kBlurRowsPerThread - 1][p] = e[p];
        }
#pragma unroll
        for (int o = 0; o < kBlurRowsPerThread; ++o) {
            float4* ap = reinterpret_cast<float4*>(as + (ry + o) * VAA_IMG + run * kBlurRun);
            ap[0] = make_float4(acc[o][0], acc[o][1], acc[o][2], acc[o][3]);
            ap[1] = make_float4(acc[o][4], acc[o][5], acc[o][6], acc[o][7]);
        }
    }
    __syncthreads();

    // the horizontal pass's transpose: gx[r, j] = sum over x ascending of w_|j - x| * a[r, x]; columns 0 and 223 with the folded taps
    for (int item = tid; item < kBlurBand * kBlurRuns; item += kBlurThreads) {
        const int rr = item / kBlurRuns, x0 = (item - rr * kBlurRuns) * kBlurRun;
        const float* arow = as + rr * VAA_IMG;
        float win[24], o[kBlurRun];
#pragma unroll
        for (int q = 0; q < 6; ++q) {  // columns x0 - 8 + 4q .. + 3; outside the row: zeros
            const int c = x0 - 8 + 4 * q;
            const bool in = c >= 0 && c < VAA_IMG;
            const float4 d = *reinterpret_cast<const float4*>(arow + min(max(c, 0), VAA_IMG - 4));
            win[4 * q] = in ? d.x : 0.0f; win[4 * q + 1] = in ? d.y : 0.0f; win[4 * q + 2] = in ? d.z : 0.0f; win[4 * q + 3] = in ? d.w : 0.0f;
        }
        blur_row13(w, win, o);
        if (x0 == 0) {  // column 0: output column x sends t = -6..-x here
            float e = 0.0f;
#pragma nounroll
            for (int x = 0; x <= kBlurHalo; ++x) {
                const float av = arow[x];
#pragma nounroll
                for (int t = -kBlurHalo; t <= -x; ++t) e = e + wd[-t] * av;
            }
            o[0] = e;
        }
        if (x0 == kBlurLastRun) {  // column 223: output column x sends t = 223 - x..6 here
            float e = 0.0f;
#pragma nounroll
            for (int x = VAA_IMG - 1 - kBlurHalo; x < VAA_IMG; ++x) {
                const float av = arow[x];
#pragma nounroll
                for (int t = VAA_IMG - 1 - x; t <= kBlurHalo; ++t) e = e + wd[t] * av;
            }
            o[7] = e;
        }
        *reinterpret_cast<uint4*>(dst + (size_t)(y0 + rr) * VAA_IMG + x0) = blur_pack8(o);
    }
}

static int check_blur_call(const char* who, const void* t_in, const float* taps_host, const float* taps_dev, int B, const void* t_out) {
    char note[96];
    snprintf(note, sizeof note, "; at most %ld: one workgroup per image, plane and band of %d rows", kBlurMaxB, kBlurBand);
    const int rc = check_stage_call(who, B, kBlurMaxB, note, {t_in, t_out, taps_dev}, {taps_host}, "taps_dev");
    if (rc != VAA_OK || B == 0) return rc;
    {   // a workgroup reads a halo that its neighbours write: no byte of the input may lie inside the output (K4's rule, by address ranges)
        const size_t nb = (size_t)B * 6 * VAA_NPIX * sizeof(uint16_t);
        const uintptr_t i0 = (uintptr_t)t_in, o0 = (uintptr_t)t_out;
        if (i0 < o0 + nb && o0 < i0 + nb) {
            set_error("%s: the input and the output must not overlap", who);
            return VAA_E_INVALID;
        }
    }
    for (int b = 0; b < B; ++b) {
        const float* w = taps_host + 8 * (size_t)b;
        double sum = 0.0;
        for (int k = 0; k < 7; ++k) {
            if (!isfinite(w[k]) || w[k] < 0.0f) {
                set_error("%s: taps row %d: w%d = %g is not a finite number >= 0", who, b, k, (double)w[k]);
                return VAA_E_INVALID;
            }
            sum += (k ? 2.0 : 1.0) * (double)w[k];
        }
        if (!(w[0] > 0.0f) || w[7] != 0.0f) {  // (a NaN in w[7] fails the comparison's negation too)
            set_error("%s: taps row %d: need w0 > 0 and row[7] == 0 (w0 = %g, row[7] = %g)", who, b, (double)w[0], (double)w[7]);
            return VAA_E_INVALID;
        }
        if (!(fabs(sum - 1.0) <= 1e-5)) {
            set_error("%s: taps row %d: w0 + 2*(w1 + ... + w6) = %.9g is further than 1e-5 from 1", who, b, sum);
            return VAA_E_INVALID;
        }
    }
    return VAA_OK;
}

static int blur_call(const char* who, bool fwd, const uint16_t* t_in, const float* taps_host, const float* taps_dev, int B, uint16_t* t_out,
                     void* stream) {
    const int rc = check_blur_call(who, t_in, taps_host, taps_dev, B, t_out);
    if (rc != VAA_OK || B == 0) return rc;
    BlurArgs a = {t_in, t_out, taps_dev};
    const dim3 grid((unsigned)((long)B * 6 * kBlurBands));
    if (fwd) VAA_LAUNCH(defocus_blur_fwd_kernel, grid, dim3(kBlurThreads), 0, (hipStream_t)stream, a);
    else VAA_LAUNCH(defocus_blur_bwd_kernel, grid, dim3(kBlurThreads), 0, (hipStream_t)stream, a);
    return check_launch(who);
}

}  // namespace vaa

extern "C" int vaa_defocus_blur_fwd(const uint16_t* x_bf16, const float* taps_host, const float* taps_dev, int B, uint16_t* out_bf16,
                                    void* stream) {
    return vaa::blur_call("vaa_defocus_blur_fwd", true, x_bf16, taps_host, taps_dev, B, out_bf16, stream);
}

extern "C" int vaa_defocus_blur_bwd(const uint16_t* gout_bf16, const float* taps_host, const float* taps_dev, int B, uint16_t* gx_bf16,
                                    void* stream) {
    return vaa::blur_call("vaa_defocus_blur_bwd", false, gout_bf16, taps_host, taps_dev, B, gx_bf16, stream);
}
