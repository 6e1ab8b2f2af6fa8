// vaa_crop_resize.hip — K9: crop + bilinear resize back to 224x224 of K1's planar pixel values (bf16 [B,6,224,224]) with one box per image,
// and its adjoint. One launch per call, whatever B is.
//
// The training-side sampling of the evaluation's image path (K7: experiments/robot/openvla_utils.py:132-155, crop_and_resize): the box's
// geometry is K7's own expressions, applied after K1's normalisation instead of before it. include/vaa.h states the arithmetic; every
// operation below is one separately rounded fp32 operation (the library is built with -ffp-contract=off; no FMA is written here).
//
// Both kernels stream memory (per image 602,112 B in and out) and share one shape:
//   * a thread owns 8 consecutive elements of one row of the tensor it WRITES (forward: the output, adjoint: the source gradient), in all
//     six planes: one 16-byte store per plane, consecutive lanes own consecutive runs (1 KiB of contiguous bytes per wave and store).
//   * the coordinates are computed once per thread (axis_tap: the one statement of in / t / b / l that forward and adjoint share) and
//     reused by the six planes.
//   * what a run READS is a short span of a row of the other tensor (the box side is in [0.5, 1] of the frame: at most kFwdWin / kBwdWin
//     elements). The span is fetched as aligned 16-byte vectors (8 bf16; the forward adds one dword) into a thread-private LDS window
//     (odd dword stride per thread) and read back at run-time indices: nothing is indexed dynamically in registers, no tap is a 2-byte
//     load from global memory. A thread touches only its own window, so no barrier is needed.
//   * every index that addresses memory is clamped to the row / the window: a device copy of the boxes that differs from the validated
//     host copy cannot read or write outside the tensors.
// The adjoint is a gather per source element (no atomics): the candidate outputs of a source index j are the 6 consecutive indices from
// floor((j - org) / scale) - 2 (a side >= 0.5 puts every output whose taps touch j among them), and each is accepted only by re-evaluating
// the forward's t and b (axis_tap) — the result is the transpose of what the forward did, not of a second formula.
#include "vaa_common.h"

#pragma clang fp contract(off)

namespace vaa {

constexpr int kCrPix = 8;                                  // elements per thread and plane (one 16-byte vector)
constexpr int kCrItemsPerRow = VAA_IMG / kCrPix;           // 28
constexpr int kCrItemsPerImg = VAA_IMG * kCrItemsPerRow;   // 6272 = 24.5 workgroups: an odd batch leaves a half-filled last workgroup
constexpr int kCrThreads = 256;
constexpr int kCrLastVec = VAA_IMG - kCrPix;               // 216: the last 16-byte vector of a row starts here
constexpr int kFwdWin = 18;                                // forward: source elements per row and run (two vectors + one dword)
constexpr int kFwdStride = 2 * (kFwdWin / 2) + 1;          // dwords per thread: two rows, odd
constexpr int kBwdCand = 6;                                // adjoint: candidate outputs per source index and axis
constexpr int kBwdWin = 32;                                // adjoint: gradient elements per row and run (four vectors)
constexpr int kBwdStride = kBwdWin / 2 + 1;                // dwords per thread, odd

struct CropArgs {
    const uint16_t* in;   // forward: x; adjoint: gout
    uint16_t* out;        // forward: out; adjoint: gx
    const float* boxes;   // dev [B,4] {y1, x1, y2, x2}
    int B;
};

struct AxisTap {
    int t, b;   // the two source indices (floor, ceil of the clamped coordinate)
    float l;    // weight of index b; index t has 1 - l
};

// include/vaa.h (K9): org = y1*223, scale = ((y2 - y1)*223)/223;  in = min(max(org + i*scale, 0), 223);  t = floorf(in), b = ceilf(in), l = in - t
__device__ __forceinline__ void axis_box(float lo, float hi, float& org, float& scale) {
    org = lo * (float)(VAA_IMG - 1);
    scale = ((hi - lo) * (float)(VAA_IMG - 1)) / (float)(VAA_IMG - 1);
}

__device__ __forceinline__ AxisTap axis_tap(float org, float scale, int i) {
    const float in = fminf(fmaxf(org + (float)i * scale, 0.0f), (float)(VAA_IMG - 1));  // fmaxf(NaN, 0) = 0: always inside the axis
    const float t = floorf(in);
    AxisTap a;
    a.t = (int)t;
    a.b = (int)ceilf(in);
    a.l = in - t;
    return a;
}

// the adjoint's weight of output index i on source index r: [t == r]*(1 - l) + [b == r]*l; never 0 for an output that touches r
// (l < 1 always, l > 0 whenever b != t), exactly 0 for one that does not, or that lies outside the axis
__device__ __forceinline__ float axis_weight(float org, float scale, int i, int r) {
    if (i < 0 || i >= VAA_IMG) return 0.0f;
    const AxisTap a = axis_tap(org, scale, i);
    const float wt = a.t == r ? 1.0f - a.l : 0.0f;
    const float wb = a.b == r ? a.l : 0.0f;
    return wt + wb;
}

// first candidate output of source index r: floor((r - org) / scale) - 2, kept inside int range for any float
__device__ __forceinline__ int first_candidate(float org, float scale, int r) {
    const float e = floorf(((float)r - org) / scale);
    return (int)fminf(fmaxf(e, -8.0f), (float)(VAA_IMG + 8)) - 2;
}

// element k (bf16) of a window of dwords -> fp32
__device__ __forceinline__ float win_at(const uint32_t* w, int k) {
    const uint32_t d = w[k >> 1];
    return __uint_as_float((k & 1) ? (d & 0xffff0000u) : (d << 16));
}

__device__ __forceinline__ uint4 pack8(const float* v) {
    uint32_t q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = f32_to_bf16_bits(v[2 * i]) | (f32_to_bf16_bits(v[2 * i + 1]) << 16);
    return make_uint4(q[0], q[1], q[2], q[3]);
}

__global__ __launch_bounds__(kCrThreads) void crop_resize_fwd_kernel(const CropArgs a) {
    __shared__ uint32_t win[kCrThreads * kFwdStride];
    const int tid = threadIdx.x;
    const long item = (long)blockIdx.x * kCrThreads + tid, total = (long)a.B * kCrItemsPerImg;
    if (item >= total) return;  // the half-filled last workgroup of an odd batch
    const long grow = item / kCrItemsPerRow;
    const int x0 = (int)(item - grow * kCrItemsPerRow) * kCrPix;
    const int b = (int)(grow / VAA_IMG), y = (int)(grow - (long)b * VAA_IMG);

    const float4 box = *reinterpret_cast<const float4*>(a.boxes + 4 * (size_t)b);  // {y1, x1, y2, x2}
    float oy, sy, ox, sx;
    axis_box(box.x, box.z, oy, sy);
    axis_box(box.y, box.w, ox, sx);
    const AxisTap ty = axis_tap(oy, sy, y);

    // columns: the run's taps lie in [left(x0), left(x0) + 9] (scale <= 1); the window starts at the vector that holds left(x0)
    float lx[kCrPix];
    int rl[kCrPix], rr[kCrPix];
    int c0 = 0;
#pragma unroll
    for (int p = 0; p < kCrPix; ++p) {
        const AxisTap tx = axis_tap(ox, sx, x0 + p);
        if (p == 0) c0 = tx.t & ~(kCrPix - 1);
        lx[p] = tx.l;
        rl[p] = min(max(tx.t - c0, 0), kFwdWin - 1);
        rr[p] = min(max(tx.b - c0, 0), kFwdWin - 1);
    }
    // window elements 0..7, 8..15, 16..17 come from columns c0, c0 + 8, c0 + 16; a piece that would leave the row is moved back into it
    // (its elements are columns >= 224 then, which no tap reads)
    const int v1 = min(c0 + kCrPix, kCrLastVec), v2 = min(c0 + 2 * kCrPix, VAA_IMG - 2);

    uint32_t* mywin = win + tid * kFwdStride;
    const size_t img = (size_t)b * 6 * VAA_NPIX;
    const size_t obase = img + (size_t)y * VAA_IMG + x0;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const uint16_t* rt = a.in + img + (size_t)c * VAA_NPIX + (size_t)ty.t * VAA_IMG;
        const uint16_t* rb = a.in + img + (size_t)c * VAA_NPIX + (size_t)ty.b * VAA_IMG;
        const uint4 t0 = *reinterpret_cast<const uint4*>(rt + c0), t1 = *reinterpret_cast<const uint4*>(rt + v1);
        const uint4 b0 = *reinterpret_cast<const uint4*>(rb + c0), b1 = *reinterpret_cast<const uint4*>(rb + v1);
        const uint32_t t2 = *reinterpret_cast<const uint32_t*>(rt + v2), b2 = *reinterpret_cast<const uint32_t*>(rb + v2);
        uint32_t* wt = mywin;
        uint32_t* wb = mywin + kFwdWin / 2;
        wt[0] = t0.x; wt[1] = t0.y; wt[2] = t0.z; wt[3] = t0.w; wt[4] = t1.x; wt[5] = t1.y; wt[6] = t1.z; wt[7] = t1.w; wt[8] = t2;
        wb[0] = b0.x; wb[1] = b0.y; wb[2] = b0.z; wb[3] = b0.w; wb[4] = b1.x; wb[5] = b1.y; wb[6] = b1.z; wb[7] = b1.w; wb[8] = b2;
        float v[kCrPix];
#pragma unroll
        for (int p = 0; p < kCrPix; ++p) {
            const float tl = win_at(wt, rl[p]), tr = win_at(wt, rr[p]), bl = win_at(wb, rl[p]), br = win_at(wb, rr[p]);
            const float top = tl + (tr - tl) * lx[p];
            const float bot = bl + (br - bl) * lx[p];
            v[p] = top + (bot - top) * ty.l;
        }
        *reinterpret_cast<uint4*>(a.out + obase + (size_t)c * VAA_NPIX) = pack8(v);
    }
}

__global__ __launch_bounds__(kCrThreads) void crop_resize_bwd_kernel(const CropArgs a) {
    __shared__ uint32_t win[kCrThreads * kBwdStride];
    const int tid = threadIdx.x;
    const long item = (long)blockIdx.x * kCrThreads + tid, total = (long)a.B * kCrItemsPerImg;
    if (item >= total) return;
    const long grow = item / kCrItemsPerRow;
    const int j0 = (int)(item - grow * kCrItemsPerRow) * kCrPix;
    const int b = (int)(grow / VAA_IMG), r = (int)(grow - (long)b * VAA_IMG);

    const float4 box = *reinterpret_cast<const float4*>(a.boxes + 4 * (size_t)b);
    float oy, sy, ox, sx;
    axis_box(box.x, box.z, oy, sy);
    axis_box(box.y, box.w, ox, sx);

    // columns: per source column j0 + q its first candidate output and the 6 candidates' weights (0: not a tap of that column)
    const int xlo = min(max(first_candidate(ox, sx, j0), 0), VAA_IMG - 1);
    const int xb = xlo & ~(kCrPix - 1);  // the window starts at the vector that holds the run's first candidate
    float wx[kCrPix][kBwdCand];
    int rx[kCrPix];
    int xhi = xlo;
#pragma unroll
    for (int q = 0; q < kCrPix; ++q) {
        const int xs = first_candidate(ox, sx, j0 + q);
        rx[q] = xs - xb;
#pragma unroll
        for (int k = 0; k < kBwdCand; ++k) {
            wx[q][k] = axis_weight(ox, sx, xs + k, j0 + q);
            if (wx[q][k] != 0.0f) xhi = max(xhi, xs + k);
        }
    }
    const int nvec = min((xhi - xb) / kCrPix + 1, kBwdWin / kCrPix);  // vectors of the window that hold a tap

    // rows: the 6 candidate output rows of source row r and their weights (0: not a tap of row r, or outside the frame: never an address)
    const int ys = first_candidate(oy, sy, r);
    float wy[kBwdCand];
#pragma unroll
    for (int k = 0; k < kBwdCand; ++k) wy[k] = axis_weight(oy, sy, ys + k, r);

    uint32_t* mywin = win + tid * kBwdStride;
    const size_t img = (size_t)b * 6 * VAA_NPIX;
    const size_t obase = img + (size_t)r * VAA_IMG + j0;
#pragma nounroll
    for (int c = 0; c < 6; ++c) {
        float acc[kCrPix];
#pragma unroll
        for (int q = 0; q < kCrPix; ++q) acc[q] = 0.0f;
#pragma unroll
        for (int k = 0; k < kBwdCand; ++k) {  // ascending output rows
            if (wy[k] == 0.0f) continue;
            const uint16_t* g = a.in + img + (size_t)c * VAA_NPIX + (size_t)(ys + k) * VAA_IMG;
#pragma unroll
            for (int v = 0; v < kBwdWin / kCrPix; ++v) {
                if (v < nvec) {
                    const uint4 d = *reinterpret_cast<const uint4*>(g + min(xb + v * kCrPix, kCrLastVec));
                    mywin[4 * v] = d.x; mywin[4 * v + 1] = d.y; mywin[4 * v + 2] = d.z; mywin[4 * v + 3] = d.w;
                }
            }
#pragma unroll
            for (int q = 0; q < kCrPix; ++q) {
                float h = 0.0f;  // ascending output columns
#pragma unroll
                for (int kk = 0; kk < kBwdCand; ++kk) {
                    const float gv = win_at(mywin, min(max(rx[q] + kk, 0), kBwdWin - 1));
                    if (wx[q][kk] != 0.0f) h = h + wx[q][kk] * gv;
                }
                acc[q] = acc[q] + wy[k] * h;
            }
        }
        *reinterpret_cast<uint4*>(a.out + obase + (size_t)c * VAA_NPIX) = pack8(acc);
    }
}

static int check_crop_call(const char* who, const void* t_in, const float* boxes_host, const float* boxes_dev, int B, const void* t_out) {
    // at most 0x7fffffff work items (B * kCrItemsPerImg)
    const int rc = check_stage_call(who, B, 0x7fffffffL / kCrItemsPerImg, "", {t_in, t_out, boxes_dev}, {boxes_host}, "boxes_dev");
    if (rc != VAA_OK || B == 0) return rc;
    for (int b = 0; b < B; ++b)
        for (int ax = 0; ax < 2; ++ax) {
            const float lo = boxes_host[4 * b + ax], hi = boxes_host[4 * b + 2 + ax];
            if (!(isfinite(lo) && isfinite(hi) && lo >= 0.0f && lo < hi && hi <= 1.0f && hi - lo >= 0.5f)) {
                set_error("%s: box %d has %s1 = %g, %s2 = %g: need 0 <= %s1 < %s2 <= 1 and a side of at least 0.5", who, b, ax ? "x" : "y",
                          (double)lo, ax ? "x" : "y", (double)hi, ax ? "x" : "y", ax ? "x" : "y");
                return VAA_E_INVALID;
            }
        }
    return VAA_OK;
}

static int crop_call(const char* who, bool fwd, const uint16_t* t_in, const float* boxes_host, const float* boxes_dev, int B, uint16_t* t_out,
                     void* stream) {
    const int rc = check_crop_call(who, t_in, boxes_host, boxes_dev, B, t_out);
    if (rc != VAA_OK || B == 0) return rc;
    CropArgs a = {t_in, t_out, boxes_dev, B};
    const long total = (long)B * kCrItemsPerImg;
    const dim3 grid((unsigned)((total + kCrThreads - 1) / kCrThreads));
    if (fwd) VAA_LAUNCH(crop_resize_fwd_kernel, grid, dim3(kCrThreads), 0, (hipStream_t)stream, a);
    else VAA_LAUNCH(crop_resize_bwd_kernel, grid, dim3(kCrThreads), 0, (hipStream_t)stream, a);
    return check_launch(who);
}

}  // namespace vaa

extern "C" int vaa_crop_resize_fwd(const uint16_t* x_bf16, const float* boxes_host, const float* boxes_dev, int B, uint16_t* out_bf16,
                                   void* stream) {
    return vaa::crop_call("vaa_crop_resize_fwd", true, x_bf16, boxes_host, boxes_dev, B, out_bf16, stream);
}

extern "C" int vaa_crop_resize_bwd(const uint16_t* gout_bf16, const float* boxes_host, const float* boxes_dev, int B, uint16_t* gx_bf16,
                                   void* stream) {
    return vaa::crop_call("vaa_crop_resize_bwd", false, gout_bf16, boxes_host, boxes_dev, B, gx_bf16, stream);
}
