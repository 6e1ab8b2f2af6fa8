// vaa_eval_pre.hip — K7: the evaluation's image front end behind the eval-time paste (K5), one launch per batch:
// centre crop + bilinear resize back to 224x224, uint8 conversion, dual normalise, bf16 cast.
//
// Replaces, per camera frame of the reference's evaluation (experiments/robot/openvla_utils.py:132-166): convert_image_dtype(float32),
// crop_and_resize (:81-124 -> tf.image.crop_and_resize, bilinear), clip_by_value, convert_image_dtype(uint8, saturate=True) and the
// processor's to-[0,1] / normalise-per-tower / 6-channel stack / bf16 cast. include/vaa.h states the arithmetic; every operation below is
// one separately rounded fp32 operation (the library is built with -ffp-contract=off; no FMA is written here).
//
// HBM-bound streaming kernel: per frame 150,528 B of u8 pixels in, 602,112 B of bf16 planes out. Layout/mapping:
//   * a thread owns 8 consecutive output pixels of one row and writes one 16-byte vector into each of the 6 planes; consecutive lanes own
//     consecutive runs, so every store instruction of a wave writes 1 KiB of contiguous bytes of a plane (K1's store shape).
//   * the run's source columns span at most kWin pixels of the two source rows (the box is never wider than the frame, so the source
//     coordinate advances by at most one pixel per output pixel): each row's span is fetched as 36 contiguous bytes (dword-aligned 16 + 16 + 4
//     byte loads), shifted to the first pixel in registers and split into one dword per source pixel at compile-time positions.
//   * which source pixel an output pixel reads is a run-time index: the per-pixel dwords go through a thread-private LDS window (an odd
//     dword stride per thread keeps the lanes on different banks) and come back as {left, right} pairs — nothing is indexed dynamically
//     in registers (that would live in scratch), no tap is a byte load from global memory.
//   * the resized byte is normalised through K1's 3x256 table in LDS (fill_norm_lut: the same fill, the same bits).
#include "vaa_common.h"

#pragma clang fp contract(off)

namespace vaa {

struct EvalPreArgs {
    const uint8_t* img;
    uint16_t* out;
    int B;
    float org;     // y1 * 223 = x1 * 223 (the box is centred and square)
    float scale;   // ((y2 - y1) * 223) / 223
    Norm6 nrm;
};

constexpr int kPrePix = 8;                                  // output pixels per thread
constexpr int kPreItemsPerRow = VAA_IMG / kPrePix;          // 28
constexpr int kPreItemsPerImg = VAA_IMG * kPreItemsPerRow;  // 6272 = 24.5 workgroups: an odd batch leaves a half-filled last workgroup
constexpr int kPreThreads = 256;
constexpr int kWin = 12;                 // source pixels fetched per row and run (36 bytes)
constexpr int kWinSlots = kWin + 1;      // + one zero slot: the (weight-0) right neighbour of the frame's last column
constexpr int kWinStride = 2 * kWinSlots + 1;  // dwords per thread: two rows, odd
constexpr int kWinLast = VAA_IMG - kWin;  // 212: the last first-column whose 12-pixel window stays inside the row

struct __attribute__((packed, aligned(4))) Dwords4 { uint32_t v[4]; };  // a 16-byte load that needs dword alignment only

// 36 bytes from `p` (dword aligned) + a shift of sh bytes (0..3) -> pixel k's three bytes in the low 24 bits of px[k], k < 12.
// Without a shift the window holds exactly 12 pixels; with one, pixel 11 is incomplete (callers never read it then: see the kernel).
__device__ __forceinline__ void load_window(const uint8_t* p, uint32_t sh, uint32_t* px) {
    const Dwords4 q0 = *reinterpret_cast<const Dwords4*>(p), q1 = *reinterpret_cast<const Dwords4*>(p + 16);
    const uint32_t w[10] = {q0.v[0], q0.v[1], q0.v[2], q0.v[3], q1.v[0], q1.v[1], q1.v[2], q1.v[3], *reinterpret_cast<const uint32_t*>(p + 32), 0u};
    uint32_t a[10];
#pragma unroll
    for (int j = 0; j < 9; ++j) a[j] = __builtin_amdgcn_alignbyte(w[j + 1], w[j], sh);  // bytes sh.. of the pair
    a[9] = 0u;
#pragma unroll
    for (int k = 0; k < kWin; ++k) px[k] = __builtin_amdgcn_alignbyte(a[(3 * k) / 4 + 1], a[(3 * k) / 4], (uint32_t)((3 * k) & 3)) & 0xffffffu;
}

template <bool kCrop>
__global__ __launch_bounds__(kPreThreads) void eval_preprocess_kernel(const EvalPreArgs a) {
    __shared__ uint32_t lut[3 * 256];
    __shared__ uint32_t win[kPreThreads * kWinStride];
    const int tid = threadIdx.x;
    fill_norm_lut(lut, a.nrm, tid, kPreThreads);
    __syncthreads();
    const long item = (long)blockIdx.x * kPreThreads + tid, total = (long)a.B * kPreItemsPerImg;
    if (item >= total) return;  // the half-filled last workgroup of an odd batch
    const long grow = item / kPreItemsPerRow;
    const int x0 = (int)(item - grow * kPreItemsPerRow) * kPrePix;
    const int b = (int)(grow / VAA_IMG), y = (int)(grow - (long)b * VAA_IMG);

    // rows: in_y = y1*223 + y*scale, top = floor, bottom = ceil, ly = in_y - top; a coordinate outside [0, 223] zeroes the pixel
    const float in_y = kCrop ? a.org + (float)y * a.scale : (float)y;
    const bool y_ok = in_y >= 0.0f && in_y <= (float)(VAA_IMG - 1);
    const float ty = floorf(in_y), ly = in_y - ty;
    const int rt = y_ok ? (int)ty : 0, rb = y_ok ? (int)ceilf(in_y) : 0;

    // columns: the same formulas. left[p] - c0 < kWin for every pixel with a coordinate inside the frame (scale <= 1, see the file comment)
    float lx[kPrePix];
    int rel[kPrePix];
    bool ok[kPrePix];
    int c0 = 0;
#pragma unroll
    for (int p = 0; p < kPrePix; ++p) {
        const float in_x = kCrop ? a.org + (float)(x0 + p) * a.scale : (float)(x0 + p);
        ok[p] = y_ok && in_x >= 0.0f && in_x <= (float)(VAA_IMG - 1);
        const float l = floorf(in_x);
        lx[p] = in_x - l;
        const int li = ok[p] ? (int)l : 0;
        if (p == 0) c0 = min(li, kWinLast);  // first fetched column: clamped so that the 36 bytes stay inside the row (then sh == 0)
        // the right tap is column left + 1: where ceil(in_x) == left the weight lx is 0 and tl + (tr - tl)*0 == tl for any finite tr
        rel[p] = min(max(li - c0, 0), kWin - 1);
    }

    // the two rows' windows -> this thread's LDS slots
    uint32_t* mywin = win + tid * kWinStride;
    {
        const size_t off_t = (((size_t)b * VAA_IMG + rt) * VAA_IMG + c0) * 3, off_b = (((size_t)b * VAA_IMG + rb) * VAA_IMG + c0) * 3;
        uint32_t pt[kWin], pb[kWin];
        load_window(a.img + (off_t & ~(size_t)3), (uint32_t)(off_t & 3), pt);
        load_window(a.img + (off_b & ~(size_t)3), (uint32_t)(off_b & 3), pb);
#pragma unroll
        for (int k = 0; k < kWin; ++k) { mywin[k] = pt[k]; mywin[kWinSlots + k] = pb[k]; }
        mywin[kWin] = 0u;
        mywin[kWinSlots + kWin] = 0u;
    }

    uint32_t L[3][kPrePix];  // packed {bf16 plane c, bf16 plane c+3} per pixel
    const float inv255 = 1.0f / 255.0f;
#pragma unroll
    for (int p = 0; p < kPrePix; ++p) {
        const uint32_t tl = mywin[rel[p]], tr = mywin[rel[p] + 1], bl = mywin[kWinSlots + rel[p]], br = mywin[kWinSlots + rel[p] + 1];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint32_t q;
            if (kCrop) {
                const float ftl = (float)((tl >> (8 * c)) & 0xffu) * inv255, ftr = (float)((tr >> (8 * c)) & 0xffu) * inv255;
                const float fbl = (float)((bl >> (8 * c)) & 0xffu) * inv255, fbr = (float)((br >> (8 * c)) & 0xffu) * inv255;
                const float top = ftl + (ftr - ftl) * lx[p];
                const float bot = fbl + (fbr - fbl) * lx[p];
                float v = top + (bot - top) * ly;
                if (!ok[p]) v = 0.0f;                    // extrapolation value of crop_and_resize
                v = fminf(fmaxf(v, 0.0f), 1.0f);         // clip_by_value(image, 0, 1)
                q = (uint32_t)min(255, (int)(v * 255.5f));  // convert_image_dtype(uint8, saturate=True): scale by 255.5, truncate
            } else {
                q = (tl >> (8 * c)) & 0xffu;
            }
            L[c][p] = lut[c * 256 + q];
        }
    }
    const size_t obase = ((size_t)b * 6 * VAA_IMG + y) * VAA_IMG + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        uint32_t lo4[4], hi4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            lo4[q] = __builtin_amdgcn_perm(L[c][2 * q + 1], L[c][2 * q], 0x05040100u);
            hi4[q] = __builtin_amdgcn_perm(L[c][2 * q + 1], L[c][2 * q], 0x07060302u);
        }
        *reinterpret_cast<uint4*>(a.out + obase + (size_t)c * VAA_NPIX) = make_uint4(lo4[0], lo4[1], lo4[2], lo4[3]);
        *reinterpret_cast<uint4*>(a.out + obase + (size_t)(c + 3) * VAA_NPIX) = make_uint4(hi4[0], hi4[1], hi4[2], hi4[3]);
    }
}

}  // namespace vaa

extern "C" int vaa_eval_preprocess(const uint8_t* img_u8, int B, float crop_scale, const float* mean6, const float* std6, uint16_t* out_bf16,
                                   void* stream) {
    using namespace vaa;
    const char* who = "vaa_eval_preprocess";
    if (!(crop_scale == 0.0f || (crop_scale > 0.0f && crop_scale <= 1.0f))) {  // NaN fails both
        set_error("%s: crop_scale %g is neither 0 (no crop) nor in (0, 1]", who, (double)crop_scale);
        return VAA_E_INVALID;
    }
    if (B < 0 || (long)B * kPreItemsPerImg > 0x7fffffffL) {
        set_error("%s: bad batch size (B=%d)", who, B);
        return VAA_E_INVALID;
    }
    if (B == 0) return VAA_OK;  // empty batch: nothing to read or write (pointers may be null)
    if (!img_u8 || !mean6 || !std6 || !out_bf16) {
        set_error("%s: null pointer argument", who);
        return VAA_E_INVALID;
    }
    if (((uintptr_t)img_u8 & 3u) || ((uintptr_t)out_bf16 & 15u)) {
        set_error("%s: img_u8 must be 4-byte and out_bf16 16-byte aligned", who);
        return VAA_E_INVALID;
    }
    EvalPreArgs a = {};
    a.img = img_u8; a.out = out_bf16; a.B = B;
    // the box of crop_and_resize (openvla_utils.py:101-115) and CropAndResize's scale, in fp32, one rounding per operation
    const float s = fminf(fmaxf(sqrtf(crop_scale), 0.0f), 1.0f);
    const float y1 = (1.0f - s) / 2.0f;
    const float y2 = y1 + s;
    a.org = y1 * (float)(VAA_IMG - 1);
    a.scale = ((y2 - y1) * (float)(VAA_IMG - 1)) / (float)(VAA_IMG - 1);
    for (int q = 0; q < 6; ++q) { a.nrm.mean[q] = mean6[q]; a.nrm.stdv[q] = std6[q]; }
    const long total = (long)B * kPreItemsPerImg;
    const dim3 grid((unsigned)((total + kPreThreads - 1) / kPreThreads));
    if (crop_scale != 0.0f) VAA_LAUNCH(eval_preprocess_kernel<true>, grid, dim3(kPreThreads), 0, (hipStream_t)stream, a);
    else VAA_LAUNCH(eval_preprocess_kernel<false>, grid, dim3(kPreThreads), 0, (hipStream_t)stream, a);  // the output byte is the source byte
    return check_launch(who);
}
