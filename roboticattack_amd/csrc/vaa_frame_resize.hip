// vaa_frame_resize.hip — K8: a simulator's camera frames [B,H,W,3] uint8 -> [B,224,224,3] uint8 through a separable filter whose taps come
// from the host (lanczos3 with antialias for the evaluation: resize.lanczos3_taps), round half to even, clip, uint8. One launch per batch.
//
// Replaces, per camera frame of the reference's evaluations, tf.image.resize(..., method="lanczos3", antialias=True) + round + clip + cast
// (experiments/robot/libero/libero_utils.py:44-45, experiments/robot/bridge/bridgev2_utils.py:112) and LIBERO's img[::-1, ::-1] in front of
// it (rot180, folded into the indexing). include/vaa.h states the arithmetic; every operation below is one separately rounded fp32 operation
// (the library is built with -ffp-contract=off; no FMA is written here) and the taps of both passes are added in ascending source index.
//
// Shape: a 256-thread workgroup owns a band of 8 output rows of one frame (28 bands per frame). It walks the source rows that band needs in
// ascending chunks of 8 (4 when a row is longer than 1024 pixels, so that the LDS stays under 64 KiB). Per chunk:
//   stage   the chunk's source rows go into LDS as they lie in memory: 3W contiguous bytes fetched as dwords from the dword-aligned address at
//           or below the row's first byte (consecutive lanes, consecutive dwords). A row's first byte sits at `lead` = offset & 3 inside its
//           first dword (the base is dword aligned, so that dword is inside the buffer); the last dword of the buffer's last row may reach
//           past the end of src and is then put together from byte loads.
//   H pass  thread x < 224 owns output column x of every row of the chunk: per tap one weight load, per row two LDS dwords + v_alignbyte give
//           the pixel's three bytes; the results go into an fp32 LDS tile [rows][672].
//   V pass  a thread owns up to three of the 672 (column, channel) elements and keeps the band's 8 running sums of each in registers: a chunk's
//           rows are added in ascending order to every output row whose span holds them (the band's 8 x Ty weights sit in LDS).
// After the last chunk the 8 x 672 result bytes are collected in LDS and stored as 336 16-byte vectors (the band is contiguous in dst).
// No atomics, no hand-over between workgroups, no inline assembly, no runtime-indexed register arrays.
#include "vaa_common.h"

#pragma clang fp contract(off)

namespace vaa {

constexpr int kRsThreads = 256;
constexpr int kRsBand = 8;                        // output rows per workgroup
constexpr int kRsBands = VAA_IMG / kRsBand;       // 28
constexpr int kRsRowElems = VAA_IMG * 3;          // 672 (column, channel) elements of an output row
constexpr int kRsMaxChunk = 8;                    // source rows per chunk (4 when W > 1024)
constexpr int kRsElemsPerThread = 3;              // ceil(672 / 256)
constexpr int kRsMinSide = 8, kRsMaxSide = 2048;

struct FrameResizeArgs {
    const uint8_t* src;
    uint8_t* dst;
    const int32_t* sx;   // [224]
    const int32_t* sy;   // [224]
    const float* wx;     // [224, Tx]
    const float* wy;     // [224, Ty]
    size_t src_bytes;    // B*H*W*3
    int H, W, Tx, Ty, rot, chunk, pitch_dw;
};

__host__ __device__ inline int rs_pitch_dw(int W) { return (3 * W + 3 + 3) / 4 + 1; }  // a row's dwords at any lead + one zero dword behind

__global__ __launch_bounds__(kRsThreads) void frame_resize_kernel(const FrameResizeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t rs_lds[];
    float* tile = reinterpret_cast<float*>(rs_lds);                 // [chunk][672] fp32; the band's result bytes at the end
    uint32_t* raw = rs_lds + a.chunk * kRsRowElems;                 // [chunk][pitch_dw] source bytes
    int* lead_s = reinterpret_cast<int*>(raw + a.chunk * a.pitch_dw);  // [8]: where each staged row's first byte sits in its first dword
    float* wyb = reinterpret_cast<float*>(lead_s + kRsMaxChunk);    // [8][Ty]: the vertical weights of the band's rows
    const int tid = threadIdx.x;
    const int b = blockIdx.x / kRsBands, y0 = (blockIdx.x - b * kRsBands) * kRsBand;
    const int H = a.H, W = a.W, Tx = a.Tx, Ty = a.Ty, C = a.chunk;
    for (int i = tid; i < kRsBand * Ty; i += kRsThreads) wyb[i] = a.wy[(size_t)y0 * Ty + i];  // read behind the first chunk's barrier

    // the band's source rows (wave-uniform), clamped to the frame
    int sy[kRsBand];
    int rlo = H - 1, rhi = 0;
#pragma unroll
    for (int y = 0; y < kRsBand; ++y) {
        sy[y] = min(max(a.sy[y0 + y], 0), H - 1);
        rlo = min(rlo, sy[y]);
        rhi = max(rhi, sy[y] + Ty - 1);
    }
    rlo = max(rlo, 0);
    rhi = min(rhi, H - 1);

    float acc[kRsElemsPerThread][kRsBand];
#pragma unroll
    for (int j = 0; j < kRsElemsPerThread; ++j)
#pragma unroll
        for (int y = 0; y < kRsBand; ++y) acc[j][y] = 0.0f;

    const int sx = tid < VAA_IMG ? min(max(a.sx[tid], 0), W - 1) : 0;
    const float* wxr = a.wx + (size_t)(tid < VAA_IMG ? tid : 0) * Tx;

    for (int r0 = rlo; r0 <= rhi; r0 += C) {
        __syncthreads();  // the previous chunk's tile and rows are no longer read
        // ---- stage: source rows r0 .. r0+C-1 (clamped to the frame) as dwords ----
        for (int k = 0; k < C; ++k) {
            const int r = min(r0 + k, H - 1);
            const int pr = a.rot ? H - 1 - r : r;
            const size_t goff = ((size_t)b * H + pr) * (size_t)(3 * W);
            const int lead = (int)(goff & 3);
            const size_t a0 = goff - lead;
            const int nd = (lead + 3 * W + 3) >> 2;
            if (tid == 0) lead_s[k] = lead;
            uint32_t* rowd = raw + k * a.pitch_dw;
            for (int d = tid; d <= nd; d += kRsThreads) {
                uint32_t v = 0u;
                const size_t off = a0 + 4 * (size_t)d;
                if (d < nd) {
                    if (off + 4 <= a.src_bytes) {
                        v = *reinterpret_cast<const uint32_t*>(a.src + off);
                    } else {  // the buffer's last dword is incomplete
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (off + q < a.src_bytes) v |= (uint32_t)a.src[off + q] << (8 * q);
                    }
                }
                rowd[d] = v;  // d == nd: the zero dword behind the row (the H pass reads dword pairs)
            }
        }
        __syncthreads();
        // ---- H pass: thread x, every row of the chunk ----
        if (tid < VAA_IMG) {
            float h[kRsMaxChunk][3];
#pragma unroll
            for (int k = 0; k < kRsMaxChunk; ++k) h[k][0] = h[k][1] = h[k][2] = 0.0f;
            for (int t = 0; t < Tx; ++t) {
                const float w = wxr[t];
                const int j = min(sx + t, W - 1);
                const int j3 = 3 * (a.rot ? W - 1 - j : j);
#pragma unroll
                for (int k = 0; k < kRsMaxChunk; ++k) {
                    if (k < C) {
                        const int q = lead_s[k] + j3;
                        const uint32_t* rowd = raw + k * a.pitch_dw + (q >> 2);
                        const uint32_t px = __builtin_amdgcn_alignbyte(rowd[1], rowd[0], (uint32_t)(q & 3));
                        h[k][0] = h[k][0] + w * (float)(px & 0xffu);
                        h[k][1] = h[k][1] + w * (float)((px >> 8) & 0xffu);
                        h[k][2] = h[k][2] + w * (float)((px >> 16) & 0xffu);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kRsMaxChunk; ++k) {
                if (k < C) {
                    float* o = tile + k * kRsRowElems + 3 * tid;
                    o[0] = h[k][0]; o[1] = h[k][1]; o[2] = h[k][2];
                }
            }
        }
        __syncthreads();
        // ---- V pass: the chunk's rows, ascending, into every output row whose span holds them ----
        const int nk = min(C, rhi - r0 + 1);
#pragma unroll
        for (int y = 0; y < kRsBand; ++y) {
            const int k_lo = max(sy[y] - r0, 0), k_hi = min(sy[y] + Ty - r0, nk);  // t = r0 + k - sy[y] in [0, Ty)
            const float* wyr = wyb + y * Ty + (r0 - sy[y]);
            for (int k = k_lo; k < k_hi; ++k) {
                const float w = wyr[k];
#pragma unroll
                for (int j = 0; j < kRsElemsPerThread; ++j) {
                    const int e = tid + j * kRsThreads;
                    if (e < kRsRowElems) acc[j][y] = acc[j][y] + w * tile[k * kRsRowElems + e];
                }
            }
        }
    }

    // ---- round half to even, clip, uint8; the band's bytes through LDS into 16-byte stores ----
    __syncthreads();
    uint8_t* outb = reinterpret_cast<uint8_t*>(rs_lds);  // 8 x 672 bytes (the tile holds at least 4 x 672 floats)
#pragma unroll
    for (int y = 0; y < kRsBand; ++y)
#pragma unroll
        for (int j = 0; j < kRsElemsPerThread; ++j) {
            const int e = tid + j * kRsThreads;
            if (e < kRsRowElems) outb[y * kRsRowElems + e] = (uint8_t)(int)fminf(fmaxf(rintf(acc[j][y]), 0.0f), 255.0f);
        }
    __syncthreads();
    uint8_t* drow = a.dst + ((size_t)b * VAA_IMG + y0) * kRsRowElems;
    for (int v = tid; v < kRsBand * kRsRowElems / 16; v += kRsThreads)
        *reinterpret_cast<uint4*>(drow + 16 * v) = *reinterpret_cast<const uint4*>(outb + 16 * v);
}

static int check_axis(const char* who, const char* axis, const int32_t* start, const float* w, int T, int n) {
    for (int i = 0; i < VAA_IMG; ++i) {
        if (start[i] < 0 || (long)start[i] + T - 1 > n - 1) {
            set_error("%s: start_%s[%d] = %d with %d taps leaves the axis of %d", who, axis, i, start[i], T, n);
            return VAA_E_INVALID;
        }
        for (int t = 0; t < T; ++t)
            if (!isfinite(w[(size_t)i * T + t])) {
                set_error("%s: w_%s[%d][%d] is not finite", who, axis, i, t);
                return VAA_E_INVALID;
            }
    }
    return VAA_OK;
}

}  // namespace vaa

extern "C" size_t vaa_frame_resize_taps_bytes(int Tx, int Ty) {
    if (Tx < 1 || Ty < 1 || Tx > VAA_FRAME_RESIZE_MAX_TAPS || Ty > VAA_FRAME_RESIZE_MAX_TAPS) return 0;
    return (size_t)VAA_IMG * (2 + Tx + Ty) * 4;
}

extern "C" int vaa_frame_resize(const uint8_t* src_u8, int B, int H, int W, int rot180, const int32_t* start_x, const float* w_x, int Tx,
                                const int32_t* start_y, const float* w_y, int Ty, const void* taps_dev, uint8_t* dst_u8, void* stream) {
    using namespace vaa;
    const char* who = "vaa_frame_resize";
    if (B < 0 || (long)B * kRsBands > 0x7fffffffL) {
        set_error("%s: bad batch size (B=%d)", who, B);
        return VAA_E_INVALID;
    }
    if (B == 0) return VAA_OK;  // empty batch: nothing to read or write (pointers may be null)
    if (!src_u8 || !start_x || !w_x || !start_y || !w_y || !taps_dev || !dst_u8) {
        set_error("%s: null pointer argument", who);
        return VAA_E_INVALID;
    }
    if (rot180 != 0 && rot180 != 1) {
        set_error("%s: rot180 must be 0 or 1 (got %d)", who, rot180);
        return VAA_E_INVALID;
    }
    if (Tx < 1 || Ty < 1) {
        set_error("%s: tap counts must be at least 1 (Tx=%d Ty=%d)", who, Tx, Ty);
        return VAA_E_INVALID;
    }
    if (H < kRsMinSide || H > kRsMaxSide || W < kRsMinSide || W > kRsMaxSide) {
        set_error("%s: source %dx%d outside [%d, %d] per side", who, H, W, kRsMinSide, kRsMaxSide);
        return VAA_E_UNSUPPORTED;
    }
    if (Tx > VAA_FRAME_RESIZE_MAX_TAPS || Ty > VAA_FRAME_RESIZE_MAX_TAPS) {
        set_error("%s: more than %d taps per output index (Tx=%d Ty=%d)", who, VAA_FRAME_RESIZE_MAX_TAPS, Tx, Ty);
        return VAA_E_UNSUPPORTED;
    }
    if (((uintptr_t)src_u8 & 3u) || ((uintptr_t)taps_dev & 3u) || ((uintptr_t)dst_u8 & 15u)) {
        set_error("%s: src_u8 and taps_dev must be 4-byte and dst_u8 16-byte aligned", who);
        return VAA_E_UNSUPPORTED;
    }
    int rc = check_axis(who, "x", start_x, w_x, Tx, W);
    if (rc != VAA_OK) return rc;
    rc = check_axis(who, "y", start_y, w_y, Ty, H);
    if (rc != VAA_OK) return rc;

    FrameResizeArgs a = {};
    a.src = src_u8; a.dst = dst_u8;
    a.sx = static_cast<const int32_t*>(taps_dev);
    a.sy = a.sx + VAA_IMG;
    a.wx = reinterpret_cast<const float*>(a.sy + VAA_IMG);
    a.wy = a.wx + (size_t)VAA_IMG * Tx;
    a.src_bytes = (size_t)B * H * W * 3;
    a.H = H; a.W = W; a.Tx = Tx; a.Ty = Ty; a.rot = rot180;
    a.chunk = W <= 1024 ? kRsMaxChunk : kRsMaxChunk / 2;
    a.pitch_dw = rs_pitch_dw(W);
    // at most 8*(672 + 770)*4 + 32 = 46,176 B (W = 1024), 4*(672 + 1538)*4 + 32 = 35,392 B (W = 2048)
    const size_t lds = (size_t)a.chunk * (kRsRowElems + a.pitch_dw) * 4 + kRsMaxChunk * 4 + (size_t)kRsBand * Ty * 4;  // + at most 1,824 B
    VAA_LAUNCH(frame_resize_kernel, dim3((unsigned)(B * kRsBands)), dim3(kRsThreads), lds, (hipStream_t)stream, a);
    return check_launch(who);
}
